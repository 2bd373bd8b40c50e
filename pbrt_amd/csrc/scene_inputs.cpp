// scene_inputs.cpp -- gather_inputs (scene_inputs.hpp) in its four parts.
#include "scene_inputs.hpp"

#include "image_texture.hpp"

namespace pbrt_hip {
namespace {

// the primitives: the caller's arrays as they are, or copies with the spheres' proxy triangles behind the mesh; and the sphere table
void gather_primitives(const pbrt_hip_scene_desc &d, SceneInputs *in) {
  in->P = d.P; in->idx = d.idx; in->mat = d.mat_id;
  in->n_verts = d.n_verts;
  in->n_prims = d.n_tris + d.n_spheres;
  if (d.n_spheres) {
    in->P_aug.assign(d.P, d.P + (d.n_tris ? 3 * (size_t)d.n_verts : 0));
    if (!d.n_tris) in->n_verts = 0;  // (a scene without triangles drops the caller's vertices)
    in->idx_aug.assign(d.idx, d.idx + 3 * (size_t)d.n_tris);
    in->mat_aug.assign(d.mat_id, d.mat_id + d.n_tris);
    for (uint32_t i = 0; i < d.n_spheres; i++) {
      const pbrt_hip_sphere &sp = d.spheres[i];
      const uint32_t v0 = in->n_verts + 2 * i;
      for (int k = 0; k < 3; k++) in->P_aug.push_back(sp.c[k] - sp.r);
      for (int k = 0; k < 3; k++) in->P_aug.push_back(sp.c[k] + sp.r);
      in->idx_aug.push_back(v0); in->idx_aug.push_back(v0 + 1); in->idx_aug.push_back(v0);
      in->mat_aug.push_back((uint16_t)sp.mat);
    }
    in->n_verts += 2 * d.n_spheres;
    in->P = in->P_aug.data(); in->idx = in->idx_aug.data(); in->mat = in->mat_aug.data();
  }
  in->spheres.resize(kSphereRows * (size_t)d.n_spheres);
  for (uint32_t i = 0; i < d.n_spheres; i++) write_sphere(&in->spheres[kSphereRows * (size_t)i], d.spheres[i]);
}

// the light table: the explicit lights, then every emissive triangle in index order; and what the lights say about the scene
void gather_lights(const pbrt_hip_scene_desc &d, const TextureTable &table, SceneInputs *in) {
  for (uint32_t i = 0; i < d.n_lights; i++) {
    const pbrt_hip_light &l = d.lights[i];
    if (l.type == PBRT_HIP_LIGHT_MAPPED) {
      push_light_mapped(&in->lights, l.p, l.c, *table.light_map(light_slot(l)));
      in->has_mapped = true;
      continue;
    }
    if (l.type == PBRT_HIP_LIGHT_SPOT) {
      push_light_spot(&in->lights, l.p, l.c, *table.cone(light_slot(l)));
      in->has_spot = true;
      continue;
    }
    if (l.type == PBRT_HIP_LIGHT_SPHERE) {  // (the sphere's row is marked for the MIS hit side)
      const uint32_t si = light_slot(l) - 1u;
      push_light_sphere(&in->lights, d.spheres[si], l.c);
      mark_sphere_listed(&in->spheres[kSphereRows * (size_t)si]);
      in->has_sphere_light = true;
      continue;
    }
    push_light_plain(&in->lights, dev_light_type(l.type), l.p, l.c);
    if (dev_light_type(l.type) == kDevLightInfinite) {
      for (int k = 0; k < 3; k++) in->le_inf[k] = in->le_inf[k] + l.c[k];
      in->has_inf = true;
    }
    if (l.type == PBRT_HIP_LIGHT_ENVMAP) {
      const pbrt_hip_envmap e = *table.envmap(light_slot(l));
      in->env = true;
      in->env_w = e.width; in->env_h = e.height;
      for (int k = 0; k < 9; k++) in->env_m[k] = e.world_to_light[k];
      for (int k = 0; k < 3; k++) in->env_c[k] = l.c[k];
      envmap_build_tables(e.rgb, e.width, e.height, &in->env_tables);
    }
  }
  for (uint32_t t = 0; t < d.n_tris; t++) {
    const pbrt_hip_material &m = d.mats[d.mat_id[t]];
    if (reuses_le(m)) continue;  // (its le is Kt / Ks: glass, plastic and substrate do not emit)
    if (!(m.le[0] > 0.f || m.le[1] > 0.f || m.le[2] > 0.f)) continue;
    const uint32_t *v = d.idx + 3 * (size_t)t;
    push_light_triangle(&in->lights, d.P + 3 * (size_t)v[0], d.P + 3 * (size_t)v[1], d.P + 3 * (size_t)v[2], m.le);
  }
}

void gather_materials(const pbrt_hip_scene_desc &d, SceneInputs *in) {
  in->mats.resize(kMatRows * (size_t)d.n_mats);
  for (uint32_t i = 0; i < d.n_mats; i++) write_material(&in->mats[kMatRows * (size_t)i], &in->mat_extra, i, d.n_mats, d.mats[i]);
}

// the texture rows and the images' texel pool: they go up only when something is textured, or a mapped light reads an image
void gather_textures(const TextureTable &table, SceneInputs *in) {
  if (!(table.textured_tris || table.textured_sph || in->has_mapped)) return;
  in->textures.resize(3 * table.kinds.size());  // (an environment map's / the normals' / the filter's / a cone's / a light map's slot: nothing on the device reads it, its rows stay zero)
  for (uint32_t i = 0; i < table.kinds.size(); i++) {
    if (table.kinds[i] != SlotKind::kChecker) continue;
    const pbrt_hip_texture tx = read_slot<pbrt_hip_texture>(table.slots, i);
    in->textures[3 * i] = make_float4(table_word(tx.type), tx.tex1[0], tx.tex1[1], tx.tex1[2]);
    in->textures[3 * i + 1] = make_float4(tx.tex2[0], tx.tex2[1], tx.tex2[2], tx.su);
    in->textures[3 * i + 2] = make_float4(tx.sv, tx.du, tx.dv, 0.f);
  }
  for (const TextureTable::Image &im : table.images)  // (its texels join the pool, its rows say where)
    image_pack(im.rec, &in->image_texels, &in->textures[3 * (size_t)im.slot]);
}

}  // namespace

void gather_inputs(const pbrt_hip_scene_desc &d, const TextureTable &table, SceneInputs *in) {
  gather_primitives(d, in);
  gather_lights(d, table, in);
  gather_materials(d, in);
  gather_textures(table, in);
}

}  // namespace pbrt_hip
