// capi_scene.cpp -- everything up to a finished scene behind the C ABI of include/pbrt_hip.h: checking a description, flattening it
// (scene_inputs.hpp), the upload, the tree (and the canonical tree a device-built scene gets on first use), the scene's getters, the host tree builders'
// entry points and the library's error text.  capi_render.cpp uses what is made here.  (Together they replace the empty body of
// PbrtAPI::world_end, /root/reference/src/core/api.rs:432-473.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pbrt_hip.h"
#include "build_stages.hpp"
#include "bvh_build.hpp"
#include "capi_internal.hpp"
#include "device_types.h"
#include "envmap.hpp"
#include "host_math.hpp"
#include "image_texture.hpp"
#include "pixel_filter.hpp"
#include "quad_nodes.hpp"
#include "scene_inputs.hpp"
#include "texture_table.hpp"

using namespace pbrt_hip;

namespace {

thread_local std::string g_err;

}  // namespace

namespace pbrt_hip {
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
const char *last_error_message() { return g_err.c_str(); }
}  // namespace pbrt_hip

namespace {

// A vertex that a triangle uses and that is NaN or infinite would send the builders' bucket index out of range:
// such input is refused at the boundary.  Returns the first offending vertex, or -1.
long long first_non_finite_vertex(const float *P, const uint32_t *idx, uint32_t n_tris) {
  for (size_t i = 0; i < 3 * (size_t)n_tris; i++) {
    const float *v = P + 3 * (size_t)idx[i];
    if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return (long long)idx[i];
  }
  return -1;
}

// `count` elements from `src` into `buf`, allocated anew, asynchronously on `stream` (src must live until the stream has caught up)
template <class T>
hipError_t upload(DevBuf<T> *buf, const T *src, size_t count, hipStream_t stream) {
  const hipError_t e = buf->alloc(count);
  if (e != hipSuccess || count == 0) return e;
  return hipMemcpyAsync(buf->p, src, count * sizeof(T), hipMemcpyHostToDevice, stream);
}

// The canonical tree (the oracle's binary tree) of the n primitives P / idx: the tree itself in s->bvh, its child-pair
// records in s->d_nodes, its leaf order in `order`, the scene's triangle records packed in that order into `tris`, and the tree's fields
// of *D (its array pointers are the caller's).  A host-built scene's tree (build_tree) and a device-built scene's counting walk (ensure_canonical) both come from here;
// `what` prefixes the refusals.  *host_ms (if asked for): the time of the tree and the pair records.
int build_canonical(pbrt_hip_scene *s, const float *P, const uint32_t *idx, uint32_t n, const std::string &what, DevBuf<uint32_t> *order,
                    DevBuf<float4> *tris, DevScene *D, double *host_ms = nullptr) {
  const auto t0 = std::chrono::steady_clock::now();
  build_bvh(P, idx, n, &s->bvh);
  if (s->bvh.depth > 64) return fail(PBRT_HIP_ERR_LIMIT, what + "BVH deeper than the 64-entry traversal stack");
  PairNodes pairs;
  std::string why;
  if (!make_pair_nodes(s->bvh, &pairs, &why)) return fail(PBRT_HIP_ERR_LIMIT, what + why);
  if (host_ms) *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  HIP_TRY(upload(&s->d_nodes, pairs.q.data(), pairs.q.size(), s->stream));
  HIP_TRY(upload(order, s->bvh.order.data(), n, s->stream));
  HIP_TRY(tris->alloc(kTriStride * (size_t)n));
  HIP_TRY(launch_pack_tris(s->d_P.p, s->d_idx.p, s->d_mat_id.p, order->p, n, D->n_tris, s->d_spheres.p, tris->p, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));  // (pairs is a local)
  D->n_nodes = (uint32_t)s->bvh.nodes.size();
  D->root_ref = pairs.root_ref;
  for (int k = 0; k < 3; k++) { D->root_lo[k] = pairs.root_lo[k]; D->root_hi[k] = pairs.root_hi[k]; }
  return PBRT_HIP_OK;
}

// ---- scene creation in stages (pbrt_hip_scene_create_ex): check_scene_desc, open, gather_inputs, upload_inputs, build_tree, set_view ----

// The accelerator's builder.  ONE default -- the device builder (binned SAH + parallel re-insertion + collapse), whoever asks and
// however (pbrt_hip_scene_create, flags 0, pbrt_hip_render_multi, the command line, bench.py); the host's binned-SAH builder only on
// request (PBRT_HIP_SCENE_HOST_BUILD / _OPTIMIZED_TREE, or PBRT_HIP_BUILDER=host in the environment when the caller left the choice open).
enum class Builder { kHost, kHostOptimized, kGpu, kGpuPlain };

// a glass material's index of refraction: the float whose bits ride in kd_tex
float glass_eta(const pbrt_hip_material &m) { float e; std::memcpy(&e, &m.kd_tex, 4); return e; }
// glass is an interface between index 1 and eta: eta = 1 (index-matched: nothing reflects, nothing bends) is legal; 16 is four times
// the densest real dielectric and keeps eta^2 and 1 / eta^2 -- the radiance scale of a refraction -- far from fp32's ends
constexpr float kGlassEtaMin = 1.0f, kGlassEtaMax = 16.0f;
// a plastic material's alpha rides in kd_tex the same way: the microfacet lobe's width, within [1e-3, 1] -- below, D's
// peak 1 / (pi alpha^2) leaves fp32's comfortable range; above, pbrt-v3's roughness remap never goes
float plastic_alpha(const pbrt_hip_material &m) { return glass_eta(m); }
constexpr float kPlasticAlphaMin = 1e-3f, kPlasticAlphaMax = 1.0f;
// how far a spot cone's axis may be from unit length, as a squared length
constexpr float kSpotAxisTolerance = 1e-4f;
// ---- check_scene_desc in stages: every refusal that depends on the description alone, before any HIP call.  Which of two faults is
// reported is part of the behaviour, so a concern whose refusals lie apart in that order has a stage for each part: the lights' and the
// materials' values early and their kinds last, the spheres' material ids and boxes apart from the mesh (check_scene_desc, below, is the order;
// tests/test_scene_refusals_host.py holds every message and pairs of faults across the stages) ----

// the camera and the crop window
int check_view(const pbrt_hip_scene_desc *d) {
  for (int k = 0; k < 16; k++)
    if (!std::isfinite(d->cam_to_world[k])) return fail(PBRT_HIP_ERR_INVALID, "scene_create: camera matrix is not finite");
  if (!(d->fov > 0.f && d->fov < 180.f)) return fail(PBRT_HIP_ERR_INVALID, "scene_create: fov must lie in (0, 180) degrees");
  for (int k = 0; k < 4; k++)  // Film "cropwindow": fractions of the film (film.rs:92-101 multiplies and rounds them up: a NaN or 1e30 there is an int overflow)
    if (!(d->crop[k] >= 0.f && d->crop[k] <= 1.f)) return fail(PBRT_HIP_ERR_INVALID, "scene_create: crop window values must lie in [0, 1]");
  return PBRT_HIP_OK;
}

// the film's size, the mesh and the spheres: arrays, counts, indices, finite coordinates
int check_mesh(const pbrt_hip_scene_desc *d) {
  if (d->xres <= 0 || d->yres <= 0) return fail(PBRT_HIP_ERR_INVALID, "scene_create: resolution must be positive");
  if (d->n_tris && (!d->P || !d->idx || !d->mat_id)) return fail(PBRT_HIP_ERR_INVALID, "scene_create: missing mesh arrays");
  if ((d->n_tris || d->n_spheres) && (!d->mats || d->n_mats == 0)) return fail(PBRT_HIP_ERR_INVALID, "scene_create: no materials");
  if (d->n_mats > 65536) return fail(PBRT_HIP_ERR_LIMIT, "scene_create: more than 65536 materials");
  if (d->n_tris > (1u << 24)) return fail(PBRT_HIP_ERR_LIMIT, "scene_create: more than 2^24 triangles (leaf references hold a 24-bit slot)");
  if ((uint64_t)d->n_tris + d->n_spheres > (1u << 24)) return fail(PBRT_HIP_ERR_LIMIT, "scene_create: more than 2^24 primitives (triangles + spheres; leaf references hold a 24-bit slot)");
  if (d->n_spheres && !d->spheres) return fail(PBRT_HIP_ERR_INVALID, "scene_create: n_spheres > 0 but no sphere table");
  for (size_t i = 0; i < 3 * (size_t)d->n_tris; i++)
    if (d->idx[i] >= d->n_verts) return fail(PBRT_HIP_ERR_INVALID, "scene_create: vertex index out of range");
  for (uint32_t t = 0; t < d->n_tris; t++)
    if (d->mat_id[t] >= d->n_mats) return fail(PBRT_HIP_ERR_INVALID, "scene_create: material id out of range");
  {
    const long long bad = first_non_finite_vertex(d->P, d->idx, d->n_tris);
    if (bad >= 0) return fail(PBRT_HIP_ERR_INVALID, "scene_create: vertex " + std::to_string(bad) + " is not finite");
  }
  for (uint32_t s = 0; s < d->n_spheres; s++) {
    const pbrt_hip_sphere &sp = d->spheres[s];
    if (!std::isfinite(sp.c[0]) || !std::isfinite(sp.c[1]) || !std::isfinite(sp.c[2]) || !std::isfinite(sp.r) || !(sp.r > 0.f))
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: sphere centre / radius must be finite and the radius positive");
  }
  return PBRT_HIP_OK;
}
// ... the spheres' material ids (after it, mats[mat_id[t]] and mats[spheres[s].mat] are there) ...
int check_sphere_materials(const pbrt_hip_scene_desc *d) {
  for (uint32_t s = 0; s < d->n_spheres; s++)
    if (d->spheres[s].mat >= d->n_mats) return fail(PBRT_HIP_ERR_INVALID, "scene_create: sphere material id out of range");
  return PBRT_HIP_OK;
}
// ... and their boxes
int check_sphere_boxes(const pbrt_hip_scene_desc *d) {
  for (uint32_t s = 0; s < d->n_spheres; s++)  // (a finite centre and radius can still make an infinite box)
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(d->spheres[s].c[k] - d->spheres[s].r) || !std::isfinite(d->spheres[s].c[k] + d->spheres[s].r))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: a sphere's bounding box is not finite");
  return PBRT_HIP_OK;
}

// (a NaN in a light's position or in a colour travels into ray directions and throughputs: a ray that is not a number is pruned by
// nothing and walks the whole tree -- minutes per frame on a large scene -- before its sample is dropped as NaN)
int check_light_values(const pbrt_hip_scene_desc *d) {
  if (d->n_lights && !d->lights) return fail(PBRT_HIP_ERR_INVALID, "scene_create: n_lights > 0 but no light table");
  for (uint32_t i = 0; i < d->n_lights; i++)
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(d->lights[i].p[k]) || !std::isfinite(d->lights[i].c[k]))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: light " + std::to_string(i) + ": position / direction / colour is not finite");
  return PBRT_HIP_OK;
}
// a spot light's cone: a unit axis and two cosines, cos_total <= cos_start
int check_spot_cone(const pbrt_hip_spot_cone &c, const std::string &what) {
  float len2 = 0.f;
  for (int k = 0; k < 3; k++) {
    if (!std::isfinite(c.axis[k])) return fail(PBRT_HIP_ERR_INVALID, what + "a spot light's axis is not finite");
    len2 += c.axis[k] * c.axis[k];
  }
  if (!(std::fabs(len2 - 1.0f) <= kSpotAxisTolerance)) return fail(PBRT_HIP_ERR_INVALID, what + "a spot light's axis must be a unit vector (squared length within 1e-4 of 1)");
  if (!std::isfinite(c.cos_total) || !std::isfinite(c.cos_start) || !(c.cos_total >= -1.f && c.cos_total <= 1.f) || !(c.cos_start >= -1.f && c.cos_start <= 1.f))
    return fail(PBRT_HIP_ERR_INVALID, what + "a spot light's cos_total / cos_start must be finite and lie in [-1, 1]");
  if (c.cos_total > c.cos_start) return fail(PBRT_HIP_ERR_INVALID, what + "a spot light's cos_total must not exceed cos_start (the falloff starts inside the cone)");
  return PBRT_HIP_OK;
}
// a mapped light's record: light_map_check's rules, and an `image` that names an image texture's slot
int check_light_map(const pbrt_hip_light_map &m, const TextureTable &table, const std::string &what) {
  const int rc = light_map_check(m, what);
  if (rc) return rc;
  if (table.named(m.image) != SlotKind::kImage) return fail(PBRT_HIP_ERR_INVALID, what + "light map: `image` must name a type-4 slot of the texture table (1-based)");
  return PBRT_HIP_OK;
}
int check_light_kinds(const pbrt_hip_scene_desc *d, const TextureTable &table) {
  for (uint32_t i = 0; i < d->n_lights; i++)
    if (d->lights[i].type > PBRT_HIP_LIGHT_ENVMAP && d->lights[i].type != PBRT_HIP_LIGHT_SPOT && d->lights[i].type != PBRT_HIP_LIGHT_MAPPED &&
        d->lights[i].type != PBRT_HIP_LIGHT_SPHERE)
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown light type");
  // (a sphere light -- DESIGN.md 3.25 -- likewise HERE, where a type-8 light was refused as unknown: the sphere it names, once, and a
  // material that emits what the light says.  check_mesh has held every sphere's radius to be finite and positive by now, and
  // check_light_values every light's p -- which this light does not use -- to be finite)
  std::vector<bool> listed(d->n_spheres, false);
  for (uint32_t i = 0; i < d->n_lights; i++) {
    if (d->lights[i].type != PBRT_HIP_LIGHT_SPHERE) continue;
    const std::string what = "scene_create: light " + std::to_string(i) + ": ";
    const uint32_t number = light_slot(d->lights[i]);
    if (number == 0u || number > d->n_spheres) return fail(PBRT_HIP_ERR_INVALID, what + "a sphere light (type 8) must name a sphere of the scene in `pad` (1-based)");
    if (listed[number - 1u]) return fail(PBRT_HIP_ERR_INVALID, what + "a second sphere light names sphere " + std::to_string(number - 1u));
    listed[number - 1u] = true;
    const pbrt_hip_material &m = d->mats[d->spheres[number - 1u].mat];
    if (reuses_le(m)) return fail(PBRT_HIP_ERR_INVALID, what + "sphere light: the sphere's material is glass, plastic or substrate, which do not emit");
    if (!(m.le[0] > 0.f || m.le[1] > 0.f || m.le[2] > 0.f)) return fail(PBRT_HIP_ERR_INVALID, what + "sphere light: the sphere's material has no positive le");
    if (std::memcmp(d->lights[i].c, m.le, sizeof m.le) != 0) return fail(PBRT_HIP_ERR_INVALID, what + "sphere light: c must equal the le of the sphere's material bit for bit");
  }
  // (a spot light and its cone are checked HERE, where the light's kind is recognised -- the place a type-5 light was refused as unknown
  // before there were spot lights --, so that every fault that used to win against it still does)
  for (uint32_t i = 0; i < d->n_lights; i++) {
    if (d->lights[i].type != PBRT_HIP_LIGHT_SPOT) continue;
    const std::string what = "scene_create: light " + std::to_string(i) + ": ";
    const pbrt_hip_spot_cone *cone = table.cone(light_slot(d->lights[i]));
    if (!cone) return fail(PBRT_HIP_ERR_INVALID, what + "a spot light (type 5) must name a type-6 slot of the texture table, its cone, in `pad`");
    const int rc = check_spot_cone(*cone, what);
    if (rc) return rc;
  }
  for (const TextureTable::Cone &c : table.cones) {  // (a cone no light names is held to the same rules)
    const int rc = check_spot_cone(c.rec, "scene_create: texture slot " + std::to_string(c.slot + 1) + ": ");
    if (rc) return rc;
  }
  // (a mapped light and its record likewise: DESIGN.md 3.23)
  for (uint32_t i = 0; i < d->n_lights; i++) {
    if (d->lights[i].type != PBRT_HIP_LIGHT_MAPPED) continue;
    const std::string what = "scene_create: light " + std::to_string(i) + ": ";
    const pbrt_hip_light_map *map = table.light_map(light_slot(d->lights[i]));
    if (!map) return fail(PBRT_HIP_ERR_INVALID, what + "a mapped light (type 6) must name a type-8 slot of the texture table, its light map, in `pad`");
    const int rc = check_light_map(*map, table, what);
    if (rc) return rc;
  }
  for (const TextureTable::LightMap &m : table.light_maps) {  // (a record no light names is held to the same rules)
    const int rc = check_light_map(m.rec, table, "scene_create: texture slot " + std::to_string(m.slot + 1) + ": ");
    if (rc) return rc;
  }
  uint32_t n_env = 0;
  for (uint32_t i = 0; i < d->n_lights; i++) {  // an environment-map light names a type-1 slot of the texture table; one per scene
    if (d->lights[i].type != PBRT_HIP_LIGHT_ENVMAP) continue;
    if (table.named(light_slot(d->lights[i])) != SlotKind::kEnvmap)
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: light " + std::to_string(i) + ": an environment-map light (type 3) must name a type-1 slot of the texture table in `pad`");
    if (++n_env > 1u) return fail(PBRT_HIP_ERR_LIMIT, "scene_create: more than one environment-map light (type 3)");
  }
  return PBRT_HIP_OK;
}

int check_material_values(const pbrt_hip_scene_desc *d) {
  for (uint32_t i = 0; i < d->n_mats; i++)
    for (int k = 0; k < 3; k++)
      if (!reuses_le(d->mats[i]) && (!std::isfinite(d->mats[i].k[k]) || !std::isfinite(d->mats[i].le[k])))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": colour / emission is not finite");
  for (uint32_t i = 0; i < d->n_mats; i++) {  // glass: k = Kr, le = Kt, kd_tex = the bits of eta
    const pbrt_hip_material &m = d->mats[i];
    if (m.type != PBRT_HIP_MATERIAL_GLASS) continue;
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(m.k[k]) || !std::isfinite(m.le[k]) || !(m.k[k] >= 0.f) || !(m.le[k] >= 0.f))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": glass Kr / Kt must be finite and >= 0");
    const float eta = glass_eta(m);
    if (!std::isfinite(eta) || !(eta >= kGlassEtaMin && eta <= kGlassEtaMax))
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": glass eta (the float in kd_tex) must be finite and lie in [1, 16]");
  }
  return PBRT_HIP_OK;
}
// what the materials' kd_tex name
int check_kd_tex(const pbrt_hip_scene_desc *d, const TextureTable &table) {
  for (uint32_t i = 0; i < d->n_mats; i++) {
    if (reuses_le(d->mats[i])) continue;  // (kd_tex holds eta / alpha)
    if (table.named(d->mats[i].kd_tex) == SlotKind::kOutOfRange) return fail(PBRT_HIP_ERR_INVALID, "scene_create: material texture number out of range");
  }
  for (uint32_t i = 0; i < d->n_mats; i++) {  // (a texture for Kd is a checkerboard or an image; a slot of no known kind is check_table's to refuse)
    if (!kd_textured(d->mats[i])) continue;
    const char *names = nullptr;
    switch (table.named(d->mats[i].kd_tex)) {
      case SlotKind::kEnvmap: names = "an environment map"; break;
      case SlotKind::kNormals: names = "the shading normals' record"; break;
      case SlotKind::kFilter: names = "the pixel filter's record"; break;
      case SlotKind::kSpot: names = "a spot light's cone"; break;
      case SlotKind::kLightMap: names = "a light map's record"; break;
      default: break;
    }
    if (names) return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": kd_tex names " + names + ", which is not a texture for Kd");
  }
  return PBRT_HIP_OK;
}
int check_material_kinds(const pbrt_hip_scene_desc *d) {
  for (uint32_t i = 0; i < d->n_mats; i++)
    if (d->mats[i].type > PBRT_HIP_MATERIAL_SUBSTRATE) return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown material type");
  // (a plastic record is checked HERE, where its kind is recognised -- the place a type-3 record was refused as unknown before there was
  // plastic --, so that every fault that used to win against it still does)
  for (uint32_t i = 0; i < d->n_mats; i++) {  // plastic: k = Kd, le = Ks, kd_tex = the bits of alpha
    const pbrt_hip_material &m = d->mats[i];
    if (m.type != PBRT_HIP_MATERIAL_PLASTIC) continue;
    // Until 0.10 type 3 was no material at all.  A type-3 record that carries NOTHING of plastic -- no Ks and no alpha word: the words a
    // matte record leaves zero -- is what a caller of that ABI wrote, and keeps the refusal it always had, word for word
    if (m.kd_tex == 0u && m.le[0] == 0.f && m.le[1] == 0.f && m.le[2] == 0.f) return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown material type");
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(m.k[k]) || !std::isfinite(m.le[k]) || !(m.k[k] >= 0.f) || !(m.le[k] >= 0.f))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": plastic Kd / Ks must be finite and >= 0");
    const float alpha = plastic_alpha(m);
    if (!std::isfinite(alpha) || !(alpha >= kPlasticAlphaMin && alpha <= kPlasticAlphaMax))  // (the message names both readings of the record)
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": plastic alpha (the float in kd_tex) must be finite and lie in [1e-3, 1]; "
                  "type 3 is plastic since 0.11, to a caller that meant anything else it is an unknown material type");
  }
  for (uint32_t i = 0; i < d->n_mats; i++) {  // substrate: the record as plastic reuses it; 1 - Ks must not go negative
    const pbrt_hip_material &m = d->mats[i];
    if (m.type != PBRT_HIP_MATERIAL_SUBSTRATE) continue;
    for (int k = 0; k < 3; k++) {
      if (!std::isfinite(m.k[k]) || !(m.k[k] >= 0.f))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": substrate Kd must be finite and >= 0");
      if (!std::isfinite(m.le[k]) || !(m.le[k] >= 0.f && m.le[k] <= 1.0f))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": substrate Ks must be finite and lie in [0, 1]");
    }
    const float alpha = plastic_alpha(m);
    if (!std::isfinite(alpha) || !(alpha >= kPlasticAlphaMin && alpha <= kPlasticAlphaMax))
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": substrate alpha (the float in kd_tex) must be finite and lie in [1e-3, 1]");
  }
  return PBRT_HIP_OK;
}
// Plastic is rendered by the GLS instantiations of render_kernel_x alone: the families that render an environment map or
// shading normals do not carry its branch, and the scene is refused here, not at render time.  Substrate (3.24) shares the branch and the
// refusal; a spot light (3.22), a mapped light (3.23) and a sphere light (3.25) are sampled under PLS alone, in the same instantiations.  Each is refused under its
// own name, and of several the first in this order is the one named
int check_pls_family(const pbrt_hip_scene_desc *d, const TextureTable &table) {
  auto has_material = [&](uint32_t type) { return std::any_of(d->mats, d->mats + d->n_mats, [&](const pbrt_hip_material &m) { return m.type == type; }); };
  auto has_light = [&](uint32_t type) { return std::any_of(d->lights, d->lights + d->n_lights, [&](const pbrt_hip_light &l) { return l.type == type; }); };
  const struct { bool present; const char *noun; } needs_pls[] = {
      {has_material(PBRT_HIP_MATERIAL_PLASTIC), "a plastic material"},
      {has_material(PBRT_HIP_MATERIAL_SUBSTRATE), "a substrate material"},
      {has_light(PBRT_HIP_LIGHT_SPOT), "a spot light"},
      {has_light(PBRT_HIP_LIGHT_MAPPED), "a light map (a projection or goniometric light)"},
      {has_light(PBRT_HIP_LIGHT_SPHERE), "a sphere light"}};
  for (const auto &n : needs_pls) {
    if (!n.present) continue;
    for (const SlotKind kind : table.kinds) {
      if (kind == SlotKind::kEnvmap) return fail(PBRT_HIP_ERR_LIMIT, std::string("scene_create: ") + n.noun + " is not available in a scene with an environment map");
      if (kind == SlotKind::kNormals) return fail(PBRT_HIP_ERR_LIMIT, std::string("scene_create: ") + n.noun + " is not available in a scene with shading normals");
    }
  }
  return PBRT_HIP_OK;
}

// the records of the texture table in slot order, then the images' texels, then the (u, v) that textured triangles need
int check_table(const pbrt_hip_scene_desc *d, const TextureTable &table) {
  uint32_t n_normals = 0, n_filters = 0, n_images = 0;
  uint64_t image_texels = 0;
  for (uint32_t i = 0; i < table.kinds.size(); i++) {
    const std::string what = "scene_create: texture slot " + std::to_string(i + 1) + ": ";
    int rc = PBRT_HIP_OK;
    switch (table.kinds[i]) {
      case SlotKind::kImage: {
        const pbrt_hip_image_texture &im = table.images[n_images].rec;
        if ((rc = image_check(im, what))) return rc;
        image_texels += (uint64_t)im.width * im.height;
        rc = image_check_totals(++n_images, image_texels, what);
        break;
      }
      case SlotKind::kFilter:
        if (++n_filters > 1u) return fail(PBRT_HIP_ERR_LIMIT, what + "more than one pixel filter record (type 3)");
        rc = filter_check(*table.filter, what);
        break;
      case SlotKind::kNormals: {
        if (++n_normals > 1u) return fail(PBRT_HIP_ERR_LIMIT, what + "shading normals: more than one normals record (type 2)");
        const pbrt_hip_normals &nr = *table.normals;
        if (nr.n_tris != d->n_tris) return fail(PBRT_HIP_ERR_INVALID, what + "shading normals: n_tris is " + std::to_string(nr.n_tris) + ", the description has " + std::to_string(d->n_tris) + " triangles");
        if (!nr.tri_n) return fail(PBRT_HIP_ERR_INVALID, what + "shading normals: tri_n is NULL");
        for (size_t k = 0; k < 9 * (size_t)nr.n_tris; k++)
          if (!std::isfinite(nr.tri_n[k])) return fail(PBRT_HIP_ERR_INVALID, what + "shading normals: component " + std::to_string(k % 9) + " of triangle " + std::to_string(k / 9) + " is not finite");
        break;
      }
      case SlotKind::kEnvmap:
        rc = envmap_check(read_slot<pbrt_hip_envmap>(table.slots, i), what);
        break;
      case SlotKind::kChecker: {
        const pbrt_hip_texture tx = read_slot<pbrt_hip_texture>(table.slots, i);
        if (!std::isfinite(tx.su) || !std::isfinite(tx.sv) || !std::isfinite(tx.du) || !std::isfinite(tx.dv))
          return fail(PBRT_HIP_ERR_INVALID, "scene_create: texture mapping is not finite");
        for (int k = 0; k < 3; k++)
          if (!std::isfinite(tx.tex1[k]) || !std::isfinite(tx.tex2[k])) return fail(PBRT_HIP_ERR_INVALID, "scene_create: texture colour is not finite");
        break;
      }
      case SlotKind::kSpot: break;  // (a cone is checked with the lights, check_light_kinds)
      case SlotKind::kLightMap: break;  // (likewise)
      default: return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown texture type");
    }
    if (rc) return rc;
  }
  for (const TextureTable::Image &im : table.images) {  // (the images' texels, once every size and the caps have passed)
    const int rc = image_check_texels(im.rec, "scene_create: texture slot " + std::to_string(im.slot + 1) + ": ");
    if (rc) return rc;
  }
  if (table.textured_tris) {
    if (!d->tri_uv) return fail(PBRT_HIP_ERR_INVALID, "scene_create: a triangle's material is textured but tri_uv is NULL");
    for (size_t i = 0; i < 6 * (size_t)d->n_tris; i++)
      if (!std::isfinite(d->tri_uv[i])) return fail(PBRT_HIP_ERR_INVALID, "scene_create: tri_uv is not finite");
  }
  return PBRT_HIP_OK;
}

// the builder that `flags` (and PBRT_HIP_BUILDER) ask for
int check_flags(uint32_t flags, Builder *builder) {
  if (flags & ~(PBRT_HIP_SCENE_GPU_BUILD | PBRT_HIP_SCENE_OPTIMIZED_TREE | PBRT_HIP_SCENE_PLAIN_TREE | PBRT_HIP_SCENE_HOST_BUILD))
    return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown flag");
  const bool want_host = (flags & (PBRT_HIP_SCENE_HOST_BUILD | PBRT_HIP_SCENE_OPTIMIZED_TREE)) != 0u;
  const bool want_gpu = (flags & (PBRT_HIP_SCENE_GPU_BUILD | PBRT_HIP_SCENE_PLAIN_TREE)) != 0u;
  if (want_host && want_gpu)
    return fail(PBRT_HIP_ERR_INVALID, "scene_create: PBRT_HIP_SCENE_HOST_BUILD / _OPTIMIZED_TREE are host builds, not combined with PBRT_HIP_SCENE_GPU_BUILD / _PLAIN_TREE");
  const char *env = want_host || want_gpu ? nullptr : std::getenv("PBRT_HIP_BUILDER");
  if (flags & PBRT_HIP_SCENE_OPTIMIZED_TREE) *builder = Builder::kHostOptimized;
  else if ((flags & PBRT_HIP_SCENE_HOST_BUILD) || (env && std::strcmp(env, "host") == 0)) *builder = Builder::kHost;
  else *builder = (flags & PBRT_HIP_SCENE_PLAIN_TREE) ? Builder::kGpuPlain : Builder::kGpu;  // (PBRT_HIP_SCENE_PLAIN_TREE alone qualifies the default)
  return PBRT_HIP_OK;
}

// The stages in their order; the description's table is decoded once the indices it goes by are known to be sound (*table: what
// gather_inputs -- scene_inputs.hpp -- and upload_inputs go by)
int check_scene_desc(const pbrt_hip_scene_desc *d, uint32_t flags, Builder *builder, TextureTable *table) {
  int rc;
  if ((rc = check_mesh(d)) || (rc = check_light_values(d)) || (rc = check_material_values(d)) || (rc = check_view(d)) || (rc = check_sphere_materials(d))) return rc;
  if (d->n_textures && !d->textures) return fail(PBRT_HIP_ERR_INVALID, "scene_create: n_textures > 0 but no texture table");
  *table = decode_texture_table(*d);
  if ((rc = check_kd_tex(d, *table)) || (rc = check_table(d, *table)) || (rc = check_flags(flags, builder)) || (rc = check_sphere_boxes(d))) return rc;
  if ((rc = check_light_kinds(d, *table))) return rc;
  if ((rc = check_material_kinds(d))) return rc;
  return check_pls_family(d, *table);
}

// The inputs into the scene's arrays (asynchronously: `in` outlives the stream's synchronisation) and the counts of s->dev they make
int upload_inputs(pbrt_hip_scene *s, const pbrt_hip_scene_desc &d, const TextureTable &table, const SceneInputs &in) {
  HIP_TRY(upload(&s->d_P, in.P, 3 * (size_t)in.n_verts, s->stream));
  HIP_TRY(upload(&s->d_idx, in.idx, 3 * (size_t)in.n_prims, s->stream));
  HIP_TRY(upload(&s->d_mat_id, in.mat, in.n_prims, s->stream));
  HIP_TRY(upload(&s->d_mats, in.mats.data(), in.mats.size(), s->stream));
  HIP_TRY(upload(&s->d_lights, in.lights.data(), in.lights.size(), s->stream));
  HIP_TRY(upload(&s->d_spheres, in.spheres.data(), in.spheres.size(), s->stream));
  HIP_TRY(upload(&s->d_textures, in.textures.data(), in.textures.size(), s->stream));
  HIP_TRY(upload(&s->d_mat_extra, in.mat_extra.data(), in.mat_extra.size(), s->stream));
  HIP_TRY(upload(&s->d_image_texels, in.image_texels.data(), in.image_texels.size(), s->stream));
  if (in.env) {
    HIP_TRY(upload(&s->d_env_texels, in.env_tables.texels.data(), in.env_tables.texels.size(), s->stream));
    HIP_TRY(upload(&s->d_env_marginal, in.env_tables.marginal.data(), in.env_tables.marginal.size(), s->stream));
    HIP_TRY(upload(&s->d_env_conditional, in.env_tables.conditional.data(), in.env_tables.conditional.size(), s->stream));
    s->env = true;
    s->env_w = in.env_w; s->env_h = in.env_h;
    for (int k = 0; k < 9; k++) s->env_m[k] = in.env_m[k];
    for (int k = 0; k < 3; k++) s->env_c[k] = in.env_c[k];
  }
  if (table.textured_tris) HIP_TRY(upload(&s->d_tri_uv_in, d.tri_uv, 6 * (size_t)d.n_tris, s->stream));
  if (table.normals) {  // (the caller's array: it outlives the call, and the stream is synchronised before the call returns)
    HIP_TRY(upload(&s->d_tri_n_in, table.normals->tri_n, 9 * (size_t)d.n_tris, s->stream));
    s->normals = in.n_prims > 0;  // (a scene without a primitive has no hit to shade and no leaf slot to hold a normal)
  }
  DevScene &D = s->dev;
  D.n_tris = d.n_tris;  // (the triangles: a hit's primitive id >= this is sphere id - n_tris)
  D.n_spheres = d.n_spheres;
  D.n_lights = (uint32_t)(in.lights.size() / kLightRows);
  D.n_lights_f = (float)D.n_lights;
  for (int k = 0; k < 3; k++) D.le_inf[k] = in.le_inf[k];
  D.has_inf = in.has_inf ? 1u : 0u;
  return PBRT_HIP_OK;
}

// The tree over the uploaded primitives, on the host or on the device: d_nodes, d_quads and d_order, the triangle records packed in
// leaf order into d_tris, s->build, and the tree's fields of s->dev (root ref and box, n_nodes, the walk's stack need).
int build_tree(pbrt_hip_scene *s, const SceneInputs &in, Builder builder) {
  DevScene &D = s->dev;
  const uint32_t np = in.n_prims;
  s->gpu_built = (builder == Builder::kGpu || builder == Builder::kGpuPlain) && np >= 2;
  if (s->gpu_built) {  // the walk enters quad 0 through the root box; there is no canonical binary tree
    HIP_TRY(s->d_order.alloc(np));
    HIP_TRY(s->d_quads.alloc(4 * (size_t)np));
    HIP_TRY(s->d_tris.alloc(kTriStride * (size_t)np));
    GpuBuildInfo gb{};
    HIP_TRY(gpu_build_quads(s->d_P.p, s->d_idx.p, np, s->d_order.p, s->d_quads.p, np, builder == Builder::kGpuPlain ? 0u : kGpuBuildReinsert, &gb,
                            s->stream));
    if (gb.stack_need + 1u > 4096u) return fail(PBRT_HIP_ERR_LIMIT, "scene_create: device-built tree too deep");
    HIP_TRY(launch_pack_tris(s->d_P.p, s->d_idx.p, s->d_mat_id.p, s->d_order.p, np, D.n_tris, s->d_spheres.p, s->d_tris.p, s->stream));
    s->build.build_ms = gb.build_ms;
    s->build.reinsert = gb.reinsert;
    s->n_quads_gpu = gb.n_quads;
    D.n_nodes = 2u * np - 1u;
    D.root_ref = 0u;
    for (int k = 0; k < 3; k++) { D.root_lo[k] = gb.root_lo[k]; D.root_hi[k] = gb.root_hi[k]; }
    D.quad_stack_need = gb.stack_need;
  } else {
    double canon_ms = 0.0;
    const int rc = build_canonical(s, in.P, in.idx, np, "scene_create: ", &s->d_order, &s->d_tris, &D, &canon_ms);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const char *sl = debug_knob("PBRT_HIP_SPLIT_LEAVES");
    QuadNodes quads;
    build_production_quads(s->bvh, in.P, in.idx, np, builder == Builder::kHostOptimized ? kTreeReinsert : production_tree_default(),
                           !(sl && sl[0] == '0'), &quads);
    s->build.build_ms = canon_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    HIP_TRY(upload(&s->d_quads, quads.q.data(), quads.q.size(), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));  // (quads is a local)
    D.quad_stack_need = quads.stack_need;
  }
  D.inv_parallel = inv_parallel_for_extent(std::max(D.root_hi[0] - D.root_lo[0], std::max(D.root_hi[1] - D.root_lo[1], D.root_hi[2] - D.root_lo[2])));
  return PBRT_HIP_OK;
}

// The perspective camera and the crop window of `d` into D: screen window from the aspect ratio, fov on the shorter axis
void set_view(DevScene *D, const pbrt_hip_scene_desc &d) {
  for (int k = 0; k < 12; k++) D->c2w[k] = d.cam_to_world[k];
  const float aspect = (float)d.xres / (float)d.yres;
  float sx0, sx1, sy0, sy1;
  if (aspect > 1.f) { sx0 = -aspect; sx1 = aspect; sy0 = -1.f; sy1 = 1.f; }
  else { sx0 = -1.f; sx1 = 1.f; sy0 = -1.f / aspect; sy1 = 1.f / aspect; }
  const float tan_half = (float)std::tan((double)d.fov * (3.14159265358979323846 / 180.0) * 0.5);
  D->cam_ax = ((sx1 - sx0) / (float)d.xres) * tan_half;
  D->cam_bx = sx0 * tan_half;
  D->cam_ay = -((sy1 - sy0) / (float)d.yres) * tan_half;
  D->cam_by = sy1 * tan_half;
  D->xres = d.xres;
  D->yres = d.yres;
  int32_t cb[4];
  film_cropped_bounds(d.xres, d.yres, d.crop, cb);
  D->cx0 = cb[0]; D->cy0 = cb[1]; D->cx1 = cb[2]; D->cy1 = cb[3];
}

}  // namespace

namespace pbrt_hip {
void bind_scene_arrays(pbrt_hip_scene *s) {
  DevScene &D = s->dev;
  D.nodes = s->d_nodes.p;
  D.quads = s->d_quads.p;
  D.tris = s->d_tris.p;
  D.mats = s->d_mats.p;
  D.lights = s->d_lights.p;
  D.spheres = s->d_spheres.p;
}

// The counter flags (PBRT_HIP_FLAG_COUNTERS, counters of pbrt_hip_intersect) count the CANONICAL walk: the oracle's binary
// tree of DESIGN.md 3.3.  A host-built scene has it; a device-built one gets it here on first use -- vertex / index buffers
// read back from the device, the host builder (one core, about a second for 1M triangles: a measurement aid, off the
// product's path), child-pair records and triangle records in the canonical leaf order uploaded beside the production arrays.
int ensure_canonical(pbrt_hip_scene *s) {
  if (s->canonical_ready) return PBRT_HIP_OK;
  if (!s->gpu_built) { s->dev_exact = s->dev; s->canonical_ready = true; return PBRT_HIP_OK; }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<float> P(s->d_P.n);
  std::vector<uint32_t> idx(s->d_idx.n);
  HIP_TRY(hipSetDevice(s->device));
  if (!P.empty()) HIP_TRY(hipMemcpy(P.data(), s->d_P.p, P.size() * 4, hipMemcpyDeviceToHost));
  if (!idx.empty()) HIP_TRY(hipMemcpy(idx.data(), s->d_idx.p, idx.size() * 4, hipMemcpyDeviceToHost));
  s->dev_exact = s->dev;
  const int rc = build_canonical(s, P.data(), idx.data(), s->n_prims, "counters: canonical ", &s->d_order_exact, &s->d_tris_exact, &s->dev_exact);
  if (rc) return rc;
  bind_scene_arrays(s);  // (d_nodes: the pre-canonical allocation was empty and has just been released, no stale pointer is kept)
  s->dev_exact.nodes = s->d_nodes.p;
  s->dev_exact.tris = s->d_tris_exact.p;
  s->device_bytes = s->bytes();
  s->canonical_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  s->canonical_ready = true;
  return PBRT_HIP_OK;
}
}  // namespace pbrt_hip

// ---- the device tree builder between its stages, and the host's runs of stages 2 and 3 on a given tree (build_stages.hpp) ----
namespace {
template <class T>
void copy_out(T *dst, const std::vector<T> &src) {
  if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(T));
}
void copy_tree_out(const StageTree &t, uint32_t *child, uint32_t *parent_internal, uint32_t *parent_leaf, float *boxes, uint32_t *order) {
  copy_out(child, t.child); copy_out(parent_internal, t.parent_internal); copy_out(parent_leaf, t.parent_leaf);
  copy_out(boxes, t.boxes); copy_out(order, t.order);
}
// a binary tree handed in as child words / boxes / leaf order: the refusals the two host hooks share (the words themselves:
// link_tree_of_child_words)
int check_stage_tree(const char *who, uint32_t n_tris, const uint32_t *child, const float *boxes, const uint32_t *order) {
  const std::string w = who;
  if (!child || !boxes || !order) return fail(PBRT_HIP_ERR_INVALID, w + ": null argument");
  if (n_tris < 2u || n_tris > 0x7fffffffu) return fail(PBRT_HIP_ERR_INVALID, w + ": fewer than two triangles (or more than 2^31 - 1)");
  for (size_t i = 0; i < 6 * (2 * (size_t)n_tris - 1); i++)
    if (!std::isfinite(boxes[i])) return fail(PBRT_HIP_ERR_INVALID, w + ": a box is not finite");
  for (uint32_t k = 0; k < n_tris; k++)
    if (order[k] >= n_tris) return fail(PBRT_HIP_ERR_INVALID, w + ": a triangle id of the leaf order is out of range");
  return PBRT_HIP_OK;
}
}  // namespace

int pbrt_hip_scene::open(int on_device) {
  device = on_device;
  HIP_TRY(hipSetDevice(device));
  int cus = 0;
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  n_cu = cus > 0 ? (uint32_t)cus : 1u;
  HIP_TRY(hipStreamCreate(&stream));
  HIP_TRY(hipEventCreate(&ev0));
  HIP_TRY(hipEventCreate(&ev1));
  HIP_TRY(d_counters.alloc(80));  // [0..4] ray / visit counters, [6..7] pixel-order scratch, [8..71] the pixel hand-out counters
  return PBRT_HIP_OK;
}

extern "C" {

int pbrt_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *pbrt_hip_last_error(void) { return pbrt_hip::last_error_message(); }
const char *pbrt_hip_version(void) { return "pbrt_hip 0.14 (gfx950; struct sizes of 0.6, as 0.7, 0.8, 0.9, 0.10, 0.11, 0.12 and 0.13)"; }
#ifndef PBRT_HIP_BUILD_ID
#define PBRT_HIP_BUILD_ID "unknown"
#endif
const char *pbrt_hip_build_id(void) { return PBRT_HIP_BUILD_ID; }

int pbrt_hip_bvh_build_host(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, uint32_t *nodes,
                            uint32_t *order, uint32_t *n_nodes, uint32_t *depth) {
  return guarded([&]() -> int {
    if ((n_tris && (!P || !idx)) || !n_nodes || !depth) return fail(PBRT_HIP_ERR_INVALID, "bvh_build_host: null argument");
    for (size_t i = 0; i < 3 * (size_t)n_tris; i++)
      if (idx[i] >= n_verts) return fail(PBRT_HIP_ERR_INVALID, "bvh_build_host: vertex index out of range");
    if (first_non_finite_vertex(P, idx, n_tris) >= 0) return fail(PBRT_HIP_ERR_INVALID, "bvh_build_host: a vertex is not finite");
    Bvh b;
    build_bvh(P, idx, n_tris, &b);
    *n_nodes = (uint32_t)b.nodes.size();
    *depth = b.depth;
    if (nodes && !b.nodes.empty()) std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(BvhNode));
    if (order && !b.order.empty()) std::memcpy(order, b.order.data(), b.order.size() * 4);
    return PBRT_HIP_OK;
  });
}

int pbrt_hip_quad_build_host(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, int split_leaves,
                             uint32_t *quads, uint32_t cap_nodes, uint32_t *n_quads, uint32_t *stack_need) {
  return pbrt_hip_quad_build_host_ex(P, n_verts, idx, n_tris, split_leaves, PBRT_HIP_TREE_DEFAULT, quads, cap_nodes, n_quads, stack_need,
                                     nullptr, nullptr, nullptr, nullptr);
}

int pbrt_hip_quad_build_host_ex(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, int split_leaves, uint32_t tree,
                                uint32_t *quads, uint32_t cap_nodes, uint32_t *n_quads, uint32_t *stack_need, uint32_t *order,
                                float *root_box, uint32_t *n_refs, float *exact_boxes) {
  return guarded([&]() -> int {
    if ((n_tris && (!P || !idx)) || !n_quads || !stack_need) return fail(PBRT_HIP_ERR_INVALID, "quad_build_host: null argument");
    if (tree != PBRT_HIP_TREE_SAH && tree != PBRT_HIP_TREE_REINSERT && tree != PBRT_HIP_TREE_DEFAULT) return fail(PBRT_HIP_ERR_INVALID, "quad_build_host: unknown tree");
    for (size_t i = 0; i < 3 * (size_t)n_tris; i++)
      if (idx[i] >= n_verts) return fail(PBRT_HIP_ERR_INVALID, "quad_build_host: vertex index out of range");
    if (first_non_finite_vertex(P, idx, n_tris) >= 0) return fail(PBRT_HIP_ERR_INVALID, "quad_build_host: a vertex is not finite");
    Bvh b;
    build_bvh(P, idx, n_tris, &b);
    QuadNodes q;
    const ProductionTree pt = tree == PBRT_HIP_TREE_DEFAULT ? production_tree_default() : (ProductionTree)tree;
    build_production_quads(b, P, idx, n_tris, pt, split_leaves != 0, &q, n_refs);
    *n_quads = (uint32_t)(q.q.size() / 4);
    *stack_need = q.stack_need;
    if (order && !b.order.empty()) std::memcpy(order, b.order.data(), b.order.size() * 4);
    if (root_box && !b.nodes.empty())
      for (int a = 0; a < 3; a++) { root_box[a] = b.nodes[0].lo[a]; root_box[3 + a] = b.nodes[0].hi[a]; }
    if (quads) {
      if (*n_quads > cap_nodes) return fail(PBRT_HIP_ERR_LIMIT, "quad_build_host: output too small");
      if (!q.q.empty()) std::memcpy(quads, q.q.data(), q.q.size() * 16);
      if (exact_boxes && !q.exact.empty()) std::memcpy(exact_boxes, q.exact.data(), q.exact.size() * 4);
    }
    return PBRT_HIP_OK;
  });
}

int pbrt_hip_gpu_build_stages_device(int device, const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, uint32_t flags,
                                     pbrt_hip_build_stages *out) {
  return guarded([&]() -> int {
    if (!P || !idx || !out) return fail(PBRT_HIP_ERR_INVALID, "gpu_build_stages: null argument");
    if (n_tris < 2u || n_tris > 0x7fffffffu) return fail(PBRT_HIP_ERR_INVALID, "gpu_build_stages: fewer than two triangles (or more than 2^31 - 1)");
    if (flags & ~PBRT_HIP_BUILD_STAGES_REINSERT) return fail(PBRT_HIP_ERR_INVALID, "gpu_build_stages: unknown flag");
    for (size_t i = 0; i < 3 * (size_t)n_tris; i++)
      if (idx[i] >= n_verts) return fail(PBRT_HIP_ERR_INVALID, "gpu_build_stages: vertex index out of range");
    if (first_non_finite_vertex(P, idx, n_tris) >= 0) return fail(PBRT_HIP_ERR_INVALID, "gpu_build_stages: a vertex is not finite");
    const int ndev = pbrt_hip_device_count();
    if (ndev <= 0) return fail(PBRT_HIP_ERR_NO_DEVICE, "gpu_build_stages: no HIP device (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(PBRT_HIP_ERR_INVALID, "gpu_build_stages: device index out of range");
    HIP_TRY(hipSetDevice(device));
    const hipStream_t stream = nullptr;  // (the device's default stream, as the other hooks)
    DevBuf<float> d_P;
    DevBuf<uint32_t> d_idx, d_order;
    DevBuf<uint4> d_quads;
    HIP_TRY(upload(&d_P, P, 3 * (size_t)n_verts, stream));
    HIP_TRY(upload(&d_idx, idx, 3 * (size_t)n_tris, stream));
    HIP_TRY(d_order.alloc(n_tris));
    HIP_TRY(d_quads.alloc(4 * (size_t)n_tris));
    GpuBuildInfo gb{};
    GpuBuildStages st;
    HIP_TRY(gpu_build_quads(d_P.p, d_idx.p, n_tris, d_order.p, d_quads.p, n_tris, (flags & PBRT_HIP_BUILD_STAGES_REINSERT) ? kGpuBuildReinsert : 0u, &gb,
                            stream, &st));
    copy_out(out->morton_keys, st.morton_keys);
    copy_tree_out(st.built, out->built_child, out->built_parent_internal, out->built_parent_leaf, out->built_boxes, out->built_order);
    copy_out(out->links_par, st.par); copy_out(out->links_kid, st.kid); copy_out(out->links_boxes, st.bx);
    copy_tree_out(st.optimised, out->opt_child, out->opt_parent_internal, out->opt_parent_leaf, out->opt_boxes, out->opt_order);
    copy_out(out->dp_F, st.F); copy_out(out->dp_Fl, st.Fl); copy_out(out->dp_G, st.G);
    out->reinsert_ran = st.reinsert_ran ? 1u : 0u;
    out->passes = st.reinsert.passes; out->moves = st.reinsert.moves; out->undone = st.reinsert.undone;
    out->visits = st.visits;
    out->cost_before = st.reinsert.cost_before; out->cost_after = st.reinsert.cost_after;
    out->dp_ran = st.dp_ran ? 1u : 0u;
    out->n_quads = st.n_quads; out->stack_need = st.stack_need;
    if (out->quads) {
      if (st.n_quads > out->quad_capacity) return fail(PBRT_HIP_ERR_LIMIT, "gpu_build_stages: output too small");
      copy_out(out->quads, st.quads);
    }
    return PBRT_HIP_OK;
  });
}

int pbrt_hip_reinsert_links_host(uint32_t n_tris, const uint32_t *child, const float *boxes, const uint32_t *order, uint32_t *par, uint32_t *kid,
                                 float *links_boxes, uint64_t *stats, int32_t *fixed_exp, uint32_t *valid) {
  return guarded([&]() -> int {
    const int rc = check_stage_tree("reinsert_links_host", n_tris, child, boxes, order);
    if (rc) return rc;
    LinkTree lt;
    std::string why;
    if (!link_tree_of_child_words(n_tris, child, boxes, &lt, &why)) return fail(PBRT_HIP_ERR_INVALID, "reinsert_links_host: " + why);
    ReinsertBatchStats st;
    reinsert_batch_links(&lt, ReinsertBatchParams{}, &st);
    copy_out(par, lt.par);
    copy_out(kid, lt.kid);
    if (links_boxes) std::memcpy(links_boxes, lt.bx.data(), lt.bx.size() * sizeof(lt.bx[0]));  // (three 64-bit words = six floats)
    if (stats) {
      const uint64_t s[8] = {st.passes, st.visits, st.found, st.applied, st.max_visits, st.undone, st.fixed_before, st.fixed_after};
      std::memcpy(stats, s, sizeof(s));
    }
    if (fixed_exp) *fixed_exp = st.fixed_exp;
    if (valid) *valid = lt.valid() ? 1u : 0u;
    return PBRT_HIP_OK;
  });
}

int pbrt_hip_collapse_host(uint32_t n_tris, const uint32_t *child, const float *boxes, const uint32_t *order, uint32_t rule, uint32_t *quads,
                           uint32_t cap_nodes, uint32_t *n_quads, uint32_t *stack_need) {
  return guarded([&]() -> int {
    const int rc = check_stage_tree("collapse_host", n_tris, child, boxes, order);
    if (rc) return rc;
    if (!n_quads || !stack_need) return fail(PBRT_HIP_ERR_INVALID, "collapse_host: null argument");
    if (rule != PBRT_HIP_COLLAPSE_GREEDY && rule != PBRT_HIP_COLLAPSE_DP) return fail(PBRT_HIP_ERR_INVALID, "collapse_host: unknown rule");
    QuadNodes q;
    std::string why;
    if (!collapse_child_words(n_tris, child, boxes, rule == PBRT_HIP_COLLAPSE_DP ? kCollapseDp : kCollapseGreedy, &q, &why))
      return fail(PBRT_HIP_ERR_INVALID, "collapse_host: " + why);
    *n_quads = (uint32_t)(q.q.size() / 4);
    *stack_need = q.stack_need;
    if (quads) {
      if (*n_quads > cap_nodes) return fail(PBRT_HIP_ERR_LIMIT, "collapse_host: output too small");
      std::memcpy(quads, q.q.data(), q.q.size() * 16);
    }
    return PBRT_HIP_OK;
  });
}

int pbrt_hip_scene_create(const pbrt_hip_scene_desc *d, int device, pbrt_hip_scene **out) {
  return pbrt_hip_scene_create_ex(d, device, 0u, out);  // the default: built and optimised on the device
}

int pbrt_hip_scene_create_ex(const pbrt_hip_scene_desc *d, int device, uint32_t flags, pbrt_hip_scene **out) {
  if (!d || !out) return fail(PBRT_HIP_ERR_INVALID, "scene_create: null argument");
  *out = nullptr;
  return guarded([&]() -> int {
    Builder builder;
    TextureTable table;
    int rc = check_scene_desc(d, flags, &builder, &table);
    if (rc) return rc;
    int ndev = pbrt_hip_device_count();
    if (ndev <= 0) return fail(PBRT_HIP_ERR_NO_DEVICE, "scene_create: no HIP device (there is no CPU fallback)");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return fail(PBRT_HIP_ERR_INVALID, "scene_create: device index out of range");

    SceneInputs in;  // (declared before the scene: freed after it, on every exit)
    std::unique_ptr<pbrt_hip_scene> s(new pbrt_hip_scene());
    if ((rc = s->open(device))) return rc;
    s->window = {d->xres, d->yres, {d->crop[0], d->crop[1], d->crop[2], d->crop[3]}};
    s->filter = table.filter;
    gather_inputs(*d, table, &in);
    s->n_prims = in.n_prims;
    s->textured = table.textured_tris || table.textured_sph;
    s->glass = !in.mat_extra.empty() || in.has_spot || in.has_mapped || in.has_sphere_light;  // (a spot, a mapped and a sphere light are sampled under PLS, in the GLS instantiations: DESIGN.md 3.22, 3.23, 3.25)
    if ((rc = upload_inputs(s.get(), *d, table, in)) || (rc = build_tree(s.get(), in, builder))) return rc;
    if (table.textured_tris) {  // corner (u, v) into leaf-slot order (whichever builder made d_order)
      HIP_TRY(s->d_tri_uv.alloc(3 * (size_t)in.n_prims));
      HIP_TRY(launch_pack_uv(s->d_tri_uv_in.p, s->d_order.p, in.n_prims, d->n_tris, s->d_tri_uv.p, s->stream));
    }
    if (s->normals) {  // corner normals into leaf-slot order likewise; a sphere's proxy slot gets zeros
      HIP_TRY(s->d_tri_n.alloc(3 * (size_t)in.n_prims));
      HIP_TRY(launch_pack_nrm(s->d_tri_n_in.p, s->d_order.p, in.n_prims, d->n_tris, s->d_tri_n.p, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->d_tri_n_in.release();  // (the gather was its one reader: a scene with normals costs 48 bytes per leaf slot)
    bind_scene_arrays(s.get());
    s->device_bytes = s->bytes();
    set_view(&s->dev, *d);
    *out = s.release();
    return PBRT_HIP_OK;
  });
}

void pbrt_hip_scene_destroy(pbrt_hip_scene *scene) {
  if (!scene) return;
  (void)hipSetDevice(scene->device);
  delete scene;
}

int pbrt_hip_scene_info(const pbrt_hip_scene *s, uint32_t *n_nodes, uint32_t *depth, uint32_t *n_lights,
                        uint64_t *device_bytes) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "scene_info: null scene");
  if (n_nodes) *n_nodes = (uint32_t)s->bvh.nodes.size();
  if (depth) *depth = s->bvh.depth;
  if (n_lights) *n_lights = s->dev.n_lights;
  if (device_bytes) *device_bytes = s->device_bytes;
  return PBRT_HIP_OK;
}

int pbrt_hip_scene_walk_info(const pbrt_hip_scene *s, uint32_t *quad_nodes, uint32_t *stack_need) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "walk_info: null scene");
  if (quad_nodes) *quad_nodes = s->gpu_built ? s->n_quads_gpu : (uint32_t)(s->d_quads.n / 4);
  if (stack_need) *stack_need = s->dev.quad_stack_need;
  return PBRT_HIP_OK;
}

int pbrt_hip_scene_build_info(const pbrt_hip_scene *s, uint32_t *gpu_built, double *build_ms) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "build_info: null scene");
  if (gpu_built) *gpu_built = s->gpu_built ? 1u : 0u;
  if (build_ms) *build_ms = s->build.build_ms;
  return PBRT_HIP_OK;
}

int pbrt_hip_scene_optimize_info(const pbrt_hip_scene *s, uint32_t *passes, uint32_t *moves, double *ms) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "optimize_info: null scene");
  if (passes) *passes = s->build.reinsert.passes;
  if (moves) *moves = s->build.reinsert.moves;
  if (ms) *ms = s->build.reinsert.ms;
  return PBRT_HIP_OK;
}

int pbrt_hip_scene_optimize_cost(const pbrt_hip_scene *s, double *before, double *after, uint32_t *undone) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "optimize_cost: null scene");
  if (before) *before = s->build.reinsert.cost_before;
  if (after) *after = s->build.reinsert.cost_after;
  if (undone) *undone = s->build.reinsert.undone;
  return PBRT_HIP_OK;
}

int pbrt_hip_scene_canonical_info(const pbrt_hip_scene *s, uint32_t *ready, double *build_ms) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "canonical_info: null scene");
  if (ready) *ready = (s->canonical_ready || !s->gpu_built) ? 1u : 0u;
  if (build_ms) *build_ms = s->gpu_built ? s->canonical_build_ms : s->build.build_ms;
  return PBRT_HIP_OK;
}


int pbrt_hip_scene_export_quads(const pbrt_hip_scene *s, uint32_t *quads, uint32_t cap_nodes, uint32_t *n_quads, uint32_t *order) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "export_quads: null scene");
  const uint32_t n = s->gpu_built ? s->n_quads_gpu : (uint32_t)(s->d_quads.n / 4);
  if (n_quads) *n_quads = n;
  HIP_TRY(hipSetDevice(s->device));
  if (quads) {
    if (cap_nodes < n) return fail(PBRT_HIP_ERR_LIMIT, "export_quads: output too small");
    if (n) HIP_TRY(hipMemcpy(quads, s->d_quads.p, 64 * (size_t)n, hipMemcpyDeviceToHost));
  }
  if (order && s->d_order.n) HIP_TRY(hipMemcpy(order, s->d_order.p, 4 * s->d_order.n, hipMemcpyDeviceToHost));
  return PBRT_HIP_OK;
}

int pbrt_hip_scene_export_bvh(const pbrt_hip_scene *s, uint32_t *nodes, uint32_t *order) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "export_bvh: null scene");
  if (nodes && !s->bvh.nodes.empty()) std::memcpy(nodes, s->bvh.nodes.data(), s->bvh.nodes.size() * sizeof(BvhNode));
  if (order && !s->bvh.order.empty()) std::memcpy(order, s->bvh.order.data(), s->bvh.order.size() * 4);
  return PBRT_HIP_OK;
}


int pbrt_hip_scene_tables_host(const pbrt_hip_scene_desc *d, pbrt_hip_scene_tables *out) {
  if (!d || !out) return fail(PBRT_HIP_ERR_INVALID, "scene_tables_host: null argument");
  return guarded([&]() -> int {
    Builder builder;
    TextureTable table;
    const int rc = check_scene_desc(d, 0u, &builder, &table);
    if (rc) return rc;
    SceneInputs in;
    gather_inputs(*d, table, &in);
    // the words of `n` elements of T at src into dst (unless NULL; a 16-bit element widens to a word of its own); *count = the words
    auto words = [](uint32_t *dst, uint32_t *count, const auto *src, size_t n) {
      constexpr size_t per = sizeof(*src) < 4 ? 1 : sizeof(*src) / 4;
      *count = (uint32_t)(n * per);
      if (!dst || !n) return;
      if (sizeof(*src) < 4) for (size_t i = 0; i < n; i++) dst[i] = (uint32_t)((const uint16_t *)src)[i];
      else std::memcpy(dst, src, n * sizeof(*src));
    };
    words(out->P, &out->n_P, in.P, 3 * (size_t)in.n_verts);
    words(out->idx, &out->n_idx, in.idx, 3 * (size_t)in.n_prims);
    words(out->mat, &out->n_mat, in.mat, in.n_prims);
    words(out->lights, &out->n_lights, in.lights.data(), in.lights.size());
    words(out->mats, &out->n_mats, in.mats.data(), in.mats.size());
    words(out->mat_extra, &out->n_mat_extra, in.mat_extra.data(), in.mat_extra.size());
    words(out->spheres, &out->n_spheres, in.spheres.data(), in.spheres.size());
    words(out->textures, &out->n_textures, in.textures.data(), in.textures.size());
    words(out->image_texels, &out->n_image_texels, in.image_texels.data(), in.image_texels.size());
    for (int k = 0; k < 3; k++) { out->le_inf[k] = in.le_inf[k]; out->env_c[k] = in.env_c[k]; }
    for (int k = 0; k < 9; k++) out->env_m[k] = in.env_m[k];
    out->has_inf = in.has_inf; out->env = in.env; out->has_spot = in.has_spot; out->has_mapped = in.has_mapped;
    out->env_w = in.env_w; out->env_h = in.env_h;
    return PBRT_HIP_OK;
  });
}

}  // extern "C"
