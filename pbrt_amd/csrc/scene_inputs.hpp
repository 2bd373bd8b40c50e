// scene_inputs.hpp -- what a checked description puts on the device, assembled on the host (the gather stage of scene creation, between
// check_scene_desc and the upload: capi_scene.cpp).  No HIP call here or in scene_inputs.cpp: pbrt_hip_scene_tables_host runs the stage on a
// machine without a device.  The rows of the light, material and sphere tables are scene_tables.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "../../include/pbrt_hip.h"
#include "envmap.hpp"
#include "scene_tables.hpp"
#include "texture_table.hpp"

namespace pbrt_hip {

// the 1-based texture-table number a light carries as the bits of its `pad`: an environment-map light's map, a spot light's
// cone (3.22), a mapped light's record (3.23)
inline uint32_t light_slot(const pbrt_hip_light &l) { uint32_t u; std::memcpy(&u, &l.pad, 4); return u; }
// the materials that reuse `le` and `kd_tex` for parameters of their own: they do not emit and name no texture
inline bool reuses_le(const pbrt_hip_material &m) { return mat_has_extra(m.type); }

// Spheres are PRIMITIVES OF THE TREE (round 6; until round 5 every ray tested every sphere after the walk).  Every builder here --
// the host's binned SAH, the device builder, the collapse, the lazily built canonical tree -- bounds a primitive by the box of its
// three vertices, so sphere s enters the vertex / index buffers as a degenerate PROXY TRIANGLE (c - r, c + r, c - r): primitive
// n_tris + s, bounded by exactly the sphere's box [c - r, c + r] (fp32 per component: the oracle's sphere_box), centroid its centre.
// Its leaf record is a sphere's (pack_tris_kernel) and the leaf pass runs the sphere test on it (trav_run<..., SPH>).
struct SceneInputs {
  const float *P = nullptr;  // the primitives' vertices, indices and material ids: the caller's arrays, or *_aug with spheres
  const uint32_t *idx = nullptr;
  const uint16_t *mat = nullptr;
  uint32_t n_verts = 0, n_prims = 0;  // primitives: the triangles + the spheres' proxies
  std::vector<float> P_aug;
  std::vector<uint32_t> idx_aug;
  std::vector<uint16_t> mat_aug;
  std::vector<float4> lights, mats, spheres, textures;  // the kernels' records: kLightRows, kMatRows, kSphereRows and 3 per light / material / sphere / texture
  std::vector<float4> mat_extra;  // a row per material, when some material is glass, plastic or substrate (scene_tables.hpp); else empty
  std::vector<float4> image_texels;  // the texel pool of the image textures, when something is textured or a mapped light reads an image (3.23); else empty
  // an environment-map light: its tables, world_to_light and factor
  bool env = false;
  EnvTables env_tables;
  uint32_t env_w = 0, env_h = 0;
  float env_m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, env_c[3] = {0, 0, 0};
  float le_inf[3] = {0.f, 0.f, 0.f};
  bool has_inf = false;
  bool has_spot = false;  // a spot light: the scene needs the GLS instantiations
  bool has_mapped = false;  // a mapped light: likewise, and the texture rows and the texel pool go up for its image
  bool has_sphere_light = false;  // a sphere light: the GLS instantiations likewise
};
// the four parts in their order: primitives and sphere proxies, lights, materials, texture rows.  `d` has passed check_scene_desc, `table` is its table
void gather_inputs(const pbrt_hip_scene_desc &d, const TextureTable &table, SceneInputs *in);

}  // namespace pbrt_hip
