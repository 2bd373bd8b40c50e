// scene_tables.hpp -- THE statement of the small device tables of a scene: `lights`, `mats`, the per-material extra row (`mat_extra`) and
// `spheres`.  What a row holds is said here once, for the host that writes the tables (scene_inputs.cpp) and for the kernels that read them
// (kernel_path.hpp, render_body.inc, kernels_blocks.hip); nothing else under csrc indexes a light's rows or compares a type word with a number.
// Plain C++17 plus the float4 type: it compiles for the device, for the host, and under plain g++ against a few-line <hip/hip_runtime.h>.
//
//   lights    kLightRows x 16 B per light: the explicit lights in the description's order, then every emissive triangle in index order
//     kind (device type word)                row 0        row 1                  row 2               row 3                  row 4
//     point 0, distant 1, infinite 2, env 4  {type, p}    0                      0                   {c, 0}                 0
//     emissive triangle 3                    {3, p0}      {p1, area}             {p2, 0}             {le, 0}                {n, 0}
//     spot 5                                 {5, p}       {axis, cos_total}      {cos_start, 0 0 0}  {I, 0}                 0
//     projection 6, goniometric 7            {type, p}    {M row 0, inv_tan}     {M row 1, sx}       {I, image slot bits}   {M row 2, sy}
//     sphere 8                               {8, centre}  {r, 0 0 0}             0                   {L, 0}                 0
//     (p: position; distant: the unit direction towards the light; infinite / env: ignored.  c: I or L; env: the factor on the texels.
//     area = 0.5 |e1 x e2|, n = (e1 x e2) / |e1 x e2|.  M = world_to_light; image slot: the 0-BASED number of the image's texture slot)
//   mats      kMatRows x 16 B per material: {type, k} {le, kd_tex}; kd_tex = the 1-based texture number of a matte material, else 0; le = 0
//             for glass, plastic and substrate, which reuse the public record's `le` for a parameter and do not emit
//   mat_extra 16 B per material, present when some material is glass, plastic or substrate: glass {Kt, eta}, plastic / substrate {Ks, alpha},
//             every other material's row {0, 0, 0, 1}
//   spheres   kSphereRows x 16 B per sphere: {c, r} {material id, listed, 0 0}; listed = 1 where a sphere light names the
//             sphere -- the MIS hit side weights its emission --, else 0: an unlisted sphere's rows are what they were before 3.25
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/pbrt_hip.h"

namespace pbrt_hip {

constexpr uint32_t kLightRows = 5u, kMatRows = 2u, kSphereRows = 2u;

// ---- the type word of a light's row 0 ----
enum DevLight : uint32_t {
  kDevLightPoint = 0u,
  kDevLightDistant = 1u,
  kDevLightInfinite = 2u,  // constant radiance
  kDevLightTriangle = 3u,  // (3 of the boundary is the environment map: it is 4 here)
  kDevLightEnv = 4u,       // taken by the ENV kernels before sample_light's chain, which never meets it
  kDevLightSpot = 5u,
  kDevLightProjection = 6u,  // the mapped lights, by their record's kind
  kDevLightGonio = 7u,
  kDevLightSphere = 8u,  // a sphere of the scene as an area light
};
// the device word of a light of public type `type` (PBRT_HIP_LIGHT_*, 0 .. 2 unnamed there); map_kind: a mapped light's record's kind
constexpr uint32_t dev_light_type(uint32_t type, uint32_t map_kind = 0u) {
  return type == PBRT_HIP_LIGHT_ENVMAP ? (uint32_t)kDevLightEnv : (type == PBRT_HIP_LIGHT_MAPPED ? kDevLightProjection + map_kind : type);  // (a sphere light keeps its 8)
}
// the types that are taken before sample_light's chain, under PLS, are the table's LARGEST (3 is an emissive triangle, 4 the environment map,
// which no PLS kernel meets): ONE compare finds them, so a scene without them pays what it paid for the spot light's test alone
constexpr bool dev_light_beyond_chain(uint32_t type) { return type >= kDevLightSpot; }
static_assert(dev_light_type(0u) == kDevLightPoint && dev_light_type(1u) == kDevLightDistant && dev_light_type(2u) == kDevLightInfinite, "the first three kinds keep their public number");
static_assert(dev_light_type(PBRT_HIP_LIGHT_ENVMAP) == 4u && PBRT_HIP_LIGHT_ENVMAP == kDevLightTriangle, "the environment map gives its public 3 to the emissive triangle");
static_assert(dev_light_type(PBRT_HIP_LIGHT_SPOT) == kDevLightSpot && kDevLightSpot == 5u, "a spot light keeps its 5");
static_assert(dev_light_type(PBRT_HIP_LIGHT_MAPPED, PBRT_HIP_LIGHT_MAP_PROJECTION) == kDevLightProjection && dev_light_type(PBRT_HIP_LIGHT_MAPPED, PBRT_HIP_LIGHT_MAP_GONIOMETRIC) == kDevLightGonio &&
                  kDevLightProjection == 6u && kDevLightGonio == 7u,
              "a mapped light is 6 + its record's kind");
static_assert(!dev_light_beyond_chain(kDevLightEnv) && dev_light_beyond_chain(kDevLightSpot) && dev_light_beyond_chain(kDevLightProjection) && dev_light_beyond_chain(kDevLightGonio),
              "spot and mapped lights are the table's largest type words");
static_assert(dev_light_type(PBRT_HIP_LIGHT_SPHERE) == kDevLightSphere && kDevLightSphere == 8u && dev_light_beyond_chain(kDevLightSphere), "a sphere light keeps its 8, beyond the chain");
static_assert(dev_light_type(PBRT_HIP_LIGHT_MAPPED, PBRT_HIP_LIGHT_MAP_GONIOMETRIC) < kDevLightSphere, "no mapped light's word reaches the sphere light's");

// ---- the type word of a material's row 0: the public PBRT_HIP_MATERIAL_* value; the predicates the kernels and the host go by ----
constexpr bool mat_is_matte(uint32_t type) { return type == PBRT_HIP_MATERIAL_MATTE; }
constexpr bool mat_is_glass(uint32_t type) { return type == PBRT_HIP_MATERIAL_GLASS; }
constexpr bool mat_is_coated(uint32_t type) { return type - PBRT_HIP_MATERIAL_PLASTIC <= PBRT_HIP_MATERIAL_SUBSTRATE - PBRT_HIP_MATERIAL_PLASTIC; }  // plastic or substrate, by ONE compare
constexpr bool mat_is_substrate(uint32_t type) { return type == PBRT_HIP_MATERIAL_SUBSTRATE; }
// the materials with a row in mat_extra: they reuse the public record's `le` and `kd_tex` for parameters, do not emit and name no texture
constexpr bool mat_has_extra(uint32_t type) { return mat_is_glass(type) || mat_is_coated(type); }
static_assert(PBRT_HIP_MATERIAL_MATTE == 0u && PBRT_HIP_MATERIAL_MIRROR == 1u && PBRT_HIP_MATERIAL_GLASS == 2u, "matte, mirror, glass");
static_assert(PBRT_HIP_MATERIAL_PLASTIC == 3u && PBRT_HIP_MATERIAL_SUBSTRATE == 4u, "plastic and substrate are neighbours: mat_is_coated is one compare");
static_assert(mat_is_coated(3u) && mat_is_coated(4u) && !mat_is_coated(2u) && !mat_is_coated(5u) && !mat_is_coated(0u), "mat_is_coated: types 3 and 4 alone");

// an integer rides in these tables as the bits of a float
constexpr uint32_t table_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
constexpr float table_word(uint32_t u) { return __builtin_bit_cast(float, u); }

// ---- the readers (S: a DevScene, or anything with a `lights` array) ----
// (a REFERENCE: returned by value, the type word's read stops being a one-dword load in the GLS instantiations of render_kernel_x)
template <class Scene>
__host__ __device__ __forceinline__ const float4 &light_row(const Scene &S, uint32_t li, uint32_t k) { return S.lights[kLightRows * li + k]; }
template <class Scene>
__host__ __device__ __forceinline__ uint32_t light_type(const Scene &S, uint32_t li) { return table_bits(light_row(S, li, 0u).x); }

// ---- the host's writers: each appends the kLightRows rows of one light, in the float operations and their order that the films are held to ----
inline float4 table_row(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
// a point, distant, constant infinite or environment-map light
inline void push_light_plain(std::vector<float4> *t, uint32_t dev_type, const float p[3], const float c[3]) {
  t->push_back(table_row(table_word(dev_type), p[0], p[1], p[2]));
  t->push_back(table_row(0, 0, 0, 0));
  t->push_back(table_row(0, 0, 0, 0));
  t->push_back(table_row(c[0], c[1], c[2], 0));
  t->push_back(table_row(0, 0, 0, 0));
}
inline void push_light_spot(std::vector<float4> *t, const float p[3], const float c[3], const pbrt_hip_spot_cone &cone) {
  t->push_back(table_row(table_word(kDevLightSpot), p[0], p[1], p[2]));
  t->push_back(table_row(cone.axis[0], cone.axis[1], cone.axis[2], cone.cos_total));
  t->push_back(table_row(cone.cos_start, 0, 0, 0));
  t->push_back(table_row(c[0], c[1], c[2], 0));
  t->push_back(table_row(0, 0, 0, 0));
}
inline void push_light_mapped(std::vector<float4> *t, const float p[3], const float c[3], const pbrt_hip_light_map &map) {
  const float *m = map.world_to_light;
  t->push_back(table_row(table_word(dev_light_type(PBRT_HIP_LIGHT_MAPPED, map.kind)), p[0], p[1], p[2]));
  t->push_back(table_row(m[0], m[1], m[2], map.inv_tan));
  t->push_back(table_row(m[3], m[4], m[5], map.sx));
  t->push_back(table_row(c[0], c[1], c[2], table_word(map.image - 1u)));
  t->push_back(table_row(m[6], m[7], m[8], map.sy));
}
// a sphere light: the sphere's centre and radius as its row of `spheres` holds them, and the radiance L = the material's le
inline void push_light_sphere(std::vector<float4> *t, const pbrt_hip_sphere &sp, const float L[3]) {
  t->push_back(table_row(table_word(kDevLightSphere), sp.c[0], sp.c[1], sp.c[2]));
  t->push_back(table_row(sp.r, 0, 0, 0));
  t->push_back(table_row(0, 0, 0, 0));
  t->push_back(table_row(L[0], L[1], L[2], 0));
  t->push_back(table_row(0, 0, 0, 0));
}
// an emissive triangle: cr = (p1 - p0) x (p2 - p0), len = |cr|; a triangle of no area gets the NaN normal of 0 / 0
inline void push_light_triangle(std::vector<float4> *t, const float p0[3], const float p1[3], const float p2[3], const float le[3]) {
  const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
  const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
  const float cx = (ay * bz) - (az * by), cy = (az * bx) - (ax * bz), cz = (ax * by) - (ay * bx);
  const float len = std::sqrt((cx * cx + cy * cy) + cz * cz);
  t->push_back(table_row(table_word(kDevLightTriangle), p0[0], p0[1], p0[2]));
  t->push_back(table_row(p1[0], p1[1], p1[2], 0.5f * len));
  t->push_back(table_row(p2[0], p2[1], p2[2], 0));
  t->push_back(table_row(le[0], le[1], le[2], 0));
  t->push_back(table_row(cx / len, cy / len, cz / len, 0));
}

// a material's kMatRows rows, and its row of mat_extra (*extra: empty until the first material that has one; then n_mats rows)
inline void write_material(float4 *rows, std::vector<float4> *extra, uint32_t i, uint32_t n_mats, const pbrt_hip_material &m) {
  rows[0] = table_row(table_word(m.type), m.k[0], m.k[1], m.k[2]);
  if (!mat_has_extra(m.type)) {
    rows[1] = table_row(m.le[0], m.le[1], m.le[2], table_word(mat_is_matte(m.type) ? m.kd_tex : 0u));
    return;
  }
  rows[1] = table_row(0.f, 0.f, 0.f, 0.f);
  if (extra->empty()) extra->assign(n_mats, table_row(0.f, 0.f, 0.f, 1.f));
  (*extra)[i] = table_row(m.le[0], m.le[1], m.le[2], table_word(m.kd_tex));  // (eta of glass, alpha of plastic and substrate: the float whose bits ride in kd_tex)
}
inline void write_sphere(float4 *rows, const pbrt_hip_sphere &sp) {
  rows[0] = table_row(sp.c[0], sp.c[1], sp.c[2], sp.r);
  rows[1] = table_row(table_word(sp.mat), 0, 0, 0);
}
// ... and the mark of a sphere that a sphere light names, read by sphere_listed
inline void mark_sphere_listed(float4 *rows) { rows[1].y = table_word(1u); }
template <class Scene>
__host__ __device__ __forceinline__ bool sphere_listed(const Scene &S, uint32_t si) { return table_bits(S.spheres[kSphereRows * si + 1u].y) != 0u; }

}  // namespace pbrt_hip
