// capi.cpp -- the extern "C" boundary declared in include/pbrt_hip.h: scene flattening + upload,
// kernel launches, film assembly.  Replaces the (empty) body of PbrtAPI::world_end,
// /root/reference/src/core/api.rs:432-473.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <exception>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pbrt_hip.h"
#include "bvh_build.hpp"
#include "capi_internal.hpp"
#include "device_types.h"
#include "envmap.hpp"
#include "host_math.hpp"
#include "quad_nodes.hpp"
#include "scene_parser.hpp"

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

// number of 64x64 super-tiles a rank owns, and the grid of super-tiles
struct Shard {
  int32_t w, h;
  uint32_t stx, sty, total, n_local;
};
// the super-tiles of a rank over the pixel rectangle b (x0 y0 x1 y1): the cropped window, or the sample bounds of a wide filter
Shard make_shard_bounds(const int32_t b[4], uint32_t rank, uint32_t world) {
  Shard s;
  s.w = b[2] - b[0];
  s.h = b[3] - b[1];
  if (s.w < 0) s.w = 0;
  if (s.h < 0) s.h = 0;
  s.stx = (uint32_t)(s.w + 63) / 64;
  s.sty = (uint32_t)(s.h + 63) / 64;
  s.total = s.stx * s.sty;
  s.n_local = (world && rank < world && s.total > rank) ? (s.total - rank + world - 1) / world : 0;
  return s;
}
Shard make_shard(int32_t xres, int32_t yres, const float crop[4], uint32_t rank, uint32_t world) {
  int32_t b[4];
  film_cropped_bounds(xres, yres, crop, b);
  return make_shard_bounds(b, rank, world);
}

// Film geometry of one render: the cropped window (film.rs:92-101), the sample bounds (film.rs:166-175) and whether the
// box filter has the default radius 0.5 -- then a sample lands in its own pixel and the two rectangles coincide -- or
// another one (samples reach pad = ceil(radius - 0.5) pixels beyond the window, fixed-point film).
struct FilmGeom {
  bool wide;
  float rx, ry;
  int32_t pad_x, pad_y;
  int32_t crop[4], sb[4];
  size_t crop_px() const { return (size_t)std::max(0, crop[2] - crop[0]) * (size_t)std::max(0, crop[3] - crop[1]); }
};
inline float filter_radius(float w) { return w == 0.f ? 0.5f : w; }
FilmGeom film_geom(const pbrt_hip_scene_desc &d, const pbrt_hip_render_desc &r) {
  FilmGeom g;
  g.rx = filter_radius(r.filter_xwidth);
  g.ry = filter_radius(r.filter_ywidth);
  g.wide = g.rx != 0.5f || g.ry != 0.5f;
  film_cropped_bounds(d.xres, d.yres, d.crop, g.crop);
  g.pad_x = g.pad_y = 0;
  for (int k = 0; k < 4; k++) g.sb[k] = g.crop[k];
  if (g.wide) {
    g.sb[0] = (int32_t)std::floor(((float)g.crop[0] + 0.5f) - g.rx);
    g.sb[1] = (int32_t)std::floor(((float)g.crop[1] + 0.5f) - g.ry);
    g.sb[2] = (int32_t)std::ceil(((float)g.crop[2] - 0.5f) + g.rx);
    g.sb[3] = (int32_t)std::ceil(((float)g.crop[3] - 0.5f) + g.ry);
    g.pad_x = std::max(0, (int32_t)std::ceil(g.rx - 0.5f));
    g.pad_y = std::max(0, (int32_t)std::ceil(g.ry - 0.5f));
    // an empty crop window has no sample bounds either: nothing is sampled for a film of no pixels (as the oracle: 0 rays)
    if (g.crop[2] <= g.crop[0] || g.crop[3] <= g.crop[1])
      for (int k = 0; k < 4; k++) g.sb[k] = g.crop[k];
  }
  return g;
}

// Scheduling thresholds of the traversal loop (kernel_walk.hpp trav_run).  They change only how lanes
// are interleaved, never a result; PBRT_HIP_MIN_WALKERS / PBRT_HIP_MIN_PARKED override them for
// tuning runs.
uint32_t tuning(const char *name, uint32_t dflt, long cap = 64) {
  const char *v = debug_knob(name);
  if (!v || !*v) return dflt;
  long x = std::strtol(v, nullptr, 10);
  return x < 0 ? 0u : (x > cap ? (uint32_t)cap : (uint32_t)x);
}
// min_walkers: 36 for deep trees (long walks: C3 +1 % over 32), 20 for shallow ones, where a frame is mostly shading and
// the shading stage should wait for more lanes (C4 +12 % over 36)
constexpr uint32_t kMinWalkers = 36, kMinWalkersShallow = 20, kShallowStackNeed = 16, kMinParked = 16;
// persistent one-wave workgroups of the render kernel per CU = what a CU holds at once: render_stack_plan (device_types.h:
// 20 with up to 30 LDS rows -- 5 waves per SIMD by the kernel's 96 VGPRs --, fewer with more rows); the kernel for scenes
// with spheres has the register budget of 3 waves per SIMD.  The grid is this x the device's CU count (hipDeviceProp_t;
// render_launch)
constexpr uint32_t kRenderWavesPerCuSpheres = 12;
// a scene with an environment map: render_kernel_env's register budget is 4 waves per SIMD (kernels_env.hip)
constexpr uint32_t kRenderWavesPerCuEnv = 16;
// the production walk's stack plan under the A-B knobs PBRT_HIP_FORCE_OVERFLOW_VARIANT (the overflow variant for every tree) and
// PBRT_HIP_PREFER_LDS_STACK (the whole stack in LDS whenever it fits kQuadLdsStack rows, whatever the occupancy), read once
RenderStackPlan stack_plan(uint32_t quad_stack_need) {
  static const bool force_overflow = debug_knob("PBRT_HIP_FORCE_OVERFLOW_VARIANT") != nullptr;
  static const bool prefer_lds = debug_knob("PBRT_HIP_PREFER_LDS_STACK") != nullptr;
  return render_stack_plan(quad_stack_need, force_overflow, prefer_lds);
}

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
// of *D.  A host-built scene's tree (build_tree) and a device-built scene's counting walk (ensure_canonical) both come from here;
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
  D->nodes = s->d_nodes.p;
  D->tris = tris->p;
  D->n_nodes = (uint32_t)s->bvh.nodes.size();
  D->root_ref = pairs.root_ref;
  for (int k = 0; k < 3; k++) { D->root_lo[k] = pairs.root_lo[k]; D->root_hi[k] = pairs.root_hi[k]; }
  return PBRT_HIP_OK;
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
  s->dev.nodes = s->d_nodes.p;  // (the pre-canonical allocation was empty and has just been released: no stale pointer is kept)
  s->device_bytes += s->d_nodes.n * 16 + s->d_tris_exact.n * 16 + s->d_order_exact.n * 4;
  s->canonical_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  s->canonical_ready = true;
  return PBRT_HIP_OK;
}

// ---- scene creation in stages (pbrt_hip_scene_create_ex): check_scene_desc, open, gather_inputs, upload_inputs, build_tree, set_view ----

// The accelerator's builder.  ONE default -- the device builder (binned SAH + parallel re-insertion + collapse), whoever asks and
// however (pbrt_hip_scene_create, flags 0, pbrt_hip_render_multi, the command line, bench.py); the host's binned-SAH builder only on
// request (PBRT_HIP_SCENE_HOST_BUILD / _OPTIMIZED_TREE, or PBRT_HIP_BUILDER=host in the environment when the caller left the choice open).
enum class Builder { kHost, kHostOptimized, kGpu, kGpuPlain };

// a material whose Kd is a texture
bool kd_textured(const pbrt_hip_material &m) { return m.kd_tex != 0u && m.type == 0u; }
// the 1-based texture-table number an environment-map light carries as the bits of its `pad`
uint32_t light_env_slot(const pbrt_hip_light &l) { uint32_t u; std::memcpy(&u, &l.pad, 4); return u; }
// a glass material's index of refraction: the float whose bits ride in kd_tex
float glass_eta(const pbrt_hip_material &m) { float e; std::memcpy(&e, &m.kd_tex, 4); return e; }
// glass is an interface between index 1 and eta: eta = 1 (index-matched: nothing reflects, nothing bends) is legal; 16 is four times
// the densest real dielectric and keeps eta^2 and 1 / eta^2 -- the radiance scale of a refraction -- far from fp32's ends
constexpr float kGlassEtaMin = 1.0f, kGlassEtaMax = 16.0f;

// Every refusal that depends on the description alone, before any HIP call, and the builder that `flags` (and PBRT_HIP_BUILDER) ask for.
int check_scene_desc(const pbrt_hip_scene_desc *d, uint32_t flags, Builder *builder) {
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
  // (a NaN in a light's position or in a colour travels into ray directions and throughputs: a ray that is not a number is pruned by
  // nothing and walks the whole tree -- minutes per frame on a large scene -- before its sample is dropped as NaN)
  if (d->n_lights && !d->lights) return fail(PBRT_HIP_ERR_INVALID, "scene_create: n_lights > 0 but no light table");
  for (uint32_t i = 0; i < d->n_lights; i++)
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(d->lights[i].p[k]) || !std::isfinite(d->lights[i].c[k]))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: light " + std::to_string(i) + ": position / direction / colour is not finite");
  for (uint32_t i = 0; i < d->n_mats; i++)
    for (int k = 0; k < 3; k++)
      if (d->mats[i].type != PBRT_HIP_MATERIAL_GLASS && (!std::isfinite(d->mats[i].k[k]) || !std::isfinite(d->mats[i].le[k])))
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
  for (int k = 0; k < 16; k++)
    if (!std::isfinite(d->cam_to_world[k])) return fail(PBRT_HIP_ERR_INVALID, "scene_create: camera matrix is not finite");
  if (!(d->fov > 0.f && d->fov < 180.f)) return fail(PBRT_HIP_ERR_INVALID, "scene_create: fov must lie in (0, 180) degrees");
  for (int k = 0; k < 4; k++)  // Film "cropwindow": fractions of the film (film.rs:92-101 multiplies and rounds them up: a NaN or 1e30 there is an int overflow)
    if (!(d->crop[k] >= 0.f && d->crop[k] <= 1.f)) return fail(PBRT_HIP_ERR_INVALID, "scene_create: crop window values must lie in [0, 1]");
  for (uint32_t s = 0; s < d->n_spheres; s++)
    if (d->spheres[s].mat >= d->n_mats) return fail(PBRT_HIP_ERR_INVALID, "scene_create: sphere material id out of range");
  if (d->n_textures && !d->textures) return fail(PBRT_HIP_ERR_INVALID, "scene_create: n_textures > 0 but no texture table");
  for (uint32_t i = 0; i < d->n_mats; i++) {
    if (d->mats[i].type == PBRT_HIP_MATERIAL_GLASS) continue;  // (kd_tex holds eta)
    if (d->mats[i].kd_tex > d->n_textures) return fail(PBRT_HIP_ERR_INVALID, "scene_create: material texture number out of range");
    if (d->mats[i].kd_tex && !d->textures) return fail(PBRT_HIP_ERR_INVALID, "scene_create: textured material but no texture table");
  }
  for (uint32_t i = 0; i < d->n_mats; i++)  // (image textures for Kd do not exist: a type-1 slot is a light's map)
    if (kd_textured(d->mats[i]) && is_envmap_slot(d->textures, d->mats[i].kd_tex - 1u))
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: material " + std::to_string(i) + ": kd_tex names an environment map, which is not a texture for Kd");
  for (uint32_t i = 0; i < d->n_textures; i++) {
    const pbrt_hip_texture &tx = d->textures[i];
    if (is_envmap_slot(d->textures, i)) {  // an environment map's record
      const int rc = envmap_check(envmap_slot(d->textures, i), "scene_create: texture slot " + std::to_string(i + 1) + ": ");
      if (rc) return rc;
      continue;
    }
    if (tx.type != 0u) return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown texture type");
    if (!std::isfinite(tx.su) || !std::isfinite(tx.sv) || !std::isfinite(tx.du) || !std::isfinite(tx.dv))
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: texture mapping is not finite");
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(tx.tex1[k]) || !std::isfinite(tx.tex2[k])) return fail(PBRT_HIP_ERR_INVALID, "scene_create: texture colour is not finite");
  }
  bool textured = false;  // a triangle whose material's Kd is a texture: its corner (u, v) must be there
  for (uint32_t t = 0; t < d->n_tris && !textured; t++) textured = kd_textured(d->mats[d->mat_id[t]]);
  if (textured) {
    if (!d->tri_uv) return fail(PBRT_HIP_ERR_INVALID, "scene_create: a triangle's material is textured but tri_uv is NULL");
    for (size_t i = 0; i < 6 * (size_t)d->n_tris; i++)
      if (!std::isfinite(d->tri_uv[i])) return fail(PBRT_HIP_ERR_INVALID, "scene_create: tri_uv is not finite");
  }
  if (flags & ~(PBRT_HIP_SCENE_GPU_BUILD | PBRT_HIP_SCENE_OPTIMIZED_TREE | PBRT_HIP_SCENE_PLAIN_TREE | PBRT_HIP_SCENE_HOST_BUILD))
    return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown flag");
  const bool want_host = (flags & (PBRT_HIP_SCENE_HOST_BUILD | PBRT_HIP_SCENE_OPTIMIZED_TREE)) != 0u;
  const bool want_gpu = (flags & (PBRT_HIP_SCENE_GPU_BUILD | PBRT_HIP_SCENE_PLAIN_TREE)) != 0u;
  if (want_host && want_gpu)
    return fail(PBRT_HIP_ERR_INVALID, "scene_create: PBRT_HIP_SCENE_HOST_BUILD / _OPTIMIZED_TREE are host builds, not combined with PBRT_HIP_SCENE_GPU_BUILD / _PLAIN_TREE");
  for (uint32_t s = 0; s < d->n_spheres; s++)  // (a finite centre and radius can still make an infinite box)
    for (int k = 0; k < 3; k++)
      if (!std::isfinite(d->spheres[s].c[k] - d->spheres[s].r) || !std::isfinite(d->spheres[s].c[k] + d->spheres[s].r))
        return fail(PBRT_HIP_ERR_INVALID, "scene_create: a sphere's bounding box is not finite");
  for (uint32_t i = 0; i < d->n_lights; i++)
    if (d->lights[i].type > PBRT_HIP_LIGHT_ENVMAP) return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown light type");
  uint32_t n_env = 0;
  for (uint32_t i = 0; i < d->n_lights; i++) {  // an environment-map light names a type-1 slot of the texture table; one per scene
    if (d->lights[i].type != PBRT_HIP_LIGHT_ENVMAP) continue;
    const uint32_t t = light_env_slot(d->lights[i]);
    if (t == 0u || t > d->n_textures || !d->textures || !is_envmap_slot(d->textures, t - 1u))
      return fail(PBRT_HIP_ERR_INVALID, "scene_create: light " + std::to_string(i) + ": an environment-map light (type 3) must name a type-1 slot of the texture table in `pad`");
    if (++n_env > 1u) return fail(PBRT_HIP_ERR_LIMIT, "scene_create: more than one environment-map light (type 3)");
  }
  for (uint32_t i = 0; i < d->n_mats; i++)
    if (d->mats[i].type > PBRT_HIP_MATERIAL_GLASS) return fail(PBRT_HIP_ERR_INVALID, "scene_create: unknown material type");
  const char *env = want_host || want_gpu ? nullptr : std::getenv("PBRT_HIP_BUILDER");
  if (flags & PBRT_HIP_SCENE_OPTIMIZED_TREE) *builder = Builder::kHostOptimized;
  else if ((flags & PBRT_HIP_SCENE_HOST_BUILD) || (env && std::strcmp(env, "host") == 0)) *builder = Builder::kHost;
  else *builder = (flags & PBRT_HIP_SCENE_PLAIN_TREE) ? Builder::kGpuPlain : Builder::kGpu;  // (PBRT_HIP_SCENE_PLAIN_TREE alone qualifies the default)
  return PBRT_HIP_OK;
}

// What a checked description puts on the device, assembled on the host.
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
  std::vector<float4> lights, mats, spheres, textures;  // the kernels' records: 5, 2, 2 and 3 per light / material / sphere / texture
  std::vector<float4> glass;  // {Kt, eta} per material, when the scene has a glass one; else empty
  // an environment-map light: its tables, world_to_light and factor
  bool env = false;
  EnvTables env_tables;
  uint32_t env_w = 0, env_h = 0;
  float env_m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, env_c[3] = {0, 0, 0};
  float le_inf[3] = {0.f, 0.f, 0.f};
  bool has_inf = false;
  bool textured_tris = false;  // a triangle whose material's Kd is a texture: its corner (u, v) go up too
  bool textured_sph = false;   // a sphere whose material's Kd is one: (u, v) from its own parametrisation (kernel_math.hpp sphere_uv)
};
void gather_inputs(const pbrt_hip_scene_desc &d, SceneInputs *in) {
  auto as_f = [](uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; };
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
  // light table: explicit lights, then every emissive triangle in index order
  for (uint32_t i = 0; i < d.n_lights; i++) {
    const pbrt_hip_light &l = d.lights[i];
    // (type 3 of the boundary, the environment map, is 4 in this table: 3 is an emissive triangle here -- kernel_path.hpp kDevLightEnv)
    in->lights.push_back(make_float4(as_f(l.type == PBRT_HIP_LIGHT_ENVMAP ? 4u : l.type), l.p[0], l.p[1], l.p[2]));
    in->lights.push_back(make_float4(0, 0, 0, 0));
    in->lights.push_back(make_float4(0, 0, 0, 0));
    in->lights.push_back(make_float4(l.c[0], l.c[1], l.c[2], 0));
    in->lights.push_back(make_float4(0, 0, 0, 0));
    if (l.type == 2) {
      for (int k = 0; k < 3; k++) in->le_inf[k] = in->le_inf[k] + l.c[k];
      in->has_inf = true;
    }
    if (l.type == PBRT_HIP_LIGHT_ENVMAP) {
      const pbrt_hip_envmap e = envmap_slot(d.textures, light_env_slot(l) - 1u);
      in->env = true;
      in->env_w = e.width; in->env_h = e.height;
      for (int k = 0; k < 9; k++) in->env_m[k] = e.world_to_light[k];
      for (int k = 0; k < 3; k++) in->env_c[k] = l.c[k];
      envmap_build_tables(e.rgb, e.width, e.height, &in->env_tables);
    }
  }
  for (uint32_t t = 0; t < d.n_tris; t++) {
    const pbrt_hip_material &m = d.mats[d.mat_id[t]];
    if (m.type == PBRT_HIP_MATERIAL_GLASS) continue;  // (its le is Kt: glass does not emit)
    if (!(m.le[0] > 0.f || m.le[1] > 0.f || m.le[2] > 0.f)) continue;
    F3 p[3];
    for (int v = 0; v < 3; v++) {
      const float *q = d.P + 3 * (size_t)d.idx[3 * (size_t)t + v];
      p[v] = {q[0], q[1], q[2]};
    }
    F3 cr = cross3(sub(p[1], p[0]), sub(p[2], p[0]));
    float len = std::sqrt(dot3(cr, cr));
    in->lights.push_back(make_float4(as_f(3u), p[0].x, p[0].y, p[0].z));
    in->lights.push_back(make_float4(p[1].x, p[1].y, p[1].z, 0.5f * len));
    in->lights.push_back(make_float4(p[2].x, p[2].y, p[2].z, 0));
    in->lights.push_back(make_float4(m.le[0], m.le[1], m.le[2], 0));
    in->lights.push_back(make_float4(cr.x / len, cr.y / len, cr.z / len, 0));
  }
  in->mats.resize(2 * (size_t)d.n_mats);
  for (uint32_t i = 0; i < d.n_mats; i++) {
    const pbrt_hip_material &m = d.mats[i];
    in->mats[2 * i] = make_float4(as_f(m.type), m.k[0], m.k[1], m.k[2]);
    in->mats[2 * i + 1] = make_float4(m.le[0], m.le[1], m.le[2], as_f(m.type == 0u ? m.kd_tex : 0u));
    if (m.type == PBRT_HIP_MATERIAL_GLASS) {  // no emission on the device; {Kt, eta} in the table of the GLS instantiations
      in->mats[2 * i + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in->glass.empty()) in->glass.assign(d.n_mats, make_float4(0.f, 0.f, 0.f, 1.f));
      in->glass[i] = make_float4(m.le[0], m.le[1], m.le[2], glass_eta(m));
    }
  }
  in->spheres.resize(2 * (size_t)d.n_spheres);
  for (uint32_t i = 0; i < d.n_spheres; i++) {
    const pbrt_hip_sphere &sp = d.spheres[i];
    in->spheres[2 * i] = make_float4(sp.c[0], sp.c[1], sp.c[2], sp.r);
    in->spheres[2 * i + 1] = make_float4(as_f(sp.mat), 0, 0, 0);
    in->textured_sph = in->textured_sph || kd_textured(d.mats[sp.mat]);
  }
  for (uint32_t t = 0; t < d.n_tris && !in->textured_tris; t++) in->textured_tris = kd_textured(d.mats[d.mat_id[t]]);
  if (in->textured_tris || in->textured_sph) {  // (the texture table goes up only when something is textured)
    in->textures.resize(3 * (size_t)d.n_textures);
    for (uint32_t i = 0; i < d.n_textures; i++) {
      const pbrt_hip_texture &tx = d.textures[i];
      if (is_envmap_slot(d.textures, i)) continue;  // (an environment map's slot: no material names it, its records stay zero)
      in->textures[3 * i] = make_float4(as_f(tx.type), tx.tex1[0], tx.tex1[1], tx.tex1[2]);
      in->textures[3 * i + 1] = make_float4(tx.tex2[0], tx.tex2[1], tx.tex2[2], tx.su);
      in->textures[3 * i + 2] = make_float4(tx.sv, tx.du, tx.dv, 0.f);
    }
  }
}

// The inputs into the scene's arrays (asynchronously: `in` outlives the stream's synchronisation) and the fields of s->dev they make
int upload_inputs(pbrt_hip_scene *s, const pbrt_hip_scene_desc &d, const SceneInputs &in) {
  HIP_TRY(upload(&s->d_P, in.P, 3 * (size_t)in.n_verts, s->stream));
  HIP_TRY(upload(&s->d_idx, in.idx, 3 * (size_t)in.n_prims, s->stream));
  HIP_TRY(upload(&s->d_mat_id, in.mat, in.n_prims, s->stream));
  HIP_TRY(upload(&s->d_mats, in.mats.data(), in.mats.size(), s->stream));
  HIP_TRY(upload(&s->d_lights, in.lights.data(), in.lights.size(), s->stream));
  HIP_TRY(upload(&s->d_spheres, in.spheres.data(), in.spheres.size(), s->stream));
  HIP_TRY(upload(&s->d_textures, in.textures.data(), in.textures.size(), s->stream));
  HIP_TRY(upload(&s->d_glass, in.glass.data(), in.glass.size(), s->stream));
  if (in.env) {
    HIP_TRY(upload(&s->d_env_texels, in.env_tables.texels.data(), in.env_tables.texels.size(), s->stream));
    HIP_TRY(upload(&s->d_env_marginal, in.env_tables.marginal.data(), in.env_tables.marginal.size(), s->stream));
    HIP_TRY(upload(&s->d_env_conditional, in.env_tables.conditional.data(), in.env_tables.conditional.size(), s->stream));
    s->env = true;
    s->env_w = in.env_w; s->env_h = in.env_h;
    for (int k = 0; k < 9; k++) s->env_m[k] = in.env_m[k];
    for (int k = 0; k < 3; k++) s->env_c[k] = in.env_c[k];
  }
  if (in.textured_tris) HIP_TRY(upload(&s->d_tri_uv_in, d.tri_uv, 6 * (size_t)d.n_tris, s->stream));
  DevScene &D = s->dev;
  D.mats = s->d_mats.p;
  D.lights = s->d_lights.p;
  D.spheres = s->d_spheres.p;
  D.n_tris = d.n_tris;  // (the triangles: a hit's primitive id >= this is sphere id - n_tris)
  D.n_spheres = d.n_spheres;
  D.n_lights = (uint32_t)(in.lights.size() / 5);
  D.n_lights_f = (float)D.n_lights;
  for (int k = 0; k < 3; k++) D.le_inf[k] = in.le_inf[k];
  D.has_inf = in.has_inf ? 1u : 0u;
  return PBRT_HIP_OK;
}

// The tree over the uploaded primitives, on the host or on the device: d_nodes, d_quads and d_order, the triangle records packed in
// leaf order into d_tris, s->build, and the tree's fields of s->dev (nodes, quads, root ref and box, n_nodes, the walk's stack need).
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
    s->build = {gb.build_ms, gb.reinsert_passes, gb.reinsert_moves, gb.reinsert_ms, gb.reinsert_cost_before, gb.reinsert_cost_after, gb.reinsert_undone};
    s->n_quads_gpu = gb.n_quads;
    D.tris = s->d_tris.p;
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
  D.quads = s->d_quads.p;
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
const char *pbrt_hip_version(void) { return "pbrt_hip 0.7 (gfx950; struct sizes of 0.6)"; }
#ifndef PBRT_HIP_BUILD_ID
#define PBRT_HIP_BUILD_ID "unknown"
#endif
const char *pbrt_hip_build_id(void) { return PBRT_HIP_BUILD_ID; }

int pbrt_hip_bvh_build_host(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, uint32_t *nodes,
                            uint32_t *order, uint32_t *n_nodes, uint32_t *depth) {
  try {
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
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

int pbrt_hip_quad_build_host(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, int split_leaves,
                             uint32_t *quads, uint32_t cap_nodes, uint32_t *n_quads, uint32_t *stack_need) {
  return pbrt_hip_quad_build_host_ex(P, n_verts, idx, n_tris, split_leaves, PBRT_HIP_TREE_DEFAULT, quads, cap_nodes, n_quads, stack_need,
                                     nullptr, nullptr, nullptr, nullptr);
}

int pbrt_hip_quad_build_host_ex(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, int split_leaves, uint32_t tree,
                                uint32_t *quads, uint32_t cap_nodes, uint32_t *n_quads, uint32_t *stack_need, uint32_t *order,
                                float *root_box, uint32_t *n_refs, float *exact_boxes) {
  try {
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
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

int pbrt_hip_scene_create(const pbrt_hip_scene_desc *d, int device, pbrt_hip_scene **out) {
  return pbrt_hip_scene_create_ex(d, device, 0u, out);  // the default: built and optimised on the device
}

int pbrt_hip_scene_create_ex(const pbrt_hip_scene_desc *d, int device, uint32_t flags, pbrt_hip_scene **out) {
  if (!d || !out) return fail(PBRT_HIP_ERR_INVALID, "scene_create: null argument");
  *out = nullptr;
  try {
    Builder builder;
    int rc = check_scene_desc(d, flags, &builder);
    if (rc) return rc;
    int ndev = pbrt_hip_device_count();
    if (ndev <= 0) return fail(PBRT_HIP_ERR_NO_DEVICE, "scene_create: no HIP device (there is no CPU fallback)");
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= ndev) return fail(PBRT_HIP_ERR_INVALID, "scene_create: device index out of range");

    SceneInputs in;  // (declared before the scene: freed after it, on every exit)
    std::unique_ptr<pbrt_hip_scene> s(new pbrt_hip_scene());
    if ((rc = s->open(device))) return rc;
    s->desc = *d;
    s->desc.P = nullptr; s->desc.idx = nullptr; s->desc.mat_id = nullptr;
    s->desc.mats = nullptr; s->desc.lights = nullptr; s->desc.spheres = nullptr;
    s->desc.tri_uv = nullptr; s->desc.textures = nullptr;
    gather_inputs(*d, &in);
    s->n_prims = in.n_prims;
    s->textured = in.textured_tris || in.textured_sph;
    s->glass = !in.glass.empty();
    if ((rc = upload_inputs(s.get(), *d, in)) || (rc = build_tree(s.get(), in, builder))) return rc;
    if (in.textured_tris) {  // corner (u, v) into leaf-slot order (whichever builder made d_order)
      HIP_TRY(s->d_tri_uv.alloc(3 * (size_t)in.n_prims));
      HIP_TRY(launch_pack_uv(s->d_tri_uv_in.p, s->d_order.p, in.n_prims, d->n_tris, s->d_tri_uv.p, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->device_bytes = s->d_env_texels.n * 16 + s->d_env_marginal.n * 4 + s->d_env_conditional.n * 4 + s->d_glass.n * 16 + s->d_tri_uv_in.n * 4 + s->d_tri_uv.n * 8 + s->d_textures.n * 16 + s->d_P.n * 4 + s->d_idx.n * 4 + s->d_mat_id.n * 2 + s->d_order.n * 4 + s->d_nodes.n * 16 + s->d_quads.n * 16 +
                      s->d_tris.n * 16 + s->d_mats.n * 16 + s->d_lights.n * 16 + s->d_spheres.n * 16;
    set_view(&s->dev, *d);
    *out = s.release();
    return PBRT_HIP_OK;
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
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
  if (passes) *passes = s->build.reinsert_passes;
  if (moves) *moves = s->build.reinsert_moves;
  if (ms) *ms = s->build.reinsert_ms;
  return PBRT_HIP_OK;
}

int pbrt_hip_scene_optimize_cost(const pbrt_hip_scene *s, double *before, double *after, uint32_t *undone) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "optimize_cost: null scene");
  if (before) *before = s->build.reinsert_cost_before;
  if (after) *after = s->build.reinsert_cost_after;
  if (undone) *undone = s->build.reinsert_undone;
  return PBRT_HIP_OK;
}

int pbrt_hip_scene_canonical_info(const pbrt_hip_scene *s, uint32_t *ready, double *build_ms) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "canonical_info: null scene");
  if (ready) *ready = (s->canonical_ready || !s->gpu_built) ? 1u : 0u;
  if (build_ms) *build_ms = s->gpu_built ? s->canonical_build_ms : s->build.build_ms;
  return PBRT_HIP_OK;
}

int pbrt_hip_render_stack_plan(uint32_t stack_need, uint32_t *lds_rows, uint32_t *waves_per_cu, uint32_t *overflow_entries) {
  const RenderStackPlan p = stack_plan(stack_need);
  if (lds_rows) *lds_rows = p.rows;
  if (waves_per_cu) *waves_per_cu = p.waves_per_cu;
  if (overflow_entries) *overflow_entries = p.extra_entries;
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

static int check_render_desc(const pbrt_hip_scene *s, const pbrt_hip_render_desc *r) {
  if (!s || !r) return fail(PBRT_HIP_ERR_INVALID, "render: null argument");
  if (r->spp_x == 0 || r->spp_y == 0) return fail(PBRT_HIP_ERR_INVALID, "render: spp_x and spp_y must be >= 1");
  if (r->world_size == 0 || r->rank >= r->world_size) return fail(PBRT_HIP_ERR_INVALID, "render: rank must be < world_size");
  if (r->integrator > PBRT_HIP_INTEGRATOR_PATH_MIS) return fail(PBRT_HIP_ERR_INVALID, "render: unknown integrator");
  if (r->sampler > PBRT_HIP_SAMPLER_HALTON) return fail(PBRT_HIP_ERR_INVALID, "render: unknown sampler");
  // (samplers 2 and 3 -- Sobol' proper and Halton -- share one instantiation of the kernel: "the table samplers")
  const bool table_sampler = r->sampler == PBRT_HIP_SAMPLER_SOBOL_ND || r->sampler == PBRT_HIP_SAMPLER_HALTON;
  if (table_sampler && (r->flags & (PBRT_HIP_FLAG_COUNTERS | PBRT_HIP_FLAG_WALK_COUNTERS)))
    return fail(PBRT_HIP_ERR_INVALID, "render: the counter flags are not available with the Sobol' / Halton samplers (samplers 2, 3)");
  // the kernels pack the sample index into 20 bits and the bounce count into 10 (kernel_path.hpp path_store): beyond that a
  // persistent wave would never see its pixel finish
  if ((uint64_t)r->spp_x * (uint64_t)r->spp_y > PBRT_HIP_MAX_SPP)
    return fail(PBRT_HIP_ERR_LIMIT, "render: more than 2^20 samples per pixel");
  if (r->max_depth > PBRT_HIP_MAX_DEPTH) return fail(PBRT_HIP_ERR_LIMIT, "render: maxdepth above 1023");
  // box filter radii, box.rs:57-61 (0 = the default 0.5): any positive radius up to 16 pixels
  const float fx = filter_radius(r->filter_xwidth), fy = filter_radius(r->filter_ywidth);
  if (!(fx > 0.f) || !(fy > 0.f) || !std::isfinite(fx) || !std::isfinite(fy)) return fail(PBRT_HIP_ERR_INVALID, "render: the filter radii must be positive");
  if (fx > 16.f || fy > 16.f) return fail(PBRT_HIP_ERR_LIMIT, "render: filter radius above 16 pixels");
  if ((fx != 0.5f || fy != 0.5f) && (r->flags & (PBRT_HIP_FLAG_COUNTERS | PBRT_HIP_FLAG_WALK_COUNTERS)))
    return fail(PBRT_HIP_ERR_INVALID, "render: the counter flags need the default box filter (radius 0.5)");
  // an environment map: render_kernel_env exists without counters and for the default box filter (kernels_env.hip).
  // Asked first, so that a scene with a map is told of the map whatever else it holds (glass, textures)
  if (s->env && (r->flags & (PBRT_HIP_FLAG_COUNTERS | PBRT_HIP_FLAG_WALK_COUNTERS)))
    return fail(PBRT_HIP_ERR_LIMIT, "render: the counter flags are not available for a scene with an environment map");
  // (textures, the MIS integrator, the table samplers and a wide box filter combine freely -- render_kernel_x --; only the counting
  // instantiations exist for the default path alone)
  if ((s->textured || r->integrator == PBRT_HIP_INTEGRATOR_PATH_MIS) && (r->flags & (PBRT_HIP_FLAG_COUNTERS | PBRT_HIP_FLAG_WALK_COUNTERS)))
    return fail(PBRT_HIP_ERR_LIMIT, "render: the counter flags are not available for textured materials / the MIS integrator");
  if (s->glass && (r->flags & (PBRT_HIP_FLAG_COUNTERS | PBRT_HIP_FLAG_WALK_COUNTERS)))
    return fail(PBRT_HIP_ERR_LIMIT, "render: the counter flags are not available for a scene with a glass material");
  if (s->env && (fx != 0.5f || fy != 0.5f))
    return fail(PBRT_HIP_ERR_LIMIT, "render: an environment map with a box filter radius other than 0.5 is a combination the library does not build");
  if (!(r->max_sample_luminance >= 0.f)) return fail(PBRT_HIP_ERR_INVALID, "render: max_sample_luminance must be >= 0 (0 = none)");
  if (fx != 0.5f || fy != 0.5f) {
    // the fixed-point film: a sample adds at most 2^39 units to a pixel's int64 accumulator, and a pixel receives
    // at most spp x footprint samples (from every rank together: the N-rank reduce adds the same samples) -- 2^24 of them fit
    const uint64_t foot = (uint64_t)(2 * (int)std::ceil(fx) + 1) * (uint64_t)(2 * (int)std::ceil(fy) + 1);
    if ((uint64_t)r->spp_x * (uint64_t)r->spp_y * foot > (1ull << 24))
      return fail(PBRT_HIP_ERR_LIMIT, "render: samples per pixel x filter footprint above 2^24 (the fixed-point film's accumulators could wrap)");
  }
  return PBRT_HIP_OK;
}

namespace {
// The partial film sums cost 16 K bytes per pixel of the rank's share (one float4 per item, K <= 16 chunks per pixel): 1.07 GB for C3, 4.3 GB
// for C4's 4096^2 on one GPU, and growing with the resolution.  A frame whose sums would pass the cap (2 GiB; PBRT_HIP_PARTIALS_CAP_KB for the
// tests) is rendered in P passes over the same buffer: pass p takes the rank's super-tiles j = p + P * j', which is exactly the share of rank
// `rank + world * p` of `world * P` ranks -- so the render kernel runs unchanged -- and the merge puts tile j' of the pass at tile j of the
// rank's slab.  Every pixel keeps its samples, chunks and order of additions: the film is the one-pass film bit for bit.  Passes also keep
// the item numbers of a launch inside 32 bits.
uint32_t partials_passes(uint32_t n_local, uint32_t n_chunks) {
  if (n_local == 0) return 1;
  const uint64_t cap_bytes = (uint64_t)std::max<uint32_t>(1u, tuning("PBRT_HIP_PARTIALS_CAP_KB", 2u << 20, 1l << 30)) << 10;
  const uint64_t per_tile = 4096ull * n_chunks * 16ull;
  uint64_t tiles = std::max<uint64_t>(1, cap_bytes / per_tile);
  tiles = std::min<uint64_t>(tiles, ((1ull << 32) - 1) / (4096ull * n_chunks));
  return (uint32_t)((n_local + tiles - 1) / tiles);
}
// How one render of `s` is launched (RenderLaunch, device_types.h), decided here and nowhere else: the instantiation's switches, the
// walk's stack, the grid, the passes and the scheduling thresholds.  The exact walk's rows follow the canonical tree, which a
// device-built scene gets here on first use.
int render_launch(pbrt_hip_scene *s, const pbrt_hip_render_desc *r, const FilmGeom &fg, const Shard &sh, RenderLaunch *out) {
  RenderLaunch L{};
  L.spheres = s->dev.n_spheres > 0;
  L.counters = (r->flags & PBRT_HIP_FLAG_COUNTERS) ? kCountExact : ((r->flags & PBRT_HIP_FLAG_WALK_COUNTERS) ? kCountWalk : kCountNone);
  L.wide = fg.wide;
  L.table_sampler = r->sampler == PBRT_HIP_SAMPLER_SOBOL_ND || r->sampler == PBRT_HIP_SAMPLER_HALTON;
  L.mis = r->integrator == PBRT_HIP_INTEGRATOR_PATH_MIS;
  L.textured = s->textured;
  L.glass = s->glass;
  L.env = s->env;
  const bool shallow = s->dev.quad_stack_need <= kShallowStackNeed;
  L.plan = stack_plan(s->dev.quad_stack_need);
  L.lds_bytes = L.plan.rows * 256u;
  const bool default_path = L.counters == kCountNone && !L.wide && !L.table_sampler && !L.mis && !L.textured && !L.glass && !L.env;
  L.steps = default_path && !L.plan.overflow && shallow ? 2u : PBRT_STEPS_PER_CHECK;
  if (L.counters == kCountExact) {
    const int ce = ensure_canonical(s);
    if (ce) return ce;
    // the exact walk holds at most depth - 1 entries (refs + entry distances): the smallest of the instantiated row counts that fits
    const uint32_t held = s->bvh.depth > 0 ? s->bvh.depth - 1 : 0;
    L.exact_rows = held > 40 ? 64 : held > 32 ? 40 : held > 26 ? 32 : held > 20 ? 26 : 20;
    L.lds_bytes = L.exact_rows * 512u;
  }
  // (the instantiations for another filter radius and for the table samplers fit the 96 VGPRs of 5 waves per SIMD like the default one)
  L.waves_per_cu = (L.spheres || L.glass) ? std::min(kRenderWavesPerCuSpheres, L.plan.waves_per_cu) : L.plan.waves_per_cu;  // (glass: the spheres' budget, kernels_x.hip)
  if (L.env) L.waves_per_cu = std::min(kRenderWavesPerCuEnv, L.plan.waves_per_cu);  // (whatever else the scene holds: render_kernel_env's own budget)
  L.chunk_shift = sample_chunk_shift(r->spp_x * r->spp_y);
  const uint32_t n_chunks = 1u << L.chunk_shift;  // K: DESIGN.md 3.1
  L.passes = fg.wide ? 1u : partials_passes(sh.n_local, n_chunks);
  L.pass_tiles = (sh.n_local + L.passes - 1) / L.passes;  // of pass 0, the largest
  if ((uint64_t)L.pass_tiles * 4096u * n_chunks >= (1ull << 32)) return fail(PBRT_HIP_ERR_LIMIT, "render: film too large for 32-bit item numbers");
  if ((uint64_t)r->world_size * L.passes >= (1ull << 32)) return fail(PBRT_HIP_ERR_LIMIT, "render: world_size x passes does not fit 32 bits");
  L.n_workgroups = std::min<uint32_t>(L.pass_tiles * 64u * n_chunks, std::max<uint32_t>(1u, tuning("PBRT_HIP_RENDER_WORKGROUPS", s->n_cu * L.waves_per_cu, 1 << 20)));
  L.min_walkers = tuning("PBRT_HIP_MIN_WALKERS", shallow ? kMinWalkersShallow : kMinWalkers);
  L.min_parked = tuning("PBRT_HIP_MIN_PARKED", kMinParked);
  *out = L;
  return PBRT_HIP_OK;
}
// The scratch launch L needs beyond the caller's slab, (re)allocated here when what the scene holds is too small: the lanes' path-state
// records, the partial film sums of the work items, the overflow area of the walk's stack, the generator matrices of sampler 2 and the
// table of sampler 3.  pbrt_hip_render_device calls it; a host that is about to launch on several GPUs calls it for every GPU FIRST
// (pbrt_hip_render_prepare), so that no hipMalloc -- a synchronising call -- sits between the launches of a frame.
int ensure_render_scratch(pbrt_hip_scene *s, const pbrt_hip_render_desc *r, const RenderLaunch &L) {
  if (r->sampler == PBRT_HIP_SAMPLER_SOBOL_ND && s->d_sobol.n == 0) {
    static_assert(kSobolNdDims == 2 * (int)kSobolNdRequests, "sampler 2: two dimensions per request");
    std::vector<uint32_t> mat((size_t)kSobolNdDims * 32);
    sobol_nd_matrices(mat.data());
    HIP_TRY(s->d_sobol.alloc(mat.size()));
    HIP_TRY(hipMemcpy(s->d_sobol.p, mat.data(), mat.size() * 4, hipMemcpyHostToDevice));
  }
  if (r->sampler == PBRT_HIP_SAMPLER_HALTON && s->d_halton.n == 0) {
    static_assert(kHaltonDims == 2 * (int)kSobolNdRequests, "sampler 3: two dimensions per request, as many requests as sampler 2");
    uint32_t tab[kHaltonDims * 4];
    halton_table(tab);
    HIP_TRY(s->d_halton.alloc(kHaltonDims * 4));
    HIP_TRY(hipMemcpy(s->d_halton.p, tab, sizeof(tab), hipMemcpyHostToDevice));
  }
  // float4 records: 5 x 64 per one-wave workgroup (kernel_path.hpp LaneRecords); with another box filter radius 16 x 2 x 64 more
  // behind them (kWideSlotFloat4: a chunk's sums per footprint)
  HIP_TRY(s->d_lane_state.grow((size_t)L.n_workgroups * (L.wide ? 320 + 2048 : 320)));
  if (!L.wide) {
    const size_t need = (size_t)L.pass_tiles * 4096u * (1u << L.chunk_shift);  // one float4 per item of a pass
    // (C3 1.07 GB in one pass; C4's 4096^2 x 16 chunks on one GPU: 3 passes over 1.43 GB; the buffer follows the frame: released when a
    // later render needs less than a quarter of it)
    if (s->d_partials.n / 4 > need) s->d_partials.release();
    HIP_TRY(s->d_partials.grow(need));
  }
  // the overflow variant keeps kQuadLdsStackOvf rows per lane in LDS; deeper entries (rare) go here
  HIP_TRY(s->d_stack_overflow.grow((size_t)L.n_workgroups * 64 * L.plan.extra_entries));
  return PBRT_HIP_OK;
}
}  // namespace

// the environment map's fields of the kernels' argument block (null / identity for a scene without one)
static void set_env_params(const pbrt_hip_scene *s, RenderParams *R) {
  R->env_texels = s->d_env_texels.p;
  R->env_marginal = s->d_env_marginal.p;
  R->env_conditional = s->d_env_conditional.p;
  R->env_w = s->env_w; R->env_h = s->env_h;
  for (int k = 0; k < 9; k++) R->env_m[k] = s->env_m[k];
  for (int k = 0; k < 3; k++) R->env_c[k] = s->env_c[k];
}

int pbrt_hip_envmap_eval_device(pbrt_hip_scene *s, int64_t n, const float *u12, float *d, uint32_t *texel, float *le, float *pdf) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "envmap_eval_device: null scene");
  if (!s->env) return fail(PBRT_HIP_ERR_INVALID, "envmap_eval_device: the scene has no environment map");
  if (n < 0 || (n && !d)) return fail(PBRT_HIP_ERR_INVALID, "envmap_eval_device: null argument");
  if (n == 0) return PBRT_HIP_OK;
  try {
    HIP_TRY(hipSetDevice(s->device));
    DevBuf<float> d_u, d_d, d_le, d_pdf;
    DevBuf<uint32_t> d_texel;
    HIP_TRY(d_d.alloc(3 * (size_t)n));
    HIP_TRY(d_le.alloc(3 * (size_t)n));
    HIP_TRY(d_pdf.alloc((size_t)n));
    HIP_TRY(d_texel.alloc((size_t)n));
    if (u12) {
      HIP_TRY(d_u.alloc(2 * (size_t)n));
      HIP_TRY(hipMemcpyAsync(d_u.p, u12, 8 * (size_t)n, hipMemcpyHostToDevice, s->stream));
    } else {
      HIP_TRY(hipMemcpyAsync(d_d.p, d, 12 * (size_t)n, hipMemcpyHostToDevice, s->stream));
    }
    RenderParams R{};
    set_env_params(s, &R);
    HIP_TRY(launch_envmap_eval(R, n, d_u.p, d_d.p, d_texel.p, d_le.p, d_pdf.p, s->stream));
    if (u12) HIP_TRY(hipMemcpyAsync(d, d_d.p, 12 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (texel) HIP_TRY(hipMemcpyAsync(texel, d_texel.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (le) HIP_TRY(hipMemcpyAsync(le, d_le.p, 12 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (pdf) HIP_TRY(hipMemcpyAsync(pdf, d_pdf.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return PBRT_HIP_OK;
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

int pbrt_hip_render_prepare(pbrt_hip_scene *s, const pbrt_hip_render_desc *r) {
  int rc = check_render_desc(s, r);
  if (rc) return rc;
  try {
    if (s->pending) return fail(PBRT_HIP_ERR_INVALID, "render_prepare: a render of this scene is still in flight (call pbrt_hip_render_wait first)");
    HIP_TRY(hipSetDevice(s->device));
    const FilmGeom fg = film_geom(s->desc, *r);
    const Shard sh = make_shard_bounds(fg.sb, r->rank, r->world_size);
    RenderLaunch L;
    rc = render_launch(s, r, fg, sh, &L);
    return rc ? rc : ensure_render_scratch(s, r, L);
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

int pbrt_hip_render_device(pbrt_hip_scene *s, const pbrt_hip_render_desc *r, void *d_slab, void *stream) {
  int rc = check_render_desc(s, r);
  if (rc) return rc;
  try {
    // the events, counters and lane-state records of a scene serve one render at a time
    if (s->pending) return fail(PBRT_HIP_ERR_INVALID, "render_device: a render of this scene is still in flight (call pbrt_hip_render_wait first)");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const FilmGeom fg = film_geom(s->desc, *r);
    const Shard sh = make_shard_bounds(fg.sb, r->rank, r->world_size);
    if ((sh.n_local || (fg.wide && fg.crop_px())) && !d_slab) return fail(PBRT_HIP_ERR_INVALID, "render_device: null slab");
    RenderParams R;
    R.sx0 = fg.sb[0]; R.sy0 = fg.sb[1]; R.sw = sh.w; R.sh = sh.h;
    R.seq_x0 = fg.sb[0] + fg.pad_x; R.seq_y0 = fg.sb[1] + fg.pad_y;
    R.seq_w = (uint32_t)(s->desc.xres + 2 * fg.pad_x); R.seq_h = (uint32_t)(s->desc.yres + 2 * fg.pad_y);
    R.max_lum = r->max_sample_luminance > 0.f ? r->max_sample_luminance : std::numeric_limits<float>::infinity();
    R.filter_rx = fg.rx; R.filter_ry = fg.ry;
    R.acc = fg.wide ? (unsigned long long *)d_slab : nullptr;
    RenderLaunch L;
    rc = render_launch(s, r, fg, sh, &L);
    if (!rc) rc = ensure_render_scratch(s, r, L);  // (no allocation when pbrt_hip_render_prepare ran for this description, or an earlier frame did)
    if (rc) return rc;
    R.sobol_mat = r->sampler == PBRT_HIP_SAMPLER_HALTON ? s->d_halton.p : (r->sampler == PBRT_HIP_SAMPLER_SOBOL_ND ? s->d_sobol.p : nullptr);
    R.tri_uv = s->d_tri_uv.p;
    R.textures = s->d_textures.p;
    R.glass = s->d_glass.p;
    set_env_params(s, &R);
    R.integrator = r->integrator;
    R.max_depth = r->max_depth;
    R.spp_x = r->spp_x;
    R.spp_y = r->spp_y;
    R.seed = r->seed;
    R.rank = r->rank;
    R.world = r->world_size;
    R.inv_nx = 1.0f / (float)r->spp_x;
    R.inv_ny = 1.0f / (float)r->spp_y;
    R.counters = s->d_counters.p;
    R.sampler = r->sampler;
    const uint32_t spp = r->spp_x * r->spp_y;
    R.spp_mask = 0;
    while (R.spp_mask + 1u < spp) R.spp_mask = 2u * R.spp_mask + 1u;
    // reciprocals for the kernel's two divisions by run-time values (render_body.inc pixel_xy, stratified sample): ceil(2^32 / d);
    // tsup / stx is exact while tsup * stx < 2^32
    auto recip32 = [](uint32_t d) { return d <= 1u ? 0u : (uint32_t)(((1ull << 32) + d - 1u) / d); };
    R.stx_recip = recip32(sh.stx);
    R.spp_x_recip = recip32(r->spp_x);
    if ((uint64_t)sh.total * (uint64_t)sh.stx >= (1ull << 32))
      return fail(PBRT_HIP_ERR_LIMIT, "render: film too large for the kernel's tile arithmetic");
    // The render kernel's waves are persistent: as many one-wave workgroups as the device holds at once (render_launch), each
    // lane drawing item after item from the rank's list.
    // An item is one CHUNK (a K-th of the samples, K <= 16 with at least 32 samples per chunk) of one pixel: DESIGN.md 3.1.
    R.chunk_shift = L.chunk_shift;
    const uint32_t n_chunks = 1u << R.chunk_shift;  // K: DESIGN.md 3.1
    R.n_workgroups = L.n_workgroups;
    R.next_item = reinterpret_cast<uint32_t *>(s->d_counters.p + 8);  // 8 counters, 64 bytes apart
    R.n_regions = std::min<uint32_t>(8u, std::max<uint32_t>(1u, tuning("PBRT_HIP_REGIONS", 8u, 8)));
    R.lane_state = s->d_lane_state.p;
    R.wide_slots = s->d_lane_state.p + (size_t)R.n_workgroups * 320;
    R.partials = fg.wide ? nullptr : s->d_partials.p;
    R.stack_overflow = s->d_stack_overflow.p;
    R.stack_overflow_entries = L.plan.extra_entries;
    R.min_walkers = L.min_walkers;
    R.min_parked = L.min_parked;
    HIP_TRY(hipMemsetAsync(s->d_counters.p, 0, 80 * sizeof(unsigned long long), st));
    if (fg.wide && fg.crop_px()) HIP_TRY(hipMemsetAsync(d_slab, 0, fg.crop_px() * 32, st));  // this rank's accumulators start at zero
    HIP_TRY(hipEventRecord(s->ev0, st));
    // one launch per pass (one pass unless the partial sums would pass the cap: partials_passes) renders every item of the pass; the merge
    // adds each pixel's K partial sums in chunk order (a wide filter has no partial sums: its samples go straight into the accumulators)
    for (uint32_t pass = 0; pass < L.passes; pass++) {
      const uint32_t n_pass = sh.n_local > pass ? (sh.n_local - pass + L.passes - 1) / L.passes : 0;
      if (n_pass == 0 && pass > 0) break;
      R.rank = r->rank + r->world_size * pass;
      R.world = r->world_size * L.passes;
      R.n_items = n_pass * 4096u * n_chunks;
      if (pass > 0)  // the hand-out positions start again; the ray counters (the first 64 bytes) run on
        HIP_TRY(hipMemsetAsync(s->d_counters.p + 8, 0, 72 * sizeof(unsigned long long), st));
      HIP_TRY(launch_render(L.counters == kCountExact ? s->dev_exact : s->dev, R, L, st));
      if (!fg.wide) HIP_TRY(launch_merge(R.partials, (float4 *)d_slab, sh.w, sh.h, R.rank, R.world, n_pass, spp, st, pass, L.passes));
    }
    HIP_TRY(hipEventRecord(s->ev1, st));
    s->pending = true;
    s->pending_counters = L.counters != kCountNone;
    // samples = pixels of this rank's super-tiles that lie inside the film
    uint64_t px = 0;
    for (uint32_t j = 0; j < sh.n_local; j++) {
      uint32_t t = r->rank + j * r->world_size;
      int32_t x0 = (int32_t)(t % sh.stx) * 64, y0 = (int32_t)(t / sh.stx) * 64;
      int32_t w = sh.w - x0 < 64 ? sh.w - x0 : 64, h = sh.h - y0 < 64 ? sh.h - y0 : 64;
      px += (uint64_t)w * (uint64_t)h;
    }
    s->pending_samples = px * (uint64_t)r->spp_x * (uint64_t)r->spp_y;
    return PBRT_HIP_OK;
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

int pbrt_hip_render_wait(pbrt_hip_scene *s, pbrt_hip_stats *stats) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "render_wait: null scene");
  if (!s->pending) return fail(PBRT_HIP_ERR_INVALID, "render_wait: no render in flight");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipEventSynchronize(s->ev1));
  s->pending = false;
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    stats->kernel_ms = ms;
    stats->samples = s->pending_samples;
    if (s->pending_counters) {
      unsigned long long c[5];
      HIP_TRY(hipMemcpy(c, s->d_counters.p, sizeof(c), hipMemcpyDeviceToHost));
      stats->camera_rays = c[0]; stats->bounce_rays = c[1]; stats->shadow_rays = c[2];
      stats->nodes_visited = c[3]; stats->tris_tested = c[4];
    }
  }
  return PBRT_HIP_OK;
}

int pbrt_hip_film_assemble_device(const pbrt_hip_scene *s, const void *d_slab, uint32_t rank, uint32_t world,
                                  void *d_film, void *stream) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "film_assemble: null argument");
  if (world == 0 || rank >= world) return fail(PBRT_HIP_ERR_INVALID, "film_assemble: rank must be < world_size");
  const Shard sh = make_shard(s->desc.xres, s->desc.yres, s->desc.crop, rank, world);
  if (sh.w <= 0 || sh.h <= 0) return PBRT_HIP_OK;  // (an empty crop window: a film of no pixels, which a caller may well hold in a NULL buffer)
  if (!d_film) return fail(PBRT_HIP_ERR_INVALID, "film_assemble: null argument");
  HIP_TRY(hipSetDevice(s->device));
  if (sh.n_local && !d_slab) return fail(PBRT_HIP_ERR_INVALID, "film_assemble: null slab");
  HIP_TRY(launch_assemble((const float4 *)d_slab, (float4 *)d_film, sh.w, sh.h, rank, world, sh.n_local,
                          (hipStream_t)stream));
  return PBRT_HIP_OK;
}

int pbrt_hip_render(pbrt_hip_scene *s, const pbrt_hip_render_desc *r, float *film, pbrt_hip_stats *stats) {
  int rc = check_render_desc(s, r);
  if (rc) return rc;
  if (!film) return fail(PBRT_HIP_ERR_INVALID, "render: null film");
  HIP_TRY(hipSetDevice(s->device));
  const FilmGeom fg = film_geom(s->desc, *r);
  const Shard sh = make_shard_bounds(fg.sb, r->rank, r->world_size);
  const size_t n_px = fg.crop_px();
  const size_t slab_n = fg.wide ? 2 * n_px : (size_t)sh.n_local * 4096;  // (wide: four int64 accumulators per pixel = two float4)
  HIP_TRY(s->d_slab.grow(slab_n));
  HIP_TRY(s->d_film.grow(n_px));
  if (n_px) HIP_TRY(hipMemsetAsync(s->d_film.p, 0, n_px * 16, s->stream));
  rc = pbrt_hip_render_device(s, r, s->d_slab.p, s->stream);
  if (rc) return rc;
  if (!n_px) rc = PBRT_HIP_OK;  // (an empty crop window: nothing was sampled, there is no film to assemble -- an empty film like the oracle's, not an error)
  else if (fg.wide) rc = pbrt_hip_film_from_acc_device(s, s->d_slab.p, s->d_film.p, s->stream);
  else rc = pbrt_hip_film_assemble_device(s, s->d_slab.p, r->rank, r->world_size, s->d_film.p, s->stream);
  hipError_t e = hipSuccess;
  if (!rc && n_px) e = hipMemcpyAsync(film, s->d_film.p, n_px * 16, hipMemcpyDeviceToHost, s->stream);
  const hipError_t e2 = hipStreamSynchronize(s->stream);  // (also on failure: the scene must not stay "in flight")
  if (rc || e != hipSuccess || e2 != hipSuccess) {
    s->pending = false;
    if (rc) return rc;
    return fail(PBRT_HIP_ERR_HIP, std::string("render: ") + hipGetErrorString(e != hipSuccess ? e : e2));
  }
  return pbrt_hip_render_wait(s, stats);
}

void pbrt_hip_sobol_matrices(uint32_t *out) { sobol_nd_matrices(out); }

int64_t pbrt_hip_render_buffer_bytes(const pbrt_hip_scene *s, const pbrt_hip_render_desc *r) {
  if (!s || !r || r->world_size == 0 || r->rank >= r->world_size) return -1;
  const FilmGeom fg = film_geom(s->desc, *r);
  if (fg.wide) return (int64_t)fg.crop_px() * 32;
  return (int64_t)make_shard_bounds(fg.sb, r->rank, r->world_size).n_local * 4096 * 16;
}

int pbrt_hip_film_from_acc_device(const pbrt_hip_scene *s, const void *d_acc, void *d_film, void *stream) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "film_from_acc: null argument");
  int32_t b[4];
  film_cropped_bounds(s->desc.xres, s->desc.yres, s->desc.crop, b);
  const size_t n_px = (size_t)std::max(0, b[2] - b[0]) * (size_t)std::max(0, b[3] - b[1]);
  if (!n_px) return PBRT_HIP_OK;  // (an empty crop window)
  if (!d_film) return fail(PBRT_HIP_ERR_INVALID, "film_from_acc: null argument");
  if (n_px && !d_acc) return fail(PBRT_HIP_ERR_INVALID, "film_from_acc: null accumulators");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(launch_film_from_acc((const unsigned long long *)d_acc, (float4 *)d_film, n_px, (hipStream_t)stream));
  return PBRT_HIP_OK;
}

int pbrt_hip_render_acc(pbrt_hip_scene *s, const pbrt_hip_render_desc *r, int64_t *acc, pbrt_hip_stats *stats) {
  int rc = check_render_desc(s, r);
  if (rc) return rc;
  const FilmGeom fg = film_geom(s->desc, *r);
  if (!fg.wide) return fail(PBRT_HIP_ERR_INVALID, "render_acc: the default box filter has no accumulators (use pbrt_hip_render)");
  const size_t n_px = fg.crop_px();
  if (n_px && !acc) return fail(PBRT_HIP_ERR_INVALID, "render_acc: null output");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(s->d_slab.grow(2 * n_px));
  rc = pbrt_hip_render_device(s, r, s->d_slab.p, s->stream);
  if (rc) return rc;
  hipError_t e = n_px ? hipMemcpyAsync(acc, s->d_slab.p, n_px * 32, hipMemcpyDeviceToHost, s->stream) : hipSuccess;
  const hipError_t e2 = hipStreamSynchronize(s->stream);
  if (e != hipSuccess || e2 != hipSuccess) {
    s->pending = false;
    return fail(PBRT_HIP_ERR_HIP, std::string("render_acc: ") + hipGetErrorString(e != hipSuccess ? e : e2));
  }
  return pbrt_hip_render_wait(s, stats);
}

// host restatement of film_from_acc_kernel (kernels.hip), for hosts that add the accumulators of several ranks themselves
void pbrt_hip_film_from_acc(const int64_t *acc, int64_t n_px, float *film) {
  const float inv = 1.0f / kFixedOne;
  for (int64_t i = 0; i < n_px; i++) {
    const float r = (float)acc[4 * i] * inv, g = (float)acc[4 * i + 1] * inv, b = (float)acc[4 * i + 2] * inv;
    film[4 * i] = 0.412453f * r + 0.357580f * g + 0.180423f * b;
    film[4 * i + 1] = 0.212671f * r + 0.715160f * g + 0.072169f * b;
    film[4 * i + 2] = 0.019334f * r + 0.119193f * g + 0.950227f * b;
    film[4 * i + 3] = (float)acc[4 * i + 3];
  }
}

int64_t pbrt_hip_slab_floats(int32_t xres, int32_t yres, const float crop[4], uint32_t rank, uint32_t world) {
  if (!crop || world == 0 || rank >= world || xres <= 0 || yres <= 0) return -1;
  return (int64_t)make_shard(xres, yres, crop, rank, world).n_local * 4096 * 4;
}

int pbrt_hip_slab_pixel_index(int32_t xres, int32_t yres, const float crop[4], uint32_t rank, uint32_t world,
                              int64_t *out) {
  if (!crop || !out || world == 0 || rank >= world || xres <= 0 || yres <= 0)
    return fail(PBRT_HIP_ERR_INVALID, "slab_pixel_index: bad argument");
  const Shard sh = make_shard(xres, yres, crop, rank, world);
  for (uint32_t j = 0; j < sh.n_local; j++) {
    const uint32_t t = rank + j * world;
    const int32_t x0 = (int32_t)(t % sh.stx) * 64, y0 = (int32_t)(t / sh.stx) * 64;
    for (int32_t py = 0; py < 64; py++)
      for (int32_t px = 0; px < 64; px++) {
        const int32_t x = x0 + px, y = y0 + py;
        out[(size_t)j * 4096 + py * 64 + px] = (x < sh.w && y < sh.h) ? (int64_t)y * sh.w + x : -1;
      }
  }
  return PBRT_HIP_OK;
}

static int ray_batch(pbrt_hip_scene *s, int64_t n, const float *o, const float *d, const float *tmax, float *t,
                     uint32_t *prim, float *b1, float *b2, uint8_t *occ, uint64_t *counters, bool any) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "intersect: null scene");
  if (n < 0 || (n && (!o || !d || !tmax))) return fail(PBRT_HIP_ERR_INVALID, "intersect: bad ray arrays");
  if (n == 0) {
    if (counters) counters[0] = counters[1] = 0;
    return PBRT_HIP_OK;
  }
  HIP_TRY(hipSetDevice(s->device));
  if (counters) {
    const int ce = ensure_canonical(s);
    if (ce) return ce;
  }
  DevBuf<float> d_o, d_d, d_tmax, d_t, d_b1, d_b2;
  DevBuf<uint32_t> d_prim;
  DevBuf<uint8_t> d_occ;
  HIP_TRY(d_o.alloc(3 * (size_t)n));
  HIP_TRY(d_d.alloc(3 * (size_t)n));
  HIP_TRY(d_tmax.alloc((size_t)n));
  HIP_TRY(hipMemcpyAsync(d_o.p, o, 12 * (size_t)n, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_d.p, d, 12 * (size_t)n, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_tmax.p, tmax, 4 * (size_t)n, hipMemcpyHostToDevice, s->stream));
  RayBatch B{};
  B.o = d_o.p; B.d = d_d.p; B.tmax = d_tmax.p; B.n = n;
  B.min_walkers = tuning("PBRT_HIP_MIN_WALKERS", kMinWalkers);
  B.min_parked = tuning("PBRT_HIP_MIN_PARKED", kMinParked);
  if (any) {
    HIP_TRY(d_occ.alloc((size_t)n));
    B.occluded = d_occ.p;
  } else {
    HIP_TRY(d_t.alloc((size_t)n)); HIP_TRY(d_prim.alloc((size_t)n)); HIP_TRY(d_b1.alloc((size_t)n)); HIP_TRY(d_b2.alloc((size_t)n));
    B.t = d_t.p; B.prim = d_prim.p; B.b1 = d_b1.p; B.b2 = d_b2.p;
  }
  if (counters) {
    HIP_TRY(hipMemsetAsync(s->d_counters.p, 0, 2 * sizeof(unsigned long long), s->stream));
    B.counters = s->d_counters.p;
  }
  // an overflow area for every wave of the largest grid launch_intersect makes
  B.stack_overflow_entries = intersect_overflow_entries(s->dev.quad_stack_need);
  HIP_TRY(s->d_stack_overflow.grow((size_t)kIntersectMaxWorkgroups * kIntersectWavesPerWorkgroup * 64 * B.stack_overflow_entries));
  B.stack_overflow = s->d_stack_overflow.p;
  const bool timed = debug_knob("PBRT_HIP_TIME_INTERSECT") != nullptr;  // tuning aid: kernel time to stderr
  if (timed) HIP_TRY(hipEventRecord(s->ev0, s->stream));
  HIP_TRY(launch_intersect(counters ? s->dev_exact : s->dev, B, any, s->bvh.depth, s->stream));
  if (timed) {
    HIP_TRY(hipEventRecord(s->ev1, s->stream));
    HIP_TRY(hipEventSynchronize(s->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    std::fprintf(stderr, "pbrt_hip intersect kernel: %lld rays %.3f ms %.1f Mrays/s\n", (long long)n, ms, (double)n / ms / 1e3);
  }
  if (any) {
    HIP_TRY(hipMemcpyAsync(occ, d_occ.p, (size_t)n, hipMemcpyDeviceToHost, s->stream));
  } else {
    HIP_TRY(hipMemcpyAsync(t, d_t.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(prim, d_prim.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(b1, d_b1.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(b2, d_b2.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
  }
  if (counters) {
    unsigned long long c[2];
    HIP_TRY(hipMemcpyAsync(c, s->d_counters.p, sizeof(c), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    counters[0] = c[0];
    counters[1] = c[1];
  } else {
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return PBRT_HIP_OK;
}

int pbrt_hip_intersect(pbrt_hip_scene *s, int64_t n, const float *o, const float *d, const float *tmax, float *t,
                       uint32_t *prim, float *b1, float *b2, uint64_t *counters) {
  if (n > 0 && (!t || !prim || !b1 || !b2)) return fail(PBRT_HIP_ERR_INVALID, "intersect: null output array");
  return ray_batch(s, n, o, d, tmax, t, prim, b1, b2, nullptr, counters, false);
}

int pbrt_hip_occluded(pbrt_hip_scene *s, int64_t n, const float *o, const float *d, const float *tmax, uint8_t *hit) {
  if (n > 0 && !hit) return fail(PBRT_HIP_ERR_INVALID, "occluded: null output array");
  return ray_batch(s, n, o, d, tmax, nullptr, nullptr, nullptr, nullptr, hit, nullptr, true);
}

// ---- host pieces ----
void pbrt_hip_film_cropped_bounds(int32_t xres, int32_t yres, const float crop[4], int32_t out[4]) {
  film_cropped_bounds(xres, yres, crop, out);
}

// Film::get_sample_bounds, core/film.rs:166-175
void pbrt_hip_film_sample_bounds(int32_t xres, int32_t yres, const float crop[4], float rx, float ry, int32_t out[4]) {
  int32_t c[4];
  film_cropped_bounds(xres, yres, crop, c);
  out[0] = (int32_t)std::floor((float)c[0] + 0.5f - rx);
  out[1] = (int32_t)std::floor((float)c[1] + 0.5f - ry);
  out[2] = (int32_t)std::ceil((float)c[2] - 0.5f + rx);
  out[3] = (int32_t)std::ceil((float)c[3] - 0.5f + ry);
}

// Film::get_film_tile, core/film.rs:264-281
void pbrt_hip_film_tile_bounds(int32_t xres, int32_t yres, const float crop[4], float rx, float ry, const int32_t sb[4],
                               int32_t out[4]) {
  int32_t c[4];
  film_cropped_bounds(xres, yres, crop, c);
  const int32_t x0 = (int32_t)std::ceil((float)sb[0] - 0.5f - rx), y0 = (int32_t)std::ceil((float)sb[1] - 0.5f - ry);
  const int32_t x1 = (int32_t)(std::floor((float)sb[2] - 0.5f + rx) + 1.f);
  const int32_t y1 = (int32_t)(std::floor((float)sb[3] - 0.5f + ry) + 1.f);
  out[0] = x0 > c[0] ? x0 : c[0];
  out[1] = y0 > c[1] ? y0 : c[1];
  out[2] = x1 < c[2] ? x1 : c[2];
  out[3] = y1 < c[3] ? y1 : c[3];
}

// Film::write_image's pixel loop, core/film.rs:346-372 (splat_xyz is never written: add_splat is
// unimplemented!() at film.rs:334-336, so the splat term is identically zero)
void pbrt_hip_film_to_rgb(const float *film, int64_t n, float scale, float *rgb) {
  for (int64_t i = 0; i < n; i++) {
    float c[3];
    xyz_to_rgb(film + 4 * i, c);
    const float w = film[4 * i + 3];
    if (w != 0.f) {
      const float inv = 1.f / w;
      for (int k = 0; k < 3; k++) {
        const float v = c[k] * inv;
        c[k] = v > 0.f ? v : 0.f;
      }
    }
    for (int k = 0; k < 3; k++) rgb[3 * i + k] = c[k] * scale;
  }
}

void pbrt_hip_look_at(const float pos[3], const float look[3], const float up[3], float m[16], float m_inv[16]) {
  look_at(pos, look, up, m, m_inv);
}

}  // extern "C"

// ---- scene ingestion (scene_parser.cpp) ----
struct pbrt_hip_loaded {
  pbrt_hip::LoadedScene s;
};

namespace {
const char *parse_error_name(pbrt_hip::ParseError e) {
  switch (e) {
    case pbrt_hip::ParseError::Eof: return "Eof";
    case pbrt_hip::ParseError::UnterminatedString: return "UnterminatedString";
    case pbrt_hip::ParseError::MixedParameters: return "MixedParameters";
    case pbrt_hip::ParseError::Unquoted: return "Unquoted";
    case pbrt_hip::ParseError::Syntax: return "Syntax";
    case pbrt_hip::ParseError::NotImplemented: return "NotImplemented";
    case pbrt_hip::ParseError::Io: return "Io";
    default: return "None";
  }
}
// "<kind>: <the reference's Display text for that kind, parser.rs:31-58>[: detail]"
std::string parse_error_text(pbrt_hip::ParseError e, const std::string &msg) {
  const std::string kind = parse_error_name(e);
  switch (e) {
    case pbrt_hip::ParseError::Eof: return kind + ": premature EOF" + (msg.empty() ? "" : " (" + msg + ")");
    case pbrt_hip::ParseError::UnterminatedString: return kind + ": unterminated string";
    case pbrt_hip::ParseError::MixedParameters: return kind + ": mixed string and numeric parameters";
    case pbrt_hip::ParseError::Unquoted: return kind + ": expected quoted string" + (msg.empty() ? "" : " (" + msg + ")");
    case pbrt_hip::ParseError::Syntax:
      return kind + (msg.rfind("input not float", 0) == 0 ? ": " + msg : ": syntax error: '" + msg + "'");
    case pbrt_hip::ParseError::NotImplemented: return kind + ": have not yet implemented '" + msg + "'";
    default: return kind + ": " + msg;
  }
}
size_t copy_out(const std::string &s, char *buf, size_t cap) {
  if (buf && cap) {
    size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return s.size();
}
}  // namespace

extern "C" {

int pbrt_hip_load_string(const char *text, size_t len, const char *base_dir, pbrt_hip_loaded **out) {
  if (!text || !out) return fail(PBRT_HIP_ERR_INVALID, "load_string: null argument");
  *out = nullptr;
  try {
    std::unique_ptr<pbrt_hip_loaded> l(new pbrt_hip_loaded());
    std::string msg;
    pbrt_hip::ParseError e = pbrt_hip::parse_scene(text, len, base_dir ? base_dir : "", &l->s, &msg);
    if (e != pbrt_hip::ParseError::None) return fail(PBRT_HIP_ERR_INVALID, parse_error_text(e, msg));
    *out = l.release();
    return PBRT_HIP_OK;
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

int pbrt_hip_load_file(const char *path, pbrt_hip_loaded **out) {
  if (!path || !out) return fail(PBRT_HIP_ERR_INVALID, "load_file: null argument");
  *out = nullptr;
  FILE *f = std::fopen(path, "rb");
  if (!f) return fail(PBRT_HIP_ERR_INVALID, std::string("Io: cannot open '") + path + "'");  // api.rs:392-395
  try {
    std::string text;
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    std::fclose(f);
    f = nullptr;
    std::string p(path);
    size_t slash = p.rfind('/');
    std::string dir = slash == std::string::npos ? "" : p.substr(0, slash);
    return pbrt_hip_load_string(text.data(), text.size(), dir.c_str(), out);
  } catch (const std::exception &e) {
    if (f) std::fclose(f);
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

void pbrt_hip_loaded_free(pbrt_hip_loaded *l) { delete l; }

int pbrt_hip_loaded_get(const pbrt_hip_loaded *l, pbrt_hip_scene_desc *d, pbrt_hip_render_desc *r, char *filename,
                        size_t cap) {
  if (!l) return fail(PBRT_HIP_ERR_INVALID, "loaded_get: null scene");
  const pbrt_hip::LoadedScene &s = l->s;
  if (d) {
    std::memset(d, 0, sizeof *d);
    d->P = s.P.data(); d->idx = s.idx.data(); d->mat_id = s.mat_id.data();
    d->mats = s.mats.data(); d->lights = s.lights.data(); d->spheres = s.spheres.data();
    d->n_verts = (uint32_t)(s.P.size() / 3); d->n_tris = (uint32_t)s.mat_id.size(); d->n_mats = (uint32_t)s.mats.size();
    d->n_lights = (uint32_t)s.lights.size(); d->n_spheres = (uint32_t)s.spheres.size();
    std::memcpy(d->cam_to_world, s.cam_to_world, 64);
    d->fov = s.fov; d->xres = s.xres; d->yres = s.yres;
    std::memcpy(d->crop, s.crop, 16);
    d->tri_uv = s.tri_uv.empty() ? nullptr : s.tri_uv.data();
    d->textures = s.textures.empty() ? nullptr : s.textures.data();
    d->n_textures = (uint32_t)s.textures.size();
  }
  if (r) {
    std::memset(r, 0, sizeof *r);
    r->integrator = s.integrator; r->max_depth = s.max_depth; r->spp_x = s.spp_x; r->spp_y = s.spp_y;
    r->seed = 0; r->rank = 0; r->world_size = 1;
    r->sampler = s.sampler;
    r->filter_xwidth = s.filter_radius[0]; r->filter_ywidth = s.filter_radius[1];
    r->max_sample_luminance = s.max_sample_luminance;
  }
  copy_out(s.filename, filename, cap);
  return PBRT_HIP_OK;
}

float pbrt_hip_loaded_film_scale(const pbrt_hip_loaded *l) { return l ? l->s.film_scale : 1.f; }

int pbrt_hip_loaded_warnings(const pbrt_hip_loaded *l, char *buf, size_t cap) {
  if (!l) return 0;
  std::string all;
  for (const std::string &w : l->s.warnings) { all += w; all += '\n'; }
  copy_out(all, buf, cap);
  return (int)l->s.warnings.size();
}

int pbrt_hip_loaded_state(const pbrt_hip_loaded *l, float ctm[16], char *names, size_t cap) {
  if (!l) return fail(PBRT_HIP_ERR_INVALID, "loaded_state: null scene");
  const pbrt_hip::LoadedScene &s = l->s;
  if (ctm) std::memcpy(ctm, s.final_ctm, 64);
  copy_out(s.camera_name + " " + s.sampler_name + " " + s.integrator_name + " " + s.filter_name + " " +
               s.accelerator_name + " " + s.film_name, names, cap);
  return PBRT_HIP_OK;
}

int pbrt_hip_tokenize(const char *text, size_t len, char *buf, size_t cap) {
  if (!text) return -1;
  pbrt_hip::Tokenizer t(text, len);
  std::string tok, all;
  int n = 0;
  pbrt_hip::ParseError e;
  while (t.next(&tok, &e)) {
    if (e != pbrt_hip::ParseError::None) { copy_out(all, buf, cap); return -(1 + n); }
    all += tok;
    all += '\n';
    n++;
  }
  copy_out(all, buf, cap);
  return n;
}

}  // extern "C"
