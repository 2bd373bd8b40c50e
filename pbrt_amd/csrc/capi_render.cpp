// capi_render.cpp -- everything that uses a finished scene behind the C ABI of include/pbrt_hip.h: the film geometry and the ranks'
// shards, the one place that plans a render's launch, the render entry points and the film's assembly, ray batches, and the film / camera
// helpers a host needs beside them.  capi_scene.cpp makes the scenes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../../include/pbrt_hip.h"
#include "capi_internal.hpp"
#include "device_types.h"
#include "host_math.hpp"
#include "pixel_filter.hpp"
#include "rgb_xyz.hpp"

using namespace pbrt_hip;

namespace pbrt_hip {
namespace {
inline float filter_radius(float w) { return w == 0.f ? 0.5f : w; }
inline bool filter_is_wide(float rx, float ry) { return rx != 0.5f || ry != 0.5f; }
// Film::get_sample_bounds, core/film.rs:166-175, of the cropped window c
void sample_bounds(const int32_t c[4], float rx, float ry, int32_t sb[4]) {
  sb[0] = (int32_t)std::floor(((float)c[0] + 0.5f) - rx);
  sb[1] = (int32_t)std::floor(((float)c[1] + 0.5f) - ry);
  sb[2] = (int32_t)std::ceil(((float)c[2] - 0.5f) + rx);
  sb[3] = (int32_t)std::ceil(((float)c[3] - 0.5f) + ry);
}
}  // namespace

FilmGeom film_geom(const FilmWindow &w, const pbrt_hip_pixel_filter *filter, float filter_xwidth, float filter_ywidth) {
  FilmGeom g;
  g.rx = filter_radius(filter_xwidth);
  g.ry = filter_radius(filter_ywidth);
  g.wide = filter_is_wide(g.rx, g.ry);
  if (filter) {  // a weighted filter: its kind's default radii, and the fixed-point film at every radius
    g.rx = filter_radius_of(*filter, filter_xwidth);
    g.ry = filter_radius_of(*filter, filter_ywidth);
    g.wide = true;
  }
  film_cropped_bounds(w.xres, w.yres, w.crop, g.crop);
  g.pad_x = g.pad_y = 0;
  for (int k = 0; k < 4; k++) g.sb[k] = g.crop[k];
  if (g.wide) {
    sample_bounds(g.crop, g.rx, g.ry, g.sb);
    g.pad_x = std::max(0, (int32_t)std::ceil(g.rx - 0.5f));
    g.pad_y = std::max(0, (int32_t)std::ceil(g.ry - 0.5f));
    // an empty crop window has no sample bounds either: nothing is sampled for a film of no pixels (as the oracle: 0 rays)
    if (!g.crop_px())
      for (int k = 0; k < 4; k++) g.sb[k] = g.crop[k];
  }
  return g;
}

}  // namespace pbrt_hip

namespace {

FilmGeom film_geom(const pbrt_hip_scene *s, const pbrt_hip_render_desc *r) {
  return pbrt_hip::film_geom(s->window, s->filter ? &*s->filter : nullptr, r->filter_xwidth, r->filter_ywidth);
}
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
// origin and clipped size of the rank's j-th super-tile, number rank + j * world in row-major order of the 64x64 grid
struct TileRect {
  int32_t x0, y0, w, h;
};
TileRect super_tile(const Shard &sh, uint32_t rank, uint32_t world, uint32_t j) {
  const uint32_t t = rank + j * world;
  const int32_t x0 = (int32_t)(t % sh.stx) * 64, y0 = (int32_t)(t / sh.stx) * 64;
  return {x0, y0, sh.w - x0 < 64 ? sh.w - x0 : 64, sh.h - y0 < 64 ? sh.h - y0 : 64};
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
// the production walk's stack plan under the A-B knobs PBRT_HIP_FORCE_OVERFLOW_VARIANT (the overflow variant for every tree) and
// PBRT_HIP_PREFER_LDS_STACK (the whole stack in LDS whenever it fits kQuadLdsStack rows, whatever the occupancy), read once
// (lds_records: the launch is the default path's, whose overflow instantiation keeps path records 0..2 in LDS behind a shorter stack)
RenderStackPlan stack_plan(uint32_t quad_stack_need, bool lds_records) {
  static const bool force_overflow = debug_knob("PBRT_HIP_FORCE_OVERFLOW_VARIANT") != nullptr;
  static const bool prefer_lds = debug_knob("PBRT_HIP_PREFER_LDS_STACK") != nullptr;
  return render_stack_plan(quad_stack_need, force_overflow, prefer_lds, lds_records);
}
// The switches of a render (render_variant.hpp), from the scene, the render description and the film geometry.  (Samplers 2 and 3 --
// Sobol' proper and Halton -- share one instantiation of the kernel: "the table samplers".)
RenderVariant render_variant(const pbrt_hip_scene *s, const pbrt_hip_render_desc *r, const FilmGeom &fg) {
  RenderVariant v{};
  v.spheres = s->dev.n_spheres > 0;
  v.wide = fg.wide;
  v.table_sampler = r->sampler == PBRT_HIP_SAMPLER_SOBOL_ND || r->sampler == PBRT_HIP_SAMPLER_HALTON;
  v.mis = r->integrator == PBRT_HIP_INTEGRATOR_PATH_MIS;
  v.textured = s->textured;
  v.glass = s->glass;
  v.env = s->env;
  v.normals = s->normals;
  v.counters = (r->flags & PBRT_HIP_FLAG_COUNTERS) ? kCountExact : ((r->flags & PBRT_HIP_FLAG_WALK_COUNTERS) ? kCountWalk : kCountNone);
  return v;
}

int check_render_desc(const pbrt_hip_scene *s, const pbrt_hip_render_desc *r) {
  if (!s || !r) return fail(PBRT_HIP_ERR_INVALID, "render: null argument");
  if (r->spp_x == 0 || r->spp_y == 0) return fail(PBRT_HIP_ERR_INVALID, "render: spp_x and spp_y must be >= 1");
  if (r->world_size == 0 || r->rank >= r->world_size) return fail(PBRT_HIP_ERR_INVALID, "render: rank must be < world_size");
  if (r->integrator > PBRT_HIP_INTEGRATOR_PATH_MIS) return fail(PBRT_HIP_ERR_INVALID, "render: unknown integrator");
  if (r->sampler > PBRT_HIP_SAMPLER_HALTON) return fail(PBRT_HIP_ERR_INVALID, "render: unknown sampler");
  // the kernels pack the sample index into 20 bits and the bounce count into 10 (kernel_path.hpp path_store): beyond that a
  // persistent wave would never see its pixel finish
  if ((uint64_t)r->spp_x * (uint64_t)r->spp_y > PBRT_HIP_MAX_SPP)
    return fail(PBRT_HIP_ERR_LIMIT, "render: more than 2^20 samples per pixel");
  if (r->max_depth > PBRT_HIP_MAX_DEPTH) return fail(PBRT_HIP_ERR_LIMIT, "render: maxdepth above 1023");
  // box filter radii, box.rs:57-61 (0 = the default 0.5): any positive radius up to 16 pixels; a weighted filter's likewise (0 = its
  // kind's default)
  const float fx = s->filter ? filter_radius_of(*s->filter, r->filter_xwidth) : filter_radius(r->filter_xwidth);
  const float fy = s->filter ? filter_radius_of(*s->filter, r->filter_ywidth) : filter_radius(r->filter_ywidth);
  if (!(fx > 0.f) || !(fy > 0.f) || !std::isfinite(fx) || !std::isfinite(fy)) return fail(PBRT_HIP_ERR_INVALID, "render: the filter radii must be positive");
  if (fx > 16.f || fy > 16.f) return fail(PBRT_HIP_ERR_LIMIT, "render: filter radius above 16 pixels");
  // the combinations of switches the library does not build
  const FilmGeom fg = film_geom(s, r);
  const RenderRefusal refusal = render_variant_refusal(render_variant(s, r, fg));
  if (refusal.code != PBRT_HIP_OK) return fail(refusal.code, refusal.text);
  if (!(r->max_sample_luminance >= 0.f)) return fail(PBRT_HIP_ERR_INVALID, "render: max_sample_luminance must be >= 0 (0 = none)");
  if (fg.wide) {
    // the fixed-point film: a sample adds at most 2^39 units to a pixel's int64 accumulator, and a pixel receives
    // at most spp x footprint samples (from every rank together: the N-rank reduce adds the same samples) -- 2^24 of them fit
    const uint64_t foot = (uint64_t)(2 * (int)std::ceil(fx) + 1) * (uint64_t)(2 * (int)std::ceil(fy) + 1);
    if ((uint64_t)r->spp_x * (uint64_t)r->spp_y * foot > (1ull << 24))
      return fail(PBRT_HIP_ERR_LIMIT, "render: samples per pixel x filter footprint above 2^24 (the fixed-point film's accumulators could wrap)");
    if (s->filter) {
      // 3.19: a sample adds at most |w| x 2^39 units, so the same rule with the table's largest weight in the product (a triangle filter
      // of radius 16 has weights up to 240.25, which count as 241); the kernel's 1 / radius must be a number
      if (!std::isfinite(1.0f / fx) || !std::isfinite(1.0f / fy)) return fail(PBRT_HIP_ERR_INVALID, "render: the filter radii must be positive");
      const pbrt_hip_pixel_filter &pf = *s->filter;
      float table[256], wmax = 0.f;
      filter_table(pf, fx, fy, table);
      for (float w : table) wmax = std::max(wmax, std::fabs(w));
      const uint64_t wceil = std::max<uint64_t>(1u, (uint64_t)std::ceil((double)wmax));
      if ((uint64_t)r->spp_x * (uint64_t)r->spp_y * foot * wceil > (1ull << 24))
        return fail(PBRT_HIP_ERR_LIMIT, std::string("render: samples per pixel x filter footprint x the largest weight of the \"") + filter_kind_name(pf.kind) +
                                            "\" pixel filter's table above 2^24 (the fixed-point film's accumulators could wrap)");
    }
  }
  return PBRT_HIP_OK;
}

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
  L.variant = render_variant(s, r, fg);
  L.family = render_family(L.variant);
  const bool shallow = s->dev.quad_stack_need <= kShallowStackNeed;
  const bool default_path = render_default_path(L.variant);
  L.plan = stack_plan(s->dev.quad_stack_need, default_path);
  L.lds_bytes = (L.plan.rows + L.plan.record_rows) * 256u;
  L.steps = default_path && !L.plan.overflow && shallow ? 2u : PBRT_STEPS_PER_CHECK;
  if (L.variant.counters == kCountExact) {
    const int ce = ensure_canonical(s);
    if (ce) return ce;
    // the exact walk holds at most depth - 1 entries (refs + entry distances): the smallest of the instantiated row counts that fits
    const uint32_t held = s->bvh.depth > 0 ? s->bvh.depth - 1 : 0;
    L.exact_rows = held > 40 ? 64 : held > 32 ? 40 : held > 26 ? 32 : held > 20 ? 26 : 20;
    L.lds_bytes = L.exact_rows * 512u;
  }
  // persistent one-wave workgroups per CU = what a CU holds at once, by the variant's registers and the plan's LDS; the grid is this x
  // the device's CU count (hipDeviceProp_t)
  L.waves_per_cu = render_waves_per_cu(L.variant, L.plan.waves_per_cu);
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
  // float4 records: 5 x 64 per one-wave workgroup (kernel_path.hpp LaneRecords; a kernel with records 0..2 in LDS uses the last two and keeps
  // the stride: 26 MB at most, and one layout for every instantiation); with another box filter radius 16 x 2 x 64 more
  // behind them (kWideSlotFloat4: a chunk's sums per footprint)
  HIP_TRY(s->d_lane_state.grow((size_t)L.n_workgroups * (L.variant.wide ? 320 + 2048 : 320)));
  if (s->filter) HIP_TRY(s->d_filter_table.grow(kFilterTableFloats));  // a weighted filter: its 256 weights and the two inverse radii
  if (!L.variant.wide) {
    const size_t need = (size_t)L.pass_tiles * 4096u * (1u << L.chunk_shift);  // one float4 per item of a pass
    // (C3 1.07 GB in one pass; C4's 4096^2 x 16 chunks on one GPU: 3 passes over 1.43 GB; the buffer follows the frame: released when a
    // later render needs less than a quarter of it)
    if (s->d_partials.n / 4 > need) s->d_partials.release();
    HIP_TRY(s->d_partials.grow(need));
  }
  // the overflow variant keeps kQuadLdsStackOvf rows per lane in LDS (the default path's: kQuadLdsWalkRows, its path records behind them);
  // deeper entries (rare) go here
  HIP_TRY(s->d_stack_overflow.grow((size_t)L.n_workgroups * 64 * L.plan.extra_entries));
  return PBRT_HIP_OK;
}
// the scene-owned fields of the kernels' argument block: (u, v) and textures, the glass table, the environment map, the corner normals and
// the image textures' texel pool (null / identity for a scene without them)
void scene_render_params(const pbrt_hip_scene *s, RenderParams *R) {
  R->tri_uv = s->d_tri_uv.p;
  R->textures = s->d_textures.p;
  R->mat_extra = s->d_mat_extra.p;
  R->env_texels = s->d_env_texels.p;
  R->env_marginal = s->d_env_marginal.p;
  R->env_conditional = s->d_env_conditional.p;
  R->env_w = s->env_w; R->env_h = s->env_h;
  for (int k = 0; k < 9; k++) R->env_m[k] = s->env_m[k];
  for (int k = 0; k < 3; k++) R->env_c[k] = s->env_c[k];
  R->tri_n = s->d_tri_n.p;
  R->image_texels = s->d_image_texels.p;
}
}  // namespace

extern "C" {

int pbrt_hip_render_stack_plan(uint32_t stack_need, uint32_t *lds_rows, uint32_t *waves_per_cu, uint32_t *overflow_entries) {
  const RenderStackPlan p = stack_plan(stack_need, false);
  if (lds_rows) *lds_rows = p.rows;
  if (waves_per_cu) *waves_per_cu = p.waves_per_cu;
  if (overflow_entries) *overflow_entries = p.extra_entries;
  return PBRT_HIP_OK;
}

int pbrt_hip_render_stack_layout(uint32_t stack_need, uint32_t *stack_rows, uint32_t *record_bytes, uint32_t *waves_per_cu, uint32_t *overflow_entries) {
  const RenderStackPlan p = stack_plan(stack_need, true);
  if (stack_rows) *stack_rows = p.rows;
  if (record_bytes) *record_bytes = p.record_rows * 256u;
  if (waves_per_cu) *waves_per_cu = p.waves_per_cu;
  if (overflow_entries) *overflow_entries = p.extra_entries;
  return PBRT_HIP_OK;
}

int pbrt_hip_envmap_eval_device(pbrt_hip_scene *s, int64_t n, const float *u12, float *d, uint32_t *texel, float *le, float *pdf) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "envmap_eval_device: null scene");
  if (!s->env) return fail(PBRT_HIP_ERR_INVALID, "envmap_eval_device: the scene has no environment map");
  if (n < 0 || (n && !d)) return fail(PBRT_HIP_ERR_INVALID, "envmap_eval_device: null argument");
  if (n == 0) return PBRT_HIP_OK;
  return guarded([&]() -> int {
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
    scene_render_params(s, &R);
    HIP_TRY(launch_envmap_eval(R, n, d_u.p, d_d.p, d_texel.p, d_le.p, d_pdf.p, s->stream));
    if (u12) HIP_TRY(hipMemcpyAsync(d, d_d.p, 12 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (texel) HIP_TRY(hipMemcpyAsync(texel, d_texel.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (le) HIP_TRY(hipMemcpyAsync(le, d_le.p, 12 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (pdf) HIP_TRY(hipMemcpyAsync(pdf, d_pdf.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return PBRT_HIP_OK;
  });
}

int pbrt_hip_shading_normal_eval_device(int device, int64_t n, const float *in, float *out) {
  if (n < 0 || !in || !out) return fail(PBRT_HIP_ERR_INVALID, "shading_normal_eval_device: null argument or negative count");
  if (n == 0) return PBRT_HIP_OK;
  return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> d_in, d_out;
    HIP_TRY(d_in.alloc(17 * (size_t)n));
    HIP_TRY(d_out.alloc(4 * (size_t)n));
    const hipStream_t stream = nullptr;  // the device's default stream
    HIP_TRY(hipMemcpyAsync(d_in.p, in, 4 * 17 * (size_t)n, hipMemcpyHostToDevice, stream));
    HIP_TRY(launch_shading_normal_eval(n, d_in.p, d_out.p, stream));
    HIP_TRY(hipMemcpyAsync(out, d_out.p, 4 * 4 * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}

int pbrt_hip_render_prepare(pbrt_hip_scene *s, const pbrt_hip_render_desc *r) {
  int rc = check_render_desc(s, r);
  if (rc) return rc;
  return guarded([&]() -> int {
    if (s->pending) return fail(PBRT_HIP_ERR_INVALID, "render_prepare: a render of this scene is still in flight (call pbrt_hip_render_wait first)");
    HIP_TRY(hipSetDevice(s->device));
    const FilmGeom fg = film_geom(s, r);
    const Shard sh = make_shard_bounds(fg.sb, r->rank, r->world_size);
    RenderLaunch L;
    rc = render_launch(s, r, fg, sh, &L);
    return rc ? rc : ensure_render_scratch(s, r, L);
  });
}

int pbrt_hip_render_device(pbrt_hip_scene *s, const pbrt_hip_render_desc *r, void *d_slab, void *stream) {
  int rc = check_render_desc(s, r);
  if (rc) return rc;
  return guarded([&]() -> int {
    // the events, counters and lane-state records of a scene serve one render at a time
    if (s->pending) return fail(PBRT_HIP_ERR_INVALID, "render_device: a render of this scene is still in flight (call pbrt_hip_render_wait first)");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const FilmGeom fg = film_geom(s, r);
    const Shard sh = make_shard_bounds(fg.sb, r->rank, r->world_size);
    if ((sh.n_local || (fg.wide && fg.crop_px())) && !d_slab) return fail(PBRT_HIP_ERR_INVALID, "render_device: null slab");
    RenderParams R;
    R.sx0 = fg.sb[0]; R.sy0 = fg.sb[1]; R.sw = sh.w; R.sh = sh.h;
    R.seq_x0 = fg.sb[0] + fg.pad_x; R.seq_y0 = fg.sb[1] + fg.pad_y;
    R.seq_w = (uint32_t)(s->window.xres + 2 * fg.pad_x); R.seq_h = (uint32_t)(s->window.yres + 2 * fg.pad_y);
    R.max_lum = r->max_sample_luminance > 0.f ? r->max_sample_luminance : std::numeric_limits<float>::infinity();
    R.filter_rx = fg.rx; R.filter_ry = fg.ry;
    R.acc = fg.wide ? (unsigned long long *)d_slab : nullptr;
    R.filter_table = nullptr;
    RenderLaunch L;
    rc = render_launch(s, r, fg, sh, &L);
    if (!rc) rc = ensure_render_scratch(s, r, L);  // (no allocation when pbrt_hip_render_prepare ran for this description, or an earlier frame did)
    if (rc) return rc;
    R.sobol_mat = r->sampler == PBRT_HIP_SAMPLER_HALTON ? s->d_halton.p : (r->sampler == PBRT_HIP_SAMPLER_SOBOL_ND ? s->d_sobol.p : nullptr);
    scene_render_params(s, &R);
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
    if (s->filter) {  // the table of this render's radii (the host copy lives in the scene: the copy is asynchronous)
      if (s->filter_table_rx != fg.rx || s->filter_table_ry != fg.ry) {
        HIP_TRY(hipStreamSynchronize(st));  // (an earlier copy from the host table may still be queued on this stream)
        filter_table(*s->filter, fg.rx, fg.ry, s->filter_table_host);
        s->filter_table_host[kFilterTableInvRx] = 1.0f / fg.rx;
        s->filter_table_host[kFilterTableInvRy] = 1.0f / fg.ry;
        s->filter_table_rx = fg.rx; s->filter_table_ry = fg.ry;
      }
      HIP_TRY(hipMemcpyAsync(s->d_filter_table.p, s->filter_table_host, sizeof(s->filter_table_host), hipMemcpyHostToDevice, st));
      R.filter_table = s->d_filter_table.p;
    }
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
      HIP_TRY(launch_render(L.variant.counters == kCountExact ? s->dev_exact : s->dev, R, L, st));
      if (!fg.wide) HIP_TRY(launch_merge(R.partials, (float4 *)d_slab, sh.w, sh.h, R.rank, R.world, n_pass, spp, st, pass, L.passes));
    }
    HIP_TRY(hipEventRecord(s->ev1, st));
    s->pending = true;
    s->pending_counters = L.variant.counters != kCountNone;
    // samples = pixels of this rank's super-tiles that lie inside the film
    uint64_t px = 0;
    for (uint32_t j = 0; j < sh.n_local; j++) {
      const TileRect t = super_tile(sh, r->rank, r->world_size, j);
      px += (uint64_t)t.w * (uint64_t)t.h;
    }
    s->pending_samples = px * (uint64_t)r->spp_x * (uint64_t)r->spp_y;
    return PBRT_HIP_OK;
  });
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
  const Shard sh = make_shard(s->window.xres, s->window.yres, s->window.crop, rank, world);
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
  const FilmGeom fg = film_geom(s, r);
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
  const FilmGeom fg = film_geom(s, r);
  if (fg.wide) return (int64_t)fg.crop_px() * 32;
  return (int64_t)make_shard_bounds(fg.sb, r->rank, r->world_size).n_local * 4096 * 16;
}

int pbrt_hip_film_from_acc_device(const pbrt_hip_scene *s, const void *d_acc, void *d_film, void *stream) {
  if (!s) return fail(PBRT_HIP_ERR_INVALID, "film_from_acc: null argument");
  const size_t n_px = film_geom(s->window).crop_px();
  if (!n_px) return PBRT_HIP_OK;  // (an empty crop window)
  if (!d_film) return fail(PBRT_HIP_ERR_INVALID, "film_from_acc: null argument");
  if (n_px && !d_acc) return fail(PBRT_HIP_ERR_INVALID, "film_from_acc: null accumulators");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(launch_film_from_acc((const unsigned long long *)d_acc, (float4 *)d_film, n_px, s->filter.has_value(), (hipStream_t)stream));
  return PBRT_HIP_OK;
}

int pbrt_hip_render_acc(pbrt_hip_scene *s, const pbrt_hip_render_desc *r, int64_t *acc, pbrt_hip_stats *stats) {
  int rc = check_render_desc(s, r);
  if (rc) return rc;
  const FilmGeom fg = film_geom(s, r);
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

// film_from_acc_kernel (kernels.hip) on the host, for hosts that add the accumulators of several ranks themselves
void pbrt_hip_film_from_acc(const int64_t *acc, int64_t n_px, float *film) {
  const float inv = 1.0f / kFixedOne;
  for (int64_t i = 0; i < n_px; i++) {
    const float r = (float)acc[4 * i] * inv, g = (float)acc[4 * i + 1] * inv, b = (float)acc[4 * i + 2] * inv;
    const Xyz c = rgb_to_xyz(r, g, b);
    film[4 * i] = c.x;
    film[4 * i + 1] = c.y;
    film[4 * i + 2] = c.z;
    film[4 * i + 3] = (float)acc[4 * i + 3];
  }
}

// the same for a weighted filter's accumulators: the fourth is the weight sum in 2^-24 units
void pbrt_hip_film_from_acc_weighted(const int64_t *acc, int64_t n_px, float *film) {
  const float inv = 1.0f / kFixedOne;
  for (int64_t i = 0; i < n_px; i++) {
    const float r = (float)acc[4 * i] * inv, g = (float)acc[4 * i + 1] * inv, b = (float)acc[4 * i + 2] * inv;
    const Xyz c = rgb_to_xyz(r, g, b);
    film[4 * i] = c.x;
    film[4 * i + 1] = c.y;
    film[4 * i + 2] = c.z;
    film[4 * i + 3] = (float)acc[4 * i + 3] * inv;
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
    const TileRect t = super_tile(sh, rank, world, j);
    for (int32_t py = 0; py < 64; py++)
      for (int32_t px = 0; px < 64; px++)
        out[(size_t)j * 4096 + py * 64 + px] = (px < t.w && py < t.h) ? (int64_t)(t.y0 + py) * sh.w + (t.x0 + px) : -1;
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

void pbrt_hip_film_sample_bounds(int32_t xres, int32_t yres, const float crop[4], float rx, float ry, int32_t out[4]) {
  int32_t c[4];
  film_cropped_bounds(xres, yres, crop, c);
  sample_bounds(c, rx, ry, out);
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
