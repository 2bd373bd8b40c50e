// device_types.h -- kernel argument blocks shared by the host launcher and the HIP kernels.
// HBM layout:
//   nodes   : 4 x 16 B per INTERIOR node of the binary BVH, holding the boxes of its two children
//             ("children in parent": one fetch tests both children, leaves need no fetch at all)
//             {c0.lo.xyz c0.hi.x} {c0.hi.yz c1.lo.xy} {c1.lo.z c1.hi.xyz} {ref0 ref1 axis 0}
//             ref = interior index, or 0x80000000 | n_prims << 24 | first leaf slot
//   tris    : 3 x 16 B per LEAF SLOT  {p0.xyz, triangle id} {p1.xyz, material id} {p2.xyz, 0}
//             (leaf order, so the <=4 triangles of a leaf are one contiguous 48..192 B run)
//   mats, lights, spheres : the small tables of 2, 5 and 2 x 16 B per material / light / sphere -- scene_tables.hpp states their rows, for
//             every kind of light and material, and holds their readers and writers.  (In the tree a sphere is a leaf record of `tris`:
//             {c.xyz, primitive id} {r, 0, 0, material id} {0, 0, 0, 1} -- word 3 of the third float4 flags it)
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include <cstdlib>

#include "render_variant.hpp"

namespace pbrt_hip {

// Tuning / A-B knobs (PBRT_HIP_MIN_WALKERS, PBRT_HIP_COLLAPSE, PBRT_HIP_TREE, ...) are read from the environment
// only when PBRT_HIP_DEBUG_KNOBS is set (to anything but "0"): a production process is not steered by stray variables.
inline const char *debug_knob(const char *name) {
  const char *on = std::getenv("PBRT_HIP_DEBUG_KNOBS");
  if (!on || !*on || (on[0] == '0' && !on[1])) return nullptr;
  return std::getenv(name);
}

// LDS stack of the production (quad) walk: one row = 64 lanes x 4 bytes.  A row count r serves trees whose worst-case stack
// bound is r - 2 (the sentinel and one scratch row).  The render kernel takes its rows as DYNAMIC shared memory, sized per
// scene (render_stack_plan below).  A CU has 160 KB of LDS, handed out in granules of 1280 bytes (measured: 31 and 32 rows run
// like 35, 30 rows 3 % faster): up to 30 rows (6 granules) a CU holds 20 one-wave workgroups -- 5 per SIMD, which is also
// what the kernel's 96 VGPRs allow --, 31..35 rows (7 granules) 18, 36..40 rows 16.  Trees that need more than 30 rows run
// the overflow variant: kQuadLdsStackOvf rows in LDS at 20 waves, deeper entries in HBM (kQuadLdsStack = the rows of the
// ray-batch kernel, and the most the render kernel takes with PBRT_HIP_PREFER_LDS_STACK).  -DPBRT_QUAD_LDS_STACK=12 forces the overflow variant on nearly every scene (tests of that path).
#ifdef PBRT_QUAD_LDS_STACK
constexpr uint32_t kQuadLdsStack = PBRT_QUAD_LDS_STACK, kQuadLdsStackOvf = PBRT_QUAD_LDS_STACK;
#else
constexpr uint32_t kQuadLdsStack = 40, kQuadLdsStackOvf = 30;
#endif
// Every tree that takes the overflow variant gets the same kQuadLdsStackOvf rows.  Round 2 gave very deep trees (stack bound
// >= 42: the 12 M-triangle `big` workload has 48) a 35-row variant at 18 waves per CU, on the assumption that they reach the
// end of a 30-row LDS part often.  They do not: the bound is a worst case that walks do not come near (tools/walk_sim.py with
// ORC_WALK_STACK_IN_TRIS: a ray's deepest stack in the 12 M-triangle tree is 8.5 entries on average, 19 at the 99.9th
// percentile, 23 at most over 40 000 rays; 1 M triangles: 7.6 / 17 / 20), so the HBM overflow area is a safety net, not a
// path; and more resident waves help this latency-bound workload (r03q / r03r: 20 waves with 30 rows 217 ms, 18 waves with
// 35 rows 219 ms, 16 waves 224 ms).
//
// The walk does not use 30 rows either, and the default path's overflow instantiations (render_kernel without counters, wide filter
// or table sampler) spend twelve of them on the path state instead: records 0..2 of kernel_path.hpp PathState, 1 KB per wave each,
// lie in LDS behind kQuadLdsWalkRows stack rows -- 18 + 12 rows are the same six granules, so the 20 waves stay -- and the service
// stage's three loads and three stores per visit never reach the L2 that the tree wants.  Entries beyond the 18
// rows go to the HBM overflow area like those beyond the 30.  A -DPBRT_QUAD_LDS_STACK below 20 is taken as the walk's rows themselves
// (the records follow them: 12 -> 24 rows); -DPBRT_PATH_RECORDS_HBM builds the records in HBM everywhere (A-B).
constexpr uint32_t kPathRecordRows = 12u;
#ifdef PBRT_PATH_RECORDS_HBM
constexpr bool kLdsPathRecords = false;
#else
constexpr bool kLdsPathRecords = true;
#endif
constexpr uint32_t kQuadLdsWalkRows = kQuadLdsStackOvf >= kPathRecordRows + 8u ? kQuadLdsStackOvf - kPathRecordRows : kQuadLdsStackOvf;
// (the two readings meet at 20: 20 -> 8 walk rows + 12, 19 -> 19 + 12 = 31 rows, a granule more and 18 waves.  The walk needs its sentinel,
// a scratch row and room for one step's four pushes before its overflow test; the records' 16-byte accesses need the rows' 256-byte grain)
static_assert(kQuadLdsWalkRows >= 8u, "PBRT_QUAD_LDS_STACK: the walk's LDS part needs at least 8 rows");
static_assert((kQuadLdsWalkRows * 256u) % 16u == 0u && (kPathRecordRows * 256u) == 3u * 1024u, "path records 0..2: three 16-byte-aligned 1 KB rows behind the stack");
constexpr uint32_t kLdsGranule = 1280u;
constexpr uint32_t kLdsBytesPerCu = 160u * 1024u;
// float4 per triangle record in `tris`: {p0, id}{p1, material}{p2, 0} + one of padding -- a 64-byte record never straddles
// a 128-byte line (a 48-byte one does so two times in eight): C3 +0.9 %, C2 +0.3 % for 16 bytes per triangle (3 = packed, A-B)
#ifndef PBRT_TRI_STRIDE
#define PBRT_TRI_STRIDE 4
#endif
constexpr uint32_t kTriStride = PBRT_TRI_STRIDE;
// node steps of the production walk between two scheduling checks (kernel_walk.hpp trav_run): 3 for deep trees (C3 +1 %, C2 +2 % over
// 2); the default path takes 2 in shallow trees, whose walks are a few steps long (capi_render.cpp render_launch; C4: 3 would cost 5 %)
#ifndef PBRT_STEPS_PER_CHECK
#define PBRT_STEPS_PER_CHECK 3
#endif
constexpr uint32_t kRenderMaxWavesPerCu = PBRT_RENDER_MAX_WAVES_PER_CU;  // (render_variant.hpp: 4 SIMDs x the largest register budget)

// An unused child slot of a quad node holds the ref of a leaf with no triangles (and an inverted box: lower planes 255,
// upper planes 0).  The box rejects it except for degenerate rays / flat nodes, and then the walk parks at an empty leaf and
// pops: harmless, so the node step needs no "is this slot used" test (it had two compares per step for it until r02c).
constexpr uint32_t kEmptyLeafRef = 0x80000000u;
// A leaf child's ref in a node record is kLeafRef | n_prims << 24 | first leaf slot (n_prims <= 64; quad_encode.hpp leaf_ref); the
// device builder's binary tree marks a leaf's child word with the same bit.
constexpr uint32_t kLeafRef = 0x80000000u;

// A pixel's spp samples are cut into K = sample_chunks(spp) chunks, each a work item with its own RNG stream and partial
// film sum (oracle/oracle.cpp has the same rule): the largest power of two <= 16 that leaves a chunk at least
// 32 samples (1 below 64 spp).  Item number: pixel-in-block (6 bits) | chunk << 6 | 8x8 block << (6 + log2 K).
constexpr uint32_t kMaxSampleChunks = 16u, kMinSamplesPerChunk = 32u;
inline uint32_t sample_chunk_shift(uint32_t spp) {  // log2 K
  uint32_t kb = 0;
  while ((2u << kb) <= kMaxSampleChunks && (2u << kb) * kMinSamplesPerChunk <= spp) kb++;
  return kb;
}

// Sampler 2: the first kSobolNdRequests requests of a sample take their own pair of Sobol' dimensions (host_math.hpp
// builds the 2 x kSobolNdRequests generator matrices; capi_render.cpp asserts the two constants agree)
constexpr uint32_t kSobolNdRequests = 64u;

struct RenderStackPlan {
  uint32_t rows;           // LDS rows of the walk's stack per wave
  bool overflow;           // the overflow variant (rows == kQuadLdsStackOvf, or kQuadLdsWalkRows with the path records behind them)
  uint32_t waves_per_cu;   // one-wave workgroups a CU holds at once with these rows (at most 20: 5 per SIMD by registers)
  uint32_t extra_entries;  // HBM entries per lane beyond the LDS part (overflow variant)
  uint32_t record_rows;    // LDS rows behind the stack's that hold path records 0..2 (kPathRecordRows, or 0: the records are in HBM)
};
// lds_records: the plan of a launch whose overflow instantiation keeps the path records in LDS (the default path's, see above); every
// other launch, and every tree that keeps its whole stack in LDS, has them in HBM
inline RenderStackPlan render_stack_plan(uint32_t quad_stack_need, bool force_overflow, bool prefer_lds = false, bool lds_records = false) {
  RenderStackPlan p;
  const uint32_t need_rows = quad_stack_need + 2u;
  auto waves = [](uint32_t rows) {
    const uint32_t bytes = (rows * 256u + kLdsGranule - 1u) / kLdsGranule * kLdsGranule, w = kLdsBytesPerCu / bytes;
    return w > kRenderMaxWavesPerCu ? kRenderMaxWavesPerCu : w;
  };
  p.rows = need_rows < 8u ? 8u : need_rows;
  // (20 waves with the overflow variant beat 18 or 16 waves with the whole stack in LDS: C2 +1 %, C3 +4 %)
  p.overflow = force_overflow || need_rows > kQuadLdsStack || (waves(p.rows) < waves(kQuadLdsStackOvf) && !prefer_lds);
  p.record_rows = p.overflow && lds_records && kLdsPathRecords ? kPathRecordRows : 0u;
  if (p.overflow) p.rows = p.record_rows ? kQuadLdsWalkRows : kQuadLdsStackOvf;
  p.waves_per_cu = waves(p.rows + p.record_rows);
  p.extra_entries = p.overflow && need_rows > p.rows ? need_rows - p.rows : 0u;
  return p;
}
// The ray-batch kernel (pbrt_hip_intersect / pbrt_hip_occluded: the walk alone, ~64 VGPRs) runs 8 waves per SIMD with 20 rows of a
// lane's stack in LDS (20 KB per 4-wave workgroup, 8 per CU) and deeper entries in HBM: +9 % on 4 waves with 40 rows, +12 % at equal
// rows (tools/experiments/dual_ray, profiles/r03y_traversal_occupancy_1m.txt)
constexpr uint32_t kIntersectLdsStack = 20;
// Its grid: persistent workgroups of 4 waves (intersect_kernel), one per 256 rays and at most kIntersectMaxWorkgroups of them.  Each
// wave has its own HBM area of intersect_overflow_entries x 64 lanes for the entries beyond the kIntersectLdsStack - 1 kept in LDS
// (+ the sentinel).
constexpr uint32_t kIntersectWavesPerWorkgroup = 4, kIntersectMaxWorkgroups = 256 * 16;
inline uint32_t intersect_workgroups(int64_t n_rays) {
  const int64_t w = (n_rays + 255) / 256;
  return w > kIntersectMaxWorkgroups ? kIntersectMaxWorkgroups : (uint32_t)w;
}
inline uint32_t intersect_overflow_entries(uint32_t quad_stack_need) {
  return quad_stack_need + 2u > kIntersectLdsStack ? quad_stack_need + 2u - kIntersectLdsStack : 0u;
}

struct DevScene {
  const uint4 *nodes;
  const uint4 *quads;  // 4 x 16 B per quantised quad node (quad_encode.hpp; on the host quad_nodes.hpp QuadNodes)
  uint32_t quad_stack_need;
  const float4 *tris;
  const float4 *mats;
  const float4 *lights;
  const float4 *spheres;
  uint32_t n_nodes, n_tris, n_spheres, n_lights;  // n_nodes: nodes of the binary tree (0 = no triangles)
  float n_lights_f;                                 // (float)n_lights
  uint32_t root_ref;                                // ref of the root (a leaf ref for tiny scenes)
  float root_lo[3], root_hi[3];                     // its box
  float le_inf[3];
  uint32_t has_inf;
  float c2w[12];  // rows 0..2 of camera_to_world
  float cam_ax, cam_bx, cam_ay, cam_by;
  int32_t xres, yres;
  int32_t cx0, cy0, cx1, cy1;  // cropped pixel bounds
  // The production walk's stand-in for 1 / 0 (a ray PARALLEL to a slab; kernel_walk.hpp trav_run): a power of two so large that every t it
  // makes lies outside any ray interval, yet small enough that (o - origin) x it stays finite for every origin inside the root box
  // (host_math.hpp inv_parallel_for_extent).
  float inv_parallel;
};

struct RenderParams {
  uint32_t integrator, max_depth, spp_x, spp_y;
  uint64_t seed;
  uint32_t rank, world;
  float inv_nx, inv_ny;
  unsigned long long *counters;  // 5: camera, bounce, shadow rays, nodes visited, triangles tested
  uint32_t min_walkers, min_parked;  // traversal scheduling thresholds (kernel_walk.hpp trav_run)
  float4 *lane_state;                // 5 x 64 float4 per workgroup: path state parked in HBM (kernel_path.hpp PathState)
  float4 *wide_slots;                // wide box filter: 16 x 2 x 64 float4 per workgroup, a chunk's sums per footprint (kernel_path.hpp)
  uint32_t *stack_overflow;          // [workgroup][entry][lane]: stack entries beyond the LDS part
  uint32_t stack_overflow_entries;
  uint32_t *next_item;    // hand-out counters of the render kernel's item list, one per region, 16 words apart (zeroed before the launch)
  uint32_t n_regions;     // contiguous parts of the list, one per XCD (render_body.inc fetch step)
  uint32_t n_items;       // n_local_super * 4096 pixels * K chunks (render_body.inc: item = block, chunk, pixel in block)
  uint32_t chunk_shift;   // log2 K, K = sample_chunks(spp)
  uint32_t n_workgroups;  // one-wave workgroups launched: what the device holds at once, not one per tile
  float4 *partials;       // [slab position][K]: the partial film sums of the chunks (merge_kernel adds them in order)
  uint32_t sampler;       // PBRT_HIP_SAMPLER_*
  uint32_t spp_mask;      // Sobol sampler: 2^ceil(log2(spp)) - 1
  uint32_t stx_recip, spp_x_recip;  // ceil(2^32 / super-tiles per row), ceil(2^32 / spp_x): the kernel's divisions by these two
  // The pixels that are SAMPLED (Film::get_sample_bounds, film.rs:166-175): the cropped window for the default box filter,
  // `pad` = ceil(radius - 0.5) pixels more on every side for a wider one.  The 64x64 super-tiles cover them.
  int32_t sx0, sy0, sw, sh;  // origin and size of the sample bounds
  int32_t seq_x0, seq_y0;    // sx0 + pad_x, sy0 + pad_y: a sampled pixel's coordinates in the numbering of the RNG streams ...
  uint32_t seq_w, seq_h;     // ... whose rows are xres + 2 pad_x long (yres + 2 pad_y of them): the image plus its halo
  float max_lum;             // Film "maxsampleluminance" (film.rs:75,279; pbrt-v3 FilmTile::AddSample); +inf = none
  // box filter radii other than 0.5 (render_kernel<..., WIDE>): fixed-point film accumulators, int64 {r, g, b, samples} per
  // pixel of the cropped window, added to with atomics
  float filter_rx, filter_ry;
  unsigned long long *acc;
  // sampler 2 (render_kernel<..., SND>): generator matrices of the first ten Sobol' dimensions, 32 columns each
  const uint32_t *sobol_mat;
  // textured materials (render_kernel_x<..., TEX>): corner (u, v) per leaf slot -- 3 x float2 --, and 3 x 16 B per
  // texture {type, tex1.rgb}{tex2.rgb, su}{sv, du, dv, 0}; a material's texture number rides in its second row's w (0 = none: scene_tables.hpp).  (Scene
  // data -- but appended HERE, to the kernel's last argument: a field added to DevScene would move every offset of this block and
  // with them the machine code of the instantiations the counter profiles are keyed by.)
  const float2 *tri_uv;
  const float4 *textures;
  // the materials' extra rows (render_kernel_x<..., GLS>; scene_tables.hpp mat_extra): 16 B per MATERIAL, read for
  // glass ({Kt.rgb, eta}) and, under PLS, for plastic and substrate ({Ks.rgb, alpha}) alone; null for a scene without such a material.  At the
  // end, for the reason given above.
  const float4 *mat_extra;
  // an environment-map infinite light (render_kernel_env): the texels {r, g, b, p_uv} row-major (row 0 = theta 0), the
  // marginal CDF over rows (env_h + 1 floats) and the rows' conditional CDFs (env_h x (env_w + 1)), world_to_light (row-major 3 x 3) and
  // the light's factor on the texels (envmap_core.hpp).  At the end, for the reason given above.
  const float4 *env_texels;
  const float *env_marginal, *env_conditional;
  uint32_t env_w, env_h;
  float env_m[9];
  float env_c[3];
  // shading normals (render_kernel_n): the corner normals of every leaf slot, 3 x float4 {n, 0}, world space, any length
  // (zeros = the triangle has none; a sphere's proxy slot: zeros), read at a shaded triangle hit alone.  At the end, for the reason given above.
  const float4 *tri_n;
  // a weighted pixel filter (the `if (R.filter_table)` of render_body.inc's WIDE finish): the 16 x 16 table of weights made on
  // the host (null: the box) with 1 / filter_rx and 1 / filter_ry behind its 256 weights (kFilterTableInvRx, kFilterTableInvRy).  (One
  // pointer is all the filter adds to the kernel's arguments: every scalar more is a register held through the kernel, and the WIDE
  // instantiations have none to spare.)  At the end, for the reason given above.
  const float *filter_table;
  // image textures for Kd (the type-4 branch of render_body.inc's TEX block): the texels of every image slot in one pool,
  // float4 {r, g, b, 0} each -- one aligned 16-byte load per texel --, a slot's first texel at the offset its rows carry (image_lookup.hpp);
  // null for a scene without an image.  At the end, for the reason given above.
  const float4 *image_texels;
};
// the device copy of a filter table: the 256 weights, then 1 / rx and 1 / ry
constexpr uint32_t kFilterTableInvRx = 256u, kFilterTableInvRy = 257u, kFilterTableFloats = 260u;
// 2^24 fixed-point units per unit of radiance, a component clamped to [0, 2^15]
constexpr float kFixedOne = 16777216.0f, kFixedMax = 32768.0f;

struct RayBatch {
  const float *o, *d, *tmax;  // 3n, 3n, n
  int64_t n;
  float *t;
  uint32_t *prim;
  float *b1, *b2;
  uint8_t *occluded;
  unsigned long long *counters;  // 2: nodes, tris (may be null)
  uint32_t min_walkers, min_parked;
  uint32_t *stack_overflow;
  uint32_t stack_overflow_entries;
};

// One launch of the render kernel, decided on the host in one place (capi_render.cpp render_launch) from the scene, the render description
// and the film geometry.  launch_render maps it to an instantiation and computes nothing.
struct RenderLaunch {
  RenderVariant variant;  // the switches, and the family that renders them (render_variant.hpp says which combinations exist)
  RenderFamily family;
  RenderStackPlan plan;  // the production walk's stack: LDS rows, the overflow variant, HBM entries per lane
  uint32_t steps;        // production walk: node steps per scheduling check (STEPS)
  uint32_t exact_rows;   // exact walk: STACK, its stack rows of refs (and as many of entry distances)
  uint32_t lds_bytes;    // dynamic shared memory per one-wave workgroup
  uint32_t waves_per_cu;  // one-wave workgroups per CU: the plan's, clamped for the variant's register budget (render_waves_per_cu)
  uint32_t n_workgroups;  // the grid: waves_per_cu x the device's CUs, at most one per item of the largest pass
  uint32_t chunk_shift;   // log2 K, K = the sample chunks of a pixel
  uint32_t passes;        // launches of a frame over one partial-sums buffer (capi_render.cpp partials_passes) ...
  uint32_t pass_tiles;    // ... and the super-tiles of the largest one
  uint32_t min_walkers, min_parked;  // traversal scheduling thresholds (RenderParams)
};

// launchers (kernels.hip)
hipError_t launch_render(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t stream);
// kernels_x.hip: the launch of render_kernel_x, the MIS / texture / glass variants (launch_render hands it over)
hipError_t launch_render_x(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t stream);
// kernels_env.hip: the launch of a scene with an environment map (launch_render hands it over), and envmap_core.hpp over device arrays
// (pbrt_hip_envmap_eval_device: u12 != nullptr samples into d, else d is looked up; R's env_* fields are the map)
hipError_t launch_render_env(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t stream);
hipError_t launch_envmap_eval(const RenderParams &R, int64_t n, const float *u12, float *d, uint32_t *texel, float *le, float *pdf, hipStream_t stream);
// kernels_n.hip: the launch of a scene with shading normals (3.18; launch_render asks this first and hands over), the gather of the corner
// normals (9 floats per triangle, triangle order) into leaf-slot order (3 x float4 per slot; a sphere's proxy slot: zeros), and
// shading_normal.inc over device arrays (pbrt_hip_shading_normal_eval_device: 17 floats in, 4 out per element)
hipError_t launch_render_n(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t stream);
hipError_t launch_pack_nrm(const float *tri_n, const uint32_t *order, uint32_t n_prims, uint32_t n_tris, float4 *out, hipStream_t stream);
hipError_t launch_shading_normal_eval(int64_t n, const float *in, float *out, hipStream_t stream);
// fixed-point accumulators -> film pixels {X, Y, Z, weight}
// (weighted: the accumulators of a weighted pixel filter, whose fourth is the weight sum in 2^-24 units: DESIGN.md 3.19)
hipError_t launch_film_from_acc(const unsigned long long *acc, float4 *film, size_t n_px, bool weighted, hipStream_t stream);
// kernels_blocks.hip: filter_weight.inc over device arrays (pbrt_hip_filter_footprint_eval_device)
hipError_t launch_filter_footprint_eval(float rx, float ry, const int32_t crop[4], int64_t n_points, const float *points, int32_t *bounds, int64_t n_pairs,
                                        const float *pair_points, const int32_t *pair_pixels, int32_t *index, hipStream_t stream);
// kernels_blocks.hip: image_lookup.hpp over device arrays (pbrt_hip_image_lookup_eval_device: the slot's three rows, the pool, n x (u, v) -> n x rgb)
hipError_t launch_image_lookup_eval(const float4 *rows, const float4 *pool, int64_t n, const float *uv, float *rgb, hipStream_t stream);
hipError_t launch_acc_add(unsigned long long *dst, const unsigned long long *src, size_t n, hipStream_t stream);  // dst[i] += src[i]
hipError_t launch_intersect(const DevScene &S, const RayBatch &B, bool any_hit, uint32_t bvh_depth, hipStream_t stream);
// (n_prims = n_tris + the spheres, whose records come from the `spheres` table: kernels.hip pack_tris_kernel)
hipError_t launch_pack_tris(const float *P, const uint32_t *idx, const uint16_t *mat_id, const uint32_t *order,
                            uint32_t n_prims, uint32_t n_tris, const float4 *spheres, float4 *tris, hipStream_t stream);
// corner (u, v) of every triangle (6 floats, triangle order) -> leaf-slot order
hipError_t launch_pack_uv(const float *tri_uv, const uint32_t *order, uint32_t n_prims, uint32_t n_tris, float2 *out, hipStream_t stream);
// adds the K partial sums of every pixel of a rank's slab in chunk order and converts to XYZ (Film::merge_film_tile)
hipError_t launch_merge(const float4 *partials, float4 *slab, int32_t w, int32_t h, uint32_t rank, uint32_t world,
                        uint32_t n_local_super, uint32_t spp, hipStream_t stream, uint32_t j0 = 0, uint32_t jstride = 1);
// bvh_gpu.hip: the accelerator built on the device.  d_order (n_tris) and d_quads (>= n_tris nodes of 4 uint4) are outputs.
// What the tree's optimisation by parallel re-insertion (reinsert_core.hpp) did: THE definition, held by GpuBuildInfo and by a scene's
// BuildStats (capi_internal.hpp) and reported by pbrt_hip_scene_optimize_info / _optimize_cost.  All zero where no pass ran.
struct ReinsertStats {
  uint32_t passes = 0, moves = 0;  // passes kept, moves applied in them
  float ms = 0.f;                  // (hipEventElapsedTime's float; the C ABI widens it)
  double cost_before = 0.0, cost_after = 0.0;  // summed half surface area of the interior nodes before the first and after the last kept pass
  uint32_t undone = 0;                         // 1: a pass raised that sum, was undone and ended the passes
};
struct GpuBuildInfo {
  uint32_t n_quads, stack_need, levels;
  float root_lo[3], root_hi[3];
  float build_ms;  // everything, the optimisation included
  ReinsertStats reinsert;
};
constexpr uint32_t kGpuBuildReinsert = 1u;  // flags of gpu_build_quads: optimise the binary tree by re-insertion before the collapse
struct GpuBuildStages;  // build_stages.hpp: host copies of the tree between the stages (null on every production path)
hipError_t gpu_build_quads(const float *d_P, const uint32_t *d_idx, uint32_t n_tris, uint32_t *d_order, uint4 *d_quads,
                           uint32_t quad_capacity, uint32_t flags, GpuBuildInfo *info, hipStream_t stream, GpuBuildStages *stages = nullptr);
hipError_t launch_assemble(const float4 *slab, float4 *film, int32_t w, int32_t h, uint32_t rank, uint32_t world,
                           uint32_t n_local_super, hipStream_t stream);

}  // namespace pbrt_hip
