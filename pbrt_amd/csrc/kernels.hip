// kernels.hip -- the CDNA4 (gfx950) kernels of the render path.
//
//   render_kernel    persistent one-wave workgroups (as many as the device holds at once); every lane draws a
//                    pixel from the rank's pixel list (XCD-aware hand-out, one atomic per wave and round), keeps
//                    it for all its samples, in order: stratified camera sample -> BVH closest hit -> emission
//                    -> one-light direct estimate (any-hit shadow ray) -> BSDF sample -> Russian roulette; then
//                    writes the film pixel and draws the next one.  The wave walks a quantised 4-wide BVH in a
//                    "while-while" loop with parked leaves; `__ballot` + popcount take every scheduling decision
//                    wave-uniformly.  Per-lane traversal stack in LDS, laid out stack[level][lane]
//                    (conflict-free: lane l -> bank l); path state parked in coalesced HBM records.
//   intersect_kernel the traversal loop alone over a ray batch (parity + roofline of the loop).
//   pack_tris_kernel builds the leaf-ordered 48-byte triangle records from the uploaded
//                    vertex / index buffers.
//   assemble_kernel  scatters a rank's tile-major slab into the row-major film.
//
// The building blocks are headers (kernel_math.hpp, kernel_walk.hpp, kernel_path.hpp) and render_body.inc, shared with the other kernel
// units, each of which holds one more family of render kernels.  render_variant.hpp says which family renders what and with which
// register budget; launch_render below hands a launch to its family's unit.
#include "kernel_path.hpp"
#include "rgb_xyz.hpp"
#include "with_bools.hpp"

namespace pbrt_hip {
namespace {

// COUNT: accumulate ray / visit counters.  EXACT (needs COUNT): walk the tree in exactly the oracle's
// order so that the counters are the oracle's; COUNT without EXACT counts the production walk itself
// (64-byte fetches and triangle tests).
// One workgroup = one wavefront = one 8x8 pixel tile; 64 workgroups per 64x64 super-tile.
// STACK: LDS entries of the exact walk; for the production walk the LDS rows of the overflow variant (deeper entries
// in the HBM overflow area), or 0 = the whole stack in LDS.
// WIDE: a box filter radius other than 0.5: a sample is added to every pixel within the radius, into
// fixed-point accumulators with atomics, instead of to its chunk's partial sum.
// SND: sampler 2, the Sobol' sampler with its own dimensions per request (3.12): generator-matrix lookups in the service stage.
// (Both variants keep the default path's register budget, no spill -- tests/test_host.py.)  What the switches stand for in render_variant.hpp:
constexpr RenderVariant default_variant(bool sph, bool count, bool exact, bool wide, bool snd) {
  return {sph, wide, snd, false, false, false, false, false, count ? (exact ? kCountExact : kCountWalk) : kCountNone};
}
template <bool SPH, bool COUNT, bool EXACT, int STACK, int STEPS = PBRT_STEPS_PER_CHECK, bool WIDE = false, bool SND = false>
__global__ void __launch_bounds__(64, (COUNT ? 1 : render_waves_per_simd(RenderFamily::kDefault, SPH, false))) render_kernel(const DevScene S, const RenderParams R) {
  constexpr bool MIS = false, TEX = false, GLS = false, ENV = false, NRM = false;  // (the other families': render_variant.hpp)
  // the plain default path's overflow instantiations keep path records 0..2 in LDS behind a shorter stack (device_types.h kLdsPathRecords)
  constexpr bool LREC = kLdsPathRecords && STACK != 0 && render_default_path(default_variant(SPH, COUNT, EXACT, WIDE, SND));
  (void)MIS;
  (void)GLS;
  constexpr bool PLS = false;  // (the plastic material, DESIGN.md 3.21: the GLS instantiations of render_kernel_x alone)
  (void)PLS;
  (void)ENV;
#include "render_body.inc"
}

#ifndef PBRT_INTERSECT_WAVES_PER_SIMD
#define PBRT_INTERSECT_WAVES_PER_SIMD 8
#endif
// The traversal loop alone over a ray batch, as persistent waves with dynamic fetch: a lane whose
// walk is over writes its result and pulls its next ray while the other lanes keep walking.
template <bool SPH, bool COUNT, int STACK>
// (scenes with spheres: the f64 quadratic of the leaf pass does not fit the 64 VGPRs of eight waves per SIMD -- four, as few rays as such scenes trace)
__global__ void __launch_bounds__(256, (COUNT ? 1 : (SPH ? 4 : PBRT_INTERSECT_WAVES_PER_SIMD))) intersect_kernel(const DevScene S, const RayBatch B, const int any_hit) {
  __shared__ uint32_t lds_stack[4][COUNT ? STACK : kIntersectLdsStack][64];
  __shared__ float lds_tn[COUNT ? 4 : 1][COUNT ? STACK : 1][64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t *stk = &lds_stack[wave][0][lane];
  float *stkt = &lds_tn[COUNT ? wave : 0][0][lane];
  uint32_t *ovf = B.stack_overflow + ((size_t)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane(wave)) * B.stack_overflow_entries * 64u;  // wave-uniform
  const TravTuning tune = {B.min_walkers, B.min_parked};
  unsigned long long cn = 0, ct = 0;
  EXP_PROBE_INIT_BLOCK();
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t next = (int64_t)blockIdx.x * 256 + threadIdx.x, idx = 0;
  bool have = false;
  Trav T;
  T.o = mk(0.f, 0.f, 0.f);
  T.d = mk(0.f, 0.f, 1.f);
  T.tmax = 0.f;
  T.cur = kDone;
  T.sp = 0;
  T.any = 0;
  T.h = HitRec{kInf, kNoPrim, kNoPrim, 0.f, 0.f};
  for (;;) {
    if (T.cur == kDone) {
      if (have) {
        if (any_hit) {
          B.occluded[idx] = T.any == 3u ? 1 : 0;
        } else {
          B.t[idx] = T.h.t;
          B.prim[idx] = T.h.prim;
          B.b1[idx] = T.h.b1;
          B.b2[idx] = T.h.b2;
        }
        have = false;
      }
      if (next < B.n) {
        idx = next;
        next += stride;
        const V3 ro = mk(B.o[3 * idx], B.o[3 * idx + 1], B.o[3 * idx + 2]), rd = mk(B.d[3 * idx], B.d[3 * idx + 1], B.d[3 * idx + 2]);
        const float rt = B.tmax[idx];
        // a probe ray with a non-finite origin / direction or a NaN tmax hits nothing and is not walked (with NaN slabs nothing prunes: such
        // a ray would visit every node of the tree; oracle.cpp probe_ray_is_sane is the same rule) -- the renderer's own rays are finite
        const bool sane = fabsf(ro.x) < kInf && fabsf(ro.y) < kInf && fabsf(ro.z) < kInf && fabsf(rd.x) < kInf && fabsf(rd.y) < kInf && fabsf(rd.z) < kInf && rt == rt;
        if (sane) {
          trav_begin<COUNT>(S, T, stk, ro, rd, rt, any_hit != 0, cn);
        } else {  // the miss is written when the loop comes round
          T.o = mk(0.f, 0.f, 0.f);
          T.d = mk(0.f, 0.f, 1.f);
          T.tmax = 0.f;
          T.any = 0;
          T.h = HitRec{kInf, kNoPrim, kNoPrim, 0.f, 0.f};
          T.cur = kDone;
        }
        have = true;
      }
    }
    if (__ballot(have) == 0ull) break;
    trav_run<COUNT, COUNT, (COUNT ? 0u : kIntersectLdsStack), PBRT_STEPS_PER_CHECK, SPH>(S, T, stk, stkt, ovf, have, tune, cn, ct);
  }
  EXP_PROBE_FINI_BLOCK();
  if (COUNT) {
    for (int off = 32; off > 0; off >>= 1) {
      cn += __shfl_down(cn, off, 64);
      ct += __shfl_down(ct, off, 64);
    }
    if (lane == 0) {
      atomicAdd(&B.counters[0], cn);
      atomicAdd(&B.counters[1], ct);
    }
  }
}

// n_prims = n_tris + the spheres: primitive t >= n_tris is sphere t - n_tris (its place in the vertex / index buffers is taken by a
// degenerate proxy triangle spanning its box, so that every builder bounds it: scene_inputs.hpp) and gets a sphere's record
__global__ void pack_tris_kernel(const float *P, const uint32_t *idx, const uint16_t *mat_id, const uint32_t *order,
                                 uint32_t n_prims, uint32_t n_tris, const float4 *spheres, float4 *tris) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_prims) return;
  const uint32_t t = order[slot];
  if (t >= n_tris) {
    const float4 cr = spheres[kSphereRows * (t - n_tris)], m = spheres[kSphereRows * (t - n_tris) + 1u];
    tris[kTriStride * slot] = make_float4(cr.x, cr.y, cr.z, __uint_as_float(t));
    tris[kTriStride * slot + 1] = make_float4(cr.w, 0.f, 0.f, m.x);
    tris[kTriStride * slot + 2] = make_float4(0.f, 0.f, 0.f, __uint_as_float(1u));
    return;
  }
  const uint32_t i0 = idx[3 * t], i1 = idx[3 * t + 1], i2 = idx[3 * t + 2];
  tris[kTriStride * slot] = make_float4(P[3 * i0], P[3 * i0 + 1], P[3 * i0 + 2], __uint_as_float(t));
  tris[kTriStride * slot + 1] = make_float4(P[3 * i1], P[3 * i1 + 1], P[3 * i1 + 2], __uint_as_float((uint32_t)mat_id[t]));
  tris[kTriStride * slot + 2] = make_float4(P[3 * i2], P[3 * i2 + 1], P[3 * i2 + 2], 0.f);
}

// corner (u, v) of the triangle in leaf slot `slot` (textured scenes: DESIGN.md 3.15)
__global__ void pack_uv_kernel(const float *tri_uv, const uint32_t *order, uint32_t n_prims, uint32_t n_tris, float2 *out) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_prims) return;
  const uint32_t t = order[slot];
  for (int v = 0; v < 3; v++) out[3u * slot + v] = t < n_tris ? make_float2(tri_uv[6 * (size_t)t + 2 * v], tri_uv[6 * (size_t)t + 2 * v + 1]) : make_float2(0.f, 0.f);  // (a sphere has its own (u, v))
}

__global__ void assemble_kernel(const float4 *slab, float4 *film, int32_t w, int32_t h, uint32_t rank, uint32_t world,
                                uint32_t n_local_super) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_local_super * 4096u) return;
  const uint32_t j = i >> 12, pys = (i >> 6) & 63u, pxs = i & 63u;
  const uint32_t stx = (uint32_t)(w + 63) >> 6;
  const uint32_t t = rank + j * world;
  const int32_t x = (int32_t)((t % stx) * 64u + pxs), y = (int32_t)((t / stx) * 64u + pys);
  if (x < w && y < h) film[(size_t)y * w + x] = slab[i];
}

// Film::merge_film_tile (core/film.rs:313-326) for one pixel of a rank's slab: contrib_sum = the K = 2^kb partial sums of
// its chunks added in chunk order, xyz = rgb_to_xyz(contrib_sum) (spectrum.rs:139-145), weight = spp.
// (rank, world, n_local_super) are those of the LAUNCH that wrote `partials`: a frame rendered in P passes (capi_render.cpp partials_passes) hands the
// rank's super-tiles j = pass + P * j' to pass `pass`, which is rank + world * pass of world * P; its tile j' lands at slab tile j0 + jstride * j'.
__global__ void merge_kernel(const float4 *partials, float4 *slab, int32_t w, int32_t h, uint32_t rank, uint32_t world,
                             uint32_t n_local_super, float weight, uint32_t kb, uint32_t j0, uint32_t jstride) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_local_super * 4096u) return;
  const uint32_t j = i >> 12, pys = (i >> 6) & 63u, pxs = i & 63u;
  const uint32_t stx = (uint32_t)(w + 63) >> 6;
  const uint32_t t = rank + j * world;
  const int32_t x = (int32_t)((t % stx) * 64u + pxs), y = (int32_t)((t / stx) * 64u + pys);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (x < w && y < h) {  // (pixels of a ragged super-tile outside the image were never rendered)
    V3 sum = {0.f, 0.f, 0.f};
    for (uint32_t c = 0; c < (1u << kb); c++) {
      const float4 p = partials[((size_t)i << kb) + c];
      sum = sum + mk(p.x, p.y, p.z);
    }
    const Xyz c = rgb_to_xyz(sum.x, sum.y, sum.z);
    o.x = c.x;
    o.y = c.y;
    o.z = c.z;
    o.w = weight;
  }
  slab[((size_t)(j0 + jstride * j) << 12) + (i & 4095u)] = o;
}

// fixed-point accumulators {r, g, b, samples} -> Film pixel {XYZ of the radiance sum, weight} (film.rs:313-326)
__global__ void film_from_acc_kernel(const unsigned long long *acc, float4 *film, size_t n_px) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_px) return;
  const float inv = 1.0f / kFixedOne;
  const V3 sum = {(float)(long long)acc[4 * i] * inv, (float)(long long)acc[4 * i + 1] * inv, (float)(long long)acc[4 * i + 2] * inv};
  float4 o;
  const Xyz c = rgb_to_xyz(sum.x, sum.y, sum.z);
  o.x = c.x;
  o.y = c.y;
  o.z = c.z;
  o.w = (float)(long long)acc[4 * i + 3];
  film[i] = o;
}

// the same for a weighted pixel filter's accumulators {r, g, b, weight sum}, all four in 2^-24 units.  A kernel of its own:
// film_from_acc_kernel keeps its arguments and its machine code.
__global__ void film_from_acc_weighted_kernel(const unsigned long long *acc, float4 *film, size_t n_px) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_px) return;
  const float inv = 1.0f / kFixedOne;
  const V3 sum = {(float)(long long)acc[4 * i] * inv, (float)(long long)acc[4 * i + 1] * inv, (float)(long long)acc[4 * i + 2] * inv};
  float4 o;
  const Xyz c = rgb_to_xyz(sum.x, sum.y, sum.z);
  o.x = c.x;
  o.y = c.y;
  o.z = c.z;
  o.w = (float)(long long)acc[4 * i + 3] * inv;
  film[i] = o;
}

}  // namespace

// the fixed-point accumulators of two ranks on one device added (multi_gpu.cpp's loopback exchange; with one rank per device ncclReduce adds them)
__global__ void acc_add_kernel(unsigned long long *dst, const unsigned long long *src, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] += src[i];
}
hipError_t launch_acc_add(unsigned long long *dst, const unsigned long long *src, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(acc_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dst, src, n);
  return hipGetLastError();
}

hipError_t launch_film_from_acc(const unsigned long long *acc, float4 *film, size_t n_px, bool weighted, hipStream_t stream) {
  if (n_px == 0) return hipSuccess;
  hipLaunchKernelGGL(weighted ? film_from_acc_weighted_kernel : film_from_acc_kernel, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, stream, acc, film, n_px);
  return hipGetLastError();
}

// RenderLaunch -> the family's launcher and the instantiation; everything else was decided by capi_render.cpp render_launch, and which
// instantiations exist by render_variant.hpp.  The production walk's STACK is the LDS rows of the overflow variant, or 0 for the whole
// stack in LDS; the exact walk's is its stack rows.
hipError_t launch_render(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t st) {
  if (R.n_items == 0) return hipSuccess;
  const RenderVariant &V = L.variant;
  switch (L.family) {
    case RenderFamily::kN: return launch_render_n(S, R, L, st);
    case RenderFamily::kEnv: return launch_render_env(S, R, L, st);
    case RenderFamily::kX: return launch_render_x(S, R, L, st);
    case RenderFamily::kDefault: break;
    default: return hipErrorInvalidValue;
  }
  auto go = [&](void (*kernel)(DevScene, RenderParams)) {
    hipLaunchKernelGGL(kernel, dim3(L.n_workgroups), dim3(64), L.lds_bytes, st, S, R);
    return hipGetLastError();
  };
  if (V.counters == kCountExact)
    return with_bools([&](auto SPH) {
      switch (L.exact_rows) {
        case 20: return go(render_kernel<SPH, true, true, 20>);
        case 26: return go(render_kernel<SPH, true, true, 26>);
        case 32: return go(render_kernel<SPH, true, true, 32>);
        case 40: return go(render_kernel<SPH, true, true, 40>);
        case 64: return go(render_kernel<SPH, true, true, 64>);
      }
      return hipErrorInvalidValue;
    }, V.spheres);
  // (ray log / phase probe builds wrap the plain default path's launch: experiments.inc)
  const bool experiment = kExperimentLaunch && render_default_path(V);
  hipError_t e = hipSuccess;
  if (experiment && experiment_launch_begin(&e)) return e;
  e = with_bools([&](auto SPH, auto OVF, auto COUNT, auto SND, auto WIDE) {
    constexpr int STACK = OVF ? (int)kQuadLdsStackOvf : 0;
    constexpr RenderVariant v = default_variant(SPH, COUNT, false, WIDE, SND);
    if constexpr (render_default_path(v) && STACK == 0) {  // (the one launch with a choice of STEPS: capi_render.cpp render_launch)
      return go(L.steps == 2 ? render_kernel<SPH, false, false, 0, 2> : render_kernel<SPH, false, false, 0>);
    } else if constexpr (render_family_builds(RenderFamily::kDefault, v)) {
      return go(render_kernel<SPH, COUNT, false, STACK, PBRT_STEPS_PER_CHECK, WIDE, SND>);
    }
    return hipErrorInvalidValue;
  }, V.spheres, L.plan.overflow, V.counters == kCountWalk, V.table_sampler, V.wide);
  if (experiment) experiment_launch_end(st);
  return e;
}

hipError_t launch_intersect(const DevScene &S, const RayBatch &B, bool any_hit, uint32_t bvh_depth, hipStream_t st) {
  if (B.n == 0) return hipSuccess;
  const dim3 grid(intersect_workgroups(B.n)), block(64 * kIntersectWavesPerWorkgroup);
  const hipError_t e = with_bools([&](auto SPH, auto COUNT) {
    hipLaunchKernelGGL((bvh_depth <= 32 ? intersect_kernel<SPH, COUNT, 32> : intersect_kernel<SPH, COUNT, 64>), grid, block, 0, st, S, B, any_hit ? 1 : 0);
    return hipGetLastError();
  }, S.n_spheres > 0, B.counters != nullptr);
  if (kExperimentLaunch) experiment_launch_end(st);
  return e;
}

hipError_t launch_pack_tris(const float *P, const uint32_t *idx, const uint16_t *mat_id, const uint32_t *order,
                            uint32_t n_prims, uint32_t n_tris, const float4 *spheres, float4 *tris, hipStream_t stream) {
  if (n_prims == 0) return hipSuccess;
  hipLaunchKernelGGL(pack_tris_kernel, dim3((n_prims + 255) / 256), dim3(256), 0, stream, P, idx, mat_id, order, n_prims, n_tris, spheres,
                     tris);
  return hipGetLastError();
}

hipError_t launch_pack_uv(const float *tri_uv, const uint32_t *order, uint32_t n_prims, uint32_t n_tris, float2 *out, hipStream_t stream) {
  if (n_prims == 0) return hipSuccess;
  hipLaunchKernelGGL(pack_uv_kernel, dim3((n_prims + 255) / 256), dim3(256), 0, stream, tri_uv, order, n_prims, n_tris, out);
  return hipGetLastError();
}

hipError_t launch_merge(const float4 *partials, float4 *slab, int32_t w, int32_t h, uint32_t rank, uint32_t world,
                        uint32_t n_local_super, uint32_t spp, hipStream_t stream, uint32_t j0, uint32_t jstride) {
  if (n_local_super == 0) return hipSuccess;
  const uint32_t n = n_local_super * 4096u;
  hipLaunchKernelGGL(merge_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, partials, slab, w, h, rank, world, n_local_super,
                     (float)spp, sample_chunk_shift(spp), j0, jstride);
  return hipGetLastError();
}

hipError_t launch_assemble(const float4 *slab, float4 *film, int32_t w, int32_t h, uint32_t rank, uint32_t world,
                           uint32_t n_local_super, hipStream_t stream) {
  if (n_local_super == 0) return hipSuccess;
  const uint32_t n = n_local_super * 4096u;
  hipLaunchKernelGGL(assemble_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, slab, film, w, h, rank, world,
                     n_local_super);
  return hipGetLastError();
}

}  // namespace pbrt_hip
