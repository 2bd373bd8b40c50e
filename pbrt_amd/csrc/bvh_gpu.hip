// BVH construction on the device, three stages:
//   1. the host builder's algorithm -- top-down binned SAH (centre bounds -> widest axis -> 16 buckets -> plane of
//      least n_l A_l + n_r A_r) -- run LEVEL-SYNCHRONOUSLY over the Morton-sorted triangles (every segment of a level is split by
//      the same launches), down to leaves of one triangle;
//   2. the built tree OPTIMISED by parallel re-insertion (reinsert_core.hpp: every node looks for the position that lowers the
//      summed surface area most, conflicting moves are dropped, boxes refitted; up to 12 passes): 4.5 % fewer node fetches per ray
//      on BASELINE C3, 6.5 % on C2;
//   3. the dynamic-programming collapse into the quantised 4-wide nodes the production walk reads (its rules and
//      the record: quad_encode.hpp, which the host builder of quad_nodes.cpp calls too).
// On the host a function per stage (sah_build, reinsert, collapse, below the kernels): each owns its scratch as typed DevBufs
// (dev_buf.hpp) and they hand on one BinaryTree; gpu_build_quads checks its arguments, times and calls them.
// 0.13 s for 1M triangles (34 ms without stage 2: PBRT_HIP_SCENE_PLAIN_TREE) against the host's second.  Round 1's LBVH and PLOC
// builders are records now (tools/experiments/r01_lbvh_ploc_builders.hip.txt).
// The reference has no accelerator at all (core/api.rs:237 is a name), so there is nothing to conform to but the RESULT:
// by the tie rule of DESIGN.md 3.4 a ray's hit does not depend on the shape of the tree, so a scene built here renders
// the same film, bit for bit, as one built by the host's SAH builder (tests/test_gpu_parity.py::test_gpu_built_scene_*).
// The canonical counters (the oracle's walk of ITS tree) of such a scene come from the oracle's tree, built on the host
// the first time they are asked for (capi_scene.cpp ensure_canonical).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>  // (rocPRIM directly: hipCUB is its CUDA-compatibility face)
#include <rocprim/device/device_scan.hpp>

#include "build_stages.hpp"
#include "dev_buf.hpp"
#include "device_types.h"
#include "quad_encode.hpp"
#include "quad_nodes.hpp"
#include "reinsert_core.hpp"

namespace pbrt_hip {
namespace {

constexpr uint32_t kNone = 0xffffffffu;

__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__device__ __forceinline__ void tri_box(const float *P, const uint32_t *idx, uint32_t t, float lo[3], float hi[3]) {
  const uint32_t i0 = idx[3 * (size_t)t], i1 = idx[3 * (size_t)t + 1], i2 = idx[3 * (size_t)t + 2];
  for (int a = 0; a < 3; a++) {
    const float v0 = P[3 * (size_t)i0 + a], v1 = P[3 * (size_t)i1 + a], v2 = P[3 * (size_t)i2 + a];
    lo[a] = fminf(v0, fminf(v1, v2));
    hi[a] = fmaxf(v0, fmaxf(v1, v2));
  }
}

// A node's box as three 64-bit words {lo.x lo.y}{lo.z hi.x}{hi.y hi.z}: the bottom-up fit reads a sibling's box with
// three device-scope atomic loads (a box another CU has just written must not come from this CU's L1).
__device__ __forceinline__ unsigned long long pack2(float a, float b) {
  return (unsigned long long)__float_as_uint(a) | ((unsigned long long)__float_as_uint(b) << 32);
}
__device__ __forceinline__ void box_store(unsigned long long *bx, uint32_t id, const float lo[3], const float hi[3]) {
  bx[3 * (size_t)id] = pack2(lo[0], lo[1]);
  bx[3 * (size_t)id + 1] = pack2(lo[2], hi[0]);
  bx[3 * (size_t)id + 2] = pack2(hi[1], hi[2]);
}
template <bool COHERENT>
__device__ __forceinline__ void box_load(const unsigned long long *bx, uint32_t id, float lo[3], float hi[3]) {
  unsigned long long w[3];
  for (int k = 0; k < 3; k++)
    w[k] = COHERENT ? __hip_atomic_load(&bx[3 * (size_t)id + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : bx[3 * (size_t)id + k];
  lo[0] = __uint_as_float((uint32_t)w[0]); lo[1] = __uint_as_float((uint32_t)(w[0] >> 32));
  lo[2] = __uint_as_float((uint32_t)w[1]); hi[0] = __uint_as_float((uint32_t)(w[1] >> 32));
  hi[1] = __uint_as_float((uint32_t)w[2]); hi[2] = __uint_as_float((uint32_t)(w[2] >> 32));
}

// bounds[0..2] = min, bounds[3..5] = max of the triangle-box centres, as order-preserving integers
__global__ void centroid_bounds_kernel(const float *P, const uint32_t *idx, uint32_t n, uint32_t *bounds) {
  __shared__ uint32_t red[6];
  if (threadIdx.x < 6) red[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
  __syncthreads();
  // a few triangles per thread, then wave, then block: 6 global atomics per 2048 triangles
  float c[3];
  uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  for (uint32_t t = blockIdx.x * blockDim.x * 8u + threadIdx.x, k = 0; k < 8u; k++, t += blockDim.x) {
    if (t >= n) break;
    float lo[3], hi[3];
    tri_box(P, idx, t, lo, hi);
    for (int a = 0; a < 3; a++) {
      c[a] = 0.5f * lo[a] + 0.5f * hi[a];
      mn[a] = min(mn[a], f2ord(c[a]));
      mx[a] = max(mx[a], f2ord(c[a]));
    }
  }
  for (int a = 0; a < 3; a++) {
    for (int off = 32; off > 0; off >>= 1) {
      mn[a] = min(mn[a], (uint32_t)__shfl_down(mn[a], off, 64));
      mx[a] = max(mx[a], (uint32_t)__shfl_down(mx[a], off, 64));
    }
    if ((threadIdx.x & 63u) == 0u) {
      atomicMin(&red[a], mn[a]);
      atomicMax(&red[3 + a], mx[a]);
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(&bounds[threadIdx.x], red[threadIdx.x]);
  else if (threadIdx.x < 6) atomicMax(&bounds[threadIdx.x], red[threadIdx.x]);
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {  // 10 bits -> every third bit
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

__global__ void morton_kernel(const float *P, const uint32_t *idx, uint32_t n, const uint32_t *bounds, uint32_t *keys, uint32_t *vals) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  float lo[3], hi[3];
  tri_box(P, idx, t, lo, hi);
  uint32_t q[3];
  for (int a = 0; a < 3; a++) {
    const float mn = ord2f(bounds[a]), mx = ord2f(bounds[3 + a]);
    const float c = 0.5f * lo[a] + 0.5f * hi[a];
    const float ext = mx - mn;
    float u = ext > 0.f ? (c - mn) / ext : 0.f;
    u = fminf(fmaxf(u * 1024.f, 0.f), 1023.f);
    q[a] = (uint32_t)u;
  }
  keys[t] = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
  vals[t] = t;
}

__device__ __forceinline__ uint32_t node_of(uint32_t ref, int n) { return (ref & kLeafRef) ? (uint32_t)(n - 1) + (ref & ~kLeafRef) : ref; }

// ---- top-down binned SAH, level-synchronous (the host builder's split rule, DESIGN.md 3.3, on the device) ----
// The triangles (in Morton order to start with) form SEGMENTS of the position array; every level every segment of two
// or more triangles is split: bounds of the triangle-box centres -> widest axis -> 16 buckets with counts and boxes ->
// the plane of least n_l * A_l + n_r * A_r (planes with an empty side excluded) -> a stable partition (one global prefix
// sum of the "goes left" flags).  No plane (all centres in one bucket), or a level past kSahMedianLevel: the segment is
// halved as it stands.  Leaves hold one triangle.  Node ids: the root is 0, the segments of the next level get
// consecutive ids in segment order, so the numbering is deterministic.  Per-segment sums go through atomics, aggregated in
// LDS when a whole block lies in one segment (the top levels).
#ifndef PBRT_SAH_BUCKETS
#define PBRT_SAH_BUCKETS 16
#endif
constexpr int kSahBuckets = PBRT_SAH_BUCKETS;
constexpr uint32_t kSahMedianLevel = 40;  // beyond this level only halving: bounds the depth at ~ 40 + log2(n)
constexpr uint32_t kBinWords = kSahBuckets * 7;  // per bucket: count, box lo xyz, hi xyz (order-preserving integers)

struct SahSegs {  // one level's segment table (structure of arrays; capacity n / 2 + 1)
  uint32_t *start, *end, *node;
};
struct SahSplit {
  uint32_t axis, best, nl, mode;  // mode 0: bucket <= best goes left; 1: position < start + nl goes left
  float c0, scale;                // bucket = min(15, (int)((c - c0) * scale))
};

__global__ void sah_tri_boxes_kernel(const float *P, const uint32_t *idx, uint32_t n, float *tlo, float *thi) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  float lo[3], hi[3];
  tri_box(P, idx, t, lo, hi);
  for (int a = 0; a < 3; a++) { tlo[3 * (size_t)t + a] = lo[a]; thi[3 * (size_t)t + a] = hi[a]; }
}

// centre bounds of every active segment: cb[s][0..2] = min, [3..5] = max (order-preserving integers, preset to ~0 / 0)
__global__ void __launch_bounds__(256) sah_bounds_kernel(const uint32_t *ids, const uint32_t *seg_of, int n, const float *tlo, const float *thi, uint32_t *cb) {
  __shared__ uint32_t red[6];
  __shared__ uint32_t s_first, s_last;
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (threadIdx.x == 0) { s_first = seg_of[blockIdx.x * 256]; s_last = seg_of[min((int)(blockIdx.x * 256 + 255), n - 1)]; }
  if (threadIdx.x < 6) red[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
  __syncthreads();
  const bool uniform = s_first == s_last && s_first != kNone;  // segments are contiguous: the whole block is in one
  const uint32_t s = i < n ? seg_of[i] : kNone;
  if (s != kNone) {
    const uint32_t t = ids[i];
    for (int a = 0; a < 3; a++) {
      const uint32_t c = f2ord(0.5f * tlo[3 * (size_t)t + a] + 0.5f * thi[3 * (size_t)t + a]);
      if (uniform) { atomicMin(&red[a], c); atomicMax(&red[3 + a], c); }
      else { atomicMin(&cb[6 * (size_t)s + a], c); atomicMax(&cb[6 * (size_t)s + 3 + a], c); }
    }
  }
  if (uniform) {
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&cb[6 * (size_t)s_first + threadIdx.x], red[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&cb[6 * (size_t)s_first + threadIdx.x], red[threadIdx.x]);
  }
}

__device__ __forceinline__ uint32_t sah_bucket(float c, float c0, float scale) {
  const int b = (int)((c - c0) * scale);
  return (uint32_t)(b < 0 ? 0 : (b >= kSahBuckets ? kSahBuckets - 1 : b));
}

// widest axis of the centre bounds and the bucket scale of every segment
__global__ void sah_prepare_kernel(int n_seg, const uint32_t *cb, SahSplit *sp) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n_seg) return;
  float ext[3], mn[3];
  for (int a = 0; a < 3; a++) { mn[a] = ord2f(cb[6 * (size_t)s + a]); ext[a] = ord2f(cb[6 * (size_t)s + 3 + a]) - mn[a]; }
  const int axis = (ext[0] > ext[1] && ext[0] > ext[2]) ? 0 : (ext[1] > ext[2] ? 1 : 2);
  SahSplit o;
  o.axis = (uint32_t)axis;
  o.c0 = mn[axis];
  o.scale = ext[axis] > 0.f ? (float)kSahBuckets / ext[axis] : 0.f;
  o.best = 0; o.nl = 0; o.mode = 1;
  sp[s] = o;
}

// bucket counts and boxes of every segment (bins preset: count 0, lo ~0, hi 0)
__global__ void __launch_bounds__(256) sah_bins_kernel(const uint32_t *ids, const uint32_t *seg_of, int n, const float *tlo, const float *thi, const SahSplit *sp,
                                                       uint32_t *bins) {
  __shared__ uint32_t lb[kBinWords];
  __shared__ uint32_t s_first, s_last;
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (threadIdx.x == 0) { s_first = seg_of[blockIdx.x * 256]; s_last = seg_of[min((int)(blockIdx.x * 256 + 255), n - 1)]; }
  if (threadIdx.x < kBinWords) lb[threadIdx.x] = (threadIdx.x % 7u == 0u || threadIdx.x % 7u > 3u) ? 0u : 0xffffffffu;
  __syncthreads();
  const bool uniform = s_first == s_last && s_first != kNone;
  const uint32_t s = i < n ? seg_of[i] : kNone;
  if (s != kNone) {
    const uint32_t t = ids[i];
    const SahSplit p = sp[s];
    const float c = 0.5f * tlo[3 * (size_t)t + p.axis] + 0.5f * thi[3 * (size_t)t + p.axis];
    const uint32_t b = sah_bucket(c, p.c0, p.scale);
    uint32_t *dst = uniform ? &lb[7u * b] : &bins[(size_t)s * kBinWords + 7u * b];
    atomicAdd(&dst[0], 1u);
    for (int a = 0; a < 3; a++) {
      atomicMin(&dst[1 + a], f2ord(tlo[3 * (size_t)t + a]));
      atomicMax(&dst[4 + a], f2ord(thi[3 * (size_t)t + a]));
    }
  }
  if (uniform) {
    __syncthreads();
    if (threadIdx.x < kBinWords) {
      uint32_t *dst = &bins[(size_t)s_first * kBinWords + threadIdx.x];
      const uint32_t k = threadIdx.x % 7u, v = lb[threadIdx.x];
      if (k == 0u) { if (v) atomicAdd(dst, v); }
      else if (k <= 3u) atomicMin(dst, v);
      else atomicMax(dst, v);
    }
  }
}

// the split of every segment: its own box (union of the buckets) goes to bx[node]; active[s] = children of >= 2 triangles
__global__ void sah_split_kernel(int n_seg, SahSegs segs, const uint32_t *bins, SahSplit *sp, uint32_t level, unsigned long long *bx, uint32_t *active) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n_seg) return;
  const uint32_t *b = bins + (size_t)s * kBinWords;
  const uint32_t n = segs.end[s] - segs.start[s];
  uint32_t cnt[kSahBuckets];
  float lo[kSahBuckets][3], hi[kSahBuckets][3];
  float all_lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()}, all_hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
  for (int k = 0; k < kSahBuckets; k++) {
    cnt[k] = b[7 * k];
    for (int a = 0; a < 3; a++) {
      lo[k][a] = ord2f(b[7 * k + 1 + a]);
      hi[k][a] = ord2f(b[7 * k + 4 + a]);
      if (cnt[k]) { all_lo[a] = fminf(all_lo[a], lo[k][a]); all_hi[a] = fmaxf(all_hi[a], hi[k][a]); }
    }
  }
  box_store(bx, segs.node[s], all_lo, all_hi);
  // suffix sweep, then prefix sweep over the 15 planes
  float area_r[kSahBuckets];
  uint32_t cnt_r[kSahBuckets];
  {
    float rl[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()}, rh[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    uint32_t c = 0;
    for (int k = kSahBuckets - 1; k >= 1; k--) {
      if (cnt[k]) { for (int a = 0; a < 3; a++) { rl[a] = fminf(rl[a], lo[k][a]); rh[a] = fmaxf(rh[a], hi[k][a]); } c += cnt[k]; }
      const float dx = rh[0] - rl[0], dy = rh[1] - rl[1], dz = rh[2] - rl[2];
      cnt_r[k - 1] = c;
      area_r[k - 1] = c ? (dx * dy + dx * dz) + dy * dz : 0.f;
    }
  }
  SahSplit o = sp[s];
  float best_cost = __builtin_huge_valf();
  int best = -1;
  {
    float ll[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()}, lh[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    uint32_t c = 0;
    for (int k = 0; k < kSahBuckets - 1; k++) {
      if (cnt[k]) { for (int a = 0; a < 3; a++) { ll[a] = fminf(ll[a], lo[k][a]); lh[a] = fmaxf(lh[a], hi[k][a]); } c += cnt[k]; }
      if (c == 0 || cnt_r[k] == 0) continue;  // a plane with an empty side splits nothing
      const float dx = lh[0] - ll[0], dy = lh[1] - ll[1], dz = lh[2] - ll[2];
      const float cost = (float)c * ((dx * dy + dx * dz) + dy * dz) + (float)cnt_r[k] * area_r[k];
      if (cost < best_cost) { best_cost = cost; best = k; o.nl = c; }
    }
  }
  if (best < 0 || level >= kSahMedianLevel) { o.mode = 1; o.nl = n / 2; o.best = 0; }
  else { o.mode = 0; o.best = (uint32_t)best; }
  sp[s] = o;
  active[s] = (o.nl >= 2u ? 1u : 0u) + (n - o.nl >= 2u ? 1u : 0u);
}

__global__ void sah_flags_kernel(const uint32_t *ids, const uint32_t *seg_of, int n, const float *tlo, const float *thi, SahSegs segs, const SahSplit *sp, uint32_t *flags) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const uint32_t s = seg_of[i];
  uint32_t f = 0;
  if (s != kNone) {
    const SahSplit p = sp[s];
    if (p.mode) f = (uint32_t)i < segs.start[s] + p.nl ? 1u : 0u;
    else {
      const uint32_t t = ids[i];
      f = sah_bucket(0.5f * tlo[3 * (size_t)t + p.axis] + 0.5f * thi[3 * (size_t)t + p.axis], p.c0, p.scale) <= p.best ? 1u : 0u;
    }
  }
  flags[i] = f;
}

// stable partition of every segment (scan = exclusive prefix sum of flags over the whole array) and the segment each
// position belongs to on the next level (kNone: a finished leaf)
__global__ void sah_scatter_kernel(const uint32_t *ids, const uint32_t *seg_of, int n, SahSegs segs, const SahSplit *sp, const uint32_t *flags, const uint32_t *scan,
                                   const uint32_t *child_base, uint32_t *ids_out, uint32_t *seg_out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const uint32_t s = seg_of[i];
  if (s == kNone) { ids_out[i] = ids[i]; seg_out[i] = kNone; return; }
  const uint32_t st = segs.start[s], nl = sp[s].nl, nr = segs.end[s] - st - nl;
  const uint32_t left_before = scan[i] - scan[st];
  const bool left = flags[i] != 0u;
  const uint32_t pos = left ? st + left_before : st + nl + ((uint32_t)i - st - left_before);
  ids_out[pos] = ids[i];
  const uint32_t first = child_base[s];  // next level's index of this segment's first active child
  seg_out[pos] = left ? (nl >= 2u ? first : kNone) : (nr >= 2u ? first + (nl >= 2u ? 1u : 0u) : kNone);
}

// the node of every segment gets its two children; the active children become the next level's segments
__global__ void sah_children_kernel(int n_seg, SahSegs segs, const SahSplit *sp, const uint32_t *child_base, uint32_t next_node_base, uint32_t *child, SahSegs next,
                                    uint32_t *parent_internal, uint32_t *parent_leaf) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n_seg) return;
  const uint32_t st = segs.start[s], en = segs.end[s], nl = sp[s].nl, nr = en - st - nl, node = segs.node[s];
  uint32_t j = child_base[s];
  uint32_t left, right;
  if (nl >= 2u) { left = next_node_base + j; next.start[j] = st; next.end[j] = st + nl; next.node[j] = left; j++; }
  else left = kLeafRef | st;
  if (nr >= 2u) { right = next_node_base + j; next.start[j] = st + nl; next.end[j] = en; next.node[j] = right; }
  else right = kLeafRef | (st + nl);
  child[2 * (size_t)node] = left;
  child[2 * (size_t)node + 1] = right;
  // (parents: the collapse's dynamic programme walks the tree bottom-up)
  if (left & kLeafRef) parent_leaf[left & ~kLeafRef] = node; else parent_internal[left] = node;
  if (right & kLeafRef) parent_leaf[right & ~kLeafRef] = node; else parent_internal[right] = node;
  if (node == 0u) parent_internal[0] = kNone;
}

__global__ void sah_leaf_boxes_kernel(const uint32_t *ids, int n, const float *tlo, const float *thi, unsigned long long *bx, uint32_t *order) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= n) return;
  const uint32_t t = ids[k];
  float lo[3], hi[3];
  for (int a = 0; a < 3; a++) { lo[a] = tlo[3 * (size_t)t + a]; hi[a] = thi[3 * (size_t)t + a]; }
  box_store(bx, (uint32_t)(n - 1 + k), lo, hi);
  order[k] = t;
}

// ---- parallel re-insertion over the built binary tree (reinsert_core.hpp has the algorithm and what each phase may touch) ----
// Unified node ids: interior nodes as the builder numbered them, [0, n - 1); the leaf of slot k = (n - 1) + k: the numbering
// of the box array `bx`.
__global__ void ri_links_kernel(int n, const uint32_t *child, uint32_t *par, uint32_t *kid) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n - 1) return;
  for (int k = 0; k < 2; k++) {
    const uint32_t c = child[2 * (size_t)i + k], id = node_of(c, n);
    kid[2 * (size_t)i + k] = id;
    par[id] = (uint32_t)i;
  }
  if (i == 0) par[0] = kNone;
}

// stats: [0] nodes visited by the searches, [1] searches that found a move, [2] moves applied (summed over the passes)
__global__ void __launch_bounds__(256) ri_search_kernel(reins::Tree t, reins::Search sp, uint32_t pass, uint32_t mu, uint32_t *mv_y, uint32_t *mv_lca,
                                                        float *mv_gain, unsigned long long *stats) {
  __shared__ unsigned int s_visits, s_found;
  if (threadIdx.x == 0) { s_visits = 0u; s_found = 0u; }
  __syncthreads();
  const uint32_t x = blockIdx.x * 256u + threadIdx.x, n_nodes = 2u * t.n_int + 1u;
  if (x < n_nodes) {
    reins::Move m;
    m.y = kNone; m.lca = kNone; m.gain = 0.f; m.visits = 0u;
    if ((x + pass) % mu == 0u) m = reins::find_move(t, x, sp);
    mv_y[x] = m.y;
    mv_lca[x] = m.lca;
    mv_gain[x] = m.gain;
    atomicAdd(&s_visits, m.visits);
    if (m.y != kNone) atomicAdd(&s_found, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_visits) atomicAdd(&stats[0], (unsigned long long)s_visits);
    if (s_found) atomicAdd(&stats[1], (unsigned long long)s_found);
  }
}

__global__ void ri_lock_kernel(reins::Tree t, const uint32_t *mv_y, const float *mv_gain, unsigned long long *lock) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2u * t.n_int + 1u || mv_y[x] == kNone) return;
  const unsigned long long key = reins::move_key(x, mv_gain[x]);
  reins::for_move_nodes(t, x, mv_y[x], [&](uint32_t q) { atomicMax(&lock[q], key); });
}

__global__ void ri_hold_kernel(reins::Tree t, const uint32_t *mv_y, const float *mv_gain, const unsigned long long *lock, uint32_t *holds) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2u * t.n_int + 1u) return;
  bool ok = mv_y[x] != kNone;
  if (ok) {
    const unsigned long long key = reins::move_key(x, mv_gain[x]);
    reins::for_move_nodes(t, x, mv_y[x], [&](uint32_t q) { if (lock[q] != key) ok = false; });
  }
  holds[x] = ok ? 1u : 0u;
}

// (a holder on the target's path blocks only with a LARGER key: reinsert_core.hpp target_path_is_free)
__global__ void ri_free_kernel(reins::Tree t, uint32_t *mv_y, const uint32_t *mv_lca, const float *mv_gain, const uint32_t *holds) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2u * t.n_int + 1u || mv_y[x] == kNone) return;
  const unsigned long long key = reins::move_key(x, mv_gain[x]);
  if (!(holds[x] && reins::target_path_is_free(t, x, mv_y[x], mv_lca[x], [&](uint32_t q) { return holds[q] != 0u && reins::move_key(q, mv_gain[q]) > key; })))
    mv_y[x] = kNone;
}

// (mv_from[x] = the grandparent x leaves: with its new parent, the two places whose ancestors' boxes the move changes)
__global__ void __launch_bounds__(256) ri_apply_kernel(reins::Tree t, const uint32_t *mv_y, uint32_t *mv_from, unsigned long long *stats) {
  __shared__ unsigned int s_applied;
  if (threadIdx.x == 0) s_applied = 0u;
  __syncthreads();
  const uint32_t x = blockIdx.x * 256u + threadIdx.x;
  if (x < 2u * t.n_int + 1u && mv_y[x] != kNone) {
    mv_from[x] = t.par[t.par[x]];  // (x's parent and grandparent are among the six nodes whose links this move alone may write)
    reins::apply_move(t, x, mv_y[x]);
    atomicAdd(&s_applied, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_applied) atomicAdd(&stats[2], (unsigned long long)s_applied);
}

// all boxes bottom-up over the links (one thread per leaf climbs; the second thread to reach a node fits it); COUNT: also the
// number of leaves below every interior node
template <bool COUNT, bool BOXES = true>
__global__ void ri_refit_kernel(reins::Tree t, uint32_t *visits, uint32_t *cnt) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > t.n_int) return;
  uint32_t node = t.n_int + k, c = 1u;
  float lo[3], hi[3];
  if (BOXES) box_load<false>(t.bx, node, lo, hi);  // (leaf boxes were written by an earlier launch)
  uint32_t p = t.par[node];
  while (p != kNone) {
    __threadfence();
    if (atomicAdd(&visits[p], 1u) == 0u) return;  // the sibling subtree is not done yet
    __threadfence();
    const uint32_t sib = reins::sibling(t, p, node);
    if (BOXES) {
      float slo[3], shi[3];
      box_load<true>(t.bx, sib, slo, shi);
      for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], slo[a]); hi[a] = fmaxf(hi[a], shi[a]); }
      box_store(t.bx, p, lo, hi);
    }
    if (COUNT) {
      c += sib >= t.n_int ? 1u : __hip_atomic_load(&cnt[sib], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      cnt[p] = c;
    }
    node = p;
    p = t.par[p];
  }
}

// ---- refit of what a pass moved (a pass moves 1.4 % of the nodes, the full refit above was 3/4 of its time) ----
// mark[i], interior node i: bit 31 = some box below i changed (i must be refitted), low bits = children that have arrived.
constexpr uint32_t kDirty = 0x80000000u;
// every applied move dirties the chain above x's new parent (the re-used node p, now y's parent too) and above the grandparent x
// left; a chain that meets a dirty node stops -- whoever dirtied it climbs on
__global__ void ri_mark_kernel(reins::Tree t, const uint32_t *mv_y, const uint32_t *mv_from, uint32_t *mark) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= 2u * t.n_int + 1u || mv_y[x] == kNone) return;
  for (int k = 0; k < 2; k++)
    for (uint32_t q = k ? mv_from[x] : t.par[x]; q != kNone; q = t.par[q])
      if (atomicOr(&mark[q], kDirty) & kDirty) break;
}
// One thread per interior node; the dirty nodes without a dirty child start (their children's boxes are final), fit their box and
// climb; at a parent whose other child is dirty too the first to arrive stops and the second fits (as in ri_refit_kernel).  The
// boxes that result are those of a full refit: a node that is not dirty has nothing changed below it, and min / max are exact.
__global__ void ri_refit_dirty_kernel(reins::Tree t, uint32_t *mark) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.n_int || !(mark[i] & kDirty)) return;
  auto dirty = [&](uint32_t c) { return c < t.n_int && (__hip_atomic_load(&mark[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kDirty) != 0u; };
  uint32_t node = i;
  const uint32_t k0 = t.kid[2 * (size_t)i], k1 = t.kid[2 * (size_t)i + 1];
  if (dirty(k0) || dirty(k1)) return;  // (a thread from below arrives here later)
  float lo[3], hi[3], slo[3], shi[3];
  box_load<false>(t.bx, k0, lo, hi);  // (neither child's box changed in this pass)
  box_load<false>(t.bx, k1, slo, shi);
  for (;;) {
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], slo[a]); hi[a] = fmaxf(hi[a], shi[a]); }
    box_store(t.bx, node, lo, hi);  // (lo, hi) stays in registers: the parent is fitted from it and the sibling's box
    const uint32_t p = t.par[node];
    if (p == kNone) return;
    const uint32_t sib = reins::sibling(t, p, node);
    if (dirty(sib)) {
      // the sibling's subtree is being refitted too: the first to arrive has published its box and stops, the second reads it
      __threadfence();
      if ((atomicAdd(&mark[p], 1u) & ~kDirty) == 0u) return;
      __threadfence();
      box_load<true>(t.bx, sib, slo, shi);
    } else {
      box_load<false>(t.bx, sib, slo, shi);  // (untouched by this pass: no ordering to establish, a chain of one thread)
    }
    node = p;
  }
}
// The summed (half) surface area of the interior nodes in fixed point -- integers add up to the same sum in any order --, units of
// 2^-se with the root's area below 2^40 units (find_move's scale): out[0] += the sum, out[1] = se + 1024.
__global__ void __launch_bounds__(256) ri_cost_kernel(reins::Tree t, unsigned long long *out) {
  __shared__ unsigned long long s_sum[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  int se = 0;
  (void)frexpf(reins::area(reins::load_box(t, 0u)), &se);
  se = 40 - se;
  se = se > 100 ? 100 : (se < -100 ? -100 : se);
  unsigned long long v = i < t.n_int ? (unsigned long long)(reins::area(reins::load_box(t, i)) * ldexpf(1.0f, se)) : 0ull;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0u) {
    const unsigned long long b = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    if (b) atomicAdd(&out[0], b);
  }
  if (i == 0u) out[1] = (unsigned long long)(se + 1024);
}

__global__ void ri_order_kernel(reins::Tree t) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < t.n_int) reins::order_children(t, i);
}

// a leaf's position in the depth-first order of the optimised tree = the leaves to its left: the triangle records follow the
// tree again (a moved triangle would otherwise keep its record where the first tree had it)
__global__ void ri_leafpos_kernel(reins::Tree t, const uint32_t *cnt, uint32_t *newslot) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > t.n_int) return;
  uint32_t node = t.n_int + k, pos = 0u;
  for (uint32_t p = t.par[node]; p != kNone; node = p, p = t.par[p]) {
    const uint32_t first = t.kid[2 * (size_t)p];
    if (first != node) pos += first >= t.n_int ? 1u : cnt[first];
  }
  newslot[k] = pos;
}

// back to the builder's own form (child words, parents of interior nodes and of leaf slots) with the new leaf slots
__global__ void ri_emit_kernel(reins::Tree t, const uint32_t *newslot, uint32_t *child, uint32_t *parent_internal, uint32_t *parent_leaf) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.n_int) return;
  for (int k = 0; k < 2; k++) {
    const uint32_t c = t.kid[2 * (size_t)i + k];
    if (c >= t.n_int) {
      const uint32_t s = newslot[c - t.n_int];
      child[2 * (size_t)i + k] = kLeafRef | s;
      parent_leaf[s] = i;
    } else {
      child[2 * (size_t)i + k] = c;
      parent_internal[c] = i;
    }
  }
  if (i == 0u) parent_internal[0] = kNone;
}
__global__ void ri_leaves_kernel(reins::Tree t, const uint32_t *newslot, const uint32_t *order_in, uint32_t *order_out, unsigned long long *leaf_bx_out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > t.n_int) return;
  const uint32_t s = newslot[k];
  order_out[s] = order_in[k];
  for (int w = 0; w < 3; w++) leaf_bx_out[3 * (size_t)s + w] = t.bx[3 * (size_t)(t.n_int + k) + w];
}

// ---- the collapse's dynamic programme (quad_encode.hpp; leaves hold one triangle here) ----
struct DpTables {
  float *F;   // [(4 * node + (k - 1)) * 3 + (d - 1)], internal nodes
  float *Fl;  // [3 * slot + (d - 1)], leaves
  float *G;   // internal nodes
  // F(c, k, d) of child word c, as quad_encode.hpp reads it (a value another CU has just written must not come from this CU's L1)
  __device__ __forceinline__ float operator()(uint32_t c, uint32_t k, uint32_t d) const {
    const float *p = (c & kLeafRef) ? &Fl[3 * (size_t)(c & ~kLeafRef) + (d - 1u)] : &F[(4 * (size_t)c + (k - 1u)) * 3 + (d - 1u)];
    return __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
};
// bottom-up: one thread per leaf climbs; the second thread to reach a node computes it (its children are complete)
__global__ void collapse_dp_kernel(int n, const uint32_t *child, const uint32_t *parent_internal, const uint32_t *parent_leaf, uint32_t *visits,
                                   const unsigned long long *bx, DpTables T) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= n) return;
  float lo[3], hi[3], qlo[3], qhi[3];
  box_load<false>(bx, (uint32_t)(n - 1 + k), lo, hi);  // (leaf boxes were written by an earlier launch)
  uint32_t anc = parent_leaf[k];
  for (uint32_t d = 1; d <= 3; d++) {
    box_load<false>(bx, anc, qlo, qhi);
    T.Fl[3 * (size_t)k + (d - 1u)] = quad::kDpTriCost * quad::area_on_grid(lo, hi, qlo, qhi);
    if (parent_internal[anc] != kNone) anc = parent_internal[anc];
  }
  uint32_t node = parent_leaf[k];
  while (node != kNone) {
    __threadfence();
    if (atomicAdd(&visits[node], 1u) == 0u) return;  // the sibling subtree is not done yet
    __threadfence();
    const uint32_t l = child[2 * (size_t)node], r = child[2 * (size_t)node + 1];
    const float g = quad::dp_dist(T, l, r, 4u, 1u);
    T.G[node] = g;
    box_load<false>(bx, node, lo, hi);
    anc = node;
    for (uint32_t d = 1; d <= 3; d++) {
      if (parent_internal[anc] != kNone) anc = parent_internal[anc];
      box_load<false>(bx, anc, qlo, qhi);
      float f[4];  // one step at the node when reached, plus what lies below -- or opened
      quad::dp_interior(T, l, r, d, quad::area_on_grid(lo, hi, qlo, qhi) + g, f);
      for (uint32_t kk = 1; kk <= 4; kk++) T.F[(4 * (size_t)node + (kk - 1u)) * 3 + (d - 1u)] = f[kk - 1u];
    }
    node = parent_internal[node];
  }
}

struct CollapseItem {
  uint32_t node, quad, path;  // binary internal node, its quad slot, stack entries held above it
};

// One level of the top-down collapse by the rules of quad_encode.hpp: a quad node's children are the ones the dynamic
// programme chose (DP) or the greedy rule picks (leaves hold one triangle here, so only interior children open); their boxes
// go onto the node's own 8-bit grid through the quantiser the host builder uses (quad_nodes.cpp).
// counters: [0] quads allocated, [1] stack need (max); level_count[0] = items of this level, level_count[1] of the next
template <bool DP>
__global__ void collapse_kernel(const CollapseItem *items, uint32_t *level_count, int n, const uint32_t *child, const unsigned long long *bx,
                                uint4 *quads, CollapseItem *next, uint32_t *counters, DpTables T) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= level_count[0]) return;
  const CollapseItem it = items[w];
  struct Kid {
    float lo[3], hi[3];
    uint32_t c;  // child word of the binary tree
  } kids[4];
  int nk = 0;
  auto add = [&](uint32_t c) {
    const uint32_t id = (c & kLeafRef) ? (uint32_t)(n - 1) + (c & ~kLeafRef) : c;
    box_load<false>(bx, id, kids[nk].lo, kids[nk].hi);
    kids[nk].c = c;
    nk++;
  };
  if (DP) {
    // follow the programme's minimising choices: node c with k slots at distance d is opened or presented as one child
    struct Open { uint32_t c, k, d; } st[8];
    int ns = 0;
    auto split = [&](uint32_t c, uint32_t k, uint32_t d) {  // the children of c share k slots at distance d
      const uint32_t l = child[2 * (size_t)c], r = child[2 * (size_t)c + 1], kl = quad::dp_best_split(T, l, r, k, d);
      st[ns++] = Open{r, k - kl, d};
      st[ns++] = Open{l, kl, d};
    };
    split(it.node, 4u, 1u);
    while (ns > 0) {
      const Open o = st[--ns];
      if (!(o.c & kLeafRef) && quad::dp_opens(T, o.c, o.k, o.d)) split(o.c, o.k, o.d + 1u);
      else add(o.c);
    }
  } else {
    add(child[2 * it.node]);
    add(child[2 * it.node + 1]);
    auto grow = [&](int k) { return (kids[k].c & kLeafRef) ? 0u : 1u; };
    for (int best; (best = quad::greedy_pick(kids, nk, grow)) >= 0;) {
      const uint32_t c = kids[best].c;
      kids[best] = kids[--nk];
      add(child[2 * c]);
      add(child[2 * c + 1]);
    }
  }
  const uint32_t path = it.path + (uint32_t)(nk - 1);
  atomicMax(&counters[1], path);
  float me_lo[3], me_hi[3];
  box_load<false>(bx, it.node, me_lo, me_hi);
  const quad::Grid grid = quad::quantise(me_lo, me_hi, kids, nk);
  // the interior children of a node are allocated side by side, as in the host's breadth-first array (one atomic for the
  // node: siblings share 128-byte lines, and a walk that has taken one child usually comes back for the next)
  uint32_t n_int = 0;
  for (int k = 0; k < nk; k++) n_int += (kids[k].c & kLeafRef) ? 0u : 1u;
  uint32_t qi = n_int ? atomicAdd(&counters[0], n_int) : 0u, slot = n_int ? atomicAdd(&level_count[1], n_int) : 0u;
  uint32_t ref[4];
  for (int k = 0; k < 4; k++) {
    if (k >= nk) { ref[k] = kEmptyLeafRef; continue; }
    const uint32_t c = kids[k].c;
    if (c & kLeafRef) {
      ref[k] = quad::leaf_ref(1u, c & ~kLeafRef);  // one triangle, leaf slot = sorted position
    } else {
      ref[k] = quad::interior_ref(qi);
      next[slot++] = CollapseItem{c, qi++, path};
    }
  }
  quad::pack_record(quads + 4 * (size_t)it.quad, me_lo, grid, ref);
}

}  // namespace

// ---- the host side: three stages over typed scratch that its stage owns (dev_buf.hpp; sizes are ELEMENT counts) ----
#define GB_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

namespace {

// Records of more than one word, as the kernels index them; every size and every offset on the host is written with these.
constexpr size_t kBoxWords = 3;                              // a node's box: three 64-bit words (box_store / box_load)
constexpr size_t kCbWords = 6;                               // a segment's centre bounds: min xyz, max xyz (sah_bounds_kernel)
constexpr size_t kBucketWords = kBinWords / kSahBuckets;     // a bucket of a segment's kBinWords of bins: count, box lo xyz, hi xyz
constexpr size_t kDpFWords = 4 * 3, kDpFlWords = 3;          // DpTables: F(k = 1..4, d = 1..3) per interior node, Fl(d) per leaf

template <class T>
hipError_t copy_on_device(T *dst, const T *src, size_t count, hipStream_t stream) {
  return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToDevice, stream);
}
template <class T>
hipError_t zero_on_device(T *p, size_t count, hipStream_t stream) { return hipMemsetAsync(p, 0, count * sizeof(T), stream); }

// rocPRIM's temporary storage.  Never empty: rocPRIM reads a null pointer as "tell me the size" and then does NOTHING, and a DevBuf
// of no elements has p == nullptr.  (Every other buffer here is sized from n >= 2 and cannot be empty.)
hipError_t alloc_rocprim_tmp(DevBuf<char> &tmp, size_t bytes) { return tmp.alloc(std::max<size_t>(bytes, 1)); }

struct Events {  // (destroyed on every exit, early returns of GB_TRY included)
  hipEvent_t a = nullptr, b = nullptr;
  ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  hipError_t create() { GB_TRY(hipEventCreate(&a)); return hipEventCreate(&b); }
};

// The binary tree that passes from stage to stage, n leaves of one triangle each.  Node ids: interior nodes [0, n - 1), the root 0;
// in `boxes` the leaf of slot k follows them as node (n - 1) + k.  The leaf order itself (slot -> triangle) is the caller's d_order.
//                                      written by                                        read by
//   child            [2 n]             sah_build; reinsert (ri_emit_kernel)              reinsert (ri_links_kernel), collapse
//   parent_internal  [n]               sah_build; reinsert (ri_emit_kernel)              collapse (the dynamic programme)
//   parent_leaf      [n]               sah_build; reinsert (ri_emit_kernel)              collapse (the dynamic programme)
//   boxes            [kBoxWords 2 n]   sah_build; reinsert (refits, leaves renumbered)   reinsert, collapse
//   visits           [n]               arrival counters of the bottom-up kernels of reinsert and collapse: zeroed by whoever launches one,
//                                      nothing is handed over in it (it lives here so that the stages share one allocation)
struct BinaryTree {
  int n = 0;
  DevBuf<uint32_t> child, parent_internal, parent_leaf, visits;
  DevBuf<unsigned long long> boxes;
  hipError_t alloc(int n_tris) {
    n = n_tris;
    GB_TRY(child.alloc(2 * (size_t)n));
    GB_TRY(parent_internal.alloc((size_t)n));
    GB_TRY(parent_leaf.alloc((size_t)n));
    GB_TRY(visits.alloc((size_t)n));
    return boxes.alloc(kBoxWords * 2 * (size_t)n);
  }
};

// ---- the observer (build_stages.hpp): copies to the host on the build's stream, for tests that look between the stages ----
template <class T, class U>
hipError_t copy_to_host(std::vector<T> &out, const U *d_src, size_t count, hipStream_t stream) {
  static_assert(sizeof(U) % sizeof(T) == 0, "whole elements");
  out.resize(count * (sizeof(U) / sizeof(T)));
  if (count) GB_TRY(hipMemcpyAsync(out.data(), d_src, count * sizeof(U), hipMemcpyDeviceToHost, stream));
  return hipStreamSynchronize(stream);
}
hipError_t copy_tree_to_host(StageTree &out, const BinaryTree &t, const uint32_t *d_order, hipStream_t stream) {
  const size_t n = (size_t)t.n;
  GB_TRY(copy_to_host(out.child, t.child.p, 2 * (n - 1), stream));
  GB_TRY(copy_to_host(out.parent_internal, t.parent_internal.p, n - 1, stream));
  GB_TRY(copy_to_host(out.parent_leaf, t.parent_leaf.p, n, stream));
  GB_TRY(copy_to_host(out.boxes, t.boxes.p, kBoxWords * (2 * n - 1), stream));  // (a box's three 64-bit words are six floats)
  return copy_to_host(out.order, d_order, n, stream);
}

// Stage 1: Morton keys, the radix sort, and the level-synchronous binned SAH build over the sorted triangles.  Fills `t` and d_order.
hipError_t sah_build(const float *d_P, const uint32_t *d_idx, BinaryTree &t, uint32_t *d_order, hipStream_t stream, GpuBuildStages *obs) {
  const int n = t.n;
  const uint32_t n_tris = (uint32_t)n;
  const dim3 block(256), grid_t((n_tris + 255u) / 256u);
  DevBuf<uint32_t> bounds, keys, keys_out, vals;
  DevBuf<char> sort_tmp;
  GB_TRY(bounds.alloc(kCbWords));
  GB_TRY(keys.alloc((size_t)n));
  GB_TRY(keys_out.alloc((size_t)n));
  GB_TRY(vals.alloc((size_t)n));
  size_t sort_bytes = 0;
  GB_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys.p, keys_out.p, vals.p, d_order, (size_t)n, 0u, 30u, stream));
  GB_TRY(alloc_rocprim_tmp(sort_tmp, sort_bytes));
  const uint32_t init_bounds[kCbWords] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  GB_TRY(hipMemcpyAsync(bounds.p, init_bounds, sizeof(init_bounds), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(centroid_bounds_kernel, dim3((n_tris + 2047u) / 2048u), block, 0, stream, d_P, d_idx, n_tris, bounds.p);
  hipLaunchKernelGGL(morton_kernel, grid_t, block, 0, stream, d_P, d_idx, n_tris, bounds.p, keys.p, vals.p);
  GB_TRY(hipGetLastError());
  GB_TRY(rocprim::radix_sort_pairs(sort_tmp.p, sort_bytes, keys.p, keys_out.p, vals.p, d_order, (size_t)n, 0u, 30u, stream));
  {
    // ---- top-down binned SAH ----
    const size_t cap = (size_t)n / 2 + 2;  // segments of >= 2 triangles on one level
    DevBuf<float> tlo, thi;
    DevBuf<uint32_t> ids_b, seg_a, seg_b, cb, bins, active, cbase, flags, scan, segtab;
    DevBuf<SahSplit> split;
    DevBuf<char> scan_tmp;
    GB_TRY(tlo.alloc(3 * (size_t)n)); GB_TRY(thi.alloc(3 * (size_t)n));
    GB_TRY(ids_b.alloc((size_t)n)); GB_TRY(seg_a.alloc((size_t)n)); GB_TRY(seg_b.alloc((size_t)n));
    GB_TRY(cb.alloc(kCbWords * cap)); GB_TRY(bins.alloc(kBinWords * cap)); GB_TRY(split.alloc(cap));
    GB_TRY(active.alloc(cap)); GB_TRY(cbase.alloc(cap)); GB_TRY(flags.alloc((size_t)n)); GB_TRY(scan.alloc((size_t)n));
    GB_TRY(segtab.alloc(2 * 3 * cap));  // this level's table and the next one's: three arrays each (SahSegs)
    size_t scan_bytes = 0;
    GB_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, flags.p, scan.p, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream));
    GB_TRY(alloc_rocprim_tmp(scan_tmp, scan_bytes));
    SahSegs cur_s{segtab.p, segtab.p + cap, segtab.p + 2 * cap};
    SahSegs nxt_s{segtab.p + 3 * cap, segtab.p + 4 * cap, segtab.p + 5 * cap};
    hipLaunchKernelGGL(sah_tri_boxes_kernel, grid_t, block, 0, stream, d_P, d_idx, n_tris, tlo.p, thi.p);
    // level 0: one segment [0, n) = node 0, triangles in Morton order (d_order holds the sorted ids)
    uint32_t *ids_in = d_order, *ids_out = ids_b.p, *seg_in = seg_a.p, *seg_out = seg_b.p;
    GB_TRY(zero_on_device(seg_in, (size_t)n, stream));
    const uint32_t seg0[3] = {0u, (uint32_t)n, 0u};
    GB_TRY(hipMemcpyAsync(cur_s.start, &seg0[0], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GB_TRY(hipMemcpyAsync(cur_s.end, &seg0[1], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GB_TRY(hipMemcpyAsync(cur_s.node, &seg0[2], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GB_TRY(hipStreamSynchronize(stream));  // (seg0 is a local)
    uint32_t n_seg = 1u, next_node = 1u;
    for (uint32_t level = 0; n_seg > 0u; level++) {
      if (level > 4096u) return hipErrorUnknown;  // (halving past kSahMedianLevel ends every segment long before)
      const dim3 gs((n_seg + 127u) / 128u), b128(128);
      // centre bounds: min words ~0, max words 0 (a strided memset over the second half of every record)
      GB_TRY(hipMemsetAsync(cb.p, 0xff, kCbWords * sizeof(uint32_t) * n_seg, stream));
      GB_TRY(hipMemset2DAsync(cb.p + kCbWords / 2, kCbWords * sizeof(uint32_t), 0, kCbWords / 2 * sizeof(uint32_t), n_seg, stream));
      GB_TRY(zero_on_device(bins.p, kBinWords * (size_t)n_seg, stream));
      hipLaunchKernelGGL(sah_bounds_kernel, grid_t, block, 0, stream, ids_in, seg_in, n, tlo.p, thi.p, cb.p);
      hipLaunchKernelGGL(sah_prepare_kernel, gs, b128, 0, stream, (int)n_seg, cb.p, split.p);
      // bins: counts 0, box lo words (the three behind a bucket's count) ~0 (hi words 0 already)
      GB_TRY(hipMemset2DAsync(bins.p + 1, kBucketWords * sizeof(uint32_t), 0xff, 3 * sizeof(uint32_t), (size_t)n_seg * kSahBuckets, stream));
      hipLaunchKernelGGL(sah_bins_kernel, grid_t, block, 0, stream, ids_in, seg_in, n, tlo.p, thi.p, split.p, bins.p);
      hipLaunchKernelGGL(sah_split_kernel, gs, b128, 0, stream, (int)n_seg, cur_s, bins.p, split.p, level, t.boxes.p, active.p);
      GB_TRY(rocprim::exclusive_scan(scan_tmp.p, scan_bytes, active.p, cbase.p, 0u, (size_t)n_seg, rocprim::plus<uint32_t>(), stream));
      hipLaunchKernelGGL(sah_flags_kernel, grid_t, block, 0, stream, ids_in, seg_in, n, tlo.p, thi.p, cur_s, split.p, flags.p);
      GB_TRY(rocprim::exclusive_scan(scan_tmp.p, scan_bytes, flags.p, scan.p, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream));
      hipLaunchKernelGGL(sah_scatter_kernel, grid_t, block, 0, stream, ids_in, seg_in, n, cur_s, split.p, flags.p, scan.p, cbase.p, ids_out, seg_out);
      hipLaunchKernelGGL(sah_children_kernel, gs, b128, 0, stream, (int)n_seg, cur_s, split.p, cbase.p, next_node, t.child.p, nxt_s,
                         t.parent_internal.p, t.parent_leaf.p);
      GB_TRY(hipGetLastError());
      uint32_t last[2];  // exclusive sum and count of the last segment: the next level's segment count
      GB_TRY(hipMemcpyAsync(&last[0], cbase.p + (n_seg - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      GB_TRY(hipMemcpyAsync(&last[1], active.p + (n_seg - 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      GB_TRY(hipStreamSynchronize(stream));
      n_seg = last[0] + last[1];
      next_node += n_seg;
      std::swap(ids_in, ids_out);
      std::swap(seg_in, seg_out);
      std::swap(cur_s, nxt_s);
    }
    // leaf boxes and the final leaf order (slot k holds triangle ids[k])
    hipLaunchKernelGGL(sah_leaf_boxes_kernel, grid_t, block, 0, stream, ids_in, n, tlo.p, thi.p, t.boxes.p, ids_out);
    if (ids_out != d_order) GB_TRY(copy_on_device(d_order, ids_out, (size_t)n, stream));
    GB_TRY(hipGetLastError());
    GB_TRY(hipStreamSynchronize(stream));  // (the scratch above is freed when this block ends)
  }
  if (obs) {  // (the sort read keys and wrote keys_out: keys is still what morton_kernel left)
    GB_TRY(copy_to_host(obs->morton_keys, keys.p, (size_t)n, stream));
    GB_TRY(copy_tree_to_host(obs->built, t, d_order, stream));
  }
  return hipSuccess;
}

// The debug knobs of stage 2 (PBRT_HIP_GPU_REINSERT, PBRT_HIP_REINSERT_*), read in one place; without them, the defaults of reinsert_core.hpp
struct ReinsertKnobs {
  reins::StopRule stop;  // (shared with the host run of the pass: reinsert_core.hpp)
  int passes = stop.max_passes;
  uint32_t mu = 1;
  reins::Search search;
  bool full_refit = false;  // (A-B: every box every pass, as until round 4)
  // Small trees are left as built: below StopRule::min_tris triangles (where the collapse is the greedy one, too) a walk is a handful
  // of steps in L1 and the surface-area objective decides nothing measurable -- BASELINE C4's 36 triangles rendered 2 % SLOWER with
  // the four moves the pass found (15 quad nodes instead of 19, profiles/r04p5_c4_ab.txt).  The test suite lowers the threshold
  // (tests/conftest.py) so that trees of 8 .. 300 triangles keep exercising the pass.
  uint32_t min_tris = stop.min_tris;
};
ReinsertKnobs read_reinsert_knobs() {
  ReinsertKnobs k;
  if (const char *v = debug_knob("PBRT_HIP_GPU_REINSERT")) k.passes = std::atoi(v);
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_MU")) k.mu = (uint32_t)std::max(1, std::atoi(v));
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_VISITS")) k.search.max_visits = (uint32_t)std::max(1, std::atoi(v));
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_MIN_REL")) k.search.min_rel = (float)std::atof(v);
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_QK")) k.search.qk = (float)std::atof(v);
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_QW")) k.search.qw = (float)std::atof(v);
  k.full_refit = debug_knob("PBRT_HIP_REINSERT_FULL_REFIT") != nullptr;
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_MIN_TRIS")) k.min_tris = (uint32_t)std::max(8, std::atoi(v));
  return k;
}

// Stage 2: parallel re-insertion, the built tree optimised before it is collapsed (reinsert_core.hpp).  `t` and
// d_order come in and go out; `st` says what was done (nothing, for a tree below the threshold).
// Passes of search / lock / check / apply / refit until a pass moves fewer than one node in 1024, `passes` at most, or the
// searches have looked at more than kVisitBudget nodes per node of the tree in total (a mesh of coincident boxes, where
// nothing prunes a search, costs a bounded amount).  The host reads two numbers per pass.
hipError_t reinsert(BinaryTree &t, uint32_t *d_order, ReinsertStats &st, hipStream_t stream, GpuBuildStages *obs) {
  const ReinsertKnobs knobs = read_reinsert_knobs();
  const int n = t.n;
  if ((uint32_t)n < knobs.min_tris || n < 8 || knobs.passes <= 0) return hipSuccess;
  const uint32_t n_int = (uint32_t)n - 1u, n_nodes = 2u * n_int + 1u;
  const dim3 block(256), grid_t(((uint32_t)n + 255u) / 256u), grid_n((n_nodes + 255u) / 256u), grid_i((n_int + 255u) / 256u);
  DevBuf<uint32_t> par, kid, mv_y, mv_lca, holds, cnt, newslot, order2, par_b, kid_b;
  DevBuf<float> mv_gain;
  DevBuf<unsigned long long> lock, stats, leaf_bx, bx_b;
  GB_TRY(par.alloc(n_nodes)); GB_TRY(kid.alloc(2 * (size_t)n_int));
  GB_TRY(mv_y.alloc(n_nodes)); GB_TRY(mv_lca.alloc(n_nodes)); GB_TRY(mv_gain.alloc(n_nodes));
  GB_TRY(lock.alloc(n_nodes)); GB_TRY(holds.alloc(n_nodes)); GB_TRY(stats.alloc(5));
  GB_TRY(cnt.alloc(n_int)); GB_TRY(newslot.alloc((size_t)n)); GB_TRY(order2.alloc((size_t)n)); GB_TRY(leaf_bx.alloc(kBoxWords * (size_t)n));
  // the tree as it stood before the pass in flight (links + interior boxes): a pass that raises the summed area is undone
  GB_TRY(par_b.alloc(n_nodes)); GB_TRY(kid_b.alloc(2 * (size_t)n_int)); GB_TRY(bx_b.alloc(kBoxWords * (size_t)n_int));
  Events ev;
  GB_TRY(ev.create());
  GB_TRY(hipEventRecord(ev.a, stream));
  const reins::Tree rt{n_int, par.p, kid.p, t.boxes.p};
  hipLaunchKernelGGL(ri_links_kernel, grid_i, block, 0, stream, n, t.child.p, par.p, kid.p);
  // stats: [0] visits [1] found [2] applied (summed over the passes); [3] the tree's cost in fixed point, [4] its scale (ri_cost_kernel)
  unsigned long long *const d_cost = stats.p + 3;
  GB_TRY(zero_on_device(stats.p, stats.n, stream));
  hipLaunchKernelGGL(ri_cost_kernel, grid_i, block, 0, stream, rt, d_cost);
  unsigned long long h_stats[5] = {0, 0, 0, 0, 0}, applied_before = 0, cost = 0;
  GB_TRY(hipMemcpyAsync(h_stats, stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, stream));
  GB_TRY(hipStreamSynchronize(stream));
  cost = h_stats[3];
  const double cost_unit = std::ldexp(1.0, -((int)h_stats[4] - 1024));
  st.cost_before = st.cost_after = (double)cost * cost_unit;
  int done = 0;
  for (int pass = 0; pass < knobs.passes; pass++) {
    GB_TRY(copy_on_device(par_b.p, par.p, n_nodes, stream));
    GB_TRY(copy_on_device(kid_b.p, kid.p, 2 * (size_t)n_int, stream));
    GB_TRY(copy_on_device(bx_b.p, t.boxes.p, kBoxWords * (size_t)n_int, stream));
    hipLaunchKernelGGL(ri_search_kernel, grid_n, block, 0, stream, rt, knobs.search, (uint32_t)pass, knobs.mu, mv_y.p, mv_lca.p, mv_gain.p, stats.p);
    GB_TRY(zero_on_device(lock.p, n_nodes, stream));
    hipLaunchKernelGGL(ri_lock_kernel, grid_n, block, 0, stream, rt, mv_y.p, mv_gain.p, lock.p);
    hipLaunchKernelGGL(ri_hold_kernel, grid_n, block, 0, stream, rt, mv_y.p, mv_gain.p, lock.p, holds.p);
    hipLaunchKernelGGL(ri_free_kernel, grid_n, block, 0, stream, rt, mv_y.p, mv_lca.p, mv_gain.p, holds.p);
    // (mv_lca has served: the apply kernel leaves there the grandparent every moved node came from)
    hipLaunchKernelGGL(ri_apply_kernel, grid_n, block, 0, stream, rt, mv_y.p, mv_lca.p, stats.p);
    GB_TRY(zero_on_device(t.visits.p, (size_t)n, stream));
    if (knobs.full_refit) {
      hipLaunchKernelGGL(ri_refit_kernel<false>, grid_t, block, 0, stream, rt, t.visits.p, cnt.p);
    } else {
      hipLaunchKernelGGL(ri_mark_kernel, grid_n, block, 0, stream, rt, mv_y.p, mv_lca.p, t.visits.p);
      hipLaunchKernelGGL(ri_refit_dirty_kernel, grid_i, block, 0, stream, rt, t.visits.p);
    }
    GB_TRY(zero_on_device(d_cost, 1, stream));
    hipLaunchKernelGGL(ri_cost_kernel, grid_i, block, 0, stream, rt, d_cost);
    GB_TRY(hipGetLastError());
    GB_TRY(hipMemcpyAsync(h_stats, stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, stream));
    GB_TRY(hipStreamSynchronize(stream));
    const unsigned long long applied = h_stats[2] - applied_before;
    if (h_stats[3] > cost) {
      // The moves of a pass hold six link nodes each, not their paths, so their gains need not add up: one pass in a
      // thousand or so comes out with MORE summed area than it went in with.  Such a pass is undone and ends the passes.
      GB_TRY(copy_on_device(par.p, par_b.p, n_nodes, stream));
      GB_TRY(copy_on_device(kid.p, kid_b.p, 2 * (size_t)n_int, stream));
      GB_TRY(copy_on_device(t.boxes.p, bx_b.p, kBoxWords * (size_t)n_int, stream));
      h_stats[2] = applied_before;
      st.undone = 1;
      break;
    }
    done = pass + 1;
    cost = h_stats[3];
    applied_before = h_stats[2];
    if (reins::stop_after_pass(knobs.stop, applied, h_stats[0], n_nodes)) break;
  }
  st.cost_after = (double)cost * cost_unit;
  if (obs) {  // the link form as the passes left it (the timing fields are set below)
    obs->reinsert_ran = true;
    GB_TRY(copy_to_host(obs->par, par.p, n_nodes, stream));
    GB_TRY(copy_to_host(obs->kid, kid.p, 2 * (size_t)n_int, stream));
    GB_TRY(copy_to_host(obs->bx, t.boxes.p, kBoxWords * (size_t)n_nodes, stream));
    obs->reinsert = st;
    obs->reinsert.passes = (uint32_t)done;
    obs->reinsert.moves = (uint32_t)std::min<unsigned long long>(h_stats[2], 0xffffffffull);
    obs->visits = h_stats[0];
  }
  // child order, leaf counts, leaves renumbered in depth-first order, and back to the builder's arrays
  hipLaunchKernelGGL(ri_order_kernel, grid_i, block, 0, stream, rt);
  GB_TRY(zero_on_device(t.visits.p, (size_t)n, stream));
  // (the leaves below every node; the boxes are right already -- the last pass refitted what it moved)
  hipLaunchKernelGGL((ri_refit_kernel<true, false>), grid_t, block, 0, stream, rt, t.visits.p, cnt.p);
  hipLaunchKernelGGL(ri_leafpos_kernel, grid_t, block, 0, stream, rt, cnt.p, newslot.p);
  hipLaunchKernelGGL(ri_emit_kernel, grid_i, block, 0, stream, rt, newslot.p, t.child.p, t.parent_internal.p, t.parent_leaf.p);
  hipLaunchKernelGGL(ri_leaves_kernel, grid_t, block, 0, stream, rt, newslot.p, d_order, order2.p, leaf_bx.p);
  GB_TRY(hipGetLastError());
  GB_TRY(copy_on_device(d_order, order2.p, (size_t)n, stream));
  GB_TRY(copy_on_device(t.boxes.p + kBoxWords * (size_t)n_int, leaf_bx.p, kBoxWords * (size_t)n, stream));  // (the leaves follow the interior nodes)
  GB_TRY(hipEventRecord(ev.b, stream));
  GB_TRY(hipStreamSynchronize(stream));  // (the scratch above is freed when this function returns)
  GB_TRY(hipEventElapsedTime(&st.ms, ev.a, ev.b));
  st.passes = (uint32_t)done;
  st.moves = (uint32_t)std::min<unsigned long long>(h_stats[2], 0xffffffffull);
  return hipSuccess;
}

// Stage 3: the top-down collapse into quad nodes, one launch per level of the quad tree.  The host does not know how many items a
// level holds (the kernel reads the count the level above left on the device) nor how deep the tree is: it launches kBatch
// levels blind -- level L holds at most min(4^L, n) items -- and looks at the device once per batch.
// Which descendants become a quad node's children: the host's choice (quad_nodes.cpp collapse_rule: the dynamic programme for
// trees of quad::kDpCollapseMinTris triangles and more, else the greedy largest-area rule); there is no plain rule here.
struct CollapseResult {
  uint32_t n_quads, stack_need, levels;
  float root_box[6];  // {lo.x lo.y lo.z hi.x hi.y hi.z} of the root
};
// Writes d_quads and `out`.  `done` is recorded behind the last read-back, so that the synchronisation which brings the results
// home completes the caller's timing too.
hipError_t collapse(const BinaryTree &t, uint4 *d_quads, hipEvent_t done, CollapseResult &out, hipStream_t stream, GpuBuildStages *obs) {
  const int n = t.n;
  DevBuf<CollapseItem> q0, q1;
  DevBuf<uint32_t> counters, level_counts;
  GB_TRY(q0.alloc((size_t)n));
  GB_TRY(q1.alloc((size_t)n));
  GB_TRY(counters.alloc(2));
  GB_TRY(level_counts.alloc(64));
  const bool use_dp = collapse_rule((uint32_t)n, /*has_plain=*/false) == kCollapseDp;
  DevBuf<float> dpF, dpFl, dpG;
  DpTables dp{nullptr, nullptr, nullptr};
  if (use_dp) {
    GB_TRY(dpF.alloc(kDpFWords * (size_t)n));
    GB_TRY(dpFl.alloc(kDpFlWords * (size_t)n));
    GB_TRY(dpG.alloc((size_t)n));
    dp = DpTables{dpF.p, dpFl.p, dpG.p};
    GB_TRY(zero_on_device(t.visits.p, (size_t)n, stream));
    hipLaunchKernelGGL(collapse_dp_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, stream, n, t.child.p, t.parent_internal.p, t.parent_leaf.p,
                       t.visits.p, t.boxes.p, dp);
    GB_TRY(hipGetLastError());
  }
  const auto kernel = use_dp ? collapse_kernel<true> : collapse_kernel<false>;
  constexpr uint32_t kBatch = 48;
  static_assert(kBatch + 1 <= 64, "level_counts holds a batch's counts and the first count of the next");
  const CollapseItem root{0u, 0u, 0u};  // the binary tree's root, quad 0, nothing on the stack
  GB_TRY(hipMemcpyAsync(q0.p, &root, sizeof(root), hipMemcpyHostToDevice, stream));
  uint32_t h_counters[2] = {1u, 0u};  // quad 0 is the root's
  GB_TRY(hipMemcpyAsync(counters.p, h_counters, sizeof(h_counters), hipMemcpyHostToDevice, stream));
  uint32_t levels = 0;
  CollapseItem *cur = q0.p, *nxt = q1.p;
  for (uint32_t first = 1;;) {  // `first`: items of the batch's first level
    std::vector<uint32_t> zeros(kBatch + 1, 0u);
    zeros[0] = first;
    GB_TRY(hipMemcpyAsync(level_counts.p, zeros.data(), sizeof(uint32_t) * zeros.size(), hipMemcpyHostToDevice, stream));
    GB_TRY(hipStreamSynchronize(stream));  // (zeros is a local)
    uint64_t bound = first;
    for (uint32_t l = 0; l < kBatch; l++) {
      const uint32_t cap = (uint32_t)std::min<uint64_t>(bound, (uint64_t)n);
      hipLaunchKernelGGL(kernel, dim3((cap + 127u) / 128u), dim3(128), 0, stream, cur, level_counts.p + l, n,
                         t.child.p, t.boxes.p, d_quads, nxt, counters.p, dp);
      std::swap(cur, nxt);
      bound = std::min<uint64_t>(bound * 4u, (uint64_t)n);
    }
    GB_TRY(hipGetLastError());
    std::vector<uint32_t> got(kBatch + 1);
    GB_TRY(hipMemcpyAsync(got.data(), level_counts.p, sizeof(uint32_t) * got.size(), hipMemcpyDeviceToHost, stream));
    GB_TRY(hipStreamSynchronize(stream));
    for (uint32_t l = 0; l < kBatch && got[l]; l++) levels++;
    first = got[kBatch];
    if (!first) break;
  }
  GB_TRY(hipMemcpyAsync(h_counters, counters.p, sizeof(h_counters), hipMemcpyDeviceToHost, stream));
  GB_TRY(hipMemcpyAsync(out.root_box, t.boxes.p, sizeof(out.root_box), hipMemcpyDeviceToHost, stream));  // (node 0's kBoxWords words are six floats)
  GB_TRY(hipEventRecord(done, stream));
  GB_TRY(hipStreamSynchronize(stream));  // (h_counters is a local; the scratch above is freed when this function returns)
  out.n_quads = h_counters[0];
  out.stack_need = h_counters[1];
  out.levels = levels;
  if (obs) {
    obs->dp_ran = use_dp;
    if (use_dp) {
      GB_TRY(copy_to_host(obs->F, dpF.p, kDpFWords * ((size_t)n - 1), stream));
      GB_TRY(copy_to_host(obs->Fl, dpFl.p, kDpFlWords * (size_t)n, stream));
      GB_TRY(copy_to_host(obs->G, dpG.p, (size_t)n - 1, stream));
    }
    GB_TRY(copy_to_host(obs->quads, d_quads, 4 * (size_t)out.n_quads, stream));
    obs->n_quads = out.n_quads;
    obs->stack_need = out.stack_need;
  }
  return hipSuccess;
}

}  // namespace

hipError_t gpu_build_quads(const float *d_P, const uint32_t *d_idx, uint32_t n_tris, uint32_t *d_order, uint4 *d_quads,
                           uint32_t quad_capacity, uint32_t flags, GpuBuildInfo *info, hipStream_t stream, GpuBuildStages *stages) {
  if (n_tris < 2u || n_tris > 0x7fffffffu) return hipErrorInvalidValue;  // (the caller builds trees of fewer than two triangles on the host)
  if (quad_capacity + 1u < n_tris) return hipErrorInvalidValue;  // a quad per interior node of the binary tree at most
  BinaryTree tree;
  GB_TRY(tree.alloc((int)n_tris));
  Events ev;
  GB_TRY(ev.create());
  GB_TRY(hipEventRecord(ev.a, stream));
  GB_TRY(sah_build(d_P, d_idx, tree, d_order, stream, stages));
  info->reinsert = ReinsertStats{};
  if (flags & kGpuBuildReinsert) GB_TRY(reinsert(tree, d_order, info->reinsert, stream, stages));
  if (stages) GB_TRY(copy_tree_to_host(stages->optimised, tree, d_order, stream));
  CollapseResult c{};
  GB_TRY(collapse(tree, d_quads, ev.b, c, stream, stages));
  GB_TRY(hipEventElapsedTime(&info->build_ms, ev.a, ev.b));
  info->n_quads = c.n_quads;
  info->stack_need = c.stack_need;
  info->levels = c.levels;
  for (int a = 0; a < 3; a++) { info->root_lo[a] = c.root_box[a]; info->root_hi[a] = c.root_box[3 + a]; }
  return hipSuccess;
}

}  // namespace pbrt_hip
