// quad_encode.hpp -- the 4-wide QUANTISED node of the production walk and the rules that pick a node's
// children, written once for the host builder (quad_nodes.cpp: what the CPU tests and tools/walk_sim.py run) and the device
// builder (bvh_gpu.hip collapse_dp_kernel / collapse_kernel: the product's default).  No STL, no allocation: each side keeps its
// own tree, tables and traversal and calls these for everything that decides a word of a record.
//
// A quad node is a binary interior node collapsed with its interior children (2..4 children); the children's boxes are stored
// as 8-bit coordinates on the node's own grid (origin = the node's lower corner, one power-of-two cell size per axis), rounded
// outwards, so a node with four children is 64 bytes:
//   {origin.x origin.y origin.z  cell.x}                    cell sizes as f32 (powers of two)
//   {qlo.x[4]  qlo.y[4]  qlo.z[4]  qhi.x[4]}               one byte per child
//   {qhi.y[4]  qhi.z[4]  cell.y  cell.z}
//   {ref[4]}                                                interior child: its byte offset in the node array (node x 64);
//                                                           leaf child: kLeafRef | count << 24 | first leaf slot
// plane = origin + q * cell (a real number): the quantiser checks in exact (double) arithmetic that every decoded box contains
// the true one, so the walk visits a superset of the exact walk's nodes and the RESULT is unchanged (tie rule of DESIGN.md 3.4).
// Why: the loop is bound by the bytes it moves from L2 to L1, and this form moves ~2.9 KB per ray instead
// of ~4.9 KB.  Unused child slots: qlo = 255, qhi = 0 (inverted), ref kEmptyLeafRef (a leaf without triangles: device_types.h).
//
// Which descendants become the children?  GREEDY: open the child with the largest surface area while the result fits four
// slots.  DP minimises, by dynamic programming over the binary tree (after Ylitie, Karras, Laine 2017, section 3.2), the expected
// work of a walk: a child of quad node R is reached with the probability of its box AS R's 8-BIT GRID HOLDS IT (about one cell
// of R wider per axis), a reached interior child costs one node step, a reached triangle kDpTriCost.  With R the ancestor at
// binary distance d = 1..3 of node n:
//   F(n, k, d) = least expected work inside subtree n when n may occupy up to k child slots of R
//              = min( present n as ONE child: Aq(n, R) * kDpTriCost * #triangles (a plain leaf), else Aq(n, R) + G(n),
//                     open n (k >= 2, d < 3): min_{k1+k2=k} F(l, k1, d+1) + F(r, k2, d+1) )
//   G(n)       = min_{k1+k2=4} F(l, k1, 1) + F(r, k2, 1), the work below n as a quad node of its own
// (areas are reach probabilities up to the factor 1/A(root), as in the SAH).  Host and device lay F out differently, so the
// rules read it through an accessor F(node, k, d) -> float.  Measured (kDpTriCost = 2): C3 40.2 instead of 41.0 fetches per ray
// but a stack bound of 41 (overflow variant): -1 %; C2 +2 %.  Without the quantisation term: 11.6 % fewer nodes, C3 6 % slower.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_vector_types.h>

#include "device_types.h"

#if defined(__HIPCC__)
#define QE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define QE_HD inline
#endif

namespace pbrt_hip {
namespace quad {

constexpr float kDpTriCost = 2.0f;
// dp for trees of this many triangles and more, greedy below.  Measured (r02f kernel): dp is 2.5 % faster on C3 (433 k instead of
// 488 k nodes), 1.6 % on C2, 3.1 % on the 12 M-triangle workload, 2 % slower on C4's 19-node tree; its build takes a third longer.
constexpr uint32_t kDpCollapseMinTris = 1024;

QE_HD uint32_t f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
QE_HD float min_(float a, float b) { return b < a ? b : a; }

// ---- refs (an interior child's is its byte offset in the node array: no shift in the walk) ----
QE_HD uint32_t leaf_ref(uint32_t n_prims, uint32_t first_slot) { return kLeafRef | (n_prims << 24) | first_slot; }
QE_HD uint32_t interior_ref(uint32_t quad) { return quad * 64u; }
QE_HD uint32_t quad_of_ref(uint32_t interior_ref) { return interior_ref / 64u; }

// ---- the grid: exponent of the smallest power-of-two cell with 255 cells covering the extent ----
QE_HD int cell_exponent(float extent) {
  int e = -126;
  if (extent > 0.f) (void)frexpf(extent / 255.0f, &e);  // extent/255 = m * 2^e, m in [0.5, 1)  =>  2^e >= extent/255
  return e < -126 ? -126 : e;
}
QE_HD float box_area(const float lo[3], const float hi[3]) {
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return (dx * dy + dx * dz) + dy * dz;
}
// surface area of box (lo, hi) as the grid of a quad node with box (node_lo, node_hi) holds it: about one cell wider per axis
QE_HD float area_on_grid(const float lo[3], const float hi[3], const float node_lo[3], const float node_hi[3]) {
  float dd[3];
  for (int a = 0; a < 3; a++) dd[a] = (hi[a] - lo[a]) + ldexpf(1.0f, cell_exponent(node_hi[a] - node_lo[a]));
  return (dd[0] * dd[1] + dd[0] * dd[2]) + dd[1] * dd[2];
}

// ---- the quantiser ----
struct Grid {
  uint32_t ebyte[3], qlo[3], qhi[3];  // per axis: the cell size's f32 exponent byte; lower / upper planes, one byte per child slot
};
// The boxes kids[0 .. nk) (anything with lo[3] / hi[3]) on the grid of the node (node_lo, node_hi); slots nk .. 3 unused.  The
// cell exponent is bumped while rounding pushes a plane past 255; it stops at 127 (reached by no finite input).
template <class Kid>
QE_HD Grid quantise(const float node_lo[3], const float node_hi[3], const Kid *kids, int nk) {
  Grid g;
  for (int a = 0; a < 3; a++) {
    const float origin = node_lo[a];
    g.qlo[a] = g.qhi[a] = 0u;
    int e = cell_exponent(node_hi[a] - node_lo[a]);
    for (; e <= 127; e++) {
      const float cell = ldexpf(1.0f, e);
      bool ok = true;
      uint32_t lo_bytes = 0, hi_bytes = 0;
      for (int k = 0; k < 4 && ok; k++) {
        if (k >= nk) { lo_bytes |= 255u << (8 * k); continue; }
        int ql = (int)floorf((kids[k].lo[a] - origin) / cell), qh = (int)ceilf((kids[k].hi[a] - origin) / cell);
        ql = ql < 0 ? 0 : ql, qh = qh < 0 ? 0 : qh;
        // enclosure checked in exact arithmetic: origin + q * cell fits a double without rounding
        const double o64 = origin, c64 = cell;
        while (ql > 0 && o64 + ql * c64 > (double)kids[k].lo[a]) ql--;
        while (qh <= 255 && o64 + qh * c64 < (double)kids[k].hi[a]) qh++;
        if (ql > 255 || qh > 255 || o64 + ql * c64 > (double)kids[k].lo[a]) { ok = false; break; }
        lo_bytes |= (uint32_t)ql << (8 * k);
        hi_bytes |= (uint32_t)qh << (8 * k);
      }
      if (ok) { g.qlo[a] = lo_bytes; g.qhi[a] = hi_bytes; break; }
    }
    g.ebyte[a] = (uint32_t)((e > 127 ? 127 : e) + 127);
  }
  return g;
}

// ---- the record (cell sizes as f32 bit patterns -- powers of two: exponent byte << 23 --, ready to be multiplied by 1 / d) ----
QE_HD void pack_record(uint4 *q, const float origin[3], const Grid &g, const uint32_t ref[4]) {
  q[0] = make_uint4(f32_bits(origin[0]), f32_bits(origin[1]), f32_bits(origin[2]), g.ebyte[0] << 23);
  q[1] = make_uint4(g.qlo[0], g.qlo[1], g.qlo[2], g.qhi[0]);
  q[2] = make_uint4(g.qhi[1], g.qhi[2], g.ebyte[1] << 23, g.ebyte[2] << 23);
  q[3] = make_uint4(ref[0], ref[1], ref[2], ref[3]);
}

// ---- the greedy rule ----
// The child to open next, or -1: the one with the largest surface area among those that still fit when opened (strict >: the
// first of equals wins).  grow(k) = the slots child k takes MORE when opened (an interior node: 1), 0 if it cannot open.
template <class Kid, class Grow>
QE_HD int greedy_pick(const Kid *kids, int nk, const Grow &grow) {
  int best = -1;
  float best_area = -1.f;
  for (int k = 0; k < nk; k++) {
    const uint32_t g = grow(k);
    if (g == 0u || (uint32_t)nk + g > 4u) continue;
    const float area = box_area(kids[k].lo, kids[k].hi);
    if (area > best_area) { best = k; best_area = area; }
  }
  return best;
}

// ---- the dynamic programme ----
// the children l, r of a node share k slots of the ancestor at distance d
template <class FAcc>
QE_HD float dp_dist(const FAcc &F, uint32_t l, uint32_t r, uint32_t k, uint32_t d) {
  float best = INFINITY;
  for (uint32_t k1 = 1; k1 < k; k1++) best = min_(best, F(l, k1, d) + F(r, k - k1, d));
  return best;
}
// F(n, 1 .. 4, d) of the interior node with children l, r, given one = Aq(n, R) + G(n)
template <class FAcc>
QE_HD void dp_interior(const FAcc &F, uint32_t l, uint32_t r, uint32_t d, float one, float out[4]) {
  out[0] = one;
  for (uint32_t k = 2; k <= 4; k++) out[k - 1] = d < 3u ? min_(one, dp_dist(F, l, r, k, d + 1u)) : one;
}
// following the minimising choices from the top: is c, given k slots at distance d, opened?  (F(c, 1, d): its cost as ONE child)
template <class FAcc>
QE_HD bool dp_opens(const FAcc &F, uint32_t c, uint32_t k, uint32_t d) {
  return k >= 2u && d < 3u && F(c, k, d) < F(c, 1u, d);
}
// ... and of the k slots its children l, r then share, the number that l takes; ties: the most even split
template <class FAcc>
QE_HD uint32_t dp_best_split(const FAcc &F, uint32_t l, uint32_t r, uint32_t k, uint32_t d) {
  uint32_t bk = 1;
  float best = INFINITY;
  for (uint32_t k1 = 1; k1 < k; k1++) {
    const float v = F(l, k1, d) + F(r, k - k1, d);
    const int ev = (int)(2 * k1) - (int)k, eb = (int)(2 * bk) - (int)k;
    if (v < best || (v == best && (ev < 0 ? -ev : ev) < (eb < 0 ? -eb : eb))) { best = v; bk = k1; }
  }
  return bk;
}

}  // namespace quad
}  // namespace pbrt_hip
