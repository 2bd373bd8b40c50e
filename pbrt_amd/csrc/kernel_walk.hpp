// kernel_walk.hpp -- the traversal of the render and ray-batch kernels: the per-lane walk state (Trav), the LDS stack helpers and
// trav_begin / trav_run, the production walk over the quantised 4-wide tree and the exact walk of the counting instantiations.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "device_types.h"
#include "kernel_math.hpp"

namespace pbrt_hip {
namespace {

constexpr uint32_t kDone = 0xffffffffu;

// The production walk addresses its LDS stack by 32-bit LDS byte addresses kept in a register (one v_add per push, no
// shift / or to form an address: tools/ubench/valu_issue.hip shows v_lshl_or_b32 and friends issue at half rate).
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ uint32_t lds_addr(const uint32_t *p) { return (uint32_t)(uintptr_t)(const lds_u32 *)p; }
__device__ __forceinline__ void lds_store(uint32_t a, uint32_t v) { *(lds_u32 *)(uintptr_t)a = v; }
__device__ __forceinline__ uint32_t lds_load(uint32_t a) { return *(const lds_u32 *)(uintptr_t)a; }
constexpr uint32_t kRowBytes = 256u;  // one stack row = 64 lanes x 4 bytes: consecutive entries of a lane are one row apart
// row of the entry at LDS address `a` of the stack whose lane column starts at `stk`: measured from the ARRAY's base, a
// link-time constant, so that no per-lane limit has to be kept in a register (the lane's 4-byte column offset is below a row)
// the lane number where it is needed only on a rare path: opaque to the optimiser, so that nothing derived from it is
// hoisted out of the kernel's loop into a register that lives for the whole kernel
__device__ __forceinline__ uint32_t lane_here() { uint32_t l = threadIdx.x & 63u; asm volatile("" : "+v"(l)); return l; }
__device__ __forceinline__ uint32_t lds_row(uint32_t a, const uint32_t *stk) { return (a - lds_addr(stk - (threadIdx.x & 63u))) / kRowBytes; }

// Per-lane traversal state.  It lives in registers across iterations of the kernels' outer loops,
// so a lane can be suspended in the middle of a walk while other lanes of the wave are served.
struct Trav {
  V3 o, d;
  float tmax;
  uint32_t cur;       // ref to process next: interior = step, leaf = the lane is PARKED there; kDone = walk over
  uint32_t sp;        // exact walk: stack entries in use; production walk: LDS byte address of the lane's first free entry
  uint32_t any;       // bit 0: any-hit (shadow) ray; bit 1: its result, occluded
  HitRec h;           // closest-hit result
};

struct TravTuning {
  uint32_t min_walkers;  // leave the loop when fewer lanes are walking and some lane waits for service
  uint32_t min_parked;   // test triangles once this many lanes are parked at a leaf
};

// s_setprio (A-B: -DPBRT_NO_PRIO compiles the priorities out; the levels can be overridden)
#ifndef PBRT_PRIO_FETCH
#define PBRT_PRIO_FETCH 3
#endif
#ifndef PBRT_PRIO_ARITH
#define PBRT_PRIO_ARITH 0
#endif
#ifndef PBRT_PRIO_SERVICE
#define PBRT_PRIO_SERVICE 1
#endif
__device__ __forceinline__ void wave_prio(int p) {
#ifndef PBRT_NO_PRIO
  switch (p) {  // (the builtin wants a constant)
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
#endif
}

// The slab test of DESIGN.md 3.4 against [kRayTMin, tfar]: near / far plane per axis by the sign of
// the inverse direction; fmin / fmax ignore a 0 * inf = NaN (conservative); far side padded.
__device__ __forceinline__ bool box_test(float lx, float ly, float lz, float hx, float hy, float hz, V3 o, V3 inv,
                                         bool negx, bool negy, bool negz, float tfar, float &tn) {
  const float nx = ((negx ? hx : lx) - o.x) * inv.x, fx = ((negx ? lx : hx) - o.x) * inv.x;
  const float ny = ((negy ? hy : ly) - o.y) * inv.y, fy = ((negy ? ly : hy) - o.y) * inv.y;
  const float nz = ((negz ? hz : lz) - o.z) * inv.z, fz = ((negz ? lz : hz) - o.z) * inv.z;
  tn = fmaxf(fmaxf(nx, ny), fmaxf(nz, kRayTMin));
  const float tf = fminf(fminf(fx, fy), fminf(fz, tfar));
  return tn <= tf * kBoxPad;
}

// Next node from the stack.  EXACT (the counting instantiation): every entry carries the entry
// distance tn of its box (NaN if the box already failed when it was pushed); the pop counts the node
// as visited and re-tests `tn <= tfar * pad`, which is equivalent to the oracle's slab test of the
// popped node with the current tfar (the far-plane part of that test can only have loosened).
// Otherwise entries are bare refs and a popped node is simply processed (a superset walk).
template <bool EXACT, uint32_t OVFR>  // OVFR: rows of the LDS part when deeper entries go to HBM (overflow variant), else 0
__device__ __forceinline__ uint32_t trav_pop(Trav &T, uint32_t *stk, float *stkt, uint32_t *ovf, unsigned long long &cn) {
  if (EXACT) {
    while (T.sp != 0u) {
      T.sp--;
      const uint32_t ref = stk[T.sp * 64u];
      const float tn = stkt[T.sp * 64u];
      cn++;  // EXACT implies counting
      if (tn <= fminf(T.h.t, T.tmax) * kBoxPad) return ref;
    }
    return kDone;
  }
  // production walk: entry 0 is the sentinel kDone (trav_begin), so a pop needs no emptiness test
  T.sp -= kRowBytes;
  if (OVFR == 0u) return lds_load(T.sp);
  const uint32_t e = lds_row(T.sp, stk);
  return e < OVFR - 1u ? lds_load(T.sp) : ovf[(e - (OVFR - 1u)) * 64u + lane_here()];
}
// production walk: the LDS part of a lane's stack has OVFR rows = OVFR - 1 entries (the
// sentinel first) + one scratch row, which the branch-free pushes below write when they do not push.  Only for
// trees whose worst-case bound exceeds that (OVF) do the deeper entries go to a per-lane HBM area.
template <uint32_t OVFR>
__device__ __forceinline__ void trav_push(Trav &T, uint32_t *stk, uint32_t *ovf, uint32_t ref) {
  if (OVFR == 0u) {
    lds_store(T.sp, ref);
  } else {
    const uint32_t e = lds_row(T.sp, stk);
    if (e < OVFR - 1u) lds_store(T.sp, ref);
    else ovf[(e - (OVFR - 1u)) * 64u + lane_here()] = ref;
  }
  T.sp += kRowBytes;
}

__device__ __forceinline__ void trav_enter(Trav &T, uint32_t ref) { T.cur = ref; }
__device__ __forceinline__ bool trav_parked(const Trav &T) { return T.cur != kDone && (T.cur & kLeafRef) != 0u; }
__device__ __forceinline__ uint32_t trav_leaf_cnt(const Trav &T) { return trav_parked(T) ? (T.cur >> 24) & 0x7fu : 0u; }

// Measurement aids (phase probe, ray log, per-pixel trace, A-B sensitivity loads / instructions, measured-negative
// variants kept for the record) live in experiments.inc and exist only in builds made with one of its switches
// (PBRT_PHASE_PROBE, PBRT_RAY_LOG, PBRT_DEBUG_PIXEL_X/Y, PBRT_EXTRA_VALU, PBRT_EXTRA_LOADS, PBRT_PREFETCH_POP: tools/README.md);
// in the product build every hook below expands to nothing.
#include "experiments.inc"
template <bool EXACT>
__device__ __forceinline__ void trav_begin(const DevScene &S, Trav &T, uint32_t *stk, V3 o, V3 d, float tmax, bool any,
                                           unsigned long long &cn) {
  T.o = o;
  T.d = d;
  T.tmax = tmax;
  T.sp = 0;
  if (!EXACT) {  // production walk: entry 0 is a sentinel, so that popping needs no emptiness test
    lds_store(lds_addr(stk), kDone);
    T.sp = lds_addr(stk) + kRowBytes;
  }
  T.any = any ? 1u : 0u;
  T.h.t = kInf;
  T.h.prim = kNoPrim;
  T.h.slot = kNoPrim;
  T.h.b1 = 0.f;
  T.h.b2 = 0.f;
  T.cur = kDone;
  if (S.n_nodes) {  // the root is the one node whose box is not held by a parent
    if (EXACT) cn++;
    // production walk: a ray that starts inside the root box needs no test (entering a node the ray might miss is
    // always allowed in a superset walk), and bounce / shadow rays always do: the three divisions are skipped
    if (!EXACT && o.x >= S.root_lo[0] && o.x <= S.root_hi[0] && o.y >= S.root_lo[1] && o.y <= S.root_hi[1] && o.z >= S.root_lo[2] &&
        o.z <= S.root_hi[2]) {
      trav_enter(T, !(S.root_ref & kLeafRef) ? 0u : S.root_ref);
      return;
    }
    const V3 inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    float tn;
    if (box_test(S.root_lo[0], S.root_lo[1], S.root_lo[2], S.root_hi[0], S.root_hi[1], S.root_hi[2], o, inv,
                 inv.x < 0.f, inv.y < 0.f, inv.z < 0.f, tmax, tn))
      trav_enter(T, (!EXACT && !(S.root_ref & kLeafRef)) ? 0u : S.root_ref);
  }
}

// The production walk's inverse direction: 1 / d, with the scene's finite stand-in for 1 / 0 on an axis the ray is parallel to
// (trav_run below says why)
__device__ __forceinline__ V3 walk_inv(const V3 d, const V3 inv1, const float inv_parallel) {
  return V3{d.x == 0.f ? copysignf(inv_parallel, inv1.x) : inv1.x, d.y == 0.f ? copysignf(inv_parallel, inv1.y) : inv1.y,
            d.z == 0.f ? copysignf(inv_parallel, inv1.z) : inv1.z};
}

// One node step's arithmetic (trav_run below; comments at its call): the four children of quantised node words W0 .. W2 against
// [kRayTMin, tfar] -> key[k] = the child's entry distance, hit[k].  A function of its own so that pbrt_hip_blocks_eval_device
// (kernels_blocks.hip) runs the walk's own statement over arrays; SCALAR_FMA: the 24 plane fmas scalar or packed (the same bits).
template <bool SCALAR_FMA>
__device__ __forceinline__ void quad_step(const uint4 W0, const uint4 W1, const uint4 W2, const V3 o, const V3 inv, const bool negx,
                                          const bool negy, const bool negz, const float tfar, float (&key)[4], bool (&hit)[4]) {
  const float gx = (o.x - __uint_as_float(W0.x)) * inv.x, gy = (o.y - __uint_as_float(W0.y)) * inv.y;
  const float gz = (o.z - __uint_as_float(W0.z)) * inv.z;
  // g +- 3 eps |g| as one fma each (|x| and -x are operand modifiers): rounded once instead of twice, at least
  // g +- 5/2 eps |g|, still beyond the 2 eps |g| the margin has to cover
  constexpr float kMargin = 0x1.8p-22f;
  const float gxn = __builtin_fmaf(fabsf(gx), kMargin, gx), gxf = __builtin_fmaf(-fabsf(gx), kMargin, gx);  // near, far: subtracted below
  const float gyn = __builtin_fmaf(fabsf(gy), kMargin, gy), gyf = __builtin_fmaf(-fabsf(gy), kMargin, gy);
  const float gzn = __builtin_fmaf(fabsf(gz), kMargin, gz), gzf = __builtin_fmaf(-fabsf(gz), kMargin, gz);
  const float cix = __uint_as_float(W0.w) * inv.x, ciy = __uint_as_float(W2.z) * inv.y, ciz = __uint_as_float(W2.w) * inv.z;
  // near / far planes by the sign of the inverse direction: one select per axis serves all four
  // children (a dword holds the four children's bytes of one plane)
  const uint32_t bnx = negx ? W1.w : W1.x, bfx = negx ? W1.x : W1.w;
  const uint32_t bny = negy ? W2.x : W1.y, bfy = negy ? W1.y : W2.x;
  const uint32_t bnz = negz ? W2.y : W1.z, bfz = negz ? W1.z : W2.y;
  // How the 24 plane fmas are issued.  A gfx950 SIMD issues, per quad-cycle, one instruction of any kind plus one of
  // the "simple" class (fma, mul, add, logic, right shift, mov) from another wave; a packed instruction goes alone
  // (tools/ubench/valu_pairing.hip, profiles/r03w_valu_pairing_ubench.txt).  This step has three converts / min /
  // max / compares / selects for every simple instruction, so 24 scalar v_fma_f32 ride along with them where 12
  // v_pk_fma_f32 take 12 quad-cycles of their own -- but they are 12 more instructions for a wave that issues one
  // every ~5 cycles at best.  Measured (profiles/r03w_scalar_fma_ab.txt): trees that sit in L2 (no wait to hide: C4
  // +4.7 %, C2 +1.6 %) gain from the scalar form; the deep trees of the overflow variant, whose waves spend their time
  // waiting for nodes, lose (C3 -0.8 %, 12 M triangles -6.5 %) and keep the packed one ({near, far} of a child side by
  // side; IEEE per element: the same bits either way).
  const f32x2 gxx = {gxn, gxf}, gyy = {gyn, gyf}, gzz = {gzn, gzf}, cxx = {cix, cix}, cyy = {ciy, ciy}, czz = {ciz, ciz};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float qxn = (float)((bnx >> (8 * k)) & 0xffu), qxf = (float)((bfx >> (8 * k)) & 0xffu);
    const float qyn = (float)((bny >> (8 * k)) & 0xffu), qyf = (float)((bfy >> (8 * k)) & 0xffu);
    const float qzn = (float)((bnz >> (8 * k)) & 0xffu), qzf = (float)((bfz >> (8 * k)) & 0xffu);
    f32x2 tx, ty, tz;  // {near, far}
    if (SCALAR_FMA) {
      tx = f32x2{__builtin_fmaf(qxn, cix, -gxn), __builtin_fmaf(qxf, cix, -gxf)};
      ty = f32x2{__builtin_fmaf(qyn, ciy, -gyn), __builtin_fmaf(qyf, ciy, -gyf)};
      tz = f32x2{__builtin_fmaf(qzn, ciz, -gzn), __builtin_fmaf(qzf, ciz, -gzf)};
    } else {
      tx = __builtin_elementwise_fma(f32x2{qxn, qxf}, cxx, -gxx);
      ty = __builtin_elementwise_fma(f32x2{qyn, qyf}, cyy, -gyy);
      tz = __builtin_elementwise_fma(f32x2{qzn, qzf}, czz, -gzz);
    }
    const float tn = fmaxf(fmaxf(tx.x, ty.x), fmaxf(tz.x, kRayTMin));
    const float tf = fminf(fminf(tx.y, ty.y), fminf(tz.y, tfar));
    hit[k] = tn <= tf * kBoxPad;
    key[k] = tn;
  }
}

// The control code of trav_run below: how its scheduling decisions are formed, not what they decide (DESIGN.md section 6, row r08a:
// C3 -4.3 % frame time, films and counters unchanged).  One switch per part puts the earlier form back for an A-B; with all of them
// set the kernels are the earlier machine code byte for byte (pbrt_amd/isa_id.py):
//   PBRT_WALK_MASKS_OLD      every decision ballots a bool of its own, `alive` included, in every iteration      (worth 1.0 % on C3)
//   PBRT_WALK_ROTATE_OLD     the exit test at the loop's head, two breaks                                          (0.9 %)
//   PBRT_WALK_LEAF_LOOP_OLD  the leaf pass is the counted loop for every tree                                      (2.6 %)
// (A fourth part, the push stride kept in a register instead of a literal moved into one in every step, measured 0.0 % and is not here.)
// wave_vote: the lanes for which a PER-LANE predicate holds, as the compare's own mask.  (__ballot goes through an int: the compiler
// materialises 0 / 1 in a register and compares it again, two vector instructions per vote on a mask that already sits in scalar
// registers.)  A predicate that is a function of votes already taken is formed from their masks on the scalar unit and not voted again.
__device__ __forceinline__ unsigned long long wave_vote(bool p) {
#ifdef PBRT_WALK_MASKS_OLD
  return __ballot(p);
#else
  return __builtin_amdgcn_ballot_w64(p);
#endif
}

// The traversal loop of a whole wave ("while-while" with parked leaves) over the child-pair nodes.
// Every lane walks its own ray through the binary tree of DESIGN.md 3.3 in the order of 3.4 (near
// child by the sign of the split axis first, far child pushed); one step fetches ONE 64-byte record
// and tests BOTH children of an interior node, leaves are never fetched (their ref holds slot and
// count).  With EXACT the sequence of nodes visited and triangles tested is the oracle's, counter
// for counter; without it the far child is dropped at once if its box fails and is not re-tested
// when popped -- a superset walk whose RESULT is identical because of the tie rule (lower primitive
// id wins at equal t).  What is scheduling, and never changes a lane's arithmetic:
//   * a lane that reaches a leaf PARKS there; the wave tests triangles (one per parked lane per
//     pass) only when `min_parked` lanes are parked or nobody can step, so the long
//     Moeller-Trumbore body runs with many lanes instead of one or two;
//   * the loop EXITS when no lane walks, or when fewer than `min_walkers` do and some lane whose
//     walk is over is waiting to be served (shade / regenerate / fetch the next ray); walking
//     lanes keep their state and resume on the next call.
// `__ballot` + popcount make both decisions wave-uniform.  `alive`: this lane has work for the
// caller once its walk is over.
// SPH: the scene has spheres -- leaf records flagged as such (pack_tris_kernel: word 3 of the third float4) take the sphere test
template <bool EXACT, bool COUNT, uint32_t OVFR, int STEPS = PBRT_STEPS_PER_CHECK, bool SPH = false>
__device__ __forceinline__ void trav_run(const DevScene &S, Trav &T, uint32_t *stk, float *stkt, uint32_t *ovf,
                                         const bool alive, const TravTuning tune, unsigned long long &cn,
                                         unsigned long long &ct) {
  const V3 o = T.o, d = T.d;
  const V3 inv1 = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
  const bool negx = inv1.x < 0.f, negy = inv1.y < 0.f, negz = inv1.z < 0.f;
  const uint32_t negbits = (negx ? 1u : 0u) | (negy ? 2u : 0u) | (negz ? 4u : 0u);
  // Production walk: a ray PARALLEL to a slab (d exactly 0 on that axis; 1 / d = +-inf) multiplies by the scene's huge finite power of
  // two instead (device_types.h inv_parallel, host_math.hpp): with inf every quantised plane's t = q * inf - inf is NaN, the axis drops
  // out of the slab test and a ray along an axis -- every shadow ray towards a sun straight overhead -- walks the whole tree.  The
  // canonical walk (EXACT) keeps 1 / 0 = inf: its planes are real floats ((lo - o) * inf is +-inf with the right sign) and its visit
  // counters are the oracle's.
#ifdef PBRT_INV_INF  // A-B switch: the walk as it was before the stand-in (tools/experiments/README.md, round 5)
  const V3 inv = inv1;
#else
  const V3 inv = EXACT ? inv1 : walk_inv(d, inv1, S.inv_parallel);
#endif
  const char *nodes = reinterpret_cast<const char *>(S.nodes);
  const char *quads = reinterpret_cast<const char *>(S.quads);
  const char *tris = reinterpret_cast<const char *>(S.tris);
#ifndef PBRT_WALK_MASKS_OLD
  // `alive` does not change in here: its vote, and the walkers the exit test asks for, are taken once
  const unsigned long long malive = wave_vote(alive);
  const uint32_t walkers_x64 = tune.min_walkers * (uint32_t)__popcll(malive);
#endif
#ifndef PBRT_WALK_ROTATE_OLD
  // The loop is rotated: the exit test stands once before it and once at its bottom, so that the loop has one exit, behind its last
  // statement, and the walk state stays in one set of registers (with the test at the head and two breaks below it the compiler kept
  // T.cur, T.sp and the hit record in two sets and copied them across at the head and at every way round: eight v_mov per batch).
  const auto go_on = [&]() -> bool {
    const bool walking = T.cur != kDone;
    const unsigned long long mwalk = wave_vote(walking);
#ifdef PBRT_WALK_MASKS_OLD
    return mwalk != 0ull && !((uint32_t)__popcll(mwalk) * 64u < tune.min_walkers * (uint32_t)__popcll(__ballot(alive)) && __ballot(!walking && alive) != 0ull);
#else
    return mwalk != 0ull && !((uint32_t)__popcll(mwalk) * 64u < walkers_x64 && (malive & ~mwalk) != 0ull);  // (alive and not walking: waiting to be served)
#endif
  };
  if (go_on()) do {
#else
  for (;;) {
    const bool walking = T.cur != kDone;
    const unsigned long long mwalk = wave_vote(walking);
    if (mwalk == 0ull) break;
    // (min_walkers is meant for a full wave: it scales with the lanes that still have work at all, so that a wave whose
    // pixel list has run dry does not visit the service stage for every single ray)
#ifdef PBRT_WALK_MASKS_OLD
    if ((uint32_t)__popcll(mwalk) * 64u < tune.min_walkers * (uint32_t)__popcll(__ballot(alive)) && __ballot(!walking && alive) != 0ull) break;
#else
    if ((uint32_t)__popcll(mwalk) * 64u < walkers_x64 && (malive & ~mwalk) != 0ull) break;  // (alive and not walking: waiting to be served)
#endif
#endif

    if (EXACT && T.cur != kDone && !trav_parked(T)) {
      // ---- one step: both children of interior node T.cur ----
      const uint32_t off = T.cur * 64u;
      const uint4 q0 = *reinterpret_cast<const uint4 *>(nodes + off);
      const uint4 q1 = *reinterpret_cast<const uint4 *>(nodes + off + 16u);
      const uint4 q2 = *reinterpret_cast<const uint4 *>(nodes + off + 32u);
      const uint4 q3 = *reinterpret_cast<const uint4 *>(nodes + off + 48u);
      const float tfar = fminf(T.h.t, T.tmax);
      // The slab test of DESIGN.md 3.4 for child 0 and child 1 side by side: element 0 / 1 of each
      // float2 belongs to child 0 / 1, so the six subtractions and six multiplications of the two
      // boxes are six packed instructions (v_pk_add_f32 / v_pk_mul_f32, IEEE per element: the
      // same bits as the scalar form).
      const f32x2 lx = {__uint_as_float(q0.x), __uint_as_float(q1.z)}, hx = {__uint_as_float(q0.w), __uint_as_float(q2.y)};
      const f32x2 ly = {__uint_as_float(q0.y), __uint_as_float(q1.w)}, hy = {__uint_as_float(q1.x), __uint_as_float(q2.z)};
      const f32x2 lz = {__uint_as_float(q0.z), __uint_as_float(q2.x)}, hz = {__uint_as_float(q1.y), __uint_as_float(q2.w)};
      const f32x2 nx = ((negx ? hx : lx) - o.x) * inv.x, fx = ((negx ? lx : hx) - o.x) * inv.x;
      const f32x2 ny = ((negy ? hy : ly) - o.y) * inv.y, fy = ((negy ? ly : hy) - o.y) * inv.y;
      const f32x2 nz = ((negz ? hz : lz) - o.z) * inv.z, fz = ((negz ? lz : hz) - o.z) * inv.z;
      const float tn0 = fmaxf(fmaxf(nx.x, ny.x), fmaxf(nz.x, kRayTMin));
      const float tn1 = fmaxf(fmaxf(nx.y, ny.y), fmaxf(nz.y, kRayTMin));
      const float tf0 = fminf(fminf(fx.x, fy.x), fminf(fz.x, tfar));
      const float tf1 = fminf(fminf(fx.y, fy.y), fminf(fz.y, tfar));
      const bool hit0 = tn0 <= tf0 * kBoxPad, hit1 = tn1 <= tf1 * kBoxPad;
      const bool far_first = ((negbits >> q3.z) & 1u) != 0u;  // child 1 is the near one
      const uint32_t ref_near = far_first ? q3.y : q3.x, ref_far = far_first ? q3.x : q3.y;
      const bool hit_near = (far_first && hit1) || (!far_first && hit0);
      const bool hit_far = (far_first && hit0) || (!far_first && hit1);
      if (EXACT) {
        cn++;  // the near child is visited now; the far one when it is popped
        stk[T.sp * 64u] = ref_far;
        stkt[T.sp * 64u] = hit_far ? (far_first ? tn0 : tn1) : __builtin_nanf("");
        T.sp++;
      }
      trav_enter(T, hit_near ? ref_near : trav_pop<EXACT, OVFR>(T, stk, stkt, ovf, cn));
    }

    // production walk: STEPS node steps between two scheduling checks (a lane that parks or
    // finishes in the first one idles through the rest; the checks cost about a fifth of a step)
#pragma unroll
    for (int rep = 0; !EXACT && rep < STEPS; rep++) {
    EXP_PROBE_LANES(0, T.cur != kDone && !trav_parked(T));
    if (T.cur != kDone && !trav_parked(T)) {
      // ---- one step of the production walk: the four children of quantised quad node T.cur (64 bytes) ----
      const uint32_t off = T.cur;  // the ref of an interior quad node IS its byte offset (node number x 64)
      // Wave priority (s_setprio; the SIMD's arbiter picks the ready wave of highest priority, the oldest among equals): 3
      // while a step issues its node fetch, 0 for the arithmetic on the node -- a wave that is about to wait ~700 cycles for
      // its next node gets its loads out before the other waves' decode and slab tests.  With the same around the leaf
      // pass's triangle fetch and 1 for the service stage: C3 +3.5 %, C2 +0.7 % (tools/experiments/README.md).
      wave_prio(PBRT_PRIO_FETCH);
      const uint4 W0 = EXP_NODE_LOAD(reinterpret_cast<const uint4 *>(quads + off));
      const uint4 W1 = EXP_NODE_LOAD(reinterpret_cast<const uint4 *>(quads + off + 16u));
      const uint4 W2 = EXP_NODE_LOAD(reinterpret_cast<const uint4 *>(quads + off + 32u));
      const uint4 W3 = EXP_NODE_LOAD(reinterpret_cast<const uint4 *>(quads + off + 48u));
      EXP_STEP_EXTRA_LOADS(quads, off, T);
      wave_prio(PBRT_PRIO_ARITH);
      if (COUNT) cn++;  // one 64-byte fetch
      const float tfar = fminf(T.h.t, T.tmax);
      EXP_STEP_EXTRA_VALU(W0, tfar, T);
      // Node-relative slab test.  A decoded plane is the REAL number origin + q * cell (the builder
      // checks in exact arithmetic that these planes enclose the true box), so
      //     t = (origin + q*cell - o) * inv = q * (cell*inv) - (o - origin)*inv = fma(q, ci, -gi):
      // one cvt + one fma per plane.  ci = cell * inv is exact (cell is a power of two); the two
      // roundings inside gi = fl(fl(o - origin) * inv) are absolute errors <= 2 eps |gi| in t, covered by
      // the margin m = 3 eps |gi|: near planes subtract gi + m, far planes gi - m, so every computed
      // t_near / t_far lies outside the true one and the walk stays a superset of the exact walk; the
      // fma's own relative rounding is what kBoxPad of DESIGN.md 3.4 is for (1 + 2^-19 since round 6).  A ray
      // parallel to the slab (d = 0) has the scene's finite stand-in for 1 / 0 in inv (above): t is then
      // negative huge or positive huge by the side of the plane the origin is on; an inv that is infinite
      // because d is a denormal yields NaN or +-inf, which fmin / fmax ignore or keep conservative.
      float key[4];
      bool hit[4];
      quad_step<OVFR == 0u>(W0, W1, W2, o, inv, negx, negy, negz, tfar, key, hit);
      // (an unused child slot holds kEmptyLeafRef behind an inverted box: if a degenerate ray gets through that box the
      // lane parks at a leaf without triangles and pops -- no test for it here)
#ifdef PBRT_PRIO_SELECT  // (A-B: raised priority from the child selection on)
      wave_prio(PBRT_PRIO_SELECT);
#endif
      // The nearest child hit is entered, the other hit ones are stacked in slot order.  Order affects only
      // speed (tie rule of 3.4) -- but a lot: visiting the hit children in slot order alone costs C3 49 node steps per
      // ray instead of 41 (measured, r02), and sorting the stacked ones cost more than it saved (r01).
#include "quad_nearest.inc"
      const bool any_hit = hit[0] || hit[1] || hit[2] || hit[3];
      const uint32_t nearest = n0 ? W3.x : (n1 ? W3.y : (n2 ? W3.z : W3.w));
      // Overflow variant (trees whose worst-case stack bound exceeds the LDS part): one wave-uniform test per step -- is
      // any lane within four rows of the end of its LDS part? -- picks the slow form with predicated pushes that go
      // to HBM beyond it; stacks rarely get that deep, so nearly every step takes the branch-free form below.  (One
      // compare against a constant: the stack array's base is a link-time constant, the lane's column offset is
      // smaller than a row.  A test per batch of steps instead, with a threshold three times as far from the end,
      // measured 1.5 % slower.  __builtin_expect moves the slow form out of line: the fast form falls through, +1.2 %.)
      if (OVFR != 0u && __builtin_expect(wave_vote(T.sp >= lds_addr(stk - (threadIdx.x & 63u)) + (OVFR - 4u) * kRowBytes) != 0ull, 0)) {
        if (hit[3] && !n3) trav_push<OVFR>(T, stk, ovf, W3.w);
        if (hit[2] && !n2) trav_push<OVFR>(T, stk, ovf, W3.z);
        if (hit[1] && !n1) trav_push<OVFR>(T, stk, ovf, W3.y);
        if (hit[0] && !n0) trav_push<OVFR>(T, stk, ovf, W3.x);
        trav_enter(T, any_hit ? nearest : trav_pop<false, OVFR>(T, stk, stkt, ovf, cn));
      } else {
        // branch-free: each ref is written above the stack top in any case (one LDS row beyond the entries is
        // scratch) and the top advances by the hit mask; entry 0 is the sentinel kDone, so the entry below the top
        // can be read in any case.  T.sp is the LDS ADDRESS of the top: a push is one ds_write + one v_add, no
        // address arithmetic (v_lshl_or_b32 and the other three-operand integer forms issue at half rate on gfx950).
        // the entry below the top is read BEFORE the pushes (a lane that pops has pushed nothing in this step): the read
        // does not wait behind four writes, and the next node's address is known that much earlier
        const uint32_t below = T.sp - kRowBytes, top = lds_load(below);
        const uint32_t next = any_hit ? nearest : top;
        lds_store(T.sp, W3.w); T.sp += (hit[3] && !n3) ? kRowBytes : 0u;
        lds_store(T.sp, W3.z); T.sp += (hit[2] && !n2) ? kRowBytes : 0u;
        lds_store(T.sp, W3.y); T.sp += (hit[1] && !n1) ? kRowBytes : 0u;
        lds_store(T.sp, W3.x); T.sp += (hit[0] && !n0) ? kRowBytes : 0u;
        T.sp = any_hit ? T.sp : below;
        trav_enter(T, next);
      }
    }
    }

    // ---- leaf flush (wave-uniform decision) ----
    const bool parked = trav_parked(T);
    const unsigned long long mleaf = wave_vote(parked);
    if (mleaf != 0ull &&
        ((uint32_t)__popcll(mleaf) >= tune.min_parked ||
         // ... or when the parked lanes are at least half as many as the lanes that can still step (with few
         // steppers left, waiting for min_parked only idles the parked ones; this also covers "nobody can step")
         (uint32_t)__popcll(mleaf) * 2u >= (uint32_t)__popcll(wave_vote(T.cur != kDone && !parked)))) {
      const uint32_t cnt = parked ? (T.cur >> 24) & 0x7fu : 0u, first = T.cur & 0xffffffu;
      bool stop = false;  // any-hit ray found its hit
      EXP_LEAF_PREFETCH_BEGIN(parked, quads, T);
      EXP_PROBE_FLUSH(cnt);
#ifndef PBRT_WALK_LEAF_LOOP_OLD
      // The production walk's trees have single-triangle leaves (a leaf of 2 .. 4 triangles is a quad node of them,
      // quad_nodes.cpp splittable; the device builder makes no other leaf) and empty ones.  So the pass is the body once, straight-line,
      // and the hit record is updated by selects where it lives; the counted loop, out of line behind one vote, goes on from the
      // second triangle for a tree that was built with larger leaves.  The exact walk's leaves are the canonical tree's: the loop alone.
      constexpr uint32_t kStraight = EXACT ? 0u : 1u;
      if (!EXACT) {
        constexpr uint32_t i = 0u;
        EXP_PROBE_LANES(2, cnt != 0u);
        if (cnt != 0u) {  // (an empty leaf, kEmptyLeafRef, tests nothing and pops)
#include "leaf_test.inc"
        }
      }
      if (EXACT || __builtin_expect(wave_vote(cnt > 1u) != 0ull, 0))
#else
      constexpr uint32_t kStraight = 0u;
#endif
      for (uint32_t i = kStraight;; i++) {
        if (wave_vote(cnt > i && !stop) == 0ull) break;
        EXP_PROBE_LANES(2, cnt > i && !stop);
        if (cnt > i && !stop) {
#include "leaf_test.inc"
        }
      }
      EXP_LEAF_PREFETCH_END();
      // (OVF: is any entry about to be popped one of the rare ones beyond the LDS part?  wave-uniform, as for the pushes)
#ifdef PBRT_WALK_MASKS_OLD
      const bool far_pop = OVFR != 0u && !EXACT &&
                           __ballot(parked && !stop && T.sp >= lds_addr(stk - (threadIdx.x & 63u)) + OVFR * kRowBytes) != 0ull;
#else
      // (the vote is the compare's own mask, met with the parked lanes' on the scalar unit.  A lane that stops no longer counts out: the
      // test only picks the FORM of the pop for the wave, each lane takes its own way through either, and an any-hit ray that ends
      // with a stack that deep is as rare as the deep stack itself.)
      const bool far_pop = OVFR != 0u && !EXACT && (wave_vote(T.sp >= lds_addr(stk - (threadIdx.x & 63u)) + OVFR * kRowBytes) & mleaf) != 0ull;
#endif
      if (parked) {  // leave the leaf: the walk is over (any-hit found) or the next node comes off the stack
        if (stop) {
          T.cur = kDone;
          T.sp = 0u;
        } else if (OVFR != 0u && __builtin_expect(far_pop, 0)) {
          trav_enter(T, trav_pop<EXACT, OVFR>(T, stk, stkt, ovf, cn));
        } else {
          trav_enter(T, trav_pop<EXACT, 0u>(T, stk, stkt, ovf, cn));
        }
      }
    }
#ifndef PBRT_WALK_ROTATE_OLD
  } while (go_on());
#else
  }
#endif
}

}  // namespace
}  // namespace pbrt_hip
