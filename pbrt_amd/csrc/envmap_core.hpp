// envmap_core.hpp -- the arithmetic of an environment-map infinite light, written once for the device (kernels_env.hip:
// render_kernel_env and the debug hook's kernel) and for the host (envmap.cpp: pbrt_hip_envmap_eval_host, what the CPU tests run), in
// the manner of reinsert_core.hpp and quad_encode.hpp: fp32, one fixed order of operations, built with -ffp-contract=off, and no call
// into libm / ocml -- atan, acos, sin and cos are the Cephes single-precision polynomials of cephes_poly.hpp, the ones the kernels use
// for a sphere's (u, v) and for cosine sampling (kernel_math.hpp), sin / cos over the full range by an octant reduction.
// The same bits on the CPU and on the GPU: tests/test_envmap_gpu.py compares the two over 2^20 inputs.
//
// The reference names the light and stops at todo!() before its MIPMap and Distribution2D (src/lights/infinite.rs:52-66); this is
// pbrt-v3's InfiniteAreaLight with ONE deliberate difference: the map is POINT-SAMPLED (as 3.15's checkerboard is), not bilinearly
// filtered through a MIPMap -- Le(d) = c * texel[row][col], a piecewise-constant sky.  The sampling density is then exactly
// proportional to the radiance it samples, and closed forms can be checked texel by texel.
//
//   lookup    w = M d (M = world_to_light, a rotation; dot in DESIGN.md 3's order), phi = atan2(w.y, w.x) in [0, 2 pi), theta = acos(w.z),
//             (u, v) = (phi / 2 pi, theta / pi), col = min((int)(u W), W - 1), row = min((int)(v H), H - 1); row 0 is theta = 0
//   texel     float4 {r, g, b, p_uv}: radiance and the density over (u, v) in one 16-byte load, p_uv = f / mean(f) with
//             f[row][col] = y(texel) sin(pi (row + 1/2) / H) (f = sin alone for a map that is black everywhere)
//   density   pdf_omega(d) = p_uv / (2 pi^2 sin theta), sin theta = sqrt(max(0, 1 - w.z^2)); sin theta == 0: density 0
//   sample    pbrt-v3's Distribution2D::SampleContinuous on (u1, u2): the row by inverting the marginal CDF (H + 1 floats) at u2, the
//             column by inverting that row's conditional CDF (W + 1 floats) at u1 -- plain binary searches, log2 H + log2 W dependent
//             loads --, the place inside the texel by linear interpolation; theta = v pi, phi = u 2 pi,
//             w = (sin theta cos phi, sin theta sin phi, cos theta), d = M^T w.  Monotone in (u2, u1): stratified and
//             low-discrepancy points keep their structure (an alias table would not).
#pragma once
#include <stdint.h>

// (every unit of the library is compiled by hipcc as HIP, the host-only ones included: float4 comes from here)
#include <hip/hip_runtime.h>

#include "cephes_poly.hpp"  // poly_sin .. poly_acos, PBRT_HD

namespace pbrt_hip {
namespace envmap {

constexpr float kPi = 3.14159265358979323846f, kTwoPi = 6.28318530717958647692f, kHalfPi = 1.5707963267948966f;
constexpr float kInvPi = 0.31830988618379067154f, kInvTwoPi = 0.15915494309189533577f;
constexpr float kTwoPiSquared = 19.739208802178716f;  // 2 pi^2: the Jacobian of (u, v) -> direction is 2 pi^2 sin theta
constexpr float kOneMinusEps = 0x1.fffffcp-1f;        // the samplers' largest value (kernel_math.hpp)

// The texels {r, g, b, p_uv} (row-major, row 0 = theta 0), the marginal CDF over rows and the conditional CDFs of the rows, in the
// memory of whoever runs the functions below; M = world_to_light, row-major 3 x 3.
struct Map {
  const float4 *texels;
  const float *marginal;     // H + 1
  const float *conditional;  // H x (W + 1)
  uint32_t W, H;
  float M[9];
};

// sin and cos of x in [0, 2 pi]: j = the nearest even multiple of pi / 4 (Cephes: the octant made even), y = x - j pi / 4 in three
// steps (pi / 4 split into DP1 + DP2 + DP3, the first two with few mantissa bits: j DP1 and j DP2 are exact), then the polynomials
// on |y| <= pi / 4 swapped and negated by the quadrant
PBRT_HD void sincos_0_2pi(float x, float *s, float *c) {
  uint32_t j = (uint32_t)(x * 1.27323954473516f);  // 4 / pi; x >= 0
  j = (j + 1u) & ~1u;
  const float jf = (float)j;
  const float y = ((x - jf * 0.78515625f) - jf * 2.4187564849853515625e-4f) - jf * 3.77489497744594108e-8f;
  const float ps = poly_sin(y), pc = poly_cos(y);
  const uint32_t q = (j >> 1) & 3u;
  *s = q == 0u ? ps : (q == 1u ? pc : (q == 2u ? -ps : -pc));
  *c = q == 0u ? pc : (q == 1u ? -ps : (q == 2u ? -pc : ps));
}

// (int)(x) clamped to [0, n - 1]; a NaN goes to 0 (a cast of one is undefined on the host and saturates on the device)
PBRT_HD uint32_t cell(float x, uint32_t n) {
  const float xp = x > 0.f ? x : 0.f;
  return xp < (float)n ? (uint32_t)xp : n - 1u;
}

// w = M d and its texel: *sin_theta for the density
PBRT_HD uint32_t lookup(const Map &m, float dx, float dy, float dz, float *sin_theta) {
  const float wx = (m.M[0] * dx + m.M[1] * dy) + m.M[2] * dz;
  const float wy = (m.M[3] * dx + m.M[4] * dy) + m.M[5] * dz;
  const float wz = (m.M[6] * dx + m.M[7] * dy) + m.M[8] * dz;
  const float ax = wx < 0.f ? -wx : wx, ay = wy < 0.f ? -wy : wy;
  float phi = (ax == 0.f && ay == 0.f) ? 0.f : poly_atan_pos(ay / ax);  // first quadrant (ax == 0: atan(+inf) = pi / 2)
  if (wx < 0.f) phi = kPi - phi;
  if (wy < 0.f) phi = kTwoPi - phi;
  const float zc = wz < -1.0f ? -1.0f : (wz > 1.0f ? 1.0f : wz);
  const float theta = poly_acos(zc);
  const float u = phi * kInvTwoPi, v = theta * kInvPi;
  const float s2 = 1.0f - zc * zc;
  *sin_theta = sqrtf(s2 > 0.f ? s2 : 0.f);
  return cell(v * (float)m.H, m.H) * m.W + cell(u * (float)m.W, m.W);
}

// the density over solid angle of a direction whose texel has p_uv and whose polar angle has this sine
PBRT_HD float pdf_omega(float p_uv, float sin_theta) { return sin_theta == 0.f ? 0.f : p_uv / (kTwoPiSquared * sin_theta); }

// pbrt-v3 FindInterval on a CDF of n + 1 entries (cdf[0] = 0, cdf[n] = 1): the largest k in [0, n - 1] with cdf[k] <= u
PBRT_HD uint32_t find_interval(const float *cdf, uint32_t n, float u) {
  uint32_t lo = 0u, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}
// Distribution1D::SampleContinuous: the interval k and (k + the place inside it) / n
PBRT_HD float sample_1d(const float *cdf, uint32_t n, float u, uint32_t *k) {
  const uint32_t i = find_interval(cdf, n, u);
  const float c0 = cdf[i], c1 = cdf[i + 1u];
  float du = u - c0;
  if (c1 - c0 > 0.f) du = du / (c1 - c0);
  du = du < kOneMinusEps ? du : kOneMinusEps;
  *k = i;
  return ((float)i + du) / (float)n;
}

// One light sample from (u1, u2), both in [0, 1): the direction d (world space), the texel drawn (row * W + col: radiance and p_uv
// are read from it, no second lookup) and the sine of its polar angle for pdf_omega -- taken from w.z exactly as lookup() takes it.
PBRT_HD uint32_t sample(const Map &m, float u1, float u2, float *dx, float *dy, float *dz, float *sin_theta) {
  uint32_t row, col;
  const float v = sample_1d(m.marginal, m.H, u2, &row);
  const float u = sample_1d(m.conditional + (size_t)row * (m.W + 1u), m.W, u1, &col);
  float st, ct, sp, cp;
  sincos_0_2pi(v * kPi, &st, &ct);
  sincos_0_2pi(u * kTwoPi, &sp, &cp);
  const float wx = st * cp, wy = st * sp, wz = ct;
  *dx = (m.M[0] * wx + m.M[3] * wy) + m.M[6] * wz;
  *dy = (m.M[1] * wx + m.M[4] * wy) + m.M[7] * wz;
  *dz = (m.M[2] * wx + m.M[5] * wy) + m.M[8] * wz;
  const float zc = wz < -1.0f ? -1.0f : (wz > 1.0f ? 1.0f : wz);
  const float s2 = 1.0f - zc * zc;
  *sin_theta = sqrtf(s2 > 0.f ? s2 : 0.f);
  return row * m.W + col;
}

}  // namespace envmap
}  // namespace pbrt_hip
