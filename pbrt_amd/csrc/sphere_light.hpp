// sphere_light.hpp -- a sphere area light's sample (pbrt-v3 Sphere::Sample(ref, u), the cone branch): a direction uniform in
// the solid angle that the sphere (c, r) subtends from the shading point po.  Written once, in the manner of spot_light.hpp: fp32, one fixed
// order of operations, built with -ffp-contract=off, nothing of libm / ocml but sqrt (and cosine_about's Cephes polynomials).
// kernel_path.hpp's sample_light_sphere and the sphere branch of sample_light_general are built on it, render_body.inc's MIS hit side reads
// pdf_omega (all under PLS alone: the GLS instantiations of render_kernel_x), kernels_blocks.hip's sphere_light_eval_kernel runs it over
// arrays (pbrt_hip_sphere_light_eval_device), and tests/test_sphere_light_host.py compiles THIS TEXT for the host and holds it to a float64
// restatement; the device's words must equal the host's bit for bit (tests/test_sphere_light_gpu.py).
//
//   wc = c - po, dc2 = wc . wc; no sample unless dc2 > r^2 (emission is one-sided, outward: a point inside or on the sphere sees none)
//   s2 = r^2 / dc2 = sin^2 theta_max, cmax = sqrt(max(0, 1 - s2)), omc = 1 - cmax formed as s2 / (1 + cmax): NEVER by subtraction, which is
//   exactly 0 in fp32 from r / d = 2.4e-4 downwards
//   (dx, dy) = cosine_about's concentric map of (u1, u2) onto the unit disk, s = min(dx^2 + dy^2, 1)
//   cos theta = ct = 1 - s omc; the tangential part is (dx, dy) sqrt(omc (1 + ct)) in cosine_about's frame about w = wc / dc:
//   sin^2 theta = (1 - ct)(1 + ct) = s omc (1 + ct) and |(dx, dy)| = sqrt(s).  No trigonometry of theta, no division by s, no 1 - ct^2
//   pdf_omega = 1 / (2 pi omc);  scale = (cs (2 pi omc)) nL with cs = wi . nf, no sample where cs <= 0
//   t = dc ct - r sqrt(max(0, 1 - s (1 + ct) / (1 + cmax))): the near intersection, the half chord without the cancellation of
//   b^2 - (dc2 - r^2): r^2 - dc2 sin^2 theta = r^2 (1 - s omc (1 + ct) / s2) and omc / s2 = 1 / (1 + cmax)
//   tmax = (t - m) kShadowShrink, m = min(2^-9 dc, 2^-18 dc2 / half chord): the shadow ray must not be stopped by the light's own sphere,
//   and sphere_hit (kernel_math.hpp) forms dot(oc, oc) - r^2 and 2 d . oc in fp32 before its double quadratic, along a direction that is
//   itself 4e-7 rad off: the discriminant it takes the root of is off by up to 1.7e-6 dc2 (DESIGN.md 3.25 adds the terms up), which
//   delta = 2^-18 dc2 = 3.8e-6 dc2 covers 2.2 times, so its near root lies at most sqrt(D + delta) - sqrt(D) <= min(sqrt(delta), delta /
//   (2 sqrt(D))) in front of t, D = (half chord)^2.  Near the rim that is 2e-3 dc -- twenty times kShadowShrink's share --, at the centre
//   2^-18 dc (dc / r).  What the margin costs: an occluder closer than m to the lamp's surface does not shadow it.
#pragma once
#include "kernel_math.hpp"

namespace pbrt_hip {
namespace {
namespace sphere_light {

constexpr float kTwoPi = 6.28318530717958647692f;
constexpr float kSelfRim = 0x1p-9f;     // sqrt(delta) / dc
constexpr float kSelfDelta = 0x1p-18f;  // delta / dc2

// 1 - cos theta_max of the sphere (c, r) seen from o, as s2 / (1 + cmax); false where o is not outside.  *dc2, *cmax: for the sampler
__device__ __forceinline__ bool one_minus_cos_max(V3 o, V3 c, float r, V3 &wc, float &dc2, float &cmax, float &omc) {
  wc = c - o;
  dc2 = dot(wc, wc);
  const float r2 = r * r;
  if (!(dc2 > r2)) return false;
  const float s2 = r2 / dc2;
  cmax = sqrtf(fmaxf(0.f, 1.0f - s2));
  omc = s2 / (1.0f + cmax);
  return true;
}

// the density over solid angle with which sample() draws a direction from o; 0 where o is not outside the sphere.  A function of (o, c, r)
// alone: the sample side and the MIS hit side (render_body.inc) call this one text
__device__ __forceinline__ float pdf_omega(V3 o, V3 c, float r) {
  V3 wc;
  float dc2, cmax, omc;
  if (!one_minus_cos_max(o, c, r, wc, dc2, cmax, omc)) return 0.f;
  return 1.0f / (kTwoPi * omc);
}

// cosine_about's concentric map of (u1, u2) onto the unit disk and its tangent frame about a unit vector (kernel_math.hpp), operation for
// operation.  COPIES, not calls: cosine_about built from two shared inline helpers gave all 240 render kernels other machine code
// (measured with isa_id), which the committed counter profiles are keyed by.  tests/test_sphere_light_host.py holds the texts equal: over
// 2^16 inputs (v2 dx + v3 dy) + n sqrt(max(0, (1 - dx dx) - dy dy)) from these two IS cosine_about's direction, bit for bit
__device__ __forceinline__ void disk(float u1, float u2, float &dx, float &dy) {
  float ox = 2.0f * u1 - 1.0f, oy = 2.0f * u2 - 1.0f;
  if (ox == 0.f && oy == 0.f) {
    dx = 0.f;
    dy = 0.f;
  } else if (fabsf(ox) > fabsf(oy)) {
    float phi = kPiOver4 * (oy / ox);
    dx = ox * poly_cos(phi);
    dy = ox * poly_sin(phi);
  } else {
    float phi = kPiOver4 * (ox / oy);
    dx = oy * poly_sin(phi);
    dy = oy * poly_cos(phi);
  }
}
__device__ __forceinline__ void frame(V3 n, V3 &v2, V3 &v3) {
  if (fabsf(n.x) > fabsf(n.y)) {
    float l = sqrtf(n.x * n.x + n.z * n.z);
    v2 = {-n.z / l, 0.f, n.x / l};
  } else {
    float l = sqrtf(n.y * n.y + n.z * n.z);
    v2 = {0.f, n.z / l, -n.y / l};
  }
  v3 = cross(n, v2);
}

// The light sample at shading point po with normal nf (turned towards the viewer) from the pair (u1, u2).  false: po is not outside the
// sphere or the direction lies behind nf, and no shadow ray is cast (the outputs are then not to be used).  scale = cs (1 / pdf) nL
__device__ __forceinline__ bool sample(V3 po, V3 nf, V3 c, float r, float u1, float u2, float nLf, V3 &wi, float &tmax, float &scale, float &pdf, float &cs) {
  V3 wc;
  float dc2, cmax, omc;
  if (!one_minus_cos_max(po, c, r, wc, dc2, cmax, omc)) return false;
  const float dc = sqrtf(dc2);
  const V3 w = wc / dc;
  float dx, dy;
  disk(u1, u2, dx, dy);
  const float s = fminf(dx * dx + dy * dy, 1.0f);
  const float ct = 1.0f - s * omc;
  const float tang = sqrtf(omc * (1.0f + ct));
  V3 v2, v3;
  frame(w, v2, v3);
  wi = (v2 * (dx * tang) + v3 * (dy * tang)) + w * ct;
  cs = dot(wi, nf);
  if (!(cs > 0.f)) return false;
  const float area = kTwoPi * omc;  // the solid angle: 1 / pdf
  pdf = 1.0f / area;
  scale = (cs * area) * nLf;
  const float half = r * sqrtf(fmaxf(0.f, 1.0f - (s * (1.0f + ct)) / (1.0f + cmax)));
  const float t = dc * ct - half;
  const float m = fminf(kSelfRim * dc, (kSelfDelta * dc2) / half);  // (half = 0: the quotient is +inf and the rim's margin holds)
  tmax = (t - m) * kShadowShrink;
  return true;
}

}  // namespace sphere_light
}  // namespace
}  // namespace pbrt_hip
