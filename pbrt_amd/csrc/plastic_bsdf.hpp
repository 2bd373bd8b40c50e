// plastic_bsdf.hpp -- the plastic material's BSDF (pbrt-v3 PlasticMaterial with a fixed index of 1.5 against 1): a
// Lambertian base Kd / pi plus ONE Trowbridge-Reitz microfacet reflection lobe of isotropic width alpha with the dielectric Fresnel term of
// kernel_math.hpp's glass_fresnel.  Written once, in the manner of envmap_core.hpp and filter_weight.inc: fp32, one fixed order of
// operations, built with -ffp-contract=off, nothing of libm / ocml but sqrt -- the azimuth's sine and cosine are envmap_core.hpp's
// sincos_0_2pi, the diffuse half of the sampler is kernel_math.hpp's cosine_about.  render_body.inc calls it under PLS (the GLS
// instantiations of render_kernel_x), kernels_blocks.hip's plastic_eval_kernel runs it over arrays (pbrt_hip_plastic_eval_device), and
// tests/test_plastic_host.py compiles THIS TEXT for the host -- a stand-alone program in which __device__ and __forceinline__ mean
// nothing -- and holds it to a float64 restatement; the device's words must equal the host's bit for bit (tests/test_plastic_gpu.py).
//
//   nf  = the geometric normal turned towards wo; cos_o = wo . nf, cos_i = wi . nf, wh = (wo + wi) / |wo + wi|, c = wh . nf
//   D   = alpha^2 / (pi e^2), e = c^2 (alpha^2 - 1) + 1
//   Lambda(w) = (sqrt(1 + alpha^2 (1 - cos^2) / cos^2) - 1) / 2, G = 1 / (1 + Lambda(wo) + Lambda(wi))
//   F   = glass_fresnel(min(|wi . wh|, 1), 1 / 1.5)
//   f   = Kd / pi + Ks (D G F / (4 cos_o cos_i)); zero where cos_i <= 0, cos_o <= 0 or wo + wi = 0
//   pdf = 1/2 cos_i / pi + 1/2 D c / (4 wo . wh); zero where f is
//   sample (u1, u2): u1 < 1/2: u = min(2 u1, 1 - eps), wi = cosine_about(nf, u, u2); else u = min(2 u1 - 1, 1 - eps) and wh is drawn from
//   D cos theta (pbrt-v3's sampleVisibleArea = false): tan^2 = alpha^2 u / (1 - u), cos theta = 1 / sqrt(1 + tan^2), sin theta = sqrt(max(0,
//   1 - cos^2 theta)), phi = 2 pi u2, wh in the frame cosine_about builds about nf, wi = -wo + wh (2 wo . wh); no sample where wo . wh <= 0
#pragma once
#include "envmap_core.hpp"
#include "kernel_math.hpp"

namespace pbrt_hip {
namespace {
namespace plastic {

constexpr float kEtaRatio = 1.0f / 1.5f;  // eta_i / eta_t of the coat: index 1 outside, pbrt-v3's fixed 1.5 inside
constexpr float kAlphaMin = 1e-3f, kAlphaMax = 1.0f;  // what pbrt_hip_scene_create takes (include/pbrt_hip.h)

// the two tangents cosine_about builds about n (pbrt-v3 CoordinateSystem), in its operations
__device__ __forceinline__ void frame_about(V3 n, V3 &v2, V3 &v3) {
  if (fabsf(n.x) > fabsf(n.y)) {
    float l = sqrtf(n.x * n.x + n.z * n.z);
    v2 = {-n.z / l, 0.f, n.x / l};
  } else {
    float l = sqrtf(n.y * n.y + n.z * n.z);
    v2 = {0.f, n.z / l, -n.y / l};
  }
  v3 = cross(n, v2);
}

// D of a half vector whose cosine to the normal is c; a2 = alpha^2
__device__ __forceinline__ float ggx_d(float c, float a2) {
  const float e = (c * c) * (a2 - 1.0f) + 1.0f;
  return a2 / (envmap::kPi * (e * e));
}
// Lambda of a direction whose cosine to the normal is cs > 0
__device__ __forceinline__ float ggx_lambda(float cs, float a2) {
  const float c2 = cs * cs;
  const float t2 = fmaxf(0.f, 1.0f - c2) / c2;
  return 0.5f * (sqrtf(1.0f + a2 * t2) - 1.0f);
}

// f(wo, wi) and the density the sampler below has for wi; both zero where the pair does not reflect
__device__ __forceinline__ void eval(V3 nf, V3 wo, V3 wi, V3 kd, V3 ks, float alpha, V3 &f, float &pdf) {
  f = {0.f, 0.f, 0.f};
  pdf = 0.f;
  const float cos_o = dot(wo, nf), cos_i = dot(wi, nf);
  if (!(cos_i > 0.f) || !(cos_o > 0.f)) return;
  const V3 hs = wo + wi;
  const float h2 = dot(hs, hs);
  if (!(h2 > 0.f)) return;
  const V3 wh = hs / sqrtf(h2);
  const float c = dot(wh, nf), oh = dot(wo, wh);
  if (!(oh > 0.f)) return;
  const float a2 = alpha * alpha;
  const float D = ggx_d(c, a2);
  const float G = 1.0f / ((1.0f + ggx_lambda(cos_o, a2)) + ggx_lambda(cos_i, a2));
  float F, ct;
  glass_fresnel(fminf(fabsf(dot(wi, wh)), 1.0f), kEtaRatio, F, ct);
  const float spec = ((D * G) * F) / ((4.0f * cos_o) * cos_i);
  f = kd * kInvPi + ks * spec;
  pdf = 0.5f * (cos_i * kInvPi) + 0.5f * ((D * c) / (4.0f * oh));
}

// wi from the pair every matte bounce draws; false: the chosen lobe has no direction for it (wi is then not to be used)
__device__ __forceinline__ bool sample(V3 nf, V3 wo, float u1, float u2, float alpha, V3 &wi) {
  if (u1 < 0.5f) {
    const float u = fminf(2.0f * u1, kOneMinusEps);
    return cosine_about(nf, u, u2, wi) != 0.f;
  }
  const float u = fminf(2.0f * u1 - 1.0f, kOneMinusEps);
  const float tan2 = ((alpha * alpha) * u) / (1.0f - u);
  const float ct = 1.0f / sqrtf(1.0f + tan2);
  const float st = sqrtf(fmaxf(0.f, 1.0f - ct * ct));
  float sp, cp;
  envmap::sincos_0_2pi(envmap::kTwoPi * u2, &sp, &cp);
  V3 v2, v3;
  frame_about(nf, v2, v3);
  const V3 wh = (v2 * (st * cp) + v3 * (st * sp)) + nf * ct;
  const float oh = dot(wo, wh);
  if (!(oh > 0.f)) return false;
  wi = -wo + wh * (2.0f * oh);
  return true;
}

// One bounce: the direction, its density, and the throughput's factor f cos_i / pdf.  false: the sample dies
__device__ __forceinline__ bool sample_f(V3 nf, V3 wo, float u1, float u2, V3 kd, V3 ks, float alpha, V3 &wi, V3 &weight, float &pdf) {
  V3 f;
  weight = {0.f, 0.f, 0.f};
  pdf = 0.f;
  if (!sample(nf, wo, u1, u2, alpha, wi)) return false;
  eval(nf, wo, wi, kd, ks, alpha, f, pdf);
  if (!(pdf > 0.f)) return false;
  weight = f * (dot(wi, nf) / pdf);
  return true;
}

}  // namespace plastic
}  // namespace
}  // namespace pbrt_hip
