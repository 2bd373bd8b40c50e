// substrate_bsdf.hpp -- the substrate material's BSDF (pbrt-v3 SubstrateMaterial, a FresnelBlend BSDF): a diffuse base that
// darkens at grazing angles and is scaled by 1 - Ks, under a glossy coat of ONE Trowbridge-Reitz lobe of isotropic width alpha with
// Schlick's Fresnel term on the specular colour Ks and NO masking term.  Written in the manner of plastic_bsdf.hpp: fp32, one fixed order
// of operations, built with -ffp-contract=off, nothing of libm / ocml but sqrt.  The direction sampler IS plastic's (plastic::sample: a
// cosine lobe for u1 < 1/2, else wh from D cos theta and wi = wo reflected about wh; pbrt-v3's sampleVisibleArea = false) and D is
// plastic::ggx_d: both are called, not copied.  render_body.inc calls this under PLS through `coated` below, kernels_blocks.hip's
// substrate_eval_kernel runs it over arrays (pbrt_hip_substrate_eval_device), and tests/test_substrate_host.py compiles THIS TEXT for the
// host and holds it to a float64 restatement; the device's words must equal the host's bit for bit (tests/test_substrate_gpu.py).
//
//   nf, cos_o, cos_i, hs = wo + wi, wh, c = wh . nf, oh = wo . wh, a2 = alpha^2: as plastic::eval forms them
//   p5(x) = ((x x) (x x)) x;  ih = min(|wi . wh|, 1)
//   f = pdf = 0 where cos_i <= 0, cos_o <= 0, hs = 0, oh <= 0 or ih is not > 0
//   dsc  = (k2823 (1 - p5(1 - 0.5 cos_i))) (1 - p5(1 - 0.5 cos_o)), k2823 = the float nearest 28 / (23 pi)
//   D    = ggx_d(c, a2);  spec = D / ((4 ih) max(cos_i, cos_o));  sch = Ks + (1 - Ks) p5(1 - ih)
//   f    = (Kd (1 - Ks)) dsc + sch spec
//   pdf  = 1/2 (cos_i / pi) + 1/2 ((D c) / (4 oh))        (plastic's density: the same sampler)
#pragma once
#include "plastic_bsdf.hpp"

namespace pbrt_hip {
namespace {
namespace substrate {

constexpr float k2823 = (float)(28.0 / (23.0 * 3.14159265358979323846));  // the float nearest 28 / (23 pi), formed in double

__device__ __forceinline__ float p5(float x) { return ((x * x) * (x * x)) * x; }

// f(wo, wi) and the density plastic::sample has for wi; both zero where the pair does not reflect
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
  const float ih = fminf(fabsf(dot(wi, wh)), 1.0f);
  if (!(ih > 0.f)) return;
  const float a2 = alpha * alpha;
  const float D = plastic::ggx_d(c, a2);
  const float dsc = (k2823 * (1.0f - p5(1.0f - 0.5f * cos_i))) * (1.0f - p5(1.0f - 0.5f * cos_o));
  const float spec = D / ((4.0f * ih) * fmaxf(cos_i, cos_o));
  const float s5 = p5(1.0f - ih);
  const V3 one = {1.0f, 1.0f, 1.0f};
  const V3 sch = ks + (one - ks) * s5;
  f = (kd * (one - ks)) * dsc + sch * spec;
  pdf = 0.5f * (cos_i * kInvPi) + 0.5f * ((D * c) / (4.0f * oh));
}

}  // namespace substrate

// The two materials that share plastic's direction sampler, as render_body.inc's one vertex branch takes them: `coat` (the material's type
// word says substrate) selects the BSDF and nothing else.  With coat = false every operation is plastic::sample_f's, in its order (a
// direction below the surface has pdf 0 there and dies either way).
namespace coated {

__device__ __forceinline__ void eval(bool coat, V3 nf, V3 wo, V3 wi, V3 kd, V3 ks, float alpha, V3 &f, float &pdf) {
  if (coat) substrate::eval(nf, wo, wi, kd, ks, alpha, f, pdf);
  else plastic::eval(nf, wo, wi, kd, ks, alpha, f, pdf);
}

// One bounce: plastic's direction, its density, and the throughput's factor f cos_i / pdf.  false: the sample dies
__device__ __forceinline__ bool sample_f(bool coat, V3 nf, V3 wo, float u1, float u2, V3 kd, V3 ks, float alpha, V3 &wi, V3 &weight, float &pdf) {
  V3 f;
  weight = {0.f, 0.f, 0.f};
  pdf = 0.f;
  if (!plastic::sample(nf, wo, u1, u2, alpha, wi)) return false;
  const float cos_i = dot(wi, nf);
  if (!(cos_i > 0.f)) return false;
  eval(coat, nf, wo, wi, kd, ks, alpha, f, pdf);
  if (!(pdf > 0.f)) return false;
  weight = f * (cos_i / pdf);
  return true;
}

}  // namespace coated

namespace substrate {

__device__ __forceinline__ bool sample_f(V3 nf, V3 wo, float u1, float u2, V3 kd, V3 ks, float alpha, V3 &wi, V3 &weight, float &pdf) {
  return coated::sample_f(true, nf, wo, u1, u2, kd, ks, alpha, wi, weight, pdf);
}

}  // namespace substrate
}  // namespace
}  // namespace pbrt_hip
