// spot_light.hpp -- the spot light's sample (pbrt-v3 SpotLight): a point light at p whose intensity falls off smoothly
// between two cones about a unit axis a that points AWAY from the light.  Written once, in the manner of plastic_bsdf.hpp: fp32, one fixed
// order of operations, built with -ffp-contract=off, nothing of libm / ocml but sqrt.  kernel_path.hpp's sample_light_spot and the spot
// branch of sample_light_general are built on it (both called under PLS alone: the GLS instantiations of render_kernel_x),
// kernels_blocks.hip's spot_eval_kernel runs it over arrays (pbrt_hip_spot_eval_device), and tests/test_spot_host.py compiles THIS TEXT
// for the host -- a stand-alone program in which __device__ and __forceinline__ mean nothing -- and holds it to a float64 restatement;
// the device's words must equal the host's bit for bit (tests/test_spot_gpu.py).
//
//   wi   = (p - po) / |p - po|, exactly as the point light's branch of sample_light forms it; cs = wi . nf
//   ct   = -(wi . a)
//   fall = 0 where ct < cos_total, 1 where ct >= cos_start, else d = (ct - cos_total) / (cos_start - cos_total), fall = (d d) (d d)
//   scale = ((cs / dist2) nL) fall -- the point light's factor with the falloff multiplied in LAST, so that fall = 1 changes no bit
//   no sample where po = p, cs <= 0 or fall = 0; tmax = dist kShadowShrink
#pragma once
#include "kernel_math.hpp"

namespace pbrt_hip {
namespace {
namespace spot {

// the falloff of a direction whose cosine to the axis is ct; cos_total <= cos_start (a hard edge where they are equal)
__device__ __forceinline__ float falloff(float ct, float cos_total, float cos_start) {
  if (ct < cos_total) return 0.f;
  if (ct >= cos_start) return 1.0f;
  const float d = (ct - cos_total) / (cos_start - cos_total);
  return (d * d) * (d * d);
}

// The light sample at shading point po with normal nf (turned towards the viewer).  false: geometry or the cone rules the light out,
// and no shadow ray is cast (the outputs are then not to be used).
__device__ __forceinline__ bool sample(V3 po, V3 nf, V3 p, V3 axis, float cos_total, float cos_start, float nLf, V3 &wi, float &tmax, float &fall,
                                       float &scale) {
  V3 dv = p - po;
  float dist2 = dot(dv, dv);
  if (!(dist2 > 0.f)) return false;
  float dist = sqrtf(dist2);
  wi = dv / dist;
  float cs = dot(wi, nf);
  if (!(cs > 0.f)) return false;
  const float ct = -dot(wi, axis);
  fall = falloff(ct, cos_total, cos_start);
  if (fall == 0.f) return false;
  scale = ((cs / dist2) * nLf) * fall;
  tmax = dist * kShadowShrink;
  return true;
}

}  // namespace spot
}  // namespace
}  // namespace pbrt_hip
