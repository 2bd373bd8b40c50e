// cephes_poly.hpp -- the Cephes single-precision polynomials (sinf / cosf / atanf / asinf) written out: one fixed order of fp32
// operations, no call into libm / ocml -- the same bits on the CPU and on the GPU.  The product's one copy: the kernels' for a sphere's
// (u, v) and cosine sampling (kernel_math.hpp), the environment map's on the host and on the device (envmap_core.hpp).
#pragma once
#include <hip/hip_runtime.h>  // (every unit of the library is compiled by hipcc as HIP, the host-only ones included)
#define PBRT_HD __host__ __device__ inline __attribute__((always_inline))

namespace pbrt_hip {

PBRT_HD float poly_sin(float x) {  // |x| <= pi / 4
  const float z = x * x;
  float p = -1.9515295891e-4f * z + 8.3321608736e-3f;
  p = p * z - 1.6666654611e-1f;
  return (p * z) * x + x;
}
PBRT_HD float poly_cos(float x) {  // |x| <= pi / 4
  const float z = x * x;
  float p = 2.443315711809948e-5f * z - 1.388731625493765e-3f;
  p = p * z + 4.166664568298827e-2f;
  return ((p * z) * z - 0.5f * z) + 1.0f;
}
PBRT_HD float poly_atan_pos(float x) {  // x >= 0 (+inf included): atan(x) in [0, pi / 2]
  float y0 = 0.f;
  if (x > 2.414213562373095f) {
    y0 = 1.5707963267948966f;
    x = -(1.0f / x);
  } else if (x > 0.4142135623730950f) {
    y0 = 0.7853981633974483f;
    x = (x - 1.0f) / (x + 1.0f);
  }
  const float z = x * x;
  float p = 8.05374449538e-2f * z - 1.38776856032e-1f;
  p = p * z + 1.99777106478e-1f;
  p = p * z - 3.33329491539e-1f;
  return y0 + ((p * z) * x + x);
}
PBRT_HD float poly_asin_small(float a) {  // |a| <= 0.5
  const float z = a * a;
  float p = 4.2163199048e-2f * z + 2.4181311049e-2f;
  p = p * z + 4.5470025998e-2f;
  p = p * z + 7.4953002686e-2f;
  p = p * z + 1.6666752422e-1f;
  return (p * z) * a + a;
}
PBRT_HD float poly_acos(float x) {  // x in [-1, 1]
  if (x < -0.5f) return 3.14159265358979323846f - 2.0f * poly_asin_small(sqrtf(0.5f * (1.0f + x)));
  if (x > 0.5f) return 2.0f * poly_asin_small(sqrtf(0.5f * (1.0f - x)));
  return 1.5707963267948966f - poly_asin_small(x);
}

}  // namespace pbrt_hip
