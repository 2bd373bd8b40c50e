// rgb_xyz.hpp -- RGB -> XYZ (core/spectrum.rs:139-145), the one statement of it: merge_kernel and film_from_acc_kernel (kernels.hip) and the
// host's pbrt_hip_film_from_acc (capi_render.cpp) convert a pixel's radiance sum with it.  Plain fp32 in this order of operations.
#pragma once
#include <hip/hip_runtime.h>

namespace pbrt_hip {
struct Xyz {
  float x, y, z;
};
__host__ __device__ inline Xyz rgb_to_xyz(float r, float g, float b) {
  Xyz c;
  c.x = 0.412453f * r + 0.357580f * g + 0.180423f * b;
  c.y = 0.212671f * r + 0.715160f * g + 0.072169f * b;
  c.z = 0.019334f * r + 0.119193f * g + 0.950227f * b;
  return c;
}
}  // namespace pbrt_hip
