// envmap.hpp -- the host side of an environment-map infinite light: the record's validation and the tables
// envmap_core.hpp samples from.  capi_scene.cpp uploads what is built here; the debug hooks of pbrt_hip_debug.h export it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pbrt_hip.h"

namespace pbrt_hip {

// Every refusal of the record (include/pbrt_hip.h): 0, or the status with the message set; `what` prefixes it
int envmap_check(const pbrt_hip_envmap &e, const std::string &what);
int envmap_check_image(const float *rgb, uint32_t width, uint32_t height, const std::string &what);
// How far the rows of a row-major 3 x 3 are from orthonormal (the largest |row_i . row_j - delta_ij|, in double), and the one bound on it:
// what envmap_check accepts as a rotation is what the scene parser passes on as one
constexpr double kEnvOrthonormalTolerance = 1e-4;
double envmap_orthonormal_error(const float m[9]);

// pbrt-v3's Distribution2D over f[row][col] = luminance x sin(pi (row + 1/2) / H) (f = the sine alone for a map that is black everywhere):
// sums in double, tables rounded to float once; texels = {r, g, b, p_uv = f / mean(f)}
struct EnvTables {
  std::vector<float4> texels;      // W x H
  std::vector<float> marginal;     // H + 1
  std::vector<float> conditional;  // H x (W + 1)
};
void envmap_build_tables(const float *rgb, uint32_t width, uint32_t height, EnvTables *out);

}  // namespace pbrt_hip
