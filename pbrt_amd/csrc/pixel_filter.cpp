// pixel_filter.cpp -- the weighted pixel filters on the host: pbrt-v3's TriangleFilter, GaussianFilter, MitchellFilter
// and LanczosSincFilter in double, the 16 x 16 table of Film::new (the reference builds it, core/film.rs:113-123, and has nothing that
// uses it), and the checks of a pbrt_hip_pixel_filter.  The render kernels read the table and evaluate nothing (filter_weight.inc).
#include "pixel_filter.hpp"

#include <cmath>

#include "capi_internal.hpp"

namespace pbrt_hip {
namespace {

constexpr double kPi = 3.14159265358979323846;

double gaussian_1d(double d, double r, double alpha) { return std::fmax(0.0, std::exp(-alpha * d * d) - std::exp(-alpha * r * r)); }
// pbrt-v3 MitchellFilter::Mitchell1D
double mitchell_1d(double x, double B, double C) {
  const double t = std::fabs(2.0 * x);
  if (t > 1.0) return ((-B - 6.0 * C) * t * t * t + (6.0 * B + 30.0 * C) * t * t + (-12.0 * B - 48.0 * C) * t + (8.0 * B + 24.0 * C)) / 6.0;
  return ((12.0 - 9.0 * B - 6.0 * C) * t * t * t + (-18.0 + 12.0 * B + 6.0 * C) * t * t + (6.0 - 2.0 * B)) / 6.0;
}
double sinc(double x) {
  x = std::fabs(x);
  if (x < 1e-5) return 1.0;
  return std::sin(kPi * x) / (kPi * x);
}
// pbrt-v3 LanczosSincFilter::WindowedSinc
double windowed_sinc(double x, double r, double tau) {
  x = std::fabs(x);
  if (x > r) return 0.0;
  return sinc(x) * sinc(x / tau);
}

}  // namespace

const char *filter_kind_name(uint32_t kind) {
  switch (kind) {
    case PBRT_HIP_FILTER_TRIANGLE: return "triangle";
    case PBRT_HIP_FILTER_GAUSSIAN: return "gaussian";
    case PBRT_HIP_FILTER_MITCHELL: return "mitchell";
    case PBRT_HIP_FILTER_SINC: return "sinc";
    default: return "box";
  }
}

float filter_default_radius(uint32_t kind) { return kind == PBRT_HIP_FILTER_SINC ? 4.0f : 2.0f; }

int filter_check(const pbrt_hip_pixel_filter &f, const std::string &what) {
  if (f.kind < PBRT_HIP_FILTER_TRIANGLE || f.kind > PBRT_HIP_FILTER_SINC)
    return fail(PBRT_HIP_ERR_INVALID, what + "pixel filter: unknown kind " + std::to_string(f.kind) + " (1 triangle, 2 gaussian, 3 mitchell, 4 sinc)");
  const std::string name = std::string("pixel filter \"") + filter_kind_name(f.kind) + "\": ";
  if (!std::isfinite(f.param[0]) || !std::isfinite(f.param[1])) return fail(PBRT_HIP_ERR_INVALID, what + name + "a parameter is not finite");
  if (f.kind == PBRT_HIP_FILTER_GAUSSIAN && !(f.param[0] > 0.f)) return fail(PBRT_HIP_ERR_INVALID, what + name + "alpha must be positive");
  if (f.kind == PBRT_HIP_FILTER_SINC && !(f.param[0] > 0.f)) return fail(PBRT_HIP_ERR_INVALID, what + name + "tau must be positive");
  return PBRT_HIP_OK;
}

double filter_eval(const pbrt_hip_pixel_filter &f, double x, double y, double rx, double ry) {
  switch (f.kind) {
    case PBRT_HIP_FILTER_TRIANGLE: return std::fmax(0.0, rx - std::fabs(x)) * std::fmax(0.0, ry - std::fabs(y));
    case PBRT_HIP_FILTER_GAUSSIAN: return gaussian_1d(x, rx, (double)f.param[0]) * gaussian_1d(y, ry, (double)f.param[0]);
    case PBRT_HIP_FILTER_MITCHELL: return mitchell_1d(x / rx, (double)f.param[0], (double)f.param[1]) * mitchell_1d(y / ry, (double)f.param[0], (double)f.param[1]);
    case PBRT_HIP_FILTER_SINC: return windowed_sinc(x, rx, (double)f.param[0]) * windowed_sinc(y, ry, (double)f.param[0]);
    default: return 1.0;
  }
}

void filter_table(const pbrt_hip_pixel_filter &f, float rx, float ry, float out[256]) {
  for (int iy = 0; iy < 16; iy++)
    for (int ix = 0; ix < 16; ix++)
      out[iy * 16 + ix] = (float)filter_eval(f, (ix + 0.5) * (double)rx / 16.0, (iy + 0.5) * (double)ry / 16.0, (double)rx, (double)ry);
}

}  // namespace pbrt_hip

using namespace pbrt_hip;

extern "C" int pbrt_hip_filter_table(const pbrt_hip_pixel_filter *filter, float rx, float ry, float out[256]) {
  if (!filter || !out) return fail(PBRT_HIP_ERR_INVALID, "filter_table: null argument");
  if (filter->type != PBRT_HIP_TEXTURE_FILTER) return fail(PBRT_HIP_ERR_INVALID, "filter_table: not a pixel filter's record (its first word must be 3)");
  const int rc = filter_check(*filter, "filter_table: ");
  if (rc) return rc;
  if (!(rx > 0.f) || !(ry > 0.f) || !std::isfinite(rx) || !std::isfinite(ry)) return fail(PBRT_HIP_ERR_INVALID, "filter_table: the filter radii must be positive");
  filter_table(*filter, rx, ry, out);
  return PBRT_HIP_OK;
}
