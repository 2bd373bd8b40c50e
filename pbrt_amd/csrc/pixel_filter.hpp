// pixel_filter.hpp -- the weighted pixel filters on the host: the record's checks, the kinds' default radii and the
// 16 x 16 table the render kernels read (pixel_filter.cpp).  Plain C++, nothing of HIP.
#pragma once
#include <string>

#include "../../include/pbrt_hip.h"

namespace pbrt_hip {

// PBRT_HIP_OK, or the refusal of a record (`what` prefixes the message, which holds "filter")
int filter_check(const pbrt_hip_pixel_filter &f, const std::string &what);
const char *filter_kind_name(uint32_t kind);  // "triangle" ... "sinc"; "box" for anything else
// pbrt-v3's default radius of a kind (both axes): 2 for the triangle, the Gaussian and the Mitchell filter, 4 for the sinc
float filter_default_radius(uint32_t kind);
// the radius a render description's width stands for under filter `f`: 0 = the kind's default
inline float filter_radius_of(const pbrt_hip_pixel_filter &f, float width) { return width == 0.f ? filter_default_radius(f.kind) : width; }
// the filter at (x, y), radii rx, ry, in double (pbrt-v3's Evaluate)
double filter_eval(const pbrt_hip_pixel_filter &f, double x, double y, double rx, double ry);
// Film::new's table (film.rs:113-123): out[iy * 16 + ix] = the filter at ((ix + 0.5) rx / 16, (iy + 0.5) ry / 16), evaluated in double
// and rounded to float once
void filter_table(const pbrt_hip_pixel_filter &f, float rx, float ry, float out[256]);

}  // namespace pbrt_hip
