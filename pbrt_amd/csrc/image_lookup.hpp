// image_lookup.hpp -- Kd from an image, written once for the device (render_body.inc's TEX block in kernels_x.hip,
// kernels_env.hip and kernels_n.hip, the mapped lights' image of light_map.hpp (3.23), and the debug hook's kernel in kernels_blocks.hip) and for the host (image_texture.cpp:
// pbrt_hip_image_lookup_eval_host, what the CPU tests run), in the manner of envmap_core.hpp: fp32, one fixed order of operations, built
// with -ffp-contract=off, no call into libm / ocml beyond floorf / fminf / fmaxf, which are exact.
//
//   slot      three float4 rows of the texture table, as for the checkerboard: t0 = {4, W, H, wrap | filter << 8} (bits), t1 = {0, 0, 0, su},
//             t2 = {sv, du, dv, offset (bits)}: the mapping sits where the checkerboard keeps it, `offset` is the slot's first texel in the pool
//   pool      float4 {r, g, b, 0} per texel, the slots' images back to back, each row-major with row 0 = the image's TOP row
//   (s, t)    = (su u + du, sv v + dv), formed by the caller exactly as the checkerboard forms it; t = 0 is the image's BOTTOM row
//             (pbrt-v3 ImageTexture): texel row iy counted from the bottom is row H - 1 - iy of the pool
//   index     stays a FLOAT until it is clamped: ix = (uint32_t)fminf(fmaxf(xf, 0), Wf - 1).  fmaxf first: a NaN becomes 0; +-inf and
//             1e30 clamp; the cast never sees a value outside [0, W - 1]
//   point     repeat: xf = floorf((s - floorf(s)) Wf); clamp, black: xf = floorf(s Wf); black: colour 0 unless 0 <= xf <= Wf - 1 on both
//             axes (tested before the clamp: a NaN is black)
//   bilinear  texel centres at (i + 0.5) / W; pbrt-v3 MIPMap::Lookup at level 0, its own order: sx = s Wf - 0.5 from the UNREDUCED s (a
//             reduction s - floorf(s) first would round by up to 2^-25 for a small negative s, which Wf then multiplies: DESIGN.md 3.20),
//             x0 = floorf(sx), dx = fminf(fmaxf(sx - x0, 0), 1) (a no-op for a finite sx; inf - inf = NaN -> 0), neighbours c = x0, x0 + 1
//             with weights 1 - dx, dx; repeat: c <- c - Wf floorf(c / Wf) (pbrt-v3's Mod; exact while |c| < 2^24); black: weight 0 unless
//             0 <= c <= Wf - 1; then every index is clamped as above.  Sum over j = 0, 1 (outer) and i = 0, 1 (inner), from 0:
//             acc = acc + texel(i, j) * (wx_i * wy_j)
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "cephes_poly.hpp"  // PBRT_HD

namespace pbrt_hip {
namespace image {

constexpr uint32_t kSlotType = 4u;  // PBRT_HIP_TEXTURE_IMAGE
constexpr uint32_t kWrapRepeat = 0u, kWrapClamp = 1u, kWrapBlack = 2u;
constexpr uint32_t kFilterPoint = 0u, kFilterBilinear = 1u;

PBRT_HD uint32_t bits_of(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
#endif
}
PBRT_HD float float_of(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
#endif
}

// the slot's rows from its numbers (capi_scene.cpp, the hooks)
PBRT_HD void encode(uint32_t W, uint32_t H, uint32_t wrap, uint32_t filter, float su, float sv, float du, float dv, uint32_t offset, float4 *t0, float4 *t1,
                    float4 *t2) {
  *t0 = make_float4(float_of(kSlotType), float_of(W), float_of(H), float_of(wrap | (filter << 8)));
  *t1 = make_float4(0.f, 0.f, 0.f, su);
  *t2 = make_float4(sv, du, dv, float_of(offset));
}

// a float index clamped to [0, nf - 1] and cast: NaN -> 0
PBRT_HD uint32_t clamp_index(float xf, float nf) { return (uint32_t)fminf(fmaxf(xf, 0.f), nf - 1.0f); }
PBRT_HD bool inside(float xf, float nf) { return xf >= 0.f && xf <= nf - 1.0f; }

// Kd at (s, t) from the image of the slot whose rows are t0 (type row) and whose pool offset rides in `offset_bits`
PBRT_HD void lookup(const float4 *pool, const float4 t0, float offset_bits, float s, float t, float *r, float *g, float *b) {
  const uint32_t W = bits_of(t0.y), H = bits_of(t0.z), mode = bits_of(t0.w);
  const uint32_t wrap = mode & 0xffu;
  const float Wf = (float)W, Hf = (float)H;
  const float4 *img = pool + bits_of(offset_bits);
  if ((mode >> 8) == kFilterPoint) {
    const float xf = wrap == kWrapRepeat ? floorf((s - floorf(s)) * Wf) : floorf(s * Wf);
    const float yf = wrap == kWrapRepeat ? floorf((t - floorf(t)) * Hf) : floorf(t * Hf);
    const uint32_t ix = clamp_index(xf, Wf), iy = clamp_index(yf, Hf);
    const float4 c = img[(H - 1u - iy) * W + ix];
    const bool lit = wrap != kWrapBlack || (inside(xf, Wf) && inside(yf, Hf));
    *r = lit ? c.x : 0.f; *g = lit ? c.y : 0.f; *b = lit ? c.z : 0.f;
    return;
  }
  const float sx = s * Wf - 0.5f, sy = t * Hf - 0.5f;
  const float x0 = floorf(sx), y0 = floorf(sy);
  const float dx = fminf(fmaxf(sx - x0, 0.f), 1.0f), dy = fminf(fmaxf(sy - y0, 0.f), 1.0f);  // (finite sx: already in [0, 1); NaN -> 0)
  float ar = 0.f, ag = 0.f, ab = 0.f;
  for (int j = 0; j < 2; j++) {
    float cy = j ? y0 + 1.0f : y0, wy = j ? dy : 1.0f - dy;
    if (wrap == kWrapRepeat) cy = cy - Hf * floorf(cy / Hf);
    if (wrap == kWrapBlack && !inside(cy, Hf)) wy = 0.f;
    const uint32_t row = (H - 1u - clamp_index(cy, Hf)) * W;
    for (int i = 0; i < 2; i++) {
      float cx = i ? x0 + 1.0f : x0, wx = i ? dx : 1.0f - dx;
      if (wrap == kWrapRepeat) cx = cx - Wf * floorf(cx / Wf);
      if (wrap == kWrapBlack && !inside(cx, Wf)) wx = 0.f;
      const float4 c = img[row + clamp_index(cx, Wf)];
      const float w = wx * wy;
      ar = ar + c.x * w; ag = ag + c.y * w; ab = ab + c.z * w;
    }
  }
  *r = ar; *g = ag; *b = ab;
}

}  // namespace image
}  // namespace pbrt_hip
