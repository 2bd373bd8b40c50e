// light_map.hpp -- the mapped lights' sample (pbrt-v3 ProjectionLight and GonioPhotometricLight): a point light at p whose
// intensity is multiplied by an image looked up in the direction from the light to the shaded point.  Written once, in the manner of
// spot_light.hpp: fp32, one fixed order of operations, built with -ffp-contract=off, nothing of libm / ocml but sqrtf / floorf / fminf /
// fmaxf and the polynomials of cephes_poly.hpp.  kernel_path.hpp's sample_light_mapped and the mapped branch of sample_light_general are
// built on it (both called under PLS alone: the GLS instantiations of render_kernel_x), kernels_blocks.hip's light_map_eval_kernel runs it
// over arrays (pbrt_hip_light_map_eval_device), and tests/test_light_map_host.py compiles THIS TEXT for the host and holds it to a float64
// restatement; the device's words must equal the host's bit for bit (tests/test_light_map_gpu.py).
//
//   wi, cs, dist2, dist, tmax and scale = (cs / dist2) nL: operation for operation spot::sample's, the point light's
//   d = -wi, w = M d, each row (M0 dx + M1 dy) + M2 dz (envmap::lookup's order)
//   projection   no light unless w.z > 1e-3; px = (w.x / w.z) inv_tan, py = (w.y / w.z) inv_tan; no light unless -sx <= px <= sx and
//                -sy <= py <= sy (a NaN is "no light"); s = (px + sx) / (2 sx), t = (py + sy) / (2 sy)
//   goniometric  yc = clamp(w.y, -1, 1), theta = poly_acos(yc); phi as envmap::lookup forms it from (w.x, w.z); s = phi (1 / 2 pi),
//                t = 1 - theta (1 / pi)
//   rgb = image::lookup(pool, rows, s, t); no sample where all three channels are 0.  The caller multiplies rgb in LAST, so a texel of
//   exactly 1 changes no bit of the point light's estimate
#pragma once
#include "image_lookup.hpp"
#include "kernel_math.hpp"

namespace pbrt_hip {
namespace {
namespace lightmap {

constexpr uint32_t kProjection = 0u, kGoniometric = 1u;  // pbrt_hip_light_map.kind
constexpr float kMinZ = 1e-3f;                           // a projection lights nothing at or behind this depth of its own space

// the light-space direction w of a projection onto its screen window: false = outside (or behind the light)
__device__ __forceinline__ bool project(V3 w, float inv_tan, float sx, float sy, float &s, float &t) {
  if (!(w.z > kMinZ)) return false;
  const float px = (w.x / w.z) * inv_tan, py = (w.y / w.z) * inv_tan;
  if (!(px >= -sx && px <= sx && py >= -sy && py <= sy)) return false;
  s = (px + sx) / (2.0f * sx);
  t = (py + sy) / (2.0f * sy);
  return true;
}

// the light-space direction w on the goniometric map: the light's +y is the pole, phi runs from +x towards +z
__device__ __forceinline__ void gonio(V3 w, float &s, float &t) {
  const float ax = w.x < 0.f ? -w.x : w.x, az = w.z < 0.f ? -w.z : w.z;
  float phi = (ax == 0.f && az == 0.f) ? 0.f : poly_atan_pos(az / ax);  // first quadrant (ax == 0: atan(+inf) = pi / 2)
  if (w.x < 0.f) phi = 3.14159265358979323846f - phi;
  if (w.z < 0.f) phi = 6.28318530717958647692f - phi;
  const float yc = w.y < -1.0f ? -1.0f : (w.y > 1.0f ? 1.0f : w.y);
  const float theta = poly_acos(yc);
  s = phi * 0.15915494309189533577f;  // 1 / (2 pi)
  t = 1.0f - theta * kInvPi;
}

// The light sample at shading point po with normal nf (turned towards the viewer).  r0, r1, r2 = {a row of world_to_light, inv_tan / sx /
// sy}; t0 and offset_bits = the image slot's type row and its place in `pool` (image_lookup.hpp).  false: geometry, the window or a black
// texel rules the light out, and no shadow ray is cast (the outputs are then not to be used).
__device__ __forceinline__ bool sample(V3 po, V3 nf, V3 p, uint32_t kind, float4 r0, float4 r1, float4 r2, float nLf, const float4 *pool, float4 t0,
                                       float offset_bits, V3 &wi, float &tmax, float &scale, float &s, float &t, V3 &rgb) {
  V3 dv = p - po;
  float dist2 = dot(dv, dv);
  if (!(dist2 > 0.f)) return false;
  float dist = sqrtf(dist2);
  wi = dv / dist;
  float cs = dot(wi, nf);
  if (!(cs > 0.f)) return false;
  const V3 d = -wi;
  const V3 w = {(r0.x * d.x + r0.y * d.y) + r0.z * d.z, (r1.x * d.x + r1.y * d.y) + r1.z * d.z, (r2.x * d.x + r2.y * d.y) + r2.z * d.z};
  if (kind == kProjection) {
    if (!project(w, r0.w, r1.w, r2.w, s, t)) return false;
  } else {
    gonio(w, s, t);
  }
  image::lookup(pool, t0, offset_bits, s, t, &rgb.x, &rgb.y, &rgb.z);
  if (rgb.x == 0.f && rgb.y == 0.f && rgb.z == 0.f) return false;
  scale = (cs / dist2) * nLf;
  tmax = dist * kShadowShrink;
  return true;
}

}  // namespace lightmap
}  // namespace
}  // namespace pbrt_hip
