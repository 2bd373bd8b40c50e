// kernel_math.hpp -- the kernels' smallest building blocks: constants, vectors, PCG32, a sphere's (u, v), the Fresnel term, cosine sampling,
// the sphere test.  Device code in the anonymous namespace of pbrt_hip (the kernels' mangled names carry it), as kernel_walk.hpp and
// kernel_path.hpp, which build on it.
//
// The reference has no renderer (core/api.rs:446-453 is a comment); the arithmetic below is
// DESIGN.md section 3, and is written so that every fp32 operation happens in the same order as
// in the CPU oracle: build with -ffp-contract=off, never -ffast-math.  No MFMA: this is branchy
// gather work (BASELINE.json north_star).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cephes_poly.hpp"

namespace pbrt_hip {
namespace {

constexpr float kInf = __builtin_huge_valf();
constexpr float kRayTMin = 1e-4f;
constexpr float kSpawnEps = 1e-4f;
constexpr float kShadowShrink = 0.9999f;
constexpr float kBoxPad = 0x1.000004p+0f;  // MEANT as 1 + 2^-19, IS 1 + 2^-22 (six hex digits are 24 bits: DESIGN.md 3.4's finding, section 12 item 4): the node test's far-side pad (pbrt-v3 pads by 1 + 2 gamma(3) = 1 + 6 * 2^-24)
constexpr float kOwnPad = 0x1.000001p+0f;  // MEANT as 1 + 2^-21, IS 1: the literal is 1 + 2^-24 and rounds to 1 (DESIGN.md 3.5's finding, section 12 item 4): the own-box rule's pad (3.5), strictly inside kBoxPad
constexpr float kInvPi = 0.31830988618379067154f;
constexpr float kPiOver4 = 0.78539816339744830961f;
constexpr float kOneMinusEps = 0x1.fffffcp-1f;  // 1 - f32::EPSILON = 1 - 2^-23, core/rng.rs:19 (NOT pbrt-v3's 1 - 2^-24)
constexpr uint32_t kNoPrim = 0xffffffffu;

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 mk(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {(a.y * b.z) - (a.z * b.y), (a.z * b.x) - (a.x * b.z), (a.x * b.y) - (a.y * b.x)};
}
__device__ __forceinline__ V3 unit(V3 a) { return a / sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 xyz(float4 v) { return {v.x, v.y, v.z}; }

// ---- PCG32, core/rng.rs:46-93 ----
struct Pcg {
  uint64_t state, inc;
};
__device__ __forceinline__ uint32_t pcg_u32(Pcg &r) {
  uint64_t old = r.state;
  r.state = old * 0x5851f42d4c957f2dULL + r.inc;
  uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
  uint32_t rot = (uint32_t)(old >> 59u);
  return (xs >> rot) | (xs << ((0u - rot) & 31u));
}
__device__ __forceinline__ void pcg_seq(Pcg &r, uint64_t seq) {
  r.state = 0;
  r.inc = (seq << 1) | 1u;
  pcg_u32(r);
  r.state += 0x853c49e6748fea9bULL;
  pcg_u32(r);
}
__device__ __forceinline__ float pcg_float(Pcg &r) {
  return fminf(kOneMinusEps, (float)pcg_u32(r) * 2.3283064365386963e-10f);
}

// ---- a sphere's (u, v) for 2-D textures (pbrt-v3 Sphere::Intersect: u = phi / 2 pi with phi = atan2(y, x) in [0, 2 pi),
// v = (theta - pi) / (0 - pi) with theta = acos(z)) on the unit normal n = (p - c) / r, the sphere's own frame being the world's axes.  atan
// and asin are the Cephes single-precision polynomials of cephes_poly.hpp (measured against float64, DESIGN.md 3.6: atan within 2.0 ulp,
// 1.4e-7 absolute; acos within 3.0e-7 absolute, 1.26 ulp of a result near 2.1), the same operations on CPU and GPU. ----
__device__ __forceinline__ void sphere_uv(float nx, float ny, float nz, float *u, float *v) {
  const float ax = fabsf(nx), ay = fabsf(ny);
  float phi = (ax == 0.f && ay == 0.f) ? 0.f : poly_atan_pos(ay / ax);  // first quadrant (ax == 0: atan(+inf) = pi / 2)
  if (nx < 0.f) phi = 3.14159265358979323846f - phi;
  if (ny < 0.f) phi = 6.28318530717958647692f - phi;
  const float zc = nz < -1.0f ? -1.0f : (nz > 1.0f ? 1.0f : nz);
  const float theta = poly_acos(zc);
  *u = phi * 0.15915494309189533577f;  // 1 / (2 pi)
  *v = (theta - 3.14159265358979323846f) / (0.f - 3.14159265358979323846f);
}

// Fresnel reflectance of a smooth dielectric interface and the cosine of the refracted ray (pbrt-v3 FrDielectric):
// ci = |cos theta_i| in [0, 1], r = eta_i / eta_t.  sin^2 theta_t = r^2 (1 - ci^2) >= 1 is total internal reflection: F = 1, ct = 0.
// With e = 1 / r = eta_t / eta_i the two amplitudes are (e ci - ct) / (e ci + ct) and (ci - e ct) / (ci + e ct): both denominators are
// positive whenever the ray is not totally reflected (ci = 0 gives sin^2 theta_t = r^2, so ct > 0 or F = 1 already) -- no 0 / 0 at
// grazing incidence, and r = 1 gives ct = ci up to rounding: F of the order of 1e-14.
__device__ __forceinline__ void glass_fresnel(float ci, float r, float &F, float &ct) {
  const float s2i = fmaxf(0.f, 1.0f - ci * ci);
  const float s2t = (r * r) * s2i;
  F = 1.0f;
  ct = 0.f;
  if (s2t < 1.0f) {
    ct = sqrtf(1.0f - s2t);
    const float e = 1.0f / r;
    const float rpar = (e * ci - ct) / (e * ci + ct);
    const float rper = (ci - e * ct) / (ci + e * ct);
    F = 0.5f * (rpar * rpar + rper * rper);
  }
}

// cosine-weighted direction about n; returns local z (0 => pdf 0)
__device__ __forceinline__ float cosine_about(V3 n, float u1, float u2, V3 &wi) {
  float ox = 2.0f * u1 - 1.0f, oy = 2.0f * u2 - 1.0f;
  float dx, dy;
  if (ox == 0.f && oy == 0.f) {
    dx = 0.f;
    dy = 0.f;
  } else if (fabsf(ox) > fabsf(oy)) {
    float phi = kPiOver4 * (oy / ox);
    dx = ox * poly_cos(phi);
    dy = ox * poly_sin(phi);
  } else {
    float phi = kPiOver4 * (ox / oy);
    dx = oy * poly_sin(phi);
    dy = oy * poly_cos(phi);
  }
  float zz = (1.0f - dx * dx) - dy * dy;
  float z = sqrtf(zz > 0.f ? zz : 0.f);
  V3 v2;
  if (fabsf(n.x) > fabsf(n.y)) {
    float l = sqrtf(n.x * n.x + n.z * n.z);
    v2 = {-n.z / l, 0.f, n.x / l};
  } else {
    float l = sqrtf(n.y * n.y + n.z * n.z);
    v2 = {0.f, n.z / l, -n.y / l};
  }
  V3 v3 = cross(n, v2);
  wi = (v2 * dx + v3 * dy) + n * z;
  return z;
}

// The power heuristic's two weights: pl = the density light sampling has for a direction, pb = the BSDF's.
// mis_weight_light is the light sample's pl^2 / (pl^2 + pb^2), mis_weight_bsdf the bounce ray's pb^2 / (pb^2 + pl^2).  The ends of the range:
// from pl = 2^64 upwards pl^2 is +inf and the quotient inf / inf -- the light's weight is its limit there, 1 (a tiny emitter far away or seen
// at a grazing angle: pl = d^2 / (cos A nL)), the bounce ray's comes out as 0 by itself; where BOTH squares round to zero (densities below
// 2^-75: no render reaches it, pb >= 2^-24 / pi) the quotient is 0 / 0 and the larger density takes the whole weight.  Everywhere else the
// value is the expression's, bit for bit.
__device__ __forceinline__ float mis_weight_light(float pl, float pb) {
  const float a = pl * pl, d = a + pb * pb;
  if (a == kInf) return 1.0f;
  if (d == 0.f) return pl >= pb ? 1.0f : 0.f;
  return a / d;
}
__device__ __forceinline__ float mis_weight_bsdf(float pb, float pl) {
  const float b = pb * pb, d = b + pl * pl;
  if (d == 0.f) return pb > pl ? 1.0f : 0.f;
  return b / d;
}

struct HitRec {
  float t;
  uint32_t prim;  // triangle id (or n_tris + sphere index); kNoPrim on a miss
  uint32_t slot;  // leaf slot of a triangle hit
  float b1, b2;
};

// lib.rs:181-203 quadratic with its f64 discriminant
__device__ __forceinline__ bool quadratic(float af, float bf, float cf, float &t0, float &t1) {
  double a = af, b = bf, c = cf;
  double disc = b * b - 4. * a * c;
  if (disc < 0.) return false;
  double rd = sqrt(disc);
  double q = (b < 0.) ? -0.5 * (b - rd) : -0.5 * (b + rd);
  float r0 = (float)(q / a), r1 = (float)(c / q);
  if (r0 > r1) { t0 = r1; t1 = r0; } else { t0 = r0; t1 = r1; }
  return true;
}

__device__ __forceinline__ bool sphere_hit(const float4 cr, V3 o, V3 d, float tmax, float &th) {  // cr = {centre, radius}
  V3 oc = o - xyz(cr);
  float a = dot(d, d);
  float b = 2.0f * dot(d, oc);
  float c = dot(oc, oc) - cr.w * cr.w;
  float t0, t1;
  if (!quadratic(a, b, c, t0, t1)) return false;
  th = t0;
  if (!(th > kRayTMin && th < tmax)) {
    th = t1;
    if (!(th > kRayTMin && th < tmax)) return false;
  }
  return true;
}

}  // namespace
}  // namespace pbrt_hip
