// kernel_path.hpp -- what render_body.inc is built from beside the walk: the one-light direct estimate and the environment map's
// light, the path state and its HBM records, the samplers, and the wide filters' film_add and film_add_sample.
#pragma once
#include "envmap_core.hpp"
#include "image_lookup.hpp"
#include "kernel_walk.hpp"
#include "light_map.hpp"
#include "plastic_bsdf.hpp"
#include "scene_tables.hpp"
#include "substrate_bsdf.hpp"
#include "sphere_light.hpp"
#include "spot_light.hpp"

namespace pbrt_hip {
namespace {

// One light of UniformSampleOneLight.  false: geometry rules the light out.
// mis: the estimate weighted with the power heuristic pl^2 / (pl^2 + pb^2), pl = this strategy's density for the
// direction (light picked with 1 / nL), pb = cos / pi the BSDF's; delta lights keep weight 1
__device__ __forceinline__ bool sample_light(const DevScene &S, uint32_t li, V3 po, V3 nf, V3 kd, float u1, float u2,
                                             float nLf, V3 &Ld, V3 &wi, float &tmax, const bool mis = false) {
  const float4 l0 = light_row(S, li, 0u);
  const float4 l3 = light_row(S, li, 3u);
  const uint32_t type = __float_as_uint(l0.x);
  const V3 p0 = {l0.y, l0.z, l0.w};
  const V3 lc = xyz(l3);
  const V3 f = kd * kInvPi;
  if (type == kDevLightPoint) {
    V3 dv = p0 - po;
    float dist2 = dot(dv, dv);
    if (!(dist2 > 0.f)) return false;
    float dist = sqrtf(dist2);
    wi = dv / dist;
    float cs = dot(wi, nf);
    if (!(cs > 0.f)) return false;
    float scale = (cs / dist2) * nLf;
    Ld = (f * lc) * scale;
    tmax = dist * kShadowShrink;
    return true;
  } else if (type == kDevLightDistant) {
    wi = p0;
    float cs = dot(wi, nf);
    if (!(cs > 0.f)) return false;
    float scale = cs * nLf;
    Ld = (f * lc) * scale;
    tmax = kInf;
    return true;
  } else if (type == kDevLightInfinite) {
    float z = cosine_about(nf, u1, u2, wi);
    if (z == 0.f) return false;
    Ld = (kd * lc) * nLf;
    if (mis) Ld = Ld * (1.0f / (1.0f + nLf * nLf));  // pl = pb / nL
    tmax = kInf;
    return true;
  } else {
    // (kDevLightTriangle.  kDevLightEnv, an environment map, never arrives here: a kernel with ENV takes it before
    // this chain, and a scene with a map is rendered by a family with ENV alone: render_variant.hpp render_family)
    const float4 l1 = light_row(S, li, 1u);
    const float4 l2 = light_row(S, li, 2u);
    const float4 l4 = light_row(S, li, 4u);
    float su0 = sqrtf(u1);
    float b0 = 1.0f - su0;
    float b1 = u2 * su0;
    float b2 = (1.0f - b0) - b1;
    V3 pl = (p0 * b0 + xyz(l1) * b1) + xyz(l2) * b2;
    V3 dv = pl - po;
    float dist2 = dot(dv, dv);
    if (!(dist2 > 0.f)) return false;
    float dist = sqrtf(dist2);
    wi = dv / dist;
    float cs = dot(wi, nf);
    if (!(cs > 0.f)) return false;
    float cl = -dot(wi, xyz(l4));
    if (!(cl > 0.f)) return false;
    float scale = (((cs * cl) * l1.w) / dist2) * nLf;
    if (mis) {
      const float pl = (dist2 / (cl * l1.w)) / nLf, pbl = cs * kInvPi;
      scale = scale * mis_weight_light(pl, pbl);
    }
    Ld = (f * lc) * scale;
    tmax = dist * kShadowShrink;
    return true;
  }
}

// A spot light at a matte vertex (spot_light.hpp): sample_light's outputs for light li, which the caller has found to be of
// type kDevLightSpot.  Called under PLS alone -- the GLS instantiations of render_kernel_x --, so that sample_light and the instantiations
// built from it keep their machine code.  A delta light: no MIS weight.
__device__ __forceinline__ bool sample_light_spot(const DevScene &S, uint32_t li, V3 po, V3 nf, V3 kd, float nLf, V3 &Ld, V3 &wi, float &tmax) {
  const float4 l0 = light_row(S, li, 0u);
  const float4 l1 = light_row(S, li, 1u);
  const float4 l2 = light_row(S, li, 2u);
  const float4 l3 = light_row(S, li, 3u);
  const V3 f = kd * kInvPi;
  float fall, scale;
  if (!spot::sample(po, nf, mk(l0.y, l0.z, l0.w), xyz(l1), l1.w, l2.x, nLf, wi, tmax, fall, scale)) return false;
  Ld = (f * xyz(l3)) * scale;
  return true;
}

// A sphere light at a matte vertex (sphere_light.hpp): sample_light's outputs for light li, which the caller has found to be of
// type kDevLightSphere, from the pair (u1, u2) the vertex drew for its light.  Called under PLS alone, as sample_light_spot is.  An area
// light: with mis the estimate carries pl^2 / (pl^2 + pb^2), pl = pdf_omega / nL, pb = cos / pi, as an emissive triangle's does.
__device__ __forceinline__ bool sample_light_sphere(const DevScene &S, uint32_t li, V3 po, V3 nf, V3 kd, float u1, float u2, float nLf, V3 &Ld, V3 &wi, float &tmax,
                                                    const bool mis) {
  const float4 l0 = light_row(S, li, 0u);
  const float4 l1 = light_row(S, li, 1u);
  const float4 l3 = light_row(S, li, 3u);
  const V3 f = kd * kInvPi;
  float scale, pdf, cs;
  if (!sphere_light::sample(po, nf, mk(l0.y, l0.z, l0.w), l1.x, u1, u2, nLf, wi, tmax, scale, pdf, cs)) return false;
  if (mis) {
    const float pl = pdf / nLf, pbl = cs * kInvPi;
    scale = scale * mis_weight_light(pl, pbl);
  }
  Ld = (f * xyz(l3)) * scale;
  return true;
}

// A mapped light (light_map.hpp) of type kDevLightProjection or kDevLightGonio: the point light's (lc scale) and the image's
// rgb apart, for the two callers to multiply in their own order.  `textures` and `texels` are RenderParams' rows and texel pool.
__device__ __forceinline__ bool sample_light_map(const DevScene &S, const float4 *textures, const float4 *texels, uint32_t li, V3 po, V3 nf, float nLf, V3 &lc,
                                                 float &scale, V3 &rgb, V3 &wi, float &tmax) {
  const float4 l0 = light_row(S, li, 0u);
  const float4 l1 = light_row(S, li, 1u);
  const float4 l2 = light_row(S, li, 2u);
  const float4 l3 = light_row(S, li, 3u);
  const float4 l4 = light_row(S, li, 4u);
  const uint32_t slot = __float_as_uint(l3.w);
  const float4 t0 = textures[3u * slot], t2 = textures[3u * slot + 2u];
  float s, t;
  lc = xyz(l3);
  return lightmap::sample(po, nf, mk(l0.y, l0.z, l0.w), __float_as_uint(l0.x) - kDevLightProjection, l1, l2, l4, nLf, texels, t0, t2.w, wi, tmax, scale, s, t, rgb);
}
// ... at a matte vertex: sample_light's outputs.  Called under PLS alone, as sample_light_spot is.  A delta light: no MIS weight.
__device__ __forceinline__ bool sample_light_mapped(const DevScene &S, const float4 *textures, const float4 *texels, uint32_t li, V3 po, V3 nf, V3 kd, float nLf,
                                                    V3 &Ld, V3 &wi, float &tmax) {
  const V3 f = kd * kInvPi;
  V3 lc, rgb;
  float scale;
  if (!sample_light_map(S, textures, texels, li, po, nf, nLf, lc, scale, rgb, wi, tmax)) return false;
  Ld = ((f * lc) * scale) * rgb;
  return true;
}

// sample_light's sibling for a BSDF that is not Lambertian (the plastic material; called under PLS alone, so that
// sample_light and the instantiations built from it keep their machine code): the same light from the same (u1, u2), WITHOUT a BSDF
// factor and without a MIS weight -- Lg = Li cos_i nL / pdf_l, the caller multiplies by f(wo, wi) -- and pl = the density that MIS
// compares with the BSDF's for wi (light picked with 1 / nL), 0 for the point and the distant light.  The operations are sample_light's.
// (textures, texels: RenderParams' rows and texel pool, which a mapped light's image is read from)
__device__ __forceinline__ bool sample_light_general(const DevScene &S, const float4 *textures, const float4 *texels, uint32_t li, V3 po, V3 nf, float u1, float u2,
                                                     float nLf, V3 &Lg, V3 &wi, float &tmax, float &pl) {
  const float4 l0 = light_row(S, li, 0u);
  const float4 l3 = light_row(S, li, 3u);
  const uint32_t type = __float_as_uint(l0.x);
  const V3 p0 = {l0.y, l0.z, l0.w};
  const V3 lc = xyz(l3);
  pl = 0.f;
  if (type == kDevLightPoint) {
    V3 dv = p0 - po;
    float dist2 = dot(dv, dv);
    if (!(dist2 > 0.f)) return false;
    float dist = sqrtf(dist2);
    wi = dv / dist;
    float cs = dot(wi, nf);
    if (!(cs > 0.f)) return false;
    Lg = lc * ((cs / dist2) * nLf);
    tmax = dist * kShadowShrink;
    return true;
  } else if (type == kDevLightDistant) {
    wi = p0;
    float cs = dot(wi, nf);
    if (!(cs > 0.f)) return false;
    Lg = lc * (cs * nLf);
    tmax = kInf;
    return true;
  } else if (type == kDevLightInfinite) {
    // the constant infinite light: a cosine-sampled direction, pdf_l = cos_i / pi, so Lg = Le pi nL
    float z = cosine_about(nf, u1, u2, wi);
    if (z == 0.f) return false;
    Lg = (lc * envmap::kPi) * nLf;
    pl = (z * kInvPi) / nLf;
    tmax = kInf;
    return true;
  } else if (dev_light_beyond_chain(type)) {
    if (type == kDevLightSpot) {
      // a spot light: the point light with the cone's falloff, a delta light like it (pl stays 0)
      const float4 l1 = light_row(S, li, 1u);
      const float4 l2 = light_row(S, li, 2u);
      float fall, scale;
      if (!spot::sample(po, nf, p0, xyz(l1), l1.w, l2.x, nLf, wi, tmax, fall, scale)) return false;
      Lg = lc * scale;
      return true;
    }
    if (type == kDevLightSphere) {
      // a sphere light: an area light, pl = pdf_omega / nL for the caller's MIS rule
      const float4 l1 = light_row(S, li, 1u);
      float scale, pdf, cs;
      if (!sphere_light::sample(po, nf, p0, l1.x, u1, u2, nLf, wi, tmax, scale, pdf, cs)) return false;
      Lg = lc * scale;
      pl = pdf / nLf;
      return true;
    }
    // a mapped light: the point light times its image, a delta light like it (pl stays 0)
    V3 lm, rgb;
    float scale;
    if (!sample_light_map(S, textures, texels, li, po, nf, nLf, lm, scale, rgb, wi, tmax)) return false;
    Lg = (lm * scale) * rgb;
    return true;
  } else {
    // an emissive triangle (kDevLightTriangle; the environment map's kDevLightEnv never arrives: a scene with plastic and a map is refused)
    const float4 l1 = light_row(S, li, 1u);
    const float4 l2 = light_row(S, li, 2u);
    const float4 l4 = light_row(S, li, 4u);
    float su0 = sqrtf(u1);
    float b0 = 1.0f - su0;
    float b1 = u2 * su0;
    float b2 = (1.0f - b0) - b1;
    V3 pt = (p0 * b0 + xyz(l1) * b1) + xyz(l2) * b2;
    V3 dv = pt - po;
    float dist2 = dot(dv, dv);
    if (!(dist2 > 0.f)) return false;
    float dist = sqrtf(dist2);
    wi = dv / dist;
    float cs = dot(wi, nf);
    if (!(cs > 0.f)) return false;
    float cl = -dot(wi, xyz(l4));
    if (!(cl > 0.f)) return false;
    Lg = lc * ((((cs * cl) * l1.w) / dist2) * nLf);
    pl = (dist2 / (cl * l1.w)) / nLf;
    tmax = dist * kShadowShrink;
    return true;
  }
}

// ---- the environment-map infinite light (the arithmetic is envmap_core.hpp's, shared with the host).  Used by the ENV
// instantiation alone (kernels_env.hip render_kernel_env): nothing below is reachable from render_kernel / render_kernel_x. ----
__device__ __forceinline__ envmap::Map env_map(const RenderParams &R) {
  envmap::Map m;
  m.texels = R.env_texels;
  m.marginal = R.env_marginal;
  m.conditional = R.env_conditional;
  m.W = R.env_w;
  m.H = R.env_h;
  for (int k = 0; k < 9; k++) m.M[k] = R.env_m[k];
  return m;
}
// Le(d) = c * texel of the direction; *pdf = its density over solid angle
__device__ __forceinline__ V3 env_le(const RenderParams &R, V3 d, float *pdf) {
  const envmap::Map m = env_map(R);
  float st;
  const float4 tx = m.texels[envmap::lookup(m, d.x, d.y, d.z, &st)];
  *pdf = envmap::pdf_omega(tx.w, st);
  return mk(R.env_c[0], R.env_c[1], R.env_c[2]) * xyz(tx);
}
// The map as the light of UniformSampleOneLight, from the (u1, u2) every light gets: Ld = (f Le) ((cos / pdf) nL), with MIS weighted by
// pl^2 / (pl^2 + pb^2), pl = pdf / nL, pb = cos / pi, in the operation order of sample_light's triangle branch; the shadow ray of a distant light
__device__ __forceinline__ bool sample_env_light(const RenderParams &R, V3 nf, V3 kd, float u1, float u2, float nLf, V3 &Ld, V3 &wi, float &tmax, const bool mis) {
  const envmap::Map m = env_map(R);
  float st;
  const float4 tx = m.texels[envmap::sample(m, u1, u2, &wi.x, &wi.y, &wi.z, &st)];
  const float pdf = envmap::pdf_omega(tx.w, st);
  const float cs = dot(wi, nf);
  if (!(cs > 0.f) || !(pdf > 0.f)) return false;
  const V3 f = kd * kInvPi;
  float scale = (cs / pdf) * nLf;
  if (mis) {
    const float pl = pdf / nLf, pbl = cs * kInvPi;
    scale = scale * mis_weight_light(pl, pbl);
  }
  Ld = (f * (mk(R.env_c[0], R.env_c[1], R.env_c[2]) * xyz(tx))) * scale;
  tmax = kInf;
  return true;
}

enum : uint32_t { ST_NEW = 0, ST_CLOSEST = 1, ST_SHADOW = 2, ST_DONE = 3, ST_FETCH = 4 };

// Path state of one work item (a CHUNK of a pixel's samples) while its lane is busy walking the BVH:
// five 16-byte records per lane in HBM, laid out [record][lane] per wave so that a wave's access is one coalesced
// 1 KB transaction.  It is loaded and stored only in the service stage (once per ray, against ~41 gather steps),
// which keeps these 20 dwords out of the registers that are live across the traversal loop.
struct PathState {
  V3 L, beta;  // radiance and throughput of the sample in flight
  V3 wi_next;  // prepared bounce direction (taken after the shadow ray returns)
  Pcg rng;     // stratified sampler: rng.inc is recomputed from the item, only the state is stored.  Sobol sampler:
               // rng.state = the pixel's scramble key | the request counter of the sample in flight << 32
  uint32_t s, bounces;
  bool specular, cont;
};
// Records 0..2 hold what every visit of the service stage needs; record 3 (beta * Ld of the light sample, added if the
// shadow ray comes back unoccluded) and record 4 (the chunk's partial film sum so far) are read and written only where
// they are used -- by the lanes whose ray was a shadow ray, and once per finished sample -- and never sit in registers
// beside the shading arithmetic (r01 loaded all five on every visit: 6 more live VGPRs, 40 % more record traffic).
// The lane's five records lie 1 KB apart around a wave-uniform base that points at record 2: -2048 ... +2048 bytes, all
// within the immediate offset of a global load / store.  The address is formed at each access from the uniform base (an
// SGPR pair) and the lane's 32-bit byte offset, which is made opaque so that base + offset is not hoisted out of the
// kernel's loop as a 64-bit per-lane pointer: one long-lived VGPR instead of the four the compiler kept (a pointer pair for
// records 0..3 and a second one for record 4, which was out of immediate range from record 0).
struct LaneRecords {
  char *base;    // wave-uniform: record 2 of lane 0
  uint32_t off;  // lane * 16
  uint32_t lds;  // the LDS form of records 0..2 (below): LDS byte address of record 0 of lane 0; else unused
};
constexpr int32_t kRecL = -2048, kRecBeta = -1024, kRecWi = 0, kRecLpend = 1024, kRecSum = 2048;  // byte offsets
__device__ __forceinline__ float4 rec_load(const LaneRecords &r, int32_t k) {
  uint32_t o = r.off;
  asm volatile("" : "+v"(o));
  return *reinterpret_cast<const float4 *>(r.base + o + k);
}
__device__ __forceinline__ void rec_store(const LaneRecords &r, int32_t k, float4 v) {
  uint32_t o = r.off;
  asm volatile("" : "+v"(o));
  *reinterpret_cast<float4 *>(r.base + o + k) = v;
}
// The LDS form of records 0..2 (device_types.h kLdsPathRecords; LDS = render_body.inc's LREC): record k of the lane at r.lds + k KB +
// lane * 16, r.lds = the LDS byte address behind the walk's stack rows -- a link-time constant, so the record's place is the
// ds_read_b128 / ds_write_b128's immediate offset and the address register holds the lane's 16 bytes alone (opaque, as above).
struct alignas(16) LdsRec { float x, y, z, w; };  // (four scalar accesses of a 16-byte-aligned record: the compiler joins them into one b128)
typedef __attribute__((address_space(3))) LdsRec lds_rec;
template <bool LDS>
__device__ __forceinline__ float4 path_rec_load(const LaneRecords &r, int32_t k) {
  if (!LDS) return rec_load(r, k);
  uint32_t o = r.off;
  asm volatile("" : "+v"(o));
  const lds_rec *p = (const lds_rec *)(uintptr_t)(r.lds + (uint32_t)(k - kRecL) + o);
  return make_float4(p->x, p->y, p->z, p->w);
}
template <bool LDS>
__device__ __forceinline__ void path_rec_store(const LaneRecords &r, int32_t k, float4 v) {
  if (!LDS) { rec_store(r, k, v); return; }
  uint32_t o = r.off;
  asm volatile("" : "+v"(o));
  lds_rec *p = (lds_rec *)(uintptr_t)(r.lds + (uint32_t)(k - kRecL) + o);
  p->x = v.x; p->y = v.y; p->z = v.z; p->w = v.w;
}
template <bool LDS = false>
__device__ __forceinline__ void path_store(const LaneRecords &rec, const PathState &P) {
  path_rec_store<LDS>(rec, kRecL, make_float4(P.L.x, P.L.y, P.L.z,
                                    __uint_as_float(P.s | (P.bounces << 20) | (P.specular ? 1u << 30 : 0u) | (P.cont ? 1u << 31 : 0u))));
  path_rec_store<LDS>(rec, kRecBeta, make_float4(P.beta.x, P.beta.y, P.beta.z, __uint_as_float((uint32_t)P.rng.state)));
  path_rec_store<LDS>(rec, kRecWi, make_float4(P.wi_next.x, P.wi_next.y, P.wi_next.z, __uint_as_float((uint32_t)(P.rng.state >> 32))));
}
template <bool LDS = false>
__device__ __forceinline__ void path_load(const LaneRecords &rec, PathState &P) {
  const float4 a = path_rec_load<LDS>(rec, kRecL), b = path_rec_load<LDS>(rec, kRecBeta), c = path_rec_load<LDS>(rec, kRecWi);
  P.L = {a.x, a.y, a.z};
  P.beta = {b.x, b.y, b.z};
  P.wi_next = {c.x, c.y, c.z};
  const uint32_t w = __float_as_uint(a.w);
  P.s = w & 0xfffffu;
  P.bounces = (w >> 20) & 0x3ffu;
  P.specular = (w >> 30) & 1u;
  P.cont = (w >> 31) & 1u;
  P.rng.state = (uint64_t)__float_as_uint(b.w) | ((uint64_t)__float_as_uint(c.w) << 32);
}

// ---- samplers (DESIGN.md 3.1 stratified, 3.10 padded (0,2)-sequence) ----
// (K = 2^kb chunks per pixel, kb = RenderParams::chunk_shift: device_types.h sample_chunk_shift)
__device__ __forceinline__ uint32_t chunk_begin(uint32_t c, uint32_t spp, uint32_t kb) { return (c * spp) >> kb; }  // spp <= 2^20, c <= 16
__device__ __forceinline__ uint32_t mix32(uint32_t v) {  // lowbias32
  v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
  return v;
}
// One 2-D request of the sample in flight.  Sobol: point (s ^ mask_j) of the first two Sobol' dimensions -- the
// van der Corput sequence (bit reversal) and the dimension whose generator matrix has the columns v, v ^ v >> 1, ...
// (Joe-Kuo s = 1, a = 0, m = 1) -- XOR-scrambled with keys hashed from the pixel and the request number j.
// SND (sampler 2): requests 0 .. 15 of a sample take their own Sobol' dimensions (2j, 2j + 1) from the
// generator matrices in `mat` at point index s, XOR-scrambled per dimension; later requests are the padded ones below.
// Sampler 3: dimension d of the Halton sampler at point index i under the pixel's key: the radical inverse of i in
// base b = the d-th prime, the D digits the frame's largest sample index can have (b^D > spp_mask) each scrambled by a random linear
// bijection of Z_b, all higher digits -- zeros for every sample of the frame -- as one random tail.  tab = {b, K, ceil(2^32 / b), bits of
// 1 / b^K} (host_math.hpp halton_table; b and the reciprocal are used): n / b by the reciprocal, the estimate is the quotient or one more.
__device__ __forceinline__ float halton_dim(const uint32_t *tab, uint32_t d, uint32_t i, uint32_t key, uint32_t spp_mask) {
  const uint4 t = reinterpret_cast<const uint4 *>(tab)[d];
  const uint32_t b = t.x;
  uint32_t h = mix32(key + (d + 1u) * 0x9e3779b9u);
  if (b == 2u) return fminf(kOneMinusEps, (float)(__builtin_bitreverse32(i) ^ h) * 2.3283064365386963e-10f);
  uint32_t v = 0u, n = i, pw = 1u;
  do {
    pw *= b;
    uint32_t q = __umulhi(n, t.z);
    if (q * b > n) q--;
    const uint32_t a = n - q * b;
    n = q;
    h = h * 0x9e3779b1u + 0x7f4a7c15u;
    const uint32_t w = a * (1u + (((h >> 16) * (b - 1u)) >> 16)) + (((h & 0xffffu) * b) >> 16);  // a m + c < b^2
    uint32_t wq = __umulhi(w, t.z);
    if (wq * b > w) wq--;
    v = v * b + (w - wq * b);
  } while (pw <= spp_mask);
  h = h * 0x9e3779b1u + 0x7f4a7c15u;
  return fminf(kOneMinusEps, ((float)v + (float)h * 2.3283064365386963e-10f) * (1.0f / (float)pw));
}
// HAL (with SND): the table sampler in use is the Halton one (sampler 3), `mat` its table
template <bool SND = false>
__device__ __forceinline__ void sample_2d(PathState &P, const bool sobol, const uint32_t spp_mask, float &u1, float &u2, const uint32_t *mat = nullptr,
                                          const bool halton = false) {
  if (!sobol) {
    u1 = pcg_float(P.rng);
    u2 = pcg_float(P.rng);
    return;
  }
  if (SND && halton && (uint32_t)(P.rng.state >> 32) < kSobolNdRequests) {
    const uint32_t key = (uint32_t)P.rng.state, d0 = 2u * (uint32_t)(P.rng.state >> 32);
    P.rng.state += 1ull << 32;  // next request
    u1 = halton_dim(mat, d0, P.s, key, spp_mask);
    u2 = halton_dim(mat, d0 + 1u, P.s, key, spp_mask);
    return;
  }
  if (SND && (uint32_t)(P.rng.state >> 32) < kSobolNdRequests) {
    const uint32_t key = (uint32_t)P.rng.state, d0 = 2u * (uint32_t)(P.rng.state >> 32);
    P.rng.state += 1ull << 32;  // next request
    // x = XOR of the columns of dimension d0's matrix at the set bits of the sample index, y likewise for d0 + 1.  Branch-free
    // over the bits a sample index of this frame can have (wave-uniform count), four columns per 16-byte load: the loads of a
    // request are in flight together, where a loop over the set bits waited for two dependent loads per bit (r03: sampler 2
    // at 64 spp 369 -> 4xx Msamples/s, profiles/r03z_variant_throughput.txt)
    const uint4 *m0 = reinterpret_cast<const uint4 *>(mat + d0 * 32u);
    uint32_t x = 0u, y = 0u;
    const uint32_t nq = ((uint32_t)__popc(spp_mask) + 3u) >> 2;  // groups of four bits below 2^ceil(log2 spp)
    for (uint32_t q = 0u, k = P.s; q < nq; q++, k >>= 4) {
      const uint4 cx = m0[q], cy = m0[8u + q];
      x ^= (cx.x & (0u - (k & 1u))) ^ (cx.y & (0u - ((k >> 1) & 1u))) ^ (cx.z & (0u - ((k >> 2) & 1u))) ^ (cx.w & (0u - ((k >> 3) & 1u)));
      y ^= (cy.x & (0u - (k & 1u))) ^ (cy.y & (0u - ((k >> 1) & 1u))) ^ (cy.z & (0u - ((k >> 2) & 1u))) ^ (cy.w & (0u - ((k >> 3) & 1u)));
    }
    x ^= mix32(key + (d0 + 1u) * 0x9e3779b9u);
    y ^= mix32(key + (d0 + 2u) * 0x9e3779b9u);
    u1 = fminf(kOneMinusEps, (float)x * 2.3283064365386963e-10f);
    u2 = fminf(kOneMinusEps, (float)y * 2.3283064365386963e-10f);
    return;
  }
  const uint32_t a = mix32((uint32_t)P.rng.state + (uint32_t)(P.rng.state >> 32) * 0x9e3779b9u);
  P.rng.state += 1ull << 32;  // next request
  const uint32_t i = P.s ^ (a & spp_mask);
  uint32_t x = __builtin_bitreverse32(i), y = 0u;
  for (uint32_t k = i, v = 0x80000000u; k != 0u; k >>= 1, v ^= v >> 1)
    if (k & 1u) y ^= v;
  x ^= mix32(a ^ 0x68e31da4u);
  y ^= mix32(a ^ 0xb5297a4du);
  u1 = fminf(kOneMinusEps, (float)x * 2.3283064365386963e-10f);
  u2 = fminf(kOneMinusEps, (float)y * 2.3283064365386963e-10f);
}
template <bool SND = false>
__device__ __forceinline__ float sample_1d(PathState &P, const bool sobol, const uint32_t spp_mask, const uint32_t *mat = nullptr, const bool halton = false) {
  if (!sobol) return pcg_float(P.rng);
  if (SND && halton && (uint32_t)(P.rng.state >> 32) < kSobolNdRequests) {  // (a 1-D request takes the first coordinate of its pair)
    const float u = halton_dim(mat, 2u * (uint32_t)(P.rng.state >> 32), P.s, (uint32_t)P.rng.state, spp_mask);
    P.rng.state += 1ull << 32;
    return u;
  }
  float u1, u2;
  sample_2d<SND>(P, true, spp_mask, u1, u2, mat, halton);
  return u1;
}

// Wide box filter: 16 footprint slots per lane, two float4 records each ({r, g} and {b, samples, footprint}), a slot's records
// of the 64 lanes side by side: 16 x 2 x 64 float4 per one-wave workgroup (RenderParams::wide_slots)
constexpr uint32_t kWideSlotFloat4 = 16u * 2u * 64u;
__device__ __forceinline__ void wide_slots_clear(float4 *slots, uint32_t lane) {
  uint32_t lo = lane * 16u;
  asm volatile("" : "+v"(lo));
  char *lb = reinterpret_cast<char *>(slots + (size_t)blockIdx.x * kWideSlotFloat4) + lo;
#pragma nounroll
  for (uint32_t sl = 0u; sl < 16u; sl++) *reinterpret_cast<float4 *>(lb + sl * 2048u + 1024u) = make_float4(0.f, 0.f, 0.f, 0.f);
}
// `n` samples of summed fixed-point radiance (r, g, b) to every pixel [x0, x1) x [y0, y1) of the cropped window
__device__ __forceinline__ void film_add(unsigned long long *acc, const DevScene &S, int32_t x0, int32_t x1, int32_t y0, int32_t y1,
                                         unsigned long long r, unsigned long long g, unsigned long long b, uint32_t n) {
  for (int32_t py = y0; py < y1; py++)
    for (int32_t px = x0; px < x1; px++) {
      unsigned long long *a = acc + 4u * ((size_t)(py - S.cy0) * (size_t)(S.cx1 - S.cx0) + (size_t)(px - S.cx0));
      atomicAdd(a, r); atomicAdd(a + 1, g); atomicAdd(a + 2, b); atomicAdd(a + 3, (unsigned long long)n);
    }
}


// ---- weighted pixel filters: the footprint and the table index are filter_weight.inc's ----
#include "filter_weight.inc"
// FilmTile::AddSample of ONE sample straight to the film's accumulators: radiance (lr, lg, lb) -- sanitised, clamped to [0, 2^15] per
// component --, footprint f.  A weighted filter (R.filter_table, wave-uniform): weight w = table[iy * 16 + ix] for every pixel, q = (int64)((w
// L) 2^24) and (int64)(w 2^24) (the casts truncate toward zero: a negative lobe subtracts).  The box: w = 1 -- the same products -- and the
// fourth accumulator counts the sample.  ONE loop over the footprint's rows end to end: a second level of divergent control flow costs the
// scalar registers of its mask, and the WIDE instantiations have none to spare.
__device__ __forceinline__ void film_add_sample(const RenderParams &R, const DevScene &S, const FilterFootprint &f, float lr, float lg, float lb) {
  // (1 / rx and 1 / ry ride behind the table's 256 weights -- as kernel arguments they would be two more scalar registers held through the
  // kernel -- and are read once per sample)
  float inv_rx = 0.f, inv_ry = 0.f;
  if (R.filter_table) { inv_rx = R.filter_table[kFilterTableInvRx]; inv_ry = R.filter_table[kFilterTableInvRy]; }
  int32_t px = f.x0, py = f.x0 < f.x1 ? f.y0 : f.y1;
#pragma nounroll
  for (; py < f.y1; px = px + 1 < f.x1 ? px + 1 : f.x0, py += px == f.x0 ? 1 : 0) {
    float w = 1.0f;
    unsigned long long qw = 1ull;
    if (R.filter_table) {
      w = R.filter_table[filter_axis_index(py, f.dy, inv_ry) * 16 + filter_axis_index(px, f.dx, inv_rx)];
      qw = (unsigned long long)(long long)(w * kFixedOne);
    }
    unsigned long long *a = R.acc + 4u * ((size_t)(py - S.cy0) * (size_t)(S.cx1 - S.cx0) + (size_t)(px - S.cx0));
    atomicAdd(a, (unsigned long long)(long long)((w * lr) * kFixedOne));
    atomicAdd(a + 1, (unsigned long long)(long long)((w * lg) * kFixedOne));
    atomicAdd(a + 2, (unsigned long long)(long long)((w * lb) * kFixedOne));
    atomicAdd(a + 3, qw);
  }
}

}  // namespace
}  // namespace pbrt_hip
