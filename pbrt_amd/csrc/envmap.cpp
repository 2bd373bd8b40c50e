// envmap.cpp -- see envmap.hpp; and the host-only debug hooks pbrt_hip_envmap_tables / pbrt_hip_envmap_eval_host.
#include "envmap.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>

#include "capi_internal.hpp"
#include "envmap_core.hpp"

namespace pbrt_hip {

int envmap_check_image(const float *rgb, uint32_t w, uint32_t h, const std::string &what) {
  if (w == 0 || h == 0) return fail(PBRT_HIP_ERR_INVALID, what + "environment map: width and height must be >= 1");
  if ((uint64_t)w * h > (1ull << 24)) return fail(PBRT_HIP_ERR_LIMIT, what + "environment map: more than 2^24 texels");
  if (!rgb) return fail(PBRT_HIP_ERR_INVALID, what + "environment map: no texels (rgb is NULL)");
  for (size_t i = 0; i < 3 * (size_t)w * h; i++)
    if (!std::isfinite(rgb[i]) || !(rgb[i] >= 0.f))
      return fail(PBRT_HIP_ERR_INVALID, what + "environment map: texel " + std::to_string(i / 3) + " is not finite or is negative");
  return PBRT_HIP_OK;
}

double envmap_orthonormal_error(const float m[9]) {
  double worst = 0.0;
  for (int i = 0; i < 3; i++)
    for (int j = i; j < 3; j++) {
      const double dt = (double)m[3 * i] * m[3 * j] + (double)m[3 * i + 1] * m[3 * j + 1] + (double)m[3 * i + 2] * m[3 * j + 2];
      worst = std::max(worst, std::fabs(dt - (i == j ? 1.0 : 0.0)));
    }
  return worst;
}

int envmap_check(const pbrt_hip_envmap &e, const std::string &what) {
  const int rc = envmap_check_image(e.rgb, e.width, e.height, what);
  if (rc) return rc;
  const float *m = e.world_to_light;
  for (int k = 0; k < 9; k++)
    if (!std::isfinite(m[k])) return fail(PBRT_HIP_ERR_INVALID, what + "environment map: world_to_light is not finite");
  if (envmap_orthonormal_error(m) > kEnvOrthonormalTolerance)
    return fail(PBRT_HIP_ERR_INVALID, what + "environment map: world_to_light is not orthonormal to 1e-4 (a rotation is expected)");
  return PBRT_HIP_OK;
}

void envmap_build_tables(const float *rgb, uint32_t W, uint32_t H, EnvTables *out) {
  const size_t n = (size_t)W * H;
  std::vector<double> f(n), sine(H);
  for (uint32_t r = 0; r < H; r++) sine[r] = std::sin(3.14159265358979323846 * ((double)r + 0.5) / (double)H);
  double total = 0.0;
  for (uint32_t r = 0; r < H; r++)
    for (uint32_t c = 0; c < W; c++) {
      const float *t = rgb + 3 * ((size_t)r * W + c);
      const double y = 0.212671 * (double)t[0] + 0.715160 * (double)t[1] + 0.072169 * (double)t[2];
      f[(size_t)r * W + c] = y * sine[r];
      total += f[(size_t)r * W + c];
    }
  if (!(total > 0.0)) {  // black everywhere: uniform over the sphere, as Distribution1D does for a zero integral
    total = 0.0;
    for (uint32_t r = 0; r < H; r++)
      for (uint32_t c = 0; c < W; c++) { f[(size_t)r * W + c] = sine[r]; total += sine[r]; }
  }
  const double mean = total / (double)n;
  out->texels.resize(n);
  out->marginal.assign((size_t)H + 1, 0.f);
  out->conditional.assign((size_t)H * (W + 1), 0.f);
  double rows_before = 0.0;
  for (uint32_t r = 0; r < H; r++) {
    double row = 0.0;
    for (uint32_t c = 0; c < W; c++) row += f[(size_t)r * W + c];
    float *cd = out->conditional.data() + (size_t)r * (W + 1);
    double before = 0.0;
    for (uint32_t c = 0; c < W; c++) {
      const size_t i = (size_t)r * W + c;
      cd[c] = row > 0.0 ? (float)(before / row) : (float)((double)c / (double)W);  // (a row of zeros: uniform, never drawn)
      before += f[i];
      out->texels[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], (float)(f[i] / mean));
    }
    cd[W] = 1.0f;
    out->marginal[r] = (float)(rows_before / total);
    rows_before += row;
  }
  out->marginal[H] = 1.0f;
}

}  // namespace pbrt_hip

using namespace pbrt_hip;

extern "C" {

int pbrt_hip_envmap_tables(const float *rgb, uint32_t width, uint32_t height, float *marginal, float *conditional, float *p_uv) {
  try {
    const int rc = envmap_check_image(rgb, width, height, "envmap_tables: ");
    if (rc) return rc;
    EnvTables t;
    envmap_build_tables(rgb, width, height, &t);
    if (marginal) std::memcpy(marginal, t.marginal.data(), t.marginal.size() * 4);
    if (conditional) std::memcpy(conditional, t.conditional.data(), t.conditional.size() * 4);
    if (p_uv)
      for (size_t i = 0; i < t.texels.size(); i++) p_uv[i] = t.texels[i].w;
    return PBRT_HIP_OK;
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

int pbrt_hip_envmap_eval_host(const float *rgb, uint32_t width, uint32_t height, const float world_to_light[9], int64_t n, const float *u12,
                              float *d, uint32_t *texel, float *le, float *pdf) {
  try {
    if (!world_to_light || n < 0 || (n && !d)) return fail(PBRT_HIP_ERR_INVALID, "envmap_eval_host: null argument");
    pbrt_hip_envmap e{};
    e.type = 1u; e.width = width; e.height = height; e.rgb = rgb;
    std::memcpy(e.world_to_light, world_to_light, sizeof e.world_to_light);
    const int rc = envmap_check(e, "envmap_eval_host: ");
    if (rc) return rc;
    EnvTables t;
    envmap_build_tables(rgb, width, height, &t);
    envmap::Map m;
    m.texels = t.texels.data(); m.marginal = t.marginal.data(); m.conditional = t.conditional.data();
    m.W = width; m.H = height;
    std::memcpy(m.M, world_to_light, sizeof m.M);
    for (int64_t i = 0; i < n; i++) {
      float st;
      uint32_t k;
      if (u12) k = envmap::sample(m, u12[2 * i], u12[2 * i + 1], &d[3 * i], &d[3 * i + 1], &d[3 * i + 2], &st);
      else k = envmap::lookup(m, d[3 * i], d[3 * i + 1], d[3 * i + 2], &st);
      const float4 tx = t.texels[k];
      if (texel) texel[i] = k;
      if (le) { le[3 * i] = tx.x; le[3 * i + 1] = tx.y; le[3 * i + 2] = tx.z; }
      if (pdf) pdf[i] = envmap::pdf_omega(tx.w, st);
    }
    return PBRT_HIP_OK;
  } catch (const std::exception &e) {
    return fail(PBRT_HIP_ERR_INTERNAL, e.what());
  }
}

}  // extern "C"
