// image_texture.cpp -- see image_texture.hpp; and the debug hooks pbrt_hip_image_lookup_eval_host / _device.
#include "image_texture.hpp"

#include <cmath>
#include <cstring>

#include "capi_internal.hpp"
#include "envmap.hpp"
#include "image_lookup.hpp"

namespace pbrt_hip {

int image_check(const pbrt_hip_image_texture &t, const std::string &what) {
  if (t.width == 0 || t.height == 0) return fail(PBRT_HIP_ERR_INVALID, what + "image texture: width and height must be >= 1");
  if (t.width > PBRT_HIP_IMAGE_MAX_SIZE || t.height > PBRT_HIP_IMAGE_MAX_SIZE)
    return fail(PBRT_HIP_ERR_LIMIT, what + "image texture: width or height above 16384");
  if ((uint64_t)t.width * t.height > PBRT_HIP_IMAGE_MAX_TEXELS) return fail(PBRT_HIP_ERR_LIMIT, what + "image texture: more than 2^26 texels");
  if (t.wrap > PBRT_HIP_WRAP_BLACK) return fail(PBRT_HIP_ERR_INVALID, what + "image texture: unknown wrap mode (0 repeat, 1 clamp, 2 black)");
  if (t.filter > PBRT_HIP_TEXFILTER_BILINEAR) return fail(PBRT_HIP_ERR_INVALID, what + "image texture: unknown filter (0 point, 1 bilinear)");
  if (!std::isfinite(t.su) || !std::isfinite(t.sv) || !std::isfinite(t.du) || !std::isfinite(t.dv))
    return fail(PBRT_HIP_ERR_INVALID, what + "image texture: the mapping is not finite");
  if (!t.rgb) return fail(PBRT_HIP_ERR_INVALID, what + "image texture: no texels (rgb is NULL)");
  return PBRT_HIP_OK;
}

int image_check_texels(const pbrt_hip_image_texture &t, const std::string &what) {
  for (size_t i = 0; i < 3 * (size_t)t.width * t.height; i++)
    if (!std::isfinite(t.rgb[i]) || !(t.rgb[i] >= 0.f))
      return fail(PBRT_HIP_ERR_INVALID, what + "image texture: texel " + std::to_string(i / 3) + " is not finite or is negative");
  return PBRT_HIP_OK;
}

int image_check_totals(uint32_t n_slots, uint64_t n_texels, const std::string &what) {
  if (n_slots > PBRT_HIP_IMAGE_MAX_SLOTS) return fail(PBRT_HIP_ERR_LIMIT, what + "more than 64 image textures");
  if (n_texels > PBRT_HIP_IMAGE_MAX_TEXELS) return fail(PBRT_HIP_ERR_LIMIT, what + "the image textures hold more than 2^26 texels together");
  return PBRT_HIP_OK;
}

void image_pack(const pbrt_hip_image_texture &t, std::vector<float4> *pool, float4 rows[3]) {
  const size_t first = pool->size(), n = (size_t)t.width * t.height;
  pool->resize(first + n);
  for (size_t i = 0; i < n; i++) (*pool)[first + i] = make_float4(t.rgb[3 * i], t.rgb[3 * i + 1], t.rgb[3 * i + 2], 0.f);
  image::encode(t.width, t.height, t.wrap, t.filter, t.su, t.sv, t.du, t.dv, (uint32_t)first, &rows[0], &rows[1], &rows[2]);
}

int light_map_check(const pbrt_hip_light_map &m, const std::string &what) {
  if (m.kind > PBRT_HIP_LIGHT_MAP_GONIOMETRIC) return fail(PBRT_HIP_ERR_INVALID, what + "light map: unknown kind (0 projection, 1 goniometric)");
  for (int k = 0; k < 9; k++)
    if (!std::isfinite(m.world_to_light[k])) return fail(PBRT_HIP_ERR_INVALID, what + "light map: world_to_light is not finite");
  if (envmap_orthonormal_error(m.world_to_light) > kEnvOrthonormalTolerance)
    return fail(PBRT_HIP_ERR_INVALID, what + "light map: world_to_light is not orthonormal to 1e-4 (a rotation is expected)");
  const float window[3] = {m.inv_tan, m.sx, m.sy};
  for (int k = 0; k < 3; k++) {
    if (m.kind == PBRT_HIP_LIGHT_MAP_PROJECTION && (!std::isfinite(window[k]) || !(window[k] > 0.f)))
      return fail(PBRT_HIP_ERR_INVALID, what + "light map: a projection's inv_tan, sx and sy must be finite and > 0");
    if (m.kind == PBRT_HIP_LIGHT_MAP_GONIOMETRIC && !(window[k] == 0.f))
      return fail(PBRT_HIP_ERR_INVALID, what + "light map: a goniometric record's inv_tan, sx and sy must be 0");
  }
  return PBRT_HIP_OK;
}

namespace {
// the hooks' common part: the records checked as scene creation checks them, packed as it packs them
int pack_records(const pbrt_hip_image_texture *records, uint32_t n_records, uint32_t which, int64_t n, const float *uv, float *rgb, const std::string &what,
                 std::vector<float4> *pool, std::vector<float4> *rows) {
  if (!records || n_records == 0 || which >= n_records || n < 0 || (n && (!uv || !rgb))) return fail(PBRT_HIP_ERR_INVALID, what + "null argument, no record or a record number out of range");
  uint64_t texels = 0;
  for (uint32_t i = 0; i < n_records; i++) {
    if (records[i].type != PBRT_HIP_TEXTURE_IMAGE) return fail(PBRT_HIP_ERR_INVALID, what + "not an image texture's record (its first word must be 4)");
    const int rc = image_check(records[i], what);
    if (rc) return rc;
    texels += (uint64_t)records[i].width * records[i].height;
  }
  int rc = image_check_totals(n_records, texels, what);
  if (rc) return rc;
  for (uint32_t i = 0; i < n_records; i++)
    if ((rc = image_check_texels(records[i], what))) return rc;
  rows->resize(3 * (size_t)n_records);
  for (uint32_t i = 0; i < n_records; i++) image_pack(records[i], pool, rows->data() + 3 * (size_t)i);
  return PBRT_HIP_OK;
}
}  // namespace

}  // namespace pbrt_hip

using namespace pbrt_hip;

extern "C" {

int pbrt_hip_image_lookup_eval_host(const pbrt_hip_image_texture *records, uint32_t n_records, uint32_t which, int64_t n, const float *uv, float *rgb) {
  return guarded([&]() -> int {
    std::vector<float4> pool, rows;
    const int rc = pack_records(records, n_records, which, n, uv, rgb, "image_lookup_eval_host: ", &pool, &rows);
    if (rc) return rc;
    const float4 t0 = rows[3 * (size_t)which], t1 = rows[3 * (size_t)which + 1], t2 = rows[3 * (size_t)which + 2];
    for (int64_t i = 0; i < n; i++) {
      const float tu = uv[2 * i], tv = uv[2 * i + 1];
      const float ss = t1.w * tu + t2.y, tt = t2.x * tv + t2.z;  // (render_body.inc's statement)
      image::lookup(pool.data(), t0, t2.w, ss, tt, &rgb[3 * i], &rgb[3 * i + 1], &rgb[3 * i + 2]);
    }
    return PBRT_HIP_OK;
  });
}

int pbrt_hip_image_lookup_eval_device(int device, const pbrt_hip_image_texture *records, uint32_t n_records, uint32_t which, int64_t n, const float *uv,
                                      float *rgb) {
  return guarded([&]() -> int {
    std::vector<float4> pool, rows;
    const int rc = pack_records(records, n_records, which, n, uv, rgb, "image_lookup_eval_device: ", &pool, &rows);
    if (rc) return rc;
    if (pbrt_hip_device_count() <= 0) return fail(PBRT_HIP_ERR_NO_DEVICE, "image_lookup_eval_device: no HIP device (there is no CPU fallback)");
    if (n == 0) return PBRT_HIP_OK;
    HIP_TRY(hipSetDevice(device));
    DevBuf<float4> d_pool, d_rows;
    DevBuf<float> d_uv, d_rgb;
    HIP_TRY(d_pool.alloc(pool.size()));
    HIP_TRY(d_rows.alloc(rows.size()));
    HIP_TRY(d_uv.alloc(2 * (size_t)n));
    HIP_TRY(d_rgb.alloc(3 * (size_t)n));
    const hipStream_t stream = nullptr;  // the device's default stream
    HIP_TRY(hipMemcpyAsync(d_pool.p, pool.data(), 16 * pool.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_rows.p, rows.data(), 16 * rows.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_uv.p, uv, 8 * (size_t)n, hipMemcpyHostToDevice, stream));
    HIP_TRY(launch_image_lookup_eval(d_rows.p + 3 * (size_t)which, d_pool.p, n, d_uv.p, d_rgb.p, stream));
    HIP_TRY(hipMemcpyAsync(rgb, d_rgb.p, 12 * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}

}  // extern "C"
