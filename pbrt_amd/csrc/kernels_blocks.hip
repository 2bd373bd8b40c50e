// kernels_blocks.hip -- the kernels' building blocks over arrays: pbrt_hip_blocks_eval_device, the hook that lets tests/ compare the
// polynomials of cephes_poly.hpp, envmap_core.hpp's sincos_0_2pi, kernel_math.hpp's sphere_uv / glass_fresnel / cosine_about /
// sphere_hit / mis_weight_light / mis_weight_bsdf, kernel_path.hpp's sample_light and the walk's node step and triangle test (kernel_walk.hpp quad_step / walk_inv, quad_nearest.inc, tri_test.inc) with a float64 reference and with the oracle's restatements, element by element, without a render around them.  In a
// translation unit of its own so that the render and intersect kernels of kernels*.hip keep their names and their machine code.
// Beside it pbrt_hip_filter_footprint_eval_device: filter_weight.inc's footprint and table index over arrays, and the kernel of
// pbrt_hip_image_lookup_eval_device: image_lookup.hpp over arrays, and pbrt_hip_plastic_eval_device with its kernel:
// plastic_bsdf.hpp over arrays, and pbrt_hip_spot_eval_device with its kernel: spot_light.hpp over arrays (3.22), and
// pbrt_hip_light_map_eval_device with its kernel: light_map.hpp over arrays (3.23), and pbrt_hip_substrate_eval_device with its kernel:
// substrate_bsdf.hpp over arrays (3.24), and pbrt_hip_sphere_light_eval_device with its kernel: sphere_light.hpp over arrays (3.25).
//
//   blocks_eval_kernel  one element per thread, 256 threads per workgroup: switches on the op code and calls the PRODUCTION function
//                       (nothing is restated here); kBlockWidth is how many floats an element reads and writes.
#include "capi_internal.hpp"
#include "envmap_core.hpp"
#include "image_texture.hpp"
#include "kernel_math.hpp"
#include "kernel_path.hpp"
#include "kernel_walk.hpp"
#include "substrate_bsdf.hpp"

namespace pbrt_hip {
namespace {

struct BlockWidth {
  uint32_t in, out;
};
// indexed by op (include/pbrt_hip_debug.h PBRT_HIP_BLOCK_*)
constexpr BlockWidth kBlockWidth[PBRT_HIP_BLOCK_COUNT] = {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 2}, {3, 2}, {2, 2}, {5, 4}, {11, 2}, {24, 6}, {24, 6}, {16, 4}, {2, 1}, {2, 1}, {33, 8}};

__global__ void __launch_bounds__(256) blocks_eval_kernel(uint32_t op, int64_t n, uint32_t w_in, uint32_t w_out, const float *in, float *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *x = in + i * (int64_t)w_in;
  float *y = out + i * (int64_t)w_out;
  switch (op) {
    case PBRT_HIP_BLOCK_SIN: y[0] = poly_sin(x[0]); break;
    case PBRT_HIP_BLOCK_COS: y[0] = poly_cos(x[0]); break;
    case PBRT_HIP_BLOCK_ATAN_POS: y[0] = poly_atan_pos(x[0]); break;
    case PBRT_HIP_BLOCK_ACOS: y[0] = poly_acos(x[0]); break;
    case PBRT_HIP_BLOCK_SINCOS: envmap::sincos_0_2pi(x[0], &y[0], &y[1]); break;
    case PBRT_HIP_BLOCK_SPHERE_UV: sphere_uv(x[0], x[1], x[2], &y[0], &y[1]); break;
    case PBRT_HIP_BLOCK_FRESNEL: {
      float F, ct;
      glass_fresnel(x[0], x[1], F, ct);
      y[0] = F; y[1] = ct;
      break;
    }
    case PBRT_HIP_BLOCK_COSINE_ABOUT: {
      V3 wi;
      const float z = cosine_about(mk(x[0], x[1], x[2]), x[3], x[4], wi);
      y[0] = wi.x; y[1] = wi.y; y[2] = wi.z; y[3] = z;
      break;
    }
    case PBRT_HIP_BLOCK_SPHERE_HIT: {
      float th = 0.f;
      const bool hit = sphere_hit(make_float4(x[0], x[1], x[2], x[3]), mk(x[4], x[5], x[6]), mk(x[7], x[8], x[9]), x[10], th);
      y[0] = hit ? 1.0f : 0.f;
      y[1] = hit ? th : 0.f;  // (a miss leaves no distance)
      break;
    }
    case PBRT_HIP_BLOCK_QUAD_STEP:
    case PBRT_HIP_BLOCK_QUAD_STEP_PK: {
      // what trav_run does around the step: the true 1 / d and its signs, the stand-in on a parallel axis
      const uint32_t *w = reinterpret_cast<const uint32_t *>(x);  // the node's 16 words as they are
      const uint4 W0 = make_uint4(w[0], w[1], w[2], w[3]), W1 = make_uint4(w[4], w[5], w[6], w[7]), W2 = make_uint4(w[8], w[9], w[10], w[11]);
      const V3 o = mk(x[16], x[17], x[18]), d = mk(x[19], x[20], x[21]);
      const V3 inv1 = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
      const bool negx = inv1.x < 0.f, negy = inv1.y < 0.f, negz = inv1.z < 0.f;
      const V3 inv = walk_inv(d, inv1, x[22]);
      float key[4];
      bool hit[4];
      if (op == PBRT_HIP_BLOCK_QUAD_STEP) quad_step<true>(W0, W1, W2, o, inv, negx, negy, negz, x[23], key, hit);
      else quad_step<false>(W0, W1, W2, o, inv, negx, negy, negz, x[23], key, hit);
      for (int k = 0; k < 4; k++) y[k] = key[k];
      y[4] = (float)((hit[0] ? 1 : 0) | (hit[1] ? 2 : 0) | (hit[2] ? 4 : 0) | (hit[3] ? 8 : 0));
#include "quad_nearest.inc"
      y[5] = !(hit[0] || hit[1] || hit[2] || hit[3]) ? 4.0f : (n0 ? 0.f : (n1 ? 1.0f : (n2 ? 2.0f : (n3 ? 3.0f : 4.0f))));
      break;
    }
    case PBRT_HIP_BLOCK_TRI_HIT: {
      const float4 a = make_float4(x[0], x[1], x[2], 0.f), b = make_float4(x[3], x[4], x[5], 0.f), c = make_float4(x[6], x[7], x[8], 0.f);
      const V3 o = mk(x[9], x[10], x[11]), d = mk(x[12], x[13], x[14]);
      const V3 inv1 = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
      Trav T;
      T.tmax = x[15];
#include "tri_test.inc"
      y[0] = valid ? 1.0f : 0.f;
      y[1] = valid ? tsnap : 0.f;  // (zeros on a miss)
      y[2] = valid ? u : 0.f;
      y[3] = valid ? v : 0.f;
      break;
    }
    case PBRT_HIP_BLOCK_MIS_W_LIGHT: y[0] = mis_weight_light(x[0], x[1]); break;
    case PBRT_HIP_BLOCK_MIS_W_BSDF: y[0] = mis_weight_bsdf(x[1], x[0]); break;
    case PBRT_HIP_BLOCK_LIGHT: {
      // the light's records in a local table (no alignment asked of the input row), light 0 of a scene that holds nothing else
      float4 rec[kLightRows];
      for (int k = 0; k < (int)kLightRows; k++) rec[k] = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
      DevScene S{};
      S.lights = rec;
      const V3 po = mk(x[20], x[21], x[22]), nf = mk(x[23], x[24], x[25]), kd = mk(x[26], x[27], x[28]);
      V3 Ld = {0.f, 0.f, 0.f}, wi = {0.f, 0.f, 0.f};
      float tmax = 0.f;
      // mis as the render kernels hand it in: a literal (their MIS template argument)
      const bool ok = x[32] != 0.f ? sample_light(S, 0u, po, nf, kd, x[29], x[30], x[31], Ld, wi, tmax, true)
                                   : sample_light(S, 0u, po, nf, kd, x[29], x[30], x[31], Ld, wi, tmax, false);
      y[0] = ok ? 1.0f : 0.f;
      y[1] = ok ? Ld.x : 0.f; y[2] = ok ? Ld.y : 0.f; y[3] = ok ? Ld.z : 0.f;
      y[4] = ok ? wi.x : 0.f; y[5] = ok ? wi.y : 0.f; y[6] = ok ? wi.z : 0.f;
      y[7] = ok ? tmax : 0.f;
      break;
    }
    default: break;
  }
}

// filter_weight.inc over arrays (pbrt_hip_filter_footprint_eval_device): the clipped footprint of film point i ...
__global__ void __launch_bounds__(256) filter_bounds_kernel(float rx, float ry, int32_t cx0, int32_t cy0, int32_t cx1, int32_t cy1, int64_t n, const float *points,
                                                            int32_t *bounds) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const FilterFootprint f = filter_footprint(points[2 * i], points[2 * i + 1], rx, ry, cx0, cy0, cx1, cy1);
  bounds[4 * i] = f.x0; bounds[4 * i + 1] = f.y0; bounds[4 * i + 2] = f.x1; bounds[4 * i + 3] = f.y1;
}
// ... and the table index of pixel i for film point i, -1 where the pixel is outside the point's clipped footprint
__global__ void __launch_bounds__(256) filter_index_kernel(float rx, float ry, float inv_rx, float inv_ry, int32_t cx0, int32_t cy0, int32_t cx1, int32_t cy1, int64_t n,
                                                           const float *points, const int32_t *pixels, int32_t *index) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const FilterFootprint f = filter_footprint(points[2 * i], points[2 * i + 1], rx, ry, cx0, cy0, cx1, cy1);
  const int32_t px = pixels[2 * i], py = pixels[2 * i + 1];
  const bool inside = px >= f.x0 && px < f.x1 && py >= f.y0 && py < f.y1;
  index[i] = inside ? filter_axis_index(py, f.dy, inv_ry) * 16 + filter_axis_index(px, f.dx, inv_rx) : -1;
}

// image_lookup.hpp over arrays (pbrt_hip_image_lookup_eval_device): the slot's three rows, the texel pool, (u, v) -> Kd, the
// mapping formed as render_body.inc forms it
__global__ void __launch_bounds__(256) image_lookup_eval_kernel(const float4 *rows, const float4 *pool, int64_t n, const float *uv, float *rgb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 t0 = rows[0], t1 = rows[1], t2 = rows[2];
  const float tu = uv[2 * i], tv = uv[2 * i + 1];
  const float ss = t1.w * tu + t2.y, tt = t2.x * tv + t2.z;
  float r, g, b;
  image::lookup(pool, t0, t2.w, ss, tt, &r, &g, &b);
  rgb[3 * i] = r; rgb[3 * i + 1] = g; rgb[3 * i + 2] = b;
}

// plastic_bsdf.hpp over arrays (pbrt_hip_plastic_eval_device): eval at the given wi, then the sampler and its weight
__global__ void __launch_bounds__(256) plastic_eval_kernel(int64_t n, const float *in, float *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *x = in + i * (int64_t)PBRT_HIP_PLASTIC_EVAL_IN;
  float *y = out + i * (int64_t)PBRT_HIP_PLASTIC_EVAL_OUT;
#include "plastic_eval.inc"
}

// substrate_bsdf.hpp over arrays (pbrt_hip_substrate_eval_device): plastic's layout, eval at the given wi, then the sampler
__global__ void __launch_bounds__(256) substrate_eval_kernel(int64_t n, const float *in, float *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *x = in + i * (int64_t)PBRT_HIP_SUBSTRATE_EVAL_IN;
  float *y = out + i * (int64_t)PBRT_HIP_SUBSTRATE_EVAL_OUT;
#include "substrate_eval.inc"
}

// spot_light.hpp over arrays (pbrt_hip_spot_eval_device): the spot light's sample at a shading point
__global__ void __launch_bounds__(256) spot_eval_kernel(int64_t n, const float *in, float *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *x = in + i * (int64_t)PBRT_HIP_SPOT_EVAL_IN;
  float *y = out + i * (int64_t)PBRT_HIP_SPOT_EVAL_OUT;
#include "spot_eval.inc"
}

// sphere_light.hpp over arrays (pbrt_hip_sphere_light_eval_device): a sphere light's sample at a shading point and the hit side's density
__global__ void __launch_bounds__(256) sphere_light_eval_kernel(int64_t n, const float *in, float *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *x = in + i * (int64_t)PBRT_HIP_SPHERE_LIGHT_EVAL_IN;
  float *y = out + i * (int64_t)PBRT_HIP_SPHERE_LIGHT_EVAL_OUT;
#include "sphere_light_eval.inc"
}

// light_map.hpp over arrays (pbrt_hip_light_map_eval_device): a mapped light's sample at a shading point.  rows = the image
// slot's three rows, map = {a row of world_to_light, inv_tan / sx / sy} x 3
__global__ void __launch_bounds__(256) light_map_eval_kernel(uint32_t e_kind, float4 e_r0, float4 e_r1, float4 e_r2, const float4 *rows, const float4 *e_pool, int64_t n,
                                                             const float *in, float *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 e_t0 = rows[0];
  const float e_offset = rows[2].w;
  const float *x = in + i * (int64_t)PBRT_HIP_LIGHT_MAP_EVAL_IN;
  float *y = out + i * (int64_t)PBRT_HIP_LIGHT_MAP_EVAL_OUT;
#include "light_map_eval.inc"
}

}  // namespace

hipError_t launch_image_lookup_eval(const float4 *rows, const float4 *pool, int64_t n, const float *uv, float *rgb, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(image_lookup_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rows, pool, n, uv, rgb);
  return hipGetLastError();
}

hipError_t launch_filter_footprint_eval(float rx, float ry, const int32_t crop[4], int64_t n_points, const float *points, int32_t *bounds, int64_t n_pairs,
                                        const float *pair_points, const int32_t *pair_pixels, int32_t *index, hipStream_t stream) {
  if (n_points > 0) {
    hipLaunchKernelGGL(filter_bounds_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, stream, rx, ry, crop[0], crop[1], crop[2], crop[3], n_points,
                       points, bounds);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (n_pairs > 0) {
    // (1 / radius as the render's launch forms it: capi_render.cpp)
    hipLaunchKernelGGL(filter_index_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, rx, ry, 1.0f / rx, 1.0f / ry, crop[0], crop[1], crop[2],
                       crop[3], n_pairs, pair_points, pair_pixels, index);
    return hipGetLastError();
  }
  return hipSuccess;
}
}  // namespace pbrt_hip

using namespace pbrt_hip;

extern "C" int pbrt_hip_filter_footprint_eval_device(int device, float rx, float ry, const int32_t crop[4], int64_t n_points, const float *points, int32_t *bounds,
                                                     int64_t n_pairs, const float *pair_points, const int32_t *pair_pixels, int32_t *index) {
  if (n_points < 0 || n_pairs < 0 || !crop || (n_points && (!points || !bounds)) || (n_pairs && (!pair_points || !pair_pixels || !index)))
    return fail(PBRT_HIP_ERR_INVALID, "filter_footprint_eval_device: null argument or negative count");
  if (!(rx > 0.f) || !(ry > 0.f) || !(rx <= 3.0e38f) || !(ry <= 3.0e38f) || !(1.0f / rx <= 3.0e38f) || !(1.0f / ry <= 3.0e38f))
    return fail(PBRT_HIP_ERR_INVALID, "filter_footprint_eval_device: the filter radii must be positive and finite");
  if (n_points == 0 && n_pairs == 0) return PBRT_HIP_OK;
  return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> d_points, d_pair_points;
    DevBuf<int32_t> d_bounds, d_pair_pixels, d_index;
    const hipStream_t stream = nullptr;  // the device's default stream
    if (n_points) {
      HIP_TRY(d_points.alloc(2 * (size_t)n_points));
      HIP_TRY(d_bounds.alloc(4 * (size_t)n_points));
      HIP_TRY(hipMemcpyAsync(d_points.p, points, 8 * (size_t)n_points, hipMemcpyHostToDevice, stream));
    }
    if (n_pairs) {
      HIP_TRY(d_pair_points.alloc(2 * (size_t)n_pairs));
      HIP_TRY(d_pair_pixels.alloc(2 * (size_t)n_pairs));
      HIP_TRY(d_index.alloc((size_t)n_pairs));
      HIP_TRY(hipMemcpyAsync(d_pair_points.p, pair_points, 8 * (size_t)n_pairs, hipMemcpyHostToDevice, stream));
      HIP_TRY(hipMemcpyAsync(d_pair_pixels.p, pair_pixels, 8 * (size_t)n_pairs, hipMemcpyHostToDevice, stream));
    }
    HIP_TRY(launch_filter_footprint_eval(rx, ry, crop, n_points, d_points.p, d_bounds.p, n_pairs, d_pair_points.p, d_pair_pixels.p, d_index.p, stream));
    if (n_points) HIP_TRY(hipMemcpyAsync(bounds, d_bounds.p, 16 * (size_t)n_points, hipMemcpyDeviceToHost, stream));
    if (n_pairs) HIP_TRY(hipMemcpyAsync(index, d_index.p, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}

extern "C" int pbrt_hip_plastic_eval_device(int device, int64_t n, const float *in, float *out) {
  if (n < 0 || !in || !out) return fail(PBRT_HIP_ERR_INVALID, "plastic_eval_device: null argument or negative count");
  if (n == 0) return PBRT_HIP_OK;
  return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> d_in, d_out;
    HIP_TRY(d_in.alloc(PBRT_HIP_PLASTIC_EVAL_IN * (size_t)n));
    HIP_TRY(d_out.alloc(PBRT_HIP_PLASTIC_EVAL_OUT * (size_t)n));
    const hipStream_t stream = nullptr;  // the device's default stream
    HIP_TRY(hipMemcpyAsync(d_in.p, in, 4 * PBRT_HIP_PLASTIC_EVAL_IN * (size_t)n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(plastic_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, d_in.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, 4 * PBRT_HIP_PLASTIC_EVAL_OUT * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}

extern "C" int pbrt_hip_substrate_eval_device(int device, int64_t n, const float *in, float *out) {
  if (n < 0 || !in || !out) return fail(PBRT_HIP_ERR_INVALID, "substrate_eval_device: null argument or negative count");
  if (n == 0) return PBRT_HIP_OK;
  return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> d_in, d_out;
    HIP_TRY(d_in.alloc(PBRT_HIP_SUBSTRATE_EVAL_IN * (size_t)n));
    HIP_TRY(d_out.alloc(PBRT_HIP_SUBSTRATE_EVAL_OUT * (size_t)n));
    const hipStream_t stream = nullptr;  // the device's default stream
    HIP_TRY(hipMemcpyAsync(d_in.p, in, 4 * PBRT_HIP_SUBSTRATE_EVAL_IN * (size_t)n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(substrate_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, d_in.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, 4 * PBRT_HIP_SUBSTRATE_EVAL_OUT * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}

extern "C" int pbrt_hip_spot_eval_device(int device, int64_t n, const float *in, float *out) {
  if (n < 0 || !in || !out) return fail(PBRT_HIP_ERR_INVALID, "spot_eval_device: null argument or negative count");
  if (n == 0) return PBRT_HIP_OK;
  return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> d_in, d_out;
    HIP_TRY(d_in.alloc(PBRT_HIP_SPOT_EVAL_IN * (size_t)n));
    HIP_TRY(d_out.alloc(PBRT_HIP_SPOT_EVAL_OUT * (size_t)n));
    const hipStream_t stream = nullptr;  // the device's default stream
    HIP_TRY(hipMemcpyAsync(d_in.p, in, 4 * PBRT_HIP_SPOT_EVAL_IN * (size_t)n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(spot_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, d_in.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, 4 * PBRT_HIP_SPOT_EVAL_OUT * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}

extern "C" int pbrt_hip_sphere_light_eval_device(int device, int64_t n, const float *in, float *out) {
  if (n < 0 || !in || !out) return fail(PBRT_HIP_ERR_INVALID, "sphere_light_eval_device: null argument or negative count");
  if (n == 0) return PBRT_HIP_OK;
  return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    DevBuf<float> d_in, d_out;
    HIP_TRY(d_in.alloc(PBRT_HIP_SPHERE_LIGHT_EVAL_IN * (size_t)n));
    HIP_TRY(d_out.alloc(PBRT_HIP_SPHERE_LIGHT_EVAL_OUT * (size_t)n));
    const hipStream_t stream = nullptr;  // the device's default stream
    HIP_TRY(hipMemcpyAsync(d_in.p, in, 4 * PBRT_HIP_SPHERE_LIGHT_EVAL_IN * (size_t)n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(sphere_light_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, d_in.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, 4 * PBRT_HIP_SPHERE_LIGHT_EVAL_OUT * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}

extern "C" int pbrt_hip_light_map_eval_device(int device, const pbrt_hip_image_texture *image, const pbrt_hip_light_map *map, int64_t n, const float *in, float *out) {
  if (n < 0 || !image || !map || !in || !out) return fail(PBRT_HIP_ERR_INVALID, "light_map_eval_device: null argument or negative count");
  return guarded([&]() -> int {
    const std::string what = "light_map_eval_device: ";  // (the records checked as scene creation checks them, packed as it packs them)
    if (image->type != PBRT_HIP_TEXTURE_IMAGE) return fail(PBRT_HIP_ERR_INVALID, what + "not an image texture's record (its first word must be 4)");
    if (map->type != PBRT_HIP_TEXTURE_LIGHT_MAP) return fail(PBRT_HIP_ERR_INVALID, what + "not a light map's record (its first word must be 8)");
    int rc;
    if ((rc = image_check(*image, what)) || (rc = image_check_totals(1u, (uint64_t)image->width * image->height, what)) || (rc = image_check_texels(*image, what)) ||
        (rc = light_map_check(*map, what)))
      return rc;
    if (n == 0) return PBRT_HIP_OK;
    std::vector<float4> pool;
    float4 rows[3];
    image_pack(*image, &pool, rows);
    HIP_TRY(hipSetDevice(device));
    DevBuf<float4> d_pool, d_rows;
    DevBuf<float> d_in, d_out;
    HIP_TRY(d_pool.alloc(pool.size()));
    HIP_TRY(d_rows.alloc(3));
    HIP_TRY(d_in.alloc(PBRT_HIP_LIGHT_MAP_EVAL_IN * (size_t)n));
    HIP_TRY(d_out.alloc(PBRT_HIP_LIGHT_MAP_EVAL_OUT * (size_t)n));
    const hipStream_t stream = nullptr;  // the device's default stream
    HIP_TRY(hipMemcpyAsync(d_pool.p, pool.data(), 16 * pool.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_rows.p, rows, 16 * 3, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_in.p, in, 4 * PBRT_HIP_LIGHT_MAP_EVAL_IN * (size_t)n, hipMemcpyHostToDevice, stream));
    const float *m = map->world_to_light;
    hipLaunchKernelGGL(light_map_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, map->kind, make_float4(m[0], m[1], m[2], map->inv_tan),
                       make_float4(m[3], m[4], m[5], map->sx), make_float4(m[6], m[7], m[8], map->sy), d_rows.p, d_pool.p, n, d_in.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, 4 * PBRT_HIP_LIGHT_MAP_EVAL_OUT * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}

extern "C" int pbrt_hip_blocks_eval_device(int device, uint32_t op, int64_t n, const float *in, float *out) {
  if (op >= PBRT_HIP_BLOCK_COUNT) return fail(PBRT_HIP_ERR_INVALID, "blocks_eval_device: unknown op");
  if (n < 0 || !in || !out) return fail(PBRT_HIP_ERR_INVALID, "blocks_eval_device: null argument or negative count");
  if (n == 0) return PBRT_HIP_OK;
  return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    const BlockWidth w = kBlockWidth[op];
    DevBuf<float> d_in, d_out;
    HIP_TRY(d_in.alloc(w.in * (size_t)n));
    HIP_TRY(d_out.alloc(w.out * (size_t)n));
    const hipStream_t stream = nullptr;  // the device's default stream
    HIP_TRY(hipMemcpyAsync(d_in.p, in, 4 * w.in * (size_t)n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(blocks_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, n, w.in, w.out, d_in.p, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, 4 * w.out * (size_t)n, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PBRT_HIP_OK;
  });
}
