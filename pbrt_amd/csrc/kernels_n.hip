// kernels_n.hip -- the render kernel of scenes that carry shading normals, in a translation unit of its own in the manner
// of kernels_env.hip: it compiles BESIDE the other kernel units (pbrt_amd/build.py) and their instantiations keep their names and their
// machine code.  The building blocks come from kernel_path.hpp, the body is render_body.inc, the normal itself is shading_normal.inc.
//
//   render_kernel_n             render_body.inc with NRM = true: at a triangle hit the corner normals of the leaf slot (RenderParams::tri_n,
//                               three 16-byte loads) are interpolated like the hit point and take the geometric normal's place where matte
//                               and mirror scatter.  GLS = true always (as render_kernel_env), ENV a template argument: 64 instantiations,
//                               so that a smooth mesh renders under every integrator and sampler, with spheres, checkerboards, glass
//                               elsewhere in the scene and under an environment map.
//   pack_nrm_kernel             the corner normals (triangle order, as uploaded) gathered into leaf-slot order, beside pack_uv_kernel's (u, v).
//   shading_normal_eval_kernel  shading_normal.inc over arrays: pbrt_hip_shading_normal_eval_device, the hook that lets a test compare
//                               the statements the render kernel runs with float64, element by element.
//
// Combinations that do NOT exist (render_variant.hpp refuses them with PBRT_HIP_ERR_LIMIT): a box filter radius other than 0.5 (WIDE) and
// the counter flags.
#include "kernel_path.hpp"
#include "with_bools.hpp"

namespace pbrt_hip {
namespace {

// (the register budget: render_variant.hpp.  The three corner normals and the interpolated one are live only between the hit's material
// fetch and the scatter; tests/test_normals_host.py holds every instantiation to the budget)
template <bool SPH, int STACK, bool MIS, bool TEX, bool SND, bool ENV>
__global__ void __launch_bounds__(64, render_waves_per_simd(RenderFamily::kN, SPH, true)) render_kernel_n(const DevScene S, const RenderParams R) {
  constexpr bool COUNT = false, EXACT = false, WIDE = false, GLS = true, NRM = true;
  constexpr bool PLS = false;  // (no plastic beside shading normals: pbrt_hip_scene_create refuses the pair)
  (void)PLS;
  constexpr bool LREC = false;  // (path records in LDS: the default path alone, kernels.hip render_kernel)
  constexpr int STEPS = PBRT_STEPS_PER_CHECK;
#include "render_body.inc"
}

// the corner normals of the triangle in leaf slot `slot`; a sphere's proxy slot gets zeros (its normal is analytic)
__global__ void pack_nrm_kernel(const float *tri_n, const uint32_t *order, uint32_t n_prims, uint32_t n_tris, float4 *out) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_prims) return;
  const uint32_t t = order[slot];
  for (int v = 0; v < 3; v++) {
    const float *q = tri_n + 9 * (size_t)t + 3 * v;
    out[3u * slot + v] = t < n_tris ? make_float4(q[0], q[1], q[2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// per element: n0 n1 n2 (9), ng (3), b1, b2, wo (3) -> nsf (3), fell_back (0 or 1)
__global__ void __launch_bounds__(256) shading_normal_eval_kernel(int64_t n, const float *in, float *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *x = in + 17 * i;
  const V3 sn_n0 = mk(x[0], x[1], x[2]), sn_n1 = mk(x[3], x[4], x[5]), sn_n2 = mk(x[6], x[7], x[8]);
  const V3 ng = mk(x[9], x[10], x[11]);
  const float sn_b1 = x[12], sn_b2 = x[13];
  const V3 wo = mk(x[14], x[15], x[16]);
#include "shading_normal.inc"
  out[4 * i] = nsf.x; out[4 * i + 1] = nsf.y; out[4 * i + 2] = nsf.z;
  out[4 * i + 3] = sn_fell_back ? 1.0f : 0.f;
}

}  // namespace

hipError_t launch_render_n(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t st) {
  if (R.n_items == 0) return hipSuccess;
  const RenderVariant &V = L.variant;
  if (!R.tri_n || (V.env && !R.env_texels)) return hipErrorInvalidValue;
  return with_bools([&](auto SPH, auto OVF, auto MIS, auto TEX, auto SND, auto ENV) {
    constexpr int STACK = OVF ? (int)kQuadLdsStackOvf : 0;
    if constexpr (render_family_builds(RenderFamily::kN, RenderVariant{SPH, false, SND, MIS, TEX, true, ENV, true, kCountNone})) {
      hipLaunchKernelGGL((render_kernel_n<SPH, STACK, MIS, TEX, SND, ENV>), dim3(L.n_workgroups), dim3(64), L.lds_bytes, st, S, R);
      return hipGetLastError();
    }
    return hipErrorInvalidValue;
  }, V.spheres, L.plan.overflow, V.mis, V.textured, V.table_sampler, V.env);
}

hipError_t launch_pack_nrm(const float *tri_n, const uint32_t *order, uint32_t n_prims, uint32_t n_tris, float4 *out, hipStream_t stream) {
  if (n_prims == 0) return hipSuccess;
  hipLaunchKernelGGL(pack_nrm_kernel, dim3((n_prims + 255) / 256), dim3(256), 0, stream, tri_n, order, n_prims, n_tris, out);
  return hipGetLastError();
}

hipError_t launch_shading_normal_eval(int64_t n, const float *in, float *out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(shading_normal_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, in, out);
  return hipGetLastError();
}

}  // namespace pbrt_hip
