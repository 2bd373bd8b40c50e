// kernels_env.hip -- the render kernel of scenes with an environment-map infinite light, in a translation unit of its
// own so that it compiles BESIDE kernels.hip and kernels_x.hip (pbrt_amd/build.py runs the units in parallel) and so that their
// instantiations keep their names and their machine code.  The building blocks -- the walk, the samplers, the path records -- come from
// kernel_path.hpp, the body is render_body.inc.
//
//   render_kernel_env   render_body.inc with ENV = true: a ray that escapes collects the map (envmap_core.hpp lookup), the map is a light
//                       of the one-light direct estimate (Distribution2D sampling, MIS against the cosine-sampled bounce ray).  GLS = true
//                       always (a glass table that is never read costs nothing, and the instantiations halve).
//   envmap_eval_kernel  envmap_core.hpp over arrays: pbrt_hip_envmap_eval_device, the hook that shows the device computes the host's bits.
//
// Combinations that do NOT exist (render_variant.hpp refuses them with PBRT_HIP_ERR_LIMIT): a box filter radius other than 0.5 (WIDE) and
// the counter flags.
#include "kernel_path.hpp"
#include "with_bools.hpp"

namespace pbrt_hip {
namespace {

// (the register budget: render_variant.hpp)
template <bool SPH, int STACK, bool MIS, bool TEX, bool SND>
__global__ void __launch_bounds__(64, render_waves_per_simd(RenderFamily::kEnv, SPH, true)) render_kernel_env(const DevScene S, const RenderParams R) {
  constexpr bool COUNT = false, EXACT = false, WIDE = false, GLS = true, ENV = true;
  constexpr bool PLS = false;  // (no plastic beside a map: pbrt_hip_scene_create refuses the pair)
  (void)PLS;
  constexpr bool NRM = false;   // (shading normals: another family's, render_variant.hpp)
  constexpr bool LREC = false;  // (path records in LDS: the default path alone, kernels.hip render_kernel)
  constexpr int STEPS = PBRT_STEPS_PER_CHECK;
#include "render_body.inc"
}

__global__ void envmap_eval_kernel(const RenderParams R, int64_t n, const float *u12, float *d, uint32_t *texel, float *le, float *pdf) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const envmap::Map m = env_map(R);
  float st;
  uint32_t t;
  if (u12) {
    float x, y, z;
    t = envmap::sample(m, u12[2 * i], u12[2 * i + 1], &x, &y, &z, &st);
    d[3 * i] = x; d[3 * i + 1] = y; d[3 * i + 2] = z;
  } else {
    t = envmap::lookup(m, d[3 * i], d[3 * i + 1], d[3 * i + 2], &st);
  }
  const float4 tx = m.texels[t];
  if (texel) texel[i] = t;
  if (le) { le[3 * i] = tx.x; le[3 * i + 1] = tx.y; le[3 * i + 2] = tx.z; }
  if (pdf) pdf[i] = envmap::pdf_omega(tx.w, st);
}

}  // namespace

hipError_t launch_render_env(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t st) {
  if (R.n_items == 0) return hipSuccess;
  if (!R.env_texels) return hipErrorInvalidValue;
  const RenderVariant &V = L.variant;
  return with_bools([&](auto SPH, auto OVF, auto MIS, auto TEX, auto SND) {
    constexpr int STACK = OVF ? (int)kQuadLdsStackOvf : 0;
    if constexpr (render_family_builds(RenderFamily::kEnv, RenderVariant{SPH, false, SND, MIS, TEX, true, true, false, kCountNone})) {
      hipLaunchKernelGGL((render_kernel_env<SPH, STACK, MIS, TEX, SND>), dim3(L.n_workgroups), dim3(64), L.lds_bytes, st, S, R);
      return hipGetLastError();
    }
    return hipErrorInvalidValue;
  }, V.spheres, L.plan.overflow, V.mis, V.textured, V.table_sampler);
}

hipError_t launch_envmap_eval(const RenderParams &R, int64_t n, const float *u12, float *d, uint32_t *texel, float *le, float *pdf, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(envmap_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, R, n, u12, d, texel, le, pdf);
  return hipGetLastError();
}

}  // namespace pbrt_hip
