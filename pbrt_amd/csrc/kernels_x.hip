// kernels_x.hip -- render_kernel_x in a translation unit of its own, in the manner of kernels_env.hip: its 116 instantiations compile
// BESIDE kernels.hip's (pbrt_amd/build.py runs the units in parallel).  launch_render (kernels.hip) hands over to launch_render_x.
#include "kernel_path.hpp"
#include "with_bools.hpp"

namespace pbrt_hip {
namespace {

// The variants of the path that BASELINE's configs do not use, in a kernel of their own name so that render_kernel's instantiations keep
// theirs (and their machine code): MIS = multiple importance sampling of the direct-light estimate, TEX = materials
// whose Kd is a checkerboard texture (3.15), GLS = glass materials (3.16) -- and every combination of the three with the table samplers
// (SND: 3.12, 3.13) and a box filter radius other than 0.5 (WIDE: 3.11), which render_kernel instantiates one at a time.  No counters.
// (The GLS instantiations get the spheres' register budget, 3 waves per SIMD: with the Fresnel / refraction branch beside the path state
// the body needs up to 9 VGPRs more than the 96 of 5 waves, and a spill costs every scene more than glass scenes lose in occupancy.)
template <bool SPH, int STACK, bool MIS, bool TEX, bool SND, bool WIDE, bool GLS = false>
__global__ void __launch_bounds__(64, ((SPH || GLS) ? 3 : PBRT_RENDER_WAVES_PER_SIMD)) render_kernel_x(const DevScene S, const RenderParams R) {
  constexpr bool COUNT = false, EXACT = false;
  constexpr bool ENV = false;  // (an environment map: kernels_env.hip render_kernel_env)
  constexpr bool NRM = false;  // (shading normals: kernels_n.hip render_kernel_n)
  constexpr bool LREC = false;  // (path records in LDS: the default path alone, kernels.hip render_kernel)
  constexpr int STEPS = PBRT_STEPS_PER_CHECK;
  (void)ENV;
#include "render_body.inc"
}

}  // namespace

// RenderLaunch -> the instantiation: MIS, TEX or GLS, or the table samplers together with a wide filter, without counters -- what
// launch_render sends here; the default path and its one-at-a-time variants are render_kernel's, and an error here.
hipError_t launch_render_x(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t st) {
  if (R.n_items == 0) return hipSuccess;
  if (L.counters != kCountNone) return hipErrorInvalidValue;
  return with_bools([&](auto SPH, auto OVF, auto MIS, auto TEX, auto SND, auto WIDE, auto GLS) {
    constexpr int STACK = OVF ? (int)kQuadLdsStackOvf : 0;
    if constexpr (GLS || MIS || TEX || (SND && WIDE)) {
      hipLaunchKernelGGL((render_kernel_x<SPH, STACK, MIS, TEX, SND, WIDE, GLS>), dim3(L.n_workgroups), dim3(64), L.lds_bytes, st, S, R);
      return hipGetLastError();
    } else {
      return hipErrorInvalidValue;
    }
  }, L.spheres, L.plan.overflow, L.mis, L.textured, L.table_sampler, L.wide, L.glass);
}

}  // namespace pbrt_hip
