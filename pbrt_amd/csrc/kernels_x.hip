// kernels_x.hip -- render_kernel_x in a translation unit of its own, in the manner of kernels_env.hip: its 116 instantiations compile
// BESIDE kernels.hip's (pbrt_amd/build.py runs the units in parallel).  launch_render (kernels.hip) hands over to launch_render_x.
#include "kernel_path.hpp"
#include "with_bools.hpp"

namespace pbrt_hip {
namespace {

// The variants of the path that BASELINE's configs do not use, in a kernel of their own name so that render_kernel's instantiations keep
// theirs (and their machine code): MIS = multiple importance sampling of the direct-light estimate, TEX = materials
// whose Kd is a checkerboard texture (3.15), GLS = glass materials (3.16) and, in the same instantiations, plastic ones (3.21) -- and every combination of the three with the table samplers
// (SND: 3.12, 3.13) and a box filter radius other than 0.5 (WIDE: 3.11), which render_kernel instantiates one at a time.  No counters.
// (The GLS instantiations get the spheres' register budget -- render_variant.hpp --: a spill costs every scene more than glass scenes
// lose in occupancy.)
template <bool SPH, int STACK, bool MIS, bool TEX, bool SND, bool WIDE, bool GLS = false>
__global__ void __launch_bounds__(64, render_waves_per_simd(RenderFamily::kX, SPH, GLS)) render_kernel_x(const DevScene S, const RenderParams R) {
  constexpr bool COUNT = false, EXACT = false, ENV = false, NRM = false;  // (the other families': render_variant.hpp)
  constexpr bool LREC = false;  // (path records in LDS: the default path alone, kernels.hip render_kernel)
  constexpr int STEPS = PBRT_STEPS_PER_CHECK;
  (void)ENV;
  constexpr bool PLS = GLS;  // the plastic material rides in the GLS instantiations, a run-time branch on the type word
  (void)PLS;
#include "render_body.inc"
}

}  // namespace

// RenderLaunch -> the instantiation, for what launch_render sends here: family kX.  What another family renders is an error here.
hipError_t launch_render_x(const DevScene &S, const RenderParams &R, const RenderLaunch &L, hipStream_t st) {
  if (R.n_items == 0) return hipSuccess;
  const RenderVariant &V = L.variant;
  return with_bools([&](auto SPH, auto OVF, auto MIS, auto TEX, auto SND, auto WIDE, auto GLS) {
    constexpr int STACK = OVF ? (int)kQuadLdsStackOvf : 0;
    if constexpr (render_family_builds(RenderFamily::kX, RenderVariant{SPH, WIDE, SND, MIS, TEX, GLS, false, false, kCountNone})) {
      hipLaunchKernelGGL((render_kernel_x<SPH, STACK, MIS, TEX, SND, WIDE, GLS>), dim3(L.n_workgroups), dim3(64), L.lds_bytes, st, S, R);
      return hipGetLastError();
    }
    return hipErrorInvalidValue;
  }, V.spheres, L.plan.overflow, V.mis, V.textured, V.table_sampler, V.wide, V.glass);
}

}  // namespace pbrt_hip
