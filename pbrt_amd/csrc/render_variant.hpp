// render_variant.hpp -- THE statement of the render-kernel variants: which combinations of switches exist, which kernel family renders a
// combination, and the register budget it gets.  capi_render.cpp (check_render_desc, render_launch), the four kernel units (their
// __launch_bounds__ and the `if constexpr` of their launchers, which decides the set of instantiations) and tests/test_render_variants.py
// (a plain g++ program) all read it from here.  Plain C++17 constexpr, nothing of HIP.
#pragma once
#include <stdint.h>

#include "../../include/pbrt_hip.h"

// waves per SIMD the register allocator must leave room for (launch_bounds' 2nd argument): 5 = the 96 VGPRs of the default path; 4 = 128
// VGPRs for render_kernel_env (the body needs 101 .. 109) and render_kernel_n (98 .. 108, 3.18)
#ifndef PBRT_RENDER_WAVES_PER_SIMD
#define PBRT_RENDER_WAVES_PER_SIMD 5
#endif
#ifndef PBRT_ENV_WAVES_PER_SIMD
#define PBRT_ENV_WAVES_PER_SIMD 4
#endif
#ifndef PBRT_NRM_WAVES_PER_SIMD
#define PBRT_NRM_WAVES_PER_SIMD 4
#endif
#ifndef PBRT_RENDER_MAX_WAVES_PER_CU  // the cap of render_stack_plan (device_types.h): 4 SIMDs x the largest budget
#define PBRT_RENDER_MAX_WAVES_PER_CU (4 * PBRT_RENDER_WAVES_PER_SIMD)
#endif

namespace pbrt_hip {

enum RenderCounters : uint32_t {
  kCountNone = 0,
  kCountExact = 1,  // PBRT_HIP_FLAG_COUNTERS: the exact walk of the canonical tree (render_kernel<..., EXACT>)
  kCountWalk = 2,   // PBRT_HIP_FLAG_WALK_COUNTERS: the production walk, counting
};
struct RenderVariant {
  bool spheres;        // SPH
  bool wide;           // WIDE: a box filter radius other than 0.5
  bool table_sampler;  // SND: samplers 2 and 3 (3.12, 3.13)
  bool mis, textured;  // MIS (3.14) and TEX (3.15)
  bool glass;          // GLS (3.16, 3.21, 3.22, 3.23, 3.25): the scene has a glass or a plastic material, or a spot, a mapped or a sphere light
  bool env;            // ENV (3.17): the scene has an environment map
  bool normals;        // NRM (3.18): the scene carries shading normals
  RenderCounters counters;
};
enum class RenderFamily { kDefault, kX, kEnv, kN };  // render_kernel, render_kernel_x, render_kernel_env, render_kernel_n
struct RenderRefusal {
  int code;  // PBRT_HIP_OK, or the code and message check_render_desc fails with
  const char *text;
};

// The combinations the library does not build.  The counting walks exist for the default path alone; a scene with a map or with normals
// is told of that first, whatever else it holds.
constexpr RenderRefusal render_variant_refusal(const RenderVariant &v) {
  const bool counting = v.counters != kCountNone;
  if (v.table_sampler && counting)
    return {PBRT_HIP_ERR_INVALID, "render: the counter flags are not available with the Sobol' / Halton samplers (samplers 2, 3)"};
  if (v.wide && counting) return {PBRT_HIP_ERR_INVALID, "render: the counter flags need the default box filter (radius 0.5)"};
  if (v.normals && counting) return {PBRT_HIP_ERR_LIMIT, "render: the counter flags are not available for a scene with shading normals"};
  if (v.normals && v.wide)
    return {PBRT_HIP_ERR_LIMIT, "render: shading normals with a box filter radius other than 0.5 is a combination the library does not build"};
  if (v.env && counting) return {PBRT_HIP_ERR_LIMIT, "render: the counter flags are not available for a scene with an environment map"};
  if ((v.textured || v.mis) && counting)
    return {PBRT_HIP_ERR_LIMIT, "render: the counter flags are not available for textured materials / the MIS integrator"};
  if (v.glass && counting) return {PBRT_HIP_ERR_LIMIT, "render: the counter flags are not available for a scene with a glass material"};
  if (v.env && v.wide)
    return {PBRT_HIP_ERR_LIMIT, "render: an environment map with a box filter radius other than 0.5 is a combination the library does not build"};
  return {PBRT_HIP_OK, nullptr};
}

// The family that renders a variant render_variant_refusal accepts.  render_kernel has the default path, and one at a time a wide filter
// or the table samplers, and the counting walks; every other combination without a map or normals is render_kernel_x's.
constexpr RenderFamily render_family(const RenderVariant &v) {
  if (v.normals) return RenderFamily::kN;
  if (v.env) return RenderFamily::kEnv;
  if (v.counters == kCountExact) return RenderFamily::kDefault;
  if (v.glass || v.mis || v.textured || (v.table_sampler && v.wide)) return RenderFamily::kX;
  return RenderFamily::kDefault;
}
// what a launcher's `if constexpr` asks of its template switches: family `f` has an instantiation for `v`
constexpr bool render_family_builds(RenderFamily f, const RenderVariant &v) {
  return render_variant_refusal(v).code == PBRT_HIP_OK && render_family(v) == f;
}

// The plain default path: the launch that may take 2 node steps per check in shallow trees, and whose overflow instantiation keeps path
// records 0..2 in LDS behind a shorter stack (device_types.h kLdsPathRecords) -- the stack plan and the kernel's LREC both ask here.
constexpr bool render_default_path(const RenderVariant &v) {
  return render_family(v) == RenderFamily::kDefault && v.counters == kCountNone && !v.wide && !v.table_sampler;
}

// The register budget.  Spheres (the f64 quadratic of lib.rs:181-203 does not fit 128 VGPRs beside the path state; C0 / C1 have nothing to
// gain from occupancy) and glass (the Fresnel / refraction branch needs up to 9 VGPRs more than the 96 of 5 waves) get 3 waves per SIMD.
constexpr uint32_t render_waves_per_simd(RenderFamily f, bool spheres, bool glass) {
  if (f == RenderFamily::kN) return PBRT_NRM_WAVES_PER_SIMD;
  if (f == RenderFamily::kEnv) return PBRT_ENV_WAVES_PER_SIMD;
  return (spheres || glass) ? 3 : PBRT_RENDER_WAVES_PER_SIMD;
}
// one-wave workgroups per CU of a launch: what the registers allow on 4 SIMDs, and no more than the LDS of the stack plan holds
constexpr uint32_t render_waves_per_cu(const RenderVariant &v, uint32_t plan_waves_per_cu) {
  const uint32_t by_registers = 4u * render_waves_per_simd(render_family(v), v.spheres, v.glass);
  return by_registers < plan_waves_per_cu ? by_registers : plan_waves_per_cu;
}

}  // namespace pbrt_hip
