// capi_internal.hpp -- what the translation units behind the C ABI share: error reporting, the scene object (its buffers: dev_buf.hpp) with the
// table of its arrays, and the film geometry (capi_scene.cpp makes single-GPU scenes, capi_render.cpp renders them, multi_gpu.cpp
// replicates them across the devices of a node).
#pragma once
#include <hip/hip_runtime.h>

#include <exception>
#include <optional>
#include <string>

#include "../../include/pbrt_hip.h"
#include "../../include/pbrt_hip_debug.h"
#include "bvh_build.hpp"
#include "dev_buf.hpp"
#include "device_types.h"

namespace pbrt_hip {
// sets the thread-local message behind pbrt_hip_last_error() and returns `code`
int fail(int code, const std::string &msg);
const char *last_error_message();
// runs the body of an extern "C" function: an exception that reaches the boundary becomes PBRT_HIP_ERR_INTERNAL with its text
template <class F>
int guarded(F &&body) {
  try { return body(); } catch (const std::exception &e) { return fail(PBRT_HIP_ERR_INTERNAL, e.what()); }
}

// A scene's build time (a double: the host path times itself) and the device builder's re-insertion statistics (zeros for a host build)
struct BuildStats {
  double build_ms = 0.0;
  ReinsertStats reinsert;
};

// A scene's own stream (of pbrt_hip_render()) and the events that time a render.  A base of pbrt_hip_scene: base classes are
// destroyed after the members, so the scene's buffers are freed before these.
struct SceneStream {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~SceneStream() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
// The device arrays that ARE a scene: what scene creation uploads and builds, what device_bytes counts and what a clone on another device
// carries.  Per-render scratch (slab, film, lane state, partial sums, counters, stack overflow, sampler tables) is not part of it.
struct SceneArrays {
  DevBuf<float> d_P;  // vertices and indices of the tree's primitives: the triangles, then the spheres' proxy triangles (scene_inputs.hpp SceneInputs)
  DevBuf<uint32_t> d_idx, d_order;
  DevBuf<uint16_t> d_mat_id;
  DevBuf<uint4> d_nodes, d_quads;
  DevBuf<float4> d_tris, d_mats, d_lights, d_spheres;
  DevBuf<float> d_tri_uv_in;  // textured scenes: corner (u, v) as uploaded (triangle order) ...
  DevBuf<float2> d_tri_uv;    // ... and in leaf-slot order (3 per slot)
  DevBuf<float4> d_textures;
  DevBuf<float4> d_mat_extra;  // a row per material of a scene with glass, plastic or substrate (scene_tables.hpp mat_extra); empty otherwise
  // an environment-map infinite light: texels {r, g, b, p_uv}, the marginal and conditional CDFs (envmap.hpp EnvTables)
  DevBuf<float4> d_env_texels;
  DevBuf<float> d_env_marginal, d_env_conditional;
  // shading normals: the corner normals as uploaded (9 floats per triangle, triangle order) and in leaf-slot order
  // (3 x float4 {n, 0} per slot); both empty for a scene without them
  DevBuf<float> d_tri_n_in;
  DevBuf<float4> d_tri_n;
  // image textures for Kd: the texels {r, g, b, 0} of every image slot, back to back; empty for a scene without one
  DevBuf<float4> d_image_texels;
  // the canonical walk's triangle records and leaf order of a device-built scene (ensure_canonical)
  DevBuf<float4> d_tris_exact;
  DevBuf<uint32_t> d_order_exact;

  // THE list of the arrays: f(pointer to member, whether a clone of the scene carries the array)
  template <class F>
  static void for_each(F &&f) {
    f(&SceneArrays::d_P, true); f(&SceneArrays::d_idx, true); f(&SceneArrays::d_order, true); f(&SceneArrays::d_mat_id, true);
    f(&SceneArrays::d_nodes, true); f(&SceneArrays::d_quads, true);
    f(&SceneArrays::d_tris, true); f(&SceneArrays::d_mats, true); f(&SceneArrays::d_lights, true); f(&SceneArrays::d_spheres, true);
    f(&SceneArrays::d_tri_uv_in, false);  // (read by pack_uv during scene creation and by nothing after it)
    f(&SceneArrays::d_tri_uv, true); f(&SceneArrays::d_textures, true); f(&SceneArrays::d_mat_extra, true);
    f(&SceneArrays::d_env_texels, true); f(&SceneArrays::d_env_marginal, true); f(&SceneArrays::d_env_conditional, true);
    f(&SceneArrays::d_tri_n_in, false);  // (read by pack_nrm during scene creation and by nothing after it: released there)
    f(&SceneArrays::d_tri_n, true); f(&SceneArrays::d_image_texels, true);
    f(&SceneArrays::d_tris_exact, false); f(&SceneArrays::d_order_exact, false);  // (canonical_ready is not copied: a clone makes its own on first use)
  }
  // bytes on the device: pbrt_hip_scene_info's device_bytes
  uint64_t bytes() const {
    uint64_t total = 0;
    for_each([&](auto m, bool) { total += (uint64_t)(this->*m).n * sizeof(*(this->*m).p); });
    return total;
  }
};
static_assert(sizeof(SceneArrays) == 22 * sizeof(DevBuf<float>), "an array of SceneArrays is missing from SceneArrays::for_each");

struct FilmWindow {  // of a description: all that a finished scene keeps of pbrt_hip_scene_desc beside what went to the device
  int32_t xres = 0, yres = 0;
  float crop[4] = {0.f, 1.f, 0.f, 1.f};
};
// What a scene is beside its arrays and its host tree: plain values, which a clone takes in one assignment
struct SceneTraits {
  FilmWindow window;
  uint32_t n_prims = 0;  // primitives of the tree: dev.n_tris triangles + the spheres
  bool gpu_built = false;  // accelerator built on the device: the canonical tree (counter flags) is made on first use
  uint32_t n_quads_gpu = 0;
  bool textured = false;  // some primitive's material has kd_tex != 0: the TEX instantiations render the scene
  bool glass = false;     // some material is glass or plastic (beyond matte and mirror), or some light is a spot, a mapped or a sphere light: the GLS instantiations render the scene
  bool env = false;       // an environment-map light: render_kernel_env renders the scene; the map's size, world_to_light and the light's factor
  uint32_t env_w = 0, env_h = 0;
  float env_m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, env_c[3] = {0, 0, 0};
  bool normals = false;  // the texture table held a pbrt_hip_normals record: render_kernel_n renders the scene
  std::optional<pbrt_hip_pixel_filter> filter;  // the texture table's pixel filter record, if it held one: every render is a wide one
  BuildStats build;
};
}  // namespace pbrt_hip

#define HIP_TRY(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess)                                                                                 \
      return pbrt_hip::fail(PBRT_HIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));         \
  } while (0)

// (base classes are destroyed in reverse order, after the members: every buffer is freed before the stream and the events)
struct pbrt_hip_scene : pbrt_hip::SceneStream, pbrt_hip::SceneArrays, pbrt_hip::SceneTraits {
  int device = 0;
  uint32_t n_cu = 256;  // hipDeviceProp_t::multiProcessorCount of `device`
  pbrt_hip::Bvh bvh;
  pbrt_hip::DevScene dev{};
  // per-render scratch
  pbrt_hip::DevBuf<uint32_t> d_stack_overflow;  // per-lane spill area of the quad walk's stack beyond its LDS part
  pbrt_hip::DevBuf<float4> d_slab, d_film;          // scratch of pbrt_hip_render()
  pbrt_hip::DevBuf<float4> d_lane_state;            // per-lane path state records of the render kernel
  pbrt_hip::DevBuf<float4> d_partials;              // partial film sums of the work items (8 chunks per slab pixel)
  pbrt_hip::DevBuf<unsigned long long> d_counters;  // 80: see open()
  pbrt_hip::DevBuf<uint32_t> d_sobol;  // generator matrices of sampler 2 (uploaded at its first use)
  pbrt_hip::DevBuf<uint32_t> d_halton; // per-dimension table of sampler 3 (likewise)
  // a weighted pixel filter: the 256 weights of the radii of the last render (made on the host at a render with other
  // radii: pixel_filter.hpp filter_table)
  pbrt_hip::DevBuf<float> d_filter_table;
  float filter_table_host[pbrt_hip::kFilterTableFloats] = {};  // (device_types.h: the weights, then 1 / rx and 1 / ry)
  float filter_table_rx = 0.f, filter_table_ry = 0.f;  // (0: no table yet)
  bool pending = false;
  bool pending_counters = false;
  uint64_t pending_samples = 0;
  // The canonical walk's view of a device-built scene (pbrt_hip::ensure_canonical): the oracle's binary tree, built on the
  // host from the vertex / index buffers read back from the device, and triangle records in ITS leaf order.  For a
  // host-built scene the production arrays serve both walks and dev_exact == dev.
  pbrt_hip::DevScene dev_exact{};
  bool canonical_ready = false;
  double canonical_build_ms = 0.0;
  uint64_t device_bytes = 0;  // SceneArrays::bytes() when the scene was finished, and again with its canonical tree

  // what every scene has on `device` beside its arrays (scene_create, clone_scene): the CU count, the stream, the events, the counters
  int open(int device);
};

namespace pbrt_hip {
// the canonical tree of a device-built scene, made on first use (capi_scene.cpp)
int ensure_canonical(pbrt_hip_scene *s);
// the array pointers of s->dev from the scene's buffers: the one place that sets them (scene creation, ensure_canonical, clone_scene)
void bind_scene_arrays(pbrt_hip_scene *s);

// ---- film geometry (capi_render.cpp) ----
// Film geometry of one render: the cropped window (film.rs:92-101), the sample bounds (film.rs:166-175) and whether the
// box filter has the default radius 0.5 -- then a sample lands in its own pixel and the two rectangles coincide -- or
// another one (samples reach pad = ceil(radius - 0.5) pixels beyond the window, fixed-point film).
struct FilmGeom {
  bool wide;
  float rx, ry;
  int32_t pad_x, pad_y;
  int32_t crop[4], sb[4];
  int32_t crop_w() const { return crop[2] > crop[0] ? crop[2] - crop[0] : 0; }
  int32_t crop_h() const { return crop[3] > crop[1] ? crop[3] - crop[1] : 0; }
  size_t crop_px() const { return (size_t)crop_w() * (size_t)crop_h(); }
};
// (a filter width of 0 is the default radius 0.5; under a pixel filter's record, DESIGN.md 3.19 -- `filter`, NULL: the box --, it is that
// kind's default radius, and the geometry is the wide one at every radius)
FilmGeom film_geom(const FilmWindow &w, const pbrt_hip_pixel_filter *filter = nullptr, float filter_xwidth = 0.f, float filter_ywidth = 0.f);
}  // namespace pbrt_hip
