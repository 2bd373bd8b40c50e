// filter_weight.inc -- where a sample of a weighted pixel filter lands and which table entry it takes there (DESIGN.md 3.19; pbrt-v3
// FilmTile::AddSample), stated once: included by kernel_path.hpp, so that the render kernels' WIDE finish (render_body.inc and, through it,
// film_add_sample) and the hook's kernels (kernels_blocks.hip filter_bounds_kernel / filter_index_kernel, behind
// pbrt_hip_filter_footprint_eval_device) run the same statements.  (Two small forceinline functions rather than text: both are used from
// inside loops of their callers.)  fp32, this operation order, no contraction.

// The footprint of a sample at film point (fx, fy) under radii (rx, ry): the pixels [x0, x1) x [y0, y1) of the cropped window
// [cx0, cx1) x [cy0, cy1) whose centres lie within the radii -- 3.11's bounds, the box's.  d = p - 0.5 on return.
struct FilterFootprint {
  int32_t x0, y0, x1, y1;
  float dx, dy;
};
__device__ __forceinline__ FilterFootprint filter_footprint(float fx, float fy, float rx, float ry, int32_t cx0, int32_t cy0, int32_t cx1, int32_t cy1) {
  FilterFootprint f;
  f.dx = fx - 0.5f;
  f.dy = fy - 0.5f;
  f.x0 = max((int32_t)ceilf(f.dx - rx), cx0);
  f.x1 = min((int32_t)floorf(f.dx + rx) + 1, cx1);
  f.y0 = max((int32_t)ceilf(f.dy - ry), cy0);
  f.y1 = min((int32_t)floorf(f.dy + ry) + 1, cy1);
  return f;
}
// One axis of the table index of pixel coordinate p for a sample at d = film point - 0.5 (inv_r = 1.0f / radius, formed on the host):
// sixteenths of the radius, the last one closed
__device__ __forceinline__ int32_t filter_axis_index(int32_t p, float d, float inv_r) {
  return min((int32_t)floorf(fabsf((((float)p - d) * inv_r) * 16.0f)), 15);
}
