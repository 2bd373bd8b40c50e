// shading_normal.inc -- the shading normal of a triangle hit (DESIGN.md 3.18), stated once as text: included by render_body.inc (the NRM
// instantiations: kernels_n.hip render_kernel_n) and by the hook's kernel (kernels_n.hip shading_normal_eval_kernel), so that
// tests/test_normals_gpu.py runs the statements the render kernels run.  (Text and not a function, as tri_test.inc is.)  Reads the locals
//   V3 sn_n0, sn_n1, sn_n2   the corner normals, world space, any length        float sn_b1, sn_b2   the hit's barycentrics
//   V3 ng                    the winding's unit normal                           V3 wo                towards where the ray came from
// and leaves  V3 nsf (the shading normal on wo's geometric side)  and  bool sn_fell_back (no usable normal: nsf is +-ng, bit for bit)
// behind.  fp32, this operation order, no contraction.
const float sn_w = (1.0f - sn_b1) - sn_b2;
const V3 sn_n = (sn_n0 * sn_w + sn_n1 * sn_b1) + sn_n2 * sn_b2;  // the order of the hit point (3.7)
const float sn_l2 = dot(sn_n, sn_n);
// (zero corner normals = "this triangle has none"; an overflowing or NaN sum is no direction either)
const bool sn_fell_back = !(sn_l2 > 0.f) || !(fabsf(sn_l2) < kInf);
V3 sn_ns = ng;
if (!sn_fell_back) {
  sn_ns = sn_n / sqrtf(sn_l2);
  if (dot(sn_ns, ng) < 0.f) sn_ns = -sn_ns;  // ng stays the winding's normal: the shading normal is turned to ITS side
}
const V3 nsf = dot(ng, wo) < 0.f ? -sn_ns : sn_ns;  // the flip that makes nf
