// sphere_light_eval.inc -- one element of pbrt_hip_sphere_light_eval_device (include/pbrt_hip_debug.h): sphere_light.hpp on the 13 floats at
// `x` into the 8 floats at `y`.  Included by kernels_blocks.hip's sphere_light_eval_kernel and by the stand-alone host program of
// tests/sphere_light_host_build.py, so that both run this text around the header.
  {
    V3 e_wi = {0.f, 0.f, 0.f};
    float e_tmax = 0.f, e_scale = 0.f, e_pdf = 0.f, e_cs = 0.f;
    const V3 e_po = mk(x[0], x[1], x[2]), e_c = mk(x[6], x[7], x[8]);
    const bool e_ok = sphere_light::sample(e_po, mk(x[3], x[4], x[5]), e_c, x[9], x[10], x[11], x[12], e_wi, e_tmax, e_scale, e_pdf, e_cs);
    y[0] = e_ok ? 1.0f : 0.f;
    y[1] = e_ok ? e_wi.x : 0.f; y[2] = e_ok ? e_wi.y : 0.f; y[3] = e_ok ? e_wi.z : 0.f;
    y[4] = e_ok ? e_tmax : 0.f;
    y[5] = e_ok ? e_scale : 0.f;
    y[6] = e_ok ? e_pdf : 0.f;
    y[7] = sphere_light::pdf_omega(e_po, e_c, x[9]);  // the hit side's density from po, whatever became of the sample
  }
