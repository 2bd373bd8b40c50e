// spot_eval.inc -- one element of pbrt_hip_spot_eval_device (include/pbrt_hip_debug.h): spot_light.hpp on the 15 floats at `x` into the 7
// floats at `y`.  Included by kernels_blocks.hip's spot_eval_kernel and by the stand-alone host program of tests/test_spot_host.py, so that
// both run this text around the header.
  {
    V3 e_wi = {0.f, 0.f, 0.f};
    float e_tmax = 0.f, e_fall = 0.f, e_scale = 0.f;
    const bool e_ok = spot::sample(mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]), mk(x[6], x[7], x[8]), mk(x[9], x[10], x[11]), x[12], x[13], x[14], e_wi, e_tmax,
                                   e_fall, e_scale);
    y[0] = e_ok ? 1.0f : 0.f;
    y[1] = e_ok ? e_wi.x : 0.f; y[2] = e_ok ? e_wi.y : 0.f; y[3] = e_ok ? e_wi.z : 0.f;
    y[4] = e_ok ? e_tmax : 0.f;
    y[5] = e_ok ? e_fall : 0.f;
    y[6] = e_ok ? e_scale : 0.f;
  }
