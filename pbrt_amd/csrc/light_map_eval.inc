// light_map_eval.inc -- one element of pbrt_hip_light_map_eval_device (include/pbrt_hip_debug.h): light_map.hpp on the 10 floats at `x` into
// the 11 floats at `y`, with the record in scope as e_kind, e_r0 / e_r1 / e_r2 ({a row of world_to_light, inv_tan / sx / sy}) and its image as
// e_pool, e_t0, e_offset.  Included by kernels_blocks.hip's light_map_eval_kernel and by the stand-alone host program of
// tests/test_light_map_host.py, so that both run this text around the header.
  {
    V3 e_wi = {0.f, 0.f, 0.f}, e_rgb = {0.f, 0.f, 0.f};
    float e_tmax = 0.f, e_scale = 0.f, e_s = 0.f, e_t = 0.f;
    const bool e_ok = lightmap::sample(mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]), mk(x[6], x[7], x[8]), e_kind, e_r0, e_r1, e_r2, x[9], e_pool, e_t0, e_offset,
                                       e_wi, e_tmax, e_scale, e_s, e_t, e_rgb);
    y[0] = e_ok ? 1.0f : 0.f;
    y[1] = e_ok ? e_wi.x : 0.f; y[2] = e_ok ? e_wi.y : 0.f; y[3] = e_ok ? e_wi.z : 0.f;
    y[4] = e_ok ? e_tmax : 0.f;
    y[5] = e_ok ? e_scale : 0.f;
    y[6] = e_ok ? e_s : 0.f; y[7] = e_ok ? e_t : 0.f;
    y[8] = e_ok ? e_rgb.x : 0.f; y[9] = e_ok ? e_rgb.y : 0.f; y[10] = e_ok ? e_rgb.z : 0.f;
  }
