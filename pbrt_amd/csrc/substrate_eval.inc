// substrate_eval.inc -- one element of pbrt_hip_substrate_eval_device (include/pbrt_hip_debug.h): substrate_bsdf.hpp on the 18 floats at `x`
// into the 10 floats at `y`, in plastic_eval.inc's layout.  Included by kernels_blocks.hip's substrate_eval_kernel and by the stand-alone
// host program of tests/test_substrate_host.py, so that both run this text around the header.
  {
    const V3 e_nf = mk(x[0], x[1], x[2]), e_wo = mk(x[3], x[4], x[5]), e_wi = mk(x[6], x[7], x[8]);
    const V3 e_kd = mk(x[11], x[12], x[13]), e_ks = mk(x[14], x[15], x[16]);
    V3 e_f, e_ws = {0.f, 0.f, 0.f}, e_wgt;
    float e_pdf, e_pdfs;
    substrate::eval(e_nf, e_wo, e_wi, e_kd, e_ks, x[17], e_f, e_pdf);
    y[0] = e_f.x; y[1] = e_f.y; y[2] = e_f.z; y[3] = e_pdf;
    if (!substrate::sample_f(e_nf, e_wo, x[9], x[10], e_kd, e_ks, x[17], e_ws, e_wgt, e_pdfs)) e_ws = e_wgt = {0.f, 0.f, 0.f};
    y[4] = e_ws.x; y[5] = e_ws.y; y[6] = e_ws.z;
    y[7] = e_wgt.x; y[8] = e_wgt.y; y[9] = e_wgt.z;
  }
