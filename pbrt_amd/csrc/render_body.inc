// render_body.inc -- the body of every family of render kernels (render_variant.hpp), included once in each family's kernel unit: they are the
// same program text, with the compile-time constants SPH, COUNT, EXACT, STACK, STEPS, WIDE, SND, MIS, TEX, GLS, PLS, ENV, NRM, LREC in scope -- template
// arguments where the family has the switch, constants where it does not.  (A shared __device__
// function would be the tidy way to say this; the text is included instead because wrapping the body in a function -- forceinline or
// not -- perturbs the register allocation of the production instantiation, whose machine code the committed counter profiles are
// keyed by: pbrt_amd/isa_id.py; measured in round 5.)  In scope as well: `S` (DevScene) and `R` (RenderParams), the kernel's arguments.
  // the walk's stack, rows of 64 lanes x 4 bytes as dynamic shared memory: the launch sizes it per scene (capi_render.cpp render_launch;
  // exact walk: STACK rows of refs followed by STACK rows of entry distances)
  extern __shared__ uint32_t lds_stack[];
  const uint32_t lane = threadIdx.x;
  uint32_t *stk = lds_stack + lane;
  float *stkt = reinterpret_cast<float *>(lds_stack + (EXACT ? STACK : 0) * 64) + lane;  // entry distances: exact walk only
  uint32_t *ovf = R.stack_overflow + (size_t)blockIdx.x * R.stack_overflow_entries * 64u;  // wave-uniform (SGPRs); the lane is added at use

  // Work is handed out dynamically (see the fetch step of the service stage) in ITEMS: item number `item` of this rank
  // is chunk ((item >> 6) & (K - 1)) of pixel (item & 63) of 8x8 block (item >> (6 + log2 K)) -- the 64 K items of a block are its 64
  // pixels at chunk 0, then at chunk 1, ... so a wave that draws 64 consecutive items holds one 8x8 block at one
  // chunk.  Pixel number q = block * 64 + pixel is pixel (q & 63) of 8x8 block ((q >> 6) & 63) of local super-tile
  // (q >> 12), both row-major.
  const int32_t W = R.sw, H = R.sh;  // the sampled pixels: the cropped window, plus the halo of a wide filter
  const uint32_t stx = (uint32_t)(W + 63) >> 6;
  const uint64_t seq0 = R.seed * (uint64_t)R.seq_w * (uint64_t)R.seq_h;
  uint32_t item = 0;
  // tsup / stx by R.stx_recip = ceil(2^32 / stx): exact for tsup * stx < 2^32 (checked by the host); the compiler's own
  // division by a run-time value keeps a float reciprocal in a VGPR for the whole kernel
  auto pixel_xy = [&](uint32_t q, int32_t &xr, int32_t &yr) {
    const uint32_t tsup = R.rank + (q >> 12) * R.world;
    const uint32_t ty = stx == 1u ? tsup : __umulhi(tsup, R.stx_recip), tx = tsup - ty * stx;
    xr = (int32_t)(tx * 64u + ((q >> 6) & 7u) * 8u + (q & 7u));
    yr = (int32_t)(ty * 64u + ((q >> 9) & 7u) * 8u + ((q >> 3) & 7u));
  };
  const uint32_t kb = R.chunk_shift, chunk_mask = (1u << kb) - 1u;  // K = 2^kb chunks per pixel
  auto item_pixel = [&](uint32_t it) { return ((it >> (6u + kb)) << 6) | (it & 63u); };
  // place of pixel q in the rank's slab (super-tiles back to back, row-major inside) and so of its 8 partial sums
  auto slab_pos = [](uint32_t q) {
    return (size_t)(q >> 12) * 4096u + (((q >> 9) & 7u) * 8u + ((q >> 3) & 7u)) * 64u + ((q >> 6) & 7u) * 8u + (q & 7u);
  };
  const bool sobol = SND ? true : R.sampler == 1u;  // (the low-discrepancy samplers keep {pixel key, request counter} in rng.state)
  const bool halton = SND && R.sampler == 3u;       // (samplers 2 and 3 share the SND instantiations: R.sobol_mat is the one's matrices or the other's table)
  const uint32_t spp = R.spp_x * R.spp_y;
  const uint32_t spp_mask = R.spp_mask;  // Sobol: 2^ceil(log2 spp) - 1
  const uint32_t nL = S.n_lights;
  const float nLf = S.n_lights_f;  // (float)nL, converted on the host: a kernel argument stays in an SGPR
  const bool direct_only = R.integrator == 1u;
  const TravTuning tune = {R.min_walkers, R.min_parked};

  // the production walk's LDS rows (0 = the whole stack in LDS); with LREC path records 0..2 lie in LDS behind them (kernel_path.hpp)
  constexpr uint32_t WROWS = (!EXACT && STACK != 0) ? (LREC ? kQuadLdsWalkRows : (uint32_t)STACK) : 0u;
  const LaneRecords rec = {reinterpret_cast<char *>(R.lane_state + (size_t)blockIdx.x * 320u + 128u), lane * 16u,
                           LREC ? lds_addr(lds_stack) + WROWS * kRowBytes : 0u};
  uint32_t state = ST_FETCH;
  if (WIDE) wide_slots_clear(R.wide_slots, lane);  // the lane's footprint slots start empty, and every flush leaves them so
  uint32_t region = blockIdx.x % R.n_regions;  // the part of the pixel list this wave draws from
  unsigned long long c_cam = 0, c_bounce = 0, c_shadow = 0, c_nodes = 0, c_tris = 0;
  Trav T;
  T.o = mk(0.f, 0.f, 0.f);
  T.d = mk(0.f, 0.f, 1.f);
  T.tmax = 0.f;
  T.cur = kDone;
  T.sp = 0;
  T.any = 0;
  T.h = HitRec{kInf, kNoPrim, kNoPrim, 0.f, 0.f};

  EXP_PROBE_INIT(lane);
  for (;;) {
    // ---- service stage: lanes whose walk is over consume the result and launch the next ray ----
    EXP_PROBE_LANES(4, state != ST_DONE && T.cur == kDone);
    const bool serve = state != ST_DONE && T.cur == kDone;
    PathState P;
    bool launch = false, launch_any = false;
    V3 ro = T.o, rd = T.d;
    float rtmax = kInf;
    int32_t xr = 0, yr = 0;
    if (serve && state != ST_FETCH) {
      path_load<LREC>(rec, P);
      pixel_xy(item_pixel(item), xr, yr);
      P.rng.inc = ((((seq0 + (uint64_t)(R.seq_y0 + yr) * (uint64_t)R.seq_w + (uint64_t)(R.seq_x0 + xr)) << kb) + ((item >> 6) & chunk_mask)) << 1) | 1u;
      PROBE_SEC(1);
      if (state != ST_NEW) {
        bool advance = false;  // take the prepared bounce (or end the sample)
        if (state == ST_SHADOW) {
          EXP_DEBUG_PIXEL("HIP s %u   shadow Lpend %08x occluded %u tmax %a\n", P.s, __float_as_uint(rec_load(rec, kRecLpend).x), T.any >> 1, T.tmax);
          if (T.any != 3u) {  // unoccluded: the light sample counts
            const float4 lp = rec_load(rec, kRecLpend);
            P.L = P.L + mk(lp.x, lp.y, lp.z);
          }
          advance = true;
        } else {
          const HitRec h = T.h;
          const bool hit = h.prim != kNoPrim;
          EXP_DEBUG_PIXEL("HIP s %u bounce %u prim %u t %08x b1 %a b2 %a L %08x beta %08x\n", P.s, P.bounces, h.prim, __float_as_uint(h.t), h.b1, h.b2,
                          __float_as_uint(P.L.x), __float_as_uint(P.beta.x));
          EXP_DEBUG_PIXEL("HIP s %u   ray o %a %a %a d %a %a %a\n", P.s, T.o.x, T.o.y, T.o.z, T.d.x, T.d.y, T.d.z);
          V3 p = {0.f, 0.f, 0.f}, ng = {0.f, 0.f, 1.f};
          float4 m0 = {0.f, 0.f, 0.f, 0.f}, m1 = {0.f, 0.f, 0.f, 0.f};
          float tri_area = 0.f;  // MIS: the hit triangle's area
          float4 gl = {0.f, 0.f, 0.f, 1.f};  // GLS: the material's row of mat_extra (scene_tables.hpp): {Kt, eta} of glass, {Ks, alpha} of plastic and substrate
          const V3 wo = -T.d;
          if (hit) {
            uint32_t mid;
            if (!SPH || h.prim < S.n_tris) {
              const float4 a = S.tris[kTriStride * h.slot], b = S.tris[kTriStride * h.slot + 1], c = S.tris[kTriStride * h.slot + 2];
              const V3 p0 = xyz(a), p1 = xyz(b), p2 = xyz(c);
              ng = unit(cross(p1 - p0, p2 - p0));
              if (MIS) { const V3 cr = cross(p1 - p0, p2 - p0); tri_area = 0.5f * sqrtf(dot(cr, cr)); }
              const float w = (1.0f - h.b1) - h.b2;
              p = (p0 * w + p1 * h.b1) + p2 * h.b2;
              mid = __float_as_uint(b.w);
            } else {
              const uint32_t si = h.prim - S.n_tris;
              const float4 cr = S.spheres[kSphereRows * si];
              const V3 c = xyz(cr);
              const V3 ph = (T.o - c) + T.d * h.t;
              ng = ph / cr.w;
              p = c + ph;
              mid = __float_as_uint(S.spheres[kSphereRows * si + 1u].x);
            }
            m0 = S.mats[kMatRows * mid];
            m1 = S.mats[kMatRows * mid + 1u];
            if (GLS && (mat_is_glass(__float_as_uint(m0.x)) || (PLS && mat_is_coated(__float_as_uint(m0.x))))) gl = R.mat_extra[mid];  // (PLS: {Ks, alpha} of a plastic or a substrate material, 3.21, 3.24)
          }
          if (P.bounces == 0 || P.specular) {
            if (hit) {
              const V3 le = xyz(m1);
              if ((le.x > 0.f || le.y > 0.f || le.z > 0.f) && dot(ng, wo) > 0.f) P.L = P.L + P.beta * le;
            } else if (ENV) {
              // the ray escapes into the environment map (DESIGN.md 3.17): L += beta (le_inf + Le(d)), in full -- no light sample stood for it
              float pdf_l;
              V3 le = env_le(R, T.d, &pdf_l);
              if (S.has_inf) le = mk(S.le_inf[0], S.le_inf[1], S.le_inf[2]) + le;
              P.L = P.L + P.beta * le;
            } else if (S.has_inf) {
              P.L = P.L + P.beta * mk(S.le_inf[0], S.le_inf[1], S.le_inf[2]);
            }
          } else if (MIS) {
            // DESIGN.md 3.14: this ray was drawn from the BSDF with density pb (kept beside the pending light sample); light sampling
            // would have drawn its direction with pl -- an emissive triangle: (t^2 / (cos_l A)) / nL, the constant environment: pb / nL
            if (hit && (!SPH || h.prim < S.n_tris)) {
              const V3 le = xyz(m1);
              const float cl = dot(ng, wo);
              if ((le.x > 0.f || le.y > 0.f || le.z > 0.f) && cl > 0.f) {
                const float pb = rec_load(rec, kRecLpend).w;
                const float pl = ((h.t * h.t) / (cl * tri_area)) / nLf;
                const float w = mis_weight_bsdf(pb, pl);
                P.L = P.L + (P.beta * le) * w;
              }
            } else if (PLS && SPH && hit) {
              // 3.25: a sphere that a sphere light names, met from outside: light sampling would have drawn this direction with
              // pl = pdf_omega(origin) / nL.  A sphere that no light names adds nothing here, as ever
              const uint32_t si = h.prim - S.n_tris;
              const V3 le = xyz(m1);
              if (sphere_listed(S, si) && (le.x > 0.f || le.y > 0.f || le.z > 0.f) && dot(ng, wo) > 0.f) {
                const float4 cr = S.spheres[kSphereRows * si];
                const float pb = rec_load(rec, kRecLpend).w;
                const float pl = sphere_light::pdf_omega(T.o, xyz(cr), cr.w) / nLf;
                const float w = mis_weight_bsdf(pb, pl);
                P.L = P.L + (P.beta * le) * w;
              }
            } else if (!hit && S.has_inf) {
              const float w = (nLf * nLf) / (nLf * nLf + 1.0f);
              P.L = P.L + (P.beta * mk(S.le_inf[0], S.le_inf[1], S.le_inf[2])) * w;
            }
            if (ENV && !hit) {
              // 3.17: the BSDF-sampled ray found the map; light sampling would have drawn this direction with pl = pdf_omega(d) / nL
              // (the constant part above keeps its own weight)
              float pdf_l;
              const V3 le = env_le(R, T.d, &pdf_l);
              const float pb = rec_load(rec, kRecLpend).w;
              const float pl = pdf_l / nLf;
              const float w = mis_weight_bsdf(pb, pl);
              P.L = P.L + (P.beta * le) * w;
            }
          }
          PROBE_SEC(2);
          P.cont = false;
          bool need_shadow = false;
          if (hit && P.bounces < R.max_depth) {
            const V3 nf = dot(ng, wo) < 0.f ? -ng : ng;
            const V3 po = p + nf * kSpawnEps;
            // NRM (DESIGN.md 3.18): a triangle's corner normals interpolated like the hit point give the shading normal nsh, which takes nf's
            // place where matte and mirror scatter; `smooth` = the triangle had a usable one (else nsh is nf and nothing below differs)
            V3 nsh = nf;
            bool smooth = false;
            if (NRM && (!SPH || h.prim < S.n_tris)) {
              const float4 q0 = R.tri_n[3u * h.slot], q1 = R.tri_n[3u * h.slot + 1u], q2 = R.tri_n[3u * h.slot + 2u];
              const V3 sn_n0 = xyz(q0), sn_n1 = xyz(q1), sn_n2 = xyz(q2);
              const float sn_b1 = h.b1, sn_b2 = h.b2;
#include "shading_normal.inc"
              nsh = nsf;
              smooth = !sn_fell_back;
            }
            V3 k = {m0.y, m0.z, m0.w};
            if (TEX && __float_as_uint(m1.w) != 0u) {
              // Kd from a texture (DESIGN.md 3.15; pbrt-v3 Checkerboard2DTexture over UVMapping2D, aamode none): the triangle's corner
              // (u, v) interpolated like the hit point -- a sphere: its own (u, v), sphere_uv --, (s, t) = (su u + du, sv v + dv), tex1 where
              // floor(s) + floor(t) is even
              const float4 t0 = R.textures[3u * (__float_as_uint(m1.w) - 1u)], t1 = R.textures[3u * (__float_as_uint(m1.w) - 1u) + 1u],
                           t2 = R.textures[3u * (__float_as_uint(m1.w) - 1u) + 2u];
              float tu, tv;
              if (!SPH || h.prim < S.n_tris) {
                const float2 uv0 = R.tri_uv[3u * h.slot], uv1 = R.tri_uv[3u * h.slot + 1u], uv2 = R.tri_uv[3u * h.slot + 2u];
                const float w = (1.0f - h.b1) - h.b2;
                tu = (uv0.x * w + uv1.x * h.b1) + uv2.x * h.b2;
                tv = (uv0.y * w + uv1.y * h.b1) + uv2.y * h.b2;
              } else {
                sphere_uv(ng.x, ng.y, ng.z, &tu, &tv);
              }
              const float ss = t1.w * tu + t2.y, tt = t2.x * tv + t2.z;
              if (__float_as_uint(t0.x) == image::kSlotType) {
                // Kd from an image (DESIGN.md 3.20): the slot's rows hold its size, wrap and filter and its place in the texel pool
                image::lookup(R.image_texels, t0, t2.w, ss, tt, &k.x, &k.y, &k.z);
              } else {
                // the cell's parity taken in FLOAT (an (int) cast of a huge or non-finite s saturates on the GPU and is undefined on the host:
                // ADVICE r05): f - 2 floor(f / 2) is 0 or 1 exactly while f is an integer below 2^24, 0 beyond (every such float is even), NaN -> tex2
                const float cf = floorf(ss) + floorf(tt);
                k = (cf - 2.0f * floorf(0.5f * cf)) == 0.f ? mk(t0.y, t0.z, t0.w) : mk(t1.x, t1.y, t1.z);
              }
            }
            V3 sh_d = {0.f, 0.f, 1.f};
            float sh_tmax = kInf;
            bool alive = true;
            V3 lpend = {0.f, 0.f, 0.f};
            bool transmitted = false;  // GLS: the bounce ray leaves on the far side of the surface
            if (GLS && mat_is_glass(__float_as_uint(m0.x))) {
              // glass (DESIGN.md 3.16; pbrt-v3 FresnelSpecular): ONE 1-D request chooses reflection (probability F, weight Kr) or
              // refraction (1 - F, weight Kt eta_i^2 / eta_t^2); no light sample, no shadow ray; specular like the mirror
              const float cos_o = dot(ng, wo);
              const float ci = fminf(fabsf(cos_o), 1.0f);
              const float r = cos_o > 0.f ? 1.0f / gl.w : gl.w;  // eta_i / eta_t: entering where wo is on the normal's side
              float F, ct;
              glass_fresnel(ci, r, F, ct);
              const float u = sample_1d<SND>(P, sobol, spp_mask, R.sobol_mat, halton);
              if (u < F) {
                P.wi_next = -wo + nf * (2.0f * ci);
                P.beta = P.beta * k;
              } else {
                P.wi_next = -wo * r + nf * (r * ci - ct);
                P.beta = P.beta * (mk(gl.x, gl.y, gl.z) * (r * r));
                transmitted = true;
              }
              P.specular = true;
            } else if (mat_is_matte(__float_as_uint(m0.x))) {
              if (nL > 0u) {
                const float xi = sample_1d<SND>(P, sobol, spp_mask, R.sobol_mat, halton);
                float u1, u2;
                sample_2d<SND>(P, sobol, spp_mask, u1, u2, R.sobol_mat, halton);
                uint32_t li = (uint32_t)(xi * nLf);
                li = min(li, nL - 1u);
                V3 Ld;
                if (ENV && light_type(S, li) == kDevLightEnv) {  // the environment map's light (3.17): the same (u1, u2)
                  // (NRM: a light sample counts only from the geometric front side as well)
                  if (sample_env_light(R, nsh, k, u1, u2, nLf, Ld, sh_d, sh_tmax, MIS) && (!(NRM && smooth) || dot(sh_d, nf) > 0.f)) {
                    need_shadow = true;
                    lpend = P.beta * Ld;
                    if (!MIS) rec_store(rec, kRecLpend, make_float4(lpend.x, lpend.y, lpend.z, 0.f));
                  }
                } else
                if (PLS && dev_light_beyond_chain(light_type(S, li))) {
                  // a spot light (3.22), a mapped light (3.23) or a sphere light (3.25): taken before sample_light's chain, which does not know them, by ONE compare
                  if (light_type(S, li) == kDevLightSpot ? sample_light_spot(S, li, po, nsh, k, nLf, Ld, sh_d, sh_tmax)
                      : light_type(S, li) == kDevLightSphere ? sample_light_sphere(S, li, po, nsh, k, u1, u2, nLf, Ld, sh_d, sh_tmax, MIS)
                                                                           : sample_light_mapped(S, R.textures, R.image_texels, li, po, nsh, k, nLf, Ld, sh_d, sh_tmax)) {
                    need_shadow = true;
                    lpend = P.beta * Ld;
                    if (!MIS) rec_store(rec, kRecLpend, make_float4(lpend.x, lpend.y, lpend.z, 0.f));
                  }
                } else
                if (sample_light(S, li, po, nsh, k, u1, u2, nLf, Ld, sh_d, sh_tmax, MIS) && (!(NRM && smooth) || dot(sh_d, nf) > 0.f)) {
                  need_shadow = true;
                  lpend = P.beta * Ld;
                  if (!MIS) rec_store(rec, kRecLpend, make_float4(lpend.x, lpend.y, lpend.z, 0.f));
                }
              }
              PROBE_SEC(3);
              if (direct_only) {
                alive = false;
              } else {
                float u1, u2;
                sample_2d<SND>(P, sobol, spp_mask, u1, u2, R.sobol_mat, halton);
                const float z = cosine_about(nsh, u1, u2, P.wi_next);
                EXP_DEBUG_PIXEL("HIP s %u   cos u1 %a u2 %a z %a nf %a %a %a wi %a %a %a\n", P.s, u1, u2, z, nf.x, nf.y, nf.z, P.wi_next.x, P.wi_next.y, P.wi_next.z);
                if (z == 0.f || (NRM && smooth && !(dot(P.wi_next, nf) > 0.f))) alive = false;  // (NRM: the lobe reflects to the geometric front side only)
                else { P.beta = P.beta * k; P.specular = false; }
                // MIS: the pending light sample and, beside it, the density the bounce ray was drawn with (read where it lands)
                if (MIS) rec_store(rec, kRecLpend, make_float4(lpend.x, lpend.y, lpend.z, z * kInvPi));
              }
            } else if (PLS && mat_is_coated(__float_as_uint(m0.x))) {  // (plastic and substrate by ONE compare)
              // plastic (DESIGN.md 3.21; plastic_bsdf.hpp) and substrate (3.24; substrate_bsdf.hpp: the same direction sampler, another f; only
              // the BSDF inside the eval / sample_f calls is chosen by the type word): k = Kd, gl = {Ks, alpha}.  The requests of a matte vertex in their order -- the
              // pick, the light's pair, the bounce's pair --; the light sample carries f(wo, wi) in the Lambertian factor's place and, with
              // MIS, the weight against THIS BSDF's density; the bounce keeps its density beside the pending light sample as matte does
              const V3 ks = mk(gl.x, gl.y, gl.z);
              const bool coat = mat_is_substrate(__float_as_uint(m0.x));
              if (nL > 0u) {
                const float xi = sample_1d<SND>(P, sobol, spp_mask, R.sobol_mat, halton);
                float u1, u2;
                sample_2d<SND>(P, sobol, spp_mask, u1, u2, R.sobol_mat, halton);
                uint32_t li = (uint32_t)(xi * nLf);
                li = min(li, nL - 1u);
                V3 Lg;
                float pl;
                if (sample_light_general(S, R.textures, R.image_texels, li, po, nf, u1, u2, nLf, Lg, sh_d, sh_tmax, pl)) {
                  V3 f;
                  float pbl;
                  coated::eval(coat, nf, wo, sh_d, k, ks, gl.w, f, pbl);
                  V3 Ld = f * Lg;
                  if (MIS && pl > 0.f) {
                    // (the constant infinite light keeps 3.14's constant pair of weights, 1 / (1 + nL^2) here and nL^2 / (nL^2 + 1) where a
                    // bounce ray escapes: the escape does not know the vertex it left, and the pair sums to one whatever the BSDF)
                    Ld = Ld * (light_type(S, li) == kDevLightInfinite ? 1.0f / (1.0f + nLf * nLf) : mis_weight_light(pl, pbl));
                  }
                  need_shadow = true;
                  lpend = P.beta * Ld;
                  if (!MIS) rec_store(rec, kRecLpend, make_float4(lpend.x, lpend.y, lpend.z, 0.f));
                }
              }
              if (direct_only) {
                alive = false;
              } else {
                float u1, u2;
                sample_2d<SND>(P, sobol, spp_mask, u1, u2, R.sobol_mat, halton);
                V3 wgt;
                float pb;
                if (!coated::sample_f(coat, nf, wo, u1, u2, k, ks, gl.w, P.wi_next, wgt, pb)) alive = false;
                else { P.beta = P.beta * wgt; P.specular = false; }
                if (MIS) rec_store(rec, kRecLpend, make_float4(lpend.x, lpend.y, lpend.z, pb));
              }
            } else {  // mirror
              const float c = dot(wo, nsh);
              P.wi_next = -wo + nsh * (2.0f * c);
              P.beta = P.beta * k;
              P.specular = true;
              if (NRM && smooth && !(dot(P.wi_next, nf) > 0.f)) alive = false;
            }
            if (alive && P.beta.x == 0.f && P.beta.y == 0.f && P.beta.z == 0.f) alive = false;
            if (alive && P.bounces > 3u) {
              const float mx = fmaxf(P.beta.x, fmaxf(P.beta.y, P.beta.z));
              const float q = fmaxf(0.05f, 1.0f - mx);
              if (sample_1d<SND>(P, sobol, spp_mask, R.sobol_mat, halton) < q) alive = false;
              else P.beta = P.beta / (1.0f - q);
            }
            P.cont = alive;
            ro = po;  // shadow ray and bounce ray both leave from the offset point
            if (GLS && transmitted) ro = p - nf * kSpawnEps;  // (a refracted ray: from below the surface)
            if (need_shadow) {
              rd = sh_d;
              rtmax = sh_tmax;
              state = ST_SHADOW;
              launch = true;
              launch_any = true;
              if (COUNT) c_shadow++;
            }
          }
          if (!need_shadow) advance = true;
        }
        PROBE_SEC(4);
        if (advance) {
          bool go = P.cont;
          if (go) {
            P.bounces++;
            // a ray at the depth limit can only collect emission, and only after a P.specular bounce
            // (with MIS it is also the BSDF-sampled half of the last vertex's direct-light estimate)
            if (P.bounces >= R.max_depth && !P.specular && !MIS) go = false;
          }
          if (go) {
            rd = P.wi_next;
            rtmax = kInf;
            state = ST_CLOSEST;
            launch = true;
            launch_any = false;
            if (COUNT) c_bounce++;
          } else {
            // radiance sanitising of SamplerIntegrator::Render, then FilmTile::AddSample (box filter)
            const float y = (0.212671f * P.L.x + 0.715160f * P.L.y) + 0.072169f * P.L.z;
            if (isnan(P.L.x) || isnan(P.L.y) || isnan(P.L.z) || y < -1e-5f || isinf(y)) P.L = {0.f, 0.f, 0.f};
            else if (y > R.max_lum) P.L = P.L * (R.max_lum / y);  // Film "maxsampleluminance" (film.rs:75,279); +inf = none
            EXP_DEBUG_PIXEL("SAMPLE %u %08x %08x %08x\n", P.s, __float_as_uint(P.L.x), __float_as_uint(P.L.y), __float_as_uint(P.L.z));  // (to diff against oracle pixel_samples())
            if (WIDE) {
              // FilmTile::AddSample for a box filter of any radius (DESIGN.md 3.11): weight 1 to every pixel of the cropped
              // window within the radius of the sample's film point (kept in the record the default path has its partial
              // sum in), as 2^-24 fixed point: integer atomics make the sums independent of the order of arrival.  A weighted
              // filter (3.19; wave-uniform: R.filter_table) has the same footprint and a table weight for each of its pixels.
              const float4 fp = rec_load(rec, kRecSum);
              const FilterFootprint fb = filter_footprint(fp.x, fp.y, R.filter_rx, R.filter_ry, S.cx0, S.cy0, S.cx1, S.cy1);
              const int32_t x0 = fb.x0, x1 = fb.x1, y0 = fb.y0, y1 = fb.y1;
              const float lr = fminf(fmaxf(P.L.x, 0.f), kFixedMax), lg = fminf(fmaxf(P.L.y, 0.f), kFixedMax), lb = fminf(fmaxf(P.L.z, 0.f), kFixedMax);
              // Integer sums do not care how they are grouped, and the samples of a chunk -- all in one pixel -- have few
              // distinct footprints: each bound takes one of two neighbouring values as the film point moves through the
              // pixel.  The chunk's samples are therefore added up per footprint in 16 slots of the lane (indexed by the
              // parities of the four bounds; a sample that finds another footprint in its slot goes to the film by
              // itself, which does not happen while a bound keeps to two values) and go to the film in ONE set of atomics
              // per footprint at the chunk's end, instead of (2r + 1)^2 x 4 atomics per sample.
              const int32_t X = R.sx0 + (int32_t)xr - 64, Y = R.sy0 + (int32_t)yr - 64;  // the bounds lie within +-20 of the pixel
              const uint32_t key = (uint32_t)(x0 - X) | ((uint32_t)(x1 - X) << 7) | ((uint32_t)(y0 - Y) << 14) | ((uint32_t)(y1 - Y) << 21);
              const uint32_t slot = ((uint32_t)x0 & 1u) | (((uint32_t)x1 & 1u) << 1) | (((uint32_t)y0 & 1u) << 2) | (((uint32_t)y1 & 1u) << 3);
              // (address = wave-uniform base + a 32-bit lane offset made opaque, as for the path records: nothing of it is
              // hoisted out of the kernel's loop into long-lived registers)
              uint32_t so = lane_here() * 16u + slot * 2048u;
              asm volatile("" : "+v"(so));
              char *sb = reinterpret_cast<char *>(R.wide_slots + (size_t)blockIdx.x * kWideSlotFloat4) + so;
              const float4 a1 = *reinterpret_cast<const float4 *>(sb + 1024);  // {b, samples, footprint}
              const uint32_t pn = __float_as_uint(a1.z), pkey = __float_as_uint(a1.w);
              P.s++;
              if (sobol) P.rng.state &= 0xffffffffull;
              if (R.filter_table != nullptr || __builtin_expect(pn != 0u && pkey != key, 0)) {
                // a weighted filter: every sample goes to the film by itself, with its pixels' weights.  The box: the slot holds
                // another footprint of this pixel (a bound that takes three values: possible only when r +- 1/2 lies within
                // rounding of an integer), and so does this sample, weight 1
                film_add_sample(R, S, fb, lr, lg, lb);
              } else {
                unsigned long long ar = (unsigned long long)(long long)(lr * kFixedOne), ag = (unsigned long long)(long long)(lg * kFixedOne),
                                   ab = (unsigned long long)(long long)(lb * kFixedOne);
                uint32_t an = 1u;
                if (pn != 0u) {
                  const float4 a0 = *reinterpret_cast<const float4 *>(sb);         // {r, g}
                  ar += (unsigned long long)__float_as_uint(a0.x) | ((unsigned long long)__float_as_uint(a0.y) << 32);
                  ag += (unsigned long long)__float_as_uint(a0.z) | ((unsigned long long)__float_as_uint(a0.w) << 32);
                  ab += (unsigned long long)__float_as_uint(a1.x) | ((unsigned long long)__float_as_uint(a1.y) << 32);
                  an += pn;
                }
                *reinterpret_cast<float4 *>(sb) = make_float4(__uint_as_float((uint32_t)ar), __uint_as_float((uint32_t)(ar >> 32)), __uint_as_float((uint32_t)ag), __uint_as_float((uint32_t)(ag >> 32)));
                *reinterpret_cast<float4 *>(sb + 1024) = make_float4(__uint_as_float((uint32_t)ab), __uint_as_float((uint32_t)(ab >> 32)), __uint_as_float(an), __uint_as_float(key));
              }
              // (a complete chunk's sums go to the film where the lane asks for its next item: fewer live registers there)
              state = P.s == chunk_begin(((item >> 6) & chunk_mask) + 1u, spp, kb) ? ST_FETCH : ST_NEW;
            } else {
            // FilmTile::AddSample with the box filter: this pixel, weight 1.  The chunk's partial sum lives in its record.
            const float4 sm = rec_load(rec, kRecSum);
            const V3 sum = mk(sm.x, sm.y, sm.z) + P.L;
            P.s++;
            if (sobol) P.rng.state &= 0xffffffffull;  // request counter of the next sample
            if (P.s == chunk_begin(((item >> 6) & chunk_mask) + 1u, spp, kb)) {
              // the chunk is complete: its partial sum goes to the item's slot; merge_kernel adds a pixel's K in
              // chunk order (Film::merge_film_tile, core/film.rs:313-326)
              R.partials[(slab_pos(item_pixel(item)) << kb) + ((item >> 6) & chunk_mask)] = make_float4(sum.x, sum.y, sum.z, 0.f);
              state = ST_FETCH;  // this lane takes another item
            } else {
              rec_store(rec, kRecSum, make_float4(sum.x, sum.y, sum.z, 0.f));
              state = ST_NEW;
            }
            }
          }
          P.cont = false;
        }
      }
    }
    PROBE_SEC(5);
    // ---- fetch: lanes without an item draw the next ones of this rank's item list (wave-uniform; one atomic per
    // wave and round).  An item stays with its lane for all its samples, so its RNG stream, sample order and partial
    // sum are those of DESIGN.md 3.1 whichever lane happens to take it; what the dynamic hand-out removes is the
    // idling of lanes whose pixels have short paths (sky) beside long ones, and -- items being a K-th of a pixel --
    // the wait for the sequential samples of the frame's most expensive pixels at its end. ----
    if (WIDE && state == ST_FETCH) {
      // the finished chunk's sums, one set of atomics per footprint (xr, yr are still its pixel)
      const int32_t X = R.sx0 + (int32_t)xr - 64, Y = R.sy0 + (int32_t)yr - 64;
      uint32_t lo = lane_here() * 16u;
      asm volatile("" : "+v"(lo));
      const char *lb = reinterpret_cast<const char *>(R.wide_slots + (size_t)blockIdx.x * kWideSlotFloat4) + lo;
#pragma nounroll
      for (uint32_t sl = 0u; sl < 16u; sl++) {
        const float4 f1 = *reinterpret_cast<const float4 *>(lb + sl * 2048u + 1024u);
        const uint32_t fn = __float_as_uint(f1.z), fk = __float_as_uint(f1.w);
        if (fn == 0u) continue;
        const float4 f0 = *reinterpret_cast<const float4 *>(lb + sl * 2048u);
        film_add(R.acc, S, X + (int32_t)(fk & 127u), X + (int32_t)((fk >> 7) & 127u), Y + (int32_t)((fk >> 14) & 127u), Y + (int32_t)((fk >> 21) & 127u),
                 (unsigned long long)__float_as_uint(f0.x) | ((unsigned long long)__float_as_uint(f0.y) << 32),
                 (unsigned long long)__float_as_uint(f0.z) | ((unsigned long long)__float_as_uint(f0.w) << 32),
                 (unsigned long long)__float_as_uint(f1.x) | ((unsigned long long)__float_as_uint(f1.y) << 32), fn);
        *reinterpret_cast<float4 *>(const_cast<char *>(lb) + sl * 2048u + 1024u) = make_float4(0.f, 0.f, 0.f, 0.f);  // empty again
      }
    }
    for (;;) {
      const unsigned long long mw = __ballot(state == ST_FETCH);
      if (mw == 0ull) break;
      // XCD-aware hand-out: workgroup w runs on XCD w mod 8 (each XCD has its own 4 MiB L2), so the list is cut into
      // n_regions contiguous parts and a wave draws from the part of its XCD -- the waves that share an L2 render
      // one part of the image -- and helps the next part when its own is exhausted.
      uint32_t base = 0, lim = R.n_items;
      for (uint32_t tries = 0; tries < R.n_regions; tries++) {
        // (parts are cut at multiples of 64 K items = whole 8x8 blocks)
        const uint32_t nblk = R.n_items >> (6u + kb);
        const uint32_t lo = ((nblk * region) / R.n_regions) << (6u + kb);  // (nblk < 2^26 / 8, at most 8 regions)
        const uint32_t hi = ((nblk * (region + 1u)) / R.n_regions) << (6u + kb);
        if (lane == 0) base = atomicAdd(R.next_item + 16u * region, (uint32_t)__popcll(mw));
        base = __builtin_amdgcn_readfirstlane(base) + lo;
        lim = hi;
        if (base < hi) break;
        region = region + 1u < R.n_regions ? region + 1u : 0u;  // own part exhausted: help the next one
        base = lim;
      }
      if (state == ST_FETCH) {
        const uint32_t it = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mw >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mw, 0u));  // set bits below this lane
        if (it >= lim) {
          if (base >= lim) state = ST_DONE;  // every part exhausted (else: this lane draws again in the next round)
        } else {
          const uint32_t q = item_pixel(it), chunk = (it >> 6) & chunk_mask;
          pixel_xy(q, xr, yr);
          if (xr < W && yr < H) {  // (pixels of a ragged super-tile outside the image are skipped)
            if (chunk_begin(chunk, spp, kb) == chunk_begin(chunk + 1u, spp, kb)) {
              // an empty chunk (fewer than 8 samples per pixel): its partial sum is zero; the lane draws again
              if (!WIDE) R.partials[(slab_pos(q) << kb) + chunk] = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
              item = it;
              if (!WIDE) rec_store(rec, kRecSum, make_float4(0.f, 0.f, 0.f, 0.f));
              P.L = {0.f, 0.f, 0.f};
              P.beta = {1.f, 1.f, 1.f};
              P.wi_next = {0.f, 0.f, 0.f};
              const uint64_t pixel_seq = seq0 + (uint64_t)(R.seq_y0 + yr) * (uint64_t)R.seq_w + (uint64_t)(R.seq_x0 + xr);
              if (sobol) P.rng.state = mix32((uint32_t)pixel_seq ^ mix32((uint32_t)(pixel_seq >> 32) + 0x9e3779b9u));
              else pcg_seq(P.rng, (pixel_seq << kb) + chunk);
              P.s = chunk_begin(chunk, spp, kb);
              P.bounces = 0;
              P.specular = false;
              P.cont = false;
              state = ST_NEW;
            }
          }
        }
      }
    }
    PROBE_SEC(6);
    if (serve && state != ST_DONE) {
      if (state == ST_NEW) {
        if (true) {
          // stratified camera sample (DESIGN.md 3.1) and PerspectiveCamera ray (3.2)
          float u1, u2;
          sample_2d<SND>(P, sobol, spp_mask, u1, u2, R.sobol_mat, halton);
          float jx = u1, jy = u2;  // Sobol: the (0,2)-net point is the film offset
          if (!sobol) {
            // P.s / spp_x by R.spp_x_recip = ceil(2^32 / spp_x): the estimate is the quotient or one more
            uint32_t sy = R.spp_x == 1u ? P.s : __umulhi(P.s, R.spp_x_recip);
            if (sy * R.spp_x > P.s) sy--;
            const uint32_t sx = P.s - sy * R.spp_x;
            jx = fminf(((float)sx + u1) * R.inv_nx, kOneMinusEps);
            jy = fminf(((float)sy + u2) * R.inv_ny, kOneMinusEps);
          }
          const float fx = (float)(R.sx0 + xr) + jx, fy = (float)(R.sy0 + yr) + jy;
          if (WIDE) rec_store(rec, kRecSum, make_float4(fx, fy, 0.f, 0.f));  // the film point, for the filter's footprint
          const V3 dc = unit(mk(fx * S.cam_ax + S.cam_bx, fy * S.cam_ay + S.cam_by, 1.0f));
          rd = {(S.c2w[0] * dc.x + S.c2w[1] * dc.y) + S.c2w[2] * dc.z,
                (S.c2w[4] * dc.x + S.c2w[5] * dc.y) + S.c2w[6] * dc.z,
                (S.c2w[8] * dc.x + S.c2w[9] * dc.y) + S.c2w[10] * dc.z};
          ro = {S.c2w[3], S.c2w[7], S.c2w[11]};
          rtmax = kInf;
          P.L = {0.f, 0.f, 0.f};
          P.beta = {1.f, 1.f, 1.f};
          P.specular = false;
          P.bounces = 0;
          state = ST_CLOSEST;
          launch = true;
          launch_any = false;
          if (COUNT) c_cam++;
        }
      }
      PROBE_SEC(7);
      path_store<LREC>(rec, P);
      EXP_RAY_LOG(launch, ro, rd, rtmax, launch_any);
      if (launch) trav_begin<EXACT>(S, T, stk, ro, rd, rtmax, launch_any, c_nodes);
    }
    PROBE_SEC(8);
    if (__ballot(state != ST_DONE) == 0ull) break;
    wave_prio(PBRT_PRIO_ARITH);  // traversal arithmetic at priority 0, its fetches at 3 (trav_run)
    trav_run<EXACT, COUNT, WROWS, STEPS, SPH>(S, T, stk, stkt, ovf, state != ST_DONE, tune, c_nodes, c_tris);
    wave_prio(PBRT_PRIO_SERVICE);  // the service stage of the next round: its lanes are not tracing while it lasts
    PROBE_SEC(0);
  }

  EXP_PROBE_FINI(lane);
  if (COUNT) {
    unsigned long long v[5] = {c_cam, c_bounce, c_shadow, c_nodes, c_tris};
    for (int i = 0; i < 5; i++) {
      unsigned long long x = v[i];
      for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
      if (lane == 0) atomicAdd(&R.counters[i], x);
    }
  }
