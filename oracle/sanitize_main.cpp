// sanitize_main.cpp -- a stand-alone program over the oracle's C API for `make -C oracle sanitize` (-fsanitize=address,undefined on the
// oracle's own sources; test infrastructure only, see pbrt_oracle.h).  Three small scenes -- shading normals beside a
// sphere and glass, plastic (3.21) under a sky and an emitter, two image textures in one pool (3.20) with (u, v) that leave [0, 1] --
// rendered under the three integrators and four samplers, through the film and the accumulators, plus the hooks over arrays with
// non-finite inputs.  Exit status 0 and no report = clean.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pbrt_oracle.h"

namespace {

struct SceneBuf {
  std::vector<float> P, tri_uv, tri_n;
  std::vector<uint32_t> idx;
  std::vector<uint16_t> mat_id;
  std::vector<orc_material> mats;
  std::vector<orc_light> lights;
  std::vector<orc_sphere> spheres;
  std::vector<orc_texture> slots;
  std::vector<std::vector<float>> images;
};

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

orc_material material(uint32_t type, float k, float le, uint32_t kd_tex) {
  orc_material m{};
  m.type = type;
  for (int i = 0; i < 3; i++) { m.k[i] = k + 0.1f * (float)i; m.le[i] = le; }
  m.kd_tex = kd_tex;
  return m;
}

void quad(SceneBuf &s, float z, float half, uint16_t mat, bool down) {
  const uint32_t b = (uint32_t)s.P.size() / 3;
  const float c[4][2] = {{-half, -half}, {half, -half}, {half, half}, {-half, half}};
  for (auto &p : c) { s.P.push_back(p[0]); s.P.push_back(p[1]); s.P.push_back(z); }
  const uint32_t up[6] = {0, 1, 2, 0, 2, 3}, dn[6] = {0, 2, 1, 0, 3, 2};
  for (int i = 0; i < 6; i++) s.idx.push_back(b + (down ? dn[i] : up[i]));
  s.mat_id.push_back(mat); s.mat_id.push_back(mat);
}

int render_all(SceneBuf &s, const char *name) {
  orc_scene_desc d{};
  d.P = s.P.data(); d.idx = s.idx.data(); d.mat_id = s.mat_id.data(); d.mats = s.mats.data(); d.lights = s.lights.data(); d.spheres = s.spheres.data();
  d.n_verts = (uint32_t)s.P.size() / 3; d.n_tris = (uint32_t)s.idx.size() / 3; d.n_mats = (uint32_t)s.mats.size();
  d.n_lights = (uint32_t)s.lights.size(); d.n_spheres = (uint32_t)s.spheres.size();
  const float c2w[16] = {1, 0, 0, 0.3f, 0, 0, 1, -4.f, 0, 1, 0, 1.2f, 0, 0, 0, 1};  // looking along +y, z up
  std::memcpy(d.cam_to_world, c2w, sizeof c2w);
  d.fov = 55.f; d.xres = 20; d.yres = 17;
  d.crop[0] = 0.f; d.crop[1] = 1.f; d.crop[2] = 0.f; d.crop[3] = 1.f;
  d.tri_uv = s.tri_uv.empty() ? nullptr : s.tri_uv.data();
  d.textures = s.slots.empty() ? nullptr : s.slots.data();
  d.n_textures = (uint32_t)s.slots.size();
  orc_scene *sc = orc_scene_create(&d);
  if (!sc) { std::fprintf(stderr, "%s: refused\n", name); return 1; }
  std::vector<float> film((size_t)d.xres * d.yres * 4);
  std::vector<int64_t> acc((size_t)d.xres * d.yres * 4);
  double sum = 0;
  for (uint32_t integrator = 0; integrator < 3; integrator++)
    for (uint32_t sampler = 0; sampler < 4; sampler++) {
      orc_render_desc r{};
      r.integrator = integrator; r.max_depth = 6; r.spp_x = 2; r.spp_y = 2; r.seed = 3; r.world_size = 1; r.sampler = sampler;
      if (orc_render(sc, &r, film.data(), nullptr, 2) != 0) return 1;
      for (float v : film) sum += v;
      if (s.tri_n.empty()) {  // (the wide box filter: not beside normals, as in the product)
        r.filter_xwidth = 1.5f; r.filter_ywidth = 0.75f; r.max_sample_luminance = 1.0f;
        std::fill(acc.begin(), acc.end(), 0);
        if (orc_render_acc(sc, &r, acc.data(), nullptr, 2) != 0) return 1;
      }
    }
  orc_scene_destroy(sc);
  std::printf("%s: film sum %.6g\n", name, sum);
  return std::isfinite(sum) && sum > 0 ? 0 : 1;
}

void put(SceneBuf &s, const void *rec) {
  orc_texture t;
  std::memcpy(&t, rec, 64);
  s.slots.push_back(t);
}

void common(SceneBuf &s) {
  quad(s, 0.f, 5.f, 0, false);  // floor
  quad(s, 3.f, 0.8f, 1, true);  // lamp, facing down
  s.lights.push_back(orc_light{2, {0, 0, 0}, {0.3f, 0.35f, 0.45f}, 0.f});
  s.lights.push_back(orc_light{0, {1.5f, -2.f, 2.5f}, {9, 8, 7}, 0.f});
}

}  // namespace

int main() {
  int bad = 0;
  {  // shading normals on every triangle (one all zero, one with a zero corner), a mirror quad, a glass sphere
    SceneBuf s;
    s.mats = {material(0, 0.5f, 0.f, 0), material(0, 0.f, 5.f, 0), material(1, 0.7f, 0.f, 0), material(2, 0.8f, 0.9f, bits_of(1.5f))};
    common(s);
    quad(s, 0.6f, 0.9f, 2, false);
    orc_sphere sp{};
    sp.c[0] = -1.2f; sp.c[1] = 0.5f; sp.c[2] = 0.7f; sp.r = 0.6f; sp.mat = 3;
    s.spheres.push_back(sp);
    const size_t nt = s.idx.size() / 3;
    for (size_t t = 0; t < nt; t++)
      for (int c = 0; c < 3; c++) {
        const bool zero = t == 0 || (t == 2 && c == 1);
        const float n[3] = {0.3f * (float)c - 0.2f, 0.25f - 0.1f * (float)t, t == 2 || t == 3 ? -1.f : 1.f};
        for (float v : n) s.tri_n.push_back(zero ? 0.f : v * (c == 2 ? 300.f : 1.f));
      }
    orc_normals rec{};
    rec.type = 2; rec.n_tris = (uint32_t)nt; rec.tri_n = s.tri_n.data();
    put(s, &rec);
    bad += render_all(s, "normals");
  }
  {  // plastic: the floor, a sphere of alpha 1e-3, a quad with Ks = 0
    SceneBuf s;
    s.mats = {material(3, 0.3f, 0.5f, bits_of(0.4618f)), material(0, 0.f, 5.f, 0), material(3, 0.4f, 0.f, bits_of(1.0f)), material(3, 0.f, 0.6f, bits_of(1e-3f))};
    common(s);
    quad(s, 0.6f, 0.9f, 2, false);
    orc_sphere sp{};
    sp.c[0] = -1.2f; sp.c[1] = 0.5f; sp.c[2] = 0.7f; sp.r = 0.6f; sp.mat = 3;
    s.spheres.push_back(sp);
    bad += render_all(s, "plastic");
  }
  {  // two images in one pool, bilinear / black and point / repeat, corner (u, v) beyond [0, 1] and a mapping that reaches negative s
    SceneBuf s;
    s.mats = {material(0, 0.5f, 0.f, 1), material(0, 0.f, 5.f, 0), material(0, 0.6f, 0.f, 2)};
    common(s);
    quad(s, 0.6f, 0.9f, 2, false);
    orc_sphere sp{};
    sp.c[0] = -1.2f; sp.c[1] = 0.5f; sp.c[2] = 0.7f; sp.r = 0.6f; sp.mat = 2;
    s.spheres.push_back(sp);
    for (size_t t = 0; t < s.idx.size() / 3; t++)
      for (int c = 0; c < 3; c++) { s.tri_uv.push_back(-1.5f + 1.3f * (float)((t + c) % 4)); s.tri_uv.push_back(2.5f - 0.9f * (float)((t + 2 * c) % 5)); }
    s.images.resize(2);
    const uint32_t dims[2][2] = {{3, 5}, {17, 4}};
    for (int k = 0; k < 2; k++) {
      for (uint32_t i = 0; i < 3 * dims[k][0] * dims[k][1]; i++) s.images[k].push_back(0.05f + 0.9f * (float)((i * 7919u + 13u * (uint32_t)k) % 101u) / 100.f);
      orc_image_texture rec{};
      rec.type = 4; rec.width = dims[k][0]; rec.height = dims[k][1]; rec.wrap = k ? 0u : 2u; rec.rgb = s.images[k].data();
      rec.su = k ? -3.1f : 1.7f; rec.sv = k ? 2.2f : -2.3f; rec.du = k ? 0.3f : -0.6f; rec.dv = k ? -0.7f : 0.4f; rec.filter = k ? 0u : 1u;
      put(s, &rec);
    }
    bad += render_all(s, "images");
    // the image hook: every wrap and filter at non-finite and huge (u, v)
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float uv[] = {nan, 0.3f, inf, 0.3f, -inf, 0.3f, 1e30f, -1e30f, 0.7f, nan, -0.25f, 1.75f, 0.f, 1.f, 1e-30f, -1e-30f};
    float rgb[3 * 8];
    orc_image_texture recs[2];
    std::memcpy(&recs[0], &s.slots[0], 64);
    std::memcpy(&recs[1], &s.slots[1], 64);
    for (uint32_t wrap = 0; wrap < 3; wrap++)
      for (uint32_t filter = 0; filter < 2; filter++)
        for (uint32_t which = 0; which < 2; which++) {
          recs[which].wrap = wrap; recs[which].filter = filter;
          bad += orc_image_lookup_eval(recs, 2, which, 8, uv, rgb) != 0;
          for (float v : rgb) bad += !std::isfinite(v);
        }
  }
  {  // the other two hooks at their edges: zero and overflowing normals; grazing, opposite and zero directions, alpha at its ends
    const float big = 3e38f;
    const float nin[2 * 17] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0.3f, 0.3f, 0.1f, 0.2f, -1.f,
                               big, big, big, big, big, big, big, big, big, 0, 0, 1, 0.3f, 0.3f, 0.1f, 0.2f, 1.f};
    float nout[2 * 4];
    bad += orc_shading_normal_eval(2, nin, nout) != 0 || nout[3] != 1.f || nout[7] != 1.f;
    const float pin[3 * 18] = {0, 0, 1, 0, 0, 1, 0, 0, -1, 0.99999994f, 0.f, .5f, .5f, .5f, .5f, .5f, .5f, 1e-3f,
                               0, 0, 1, 1, 0, 1e-4f, -1, 0, 1e-4f, 0.5f, 0.99999994f, .5f, .5f, .5f, .5f, .5f, .5f, 1.f,
                               0, 0, 1, 0, 0, 0, 0, 0, 0, 0.f, 0.5f, .5f, .5f, .5f, .5f, .5f, .5f, 0.05f};
    float pout[3 * 10];
    bad += orc_plastic_eval(3, pin, pout) != 0;
  }
  if (bad) std::fprintf(stderr, "sanitize_main: %d checks failed\n", bad);
  return bad ? 1 : 0;
}
