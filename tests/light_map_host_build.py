"""pbrt_amd/csrc/light_map.hpp compiled FOR THE HOST into a stand-alone program (plain g++ with -ffp-contract=off, nothing of HIP): the
header's text, and light_map_eval.inc around it, exactly as kernels_blocks.hip's light_map_eval_kernel compiles them for the device.  The
program's <hip/hip_runtime.h> is a stub of a few lines in which __device__ and __forceinline__ mean nothing and float4 is four floats.
Shared by tests/test_light_map_host.py (the header against float64) and tests/test_light_map_gpu.py (the device against this program, bit
for bit), with the inputs both use.

An input set is a list of CASES: one light-map record and one image (the hook takes one of each per call) with the rows of 10 floats --
po, nf, p, nL -- that are evaluated under them."""
import os
import subprocess
from dataclasses import dataclass, field

import numpy as np

from spot_host_build import _about

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IN, N_OUT = 10, 11  # include/pbrt_hip_debug.h PBRT_HIP_LIGHT_MAP_EVAL_IN / _OUT
F32 = np.float32
PROJECTION, GONIOMETRIC = 0, 1
REPEAT, CLAMP = 0, 1
POINT, BILINEAR = 0, 1
MIN_Z = F32(1e-3)

STUB = """#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#define __host__
#define __device__
#define __forceinline__ inline
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
"""

# argv: in.bin out.bin record.bin; record.bin = 17 floats -- kind, world_to_light[9], inv_tan, sx, sy, W, H, wrap, filter -- then 3 W H texels,
# row 0 = the image's top
MAIN = """#include <cstdio>
#include <vector>
#include "light_map.hpp"
using namespace pbrt_hip;
static bool slurp(const char *name, std::vector<float> *v) {
  FILE *f = std::fopen(name, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v->resize((size_t)bytes / 4);
  const bool ok = std::fread(v->data(), 4, v->size(), f) == v->size();
  std::fclose(f);
  return ok;
}
int main(int argc, char **argv) {
  if (argc != 4) return 2;
  std::vector<float> in, rec;
  if (!slurp(argv[1], &in) || !slurp(argv[3], &rec) || rec.size() < 17) return 3;
  const uint32_t e_kind = (uint32_t)rec[0], W = (uint32_t)rec[13], H = (uint32_t)rec[14];
  if (rec.size() != 17 + 3 * (size_t)W * H) return 4;
  const float4 e_r0 = make_float4(rec[1], rec[2], rec[3], rec[10]), e_r1 = make_float4(rec[4], rec[5], rec[6], rec[11]),
               e_r2 = make_float4(rec[7], rec[8], rec[9], rec[12]);
  std::vector<float4> pool((size_t)W * H);
  for (size_t i = 0; i < pool.size(); i++) pool[i] = make_float4(rec[17 + 3 * i], rec[18 + 3 * i], rec[19 + 3 * i], 0.f);
  float4 e_t0, t1, t2;
  image::encode(W, H, (uint32_t)rec[15], (uint32_t)rec[16], 1.f, 1.f, 0.f, 0.f, 0u, &e_t0, &t1, &t2);
  const float e_offset = t2.w;
  const float4 *e_pool = pool.data();
  const size_t n = in.size() / %d;
  std::vector<float> out(n * %d);
  for (size_t i = 0; i < n; i++) {
    const float *x = in.data() + i * %d;
    float *y = out.data() + i * %d;
#include "light_map_eval.inc"
  }
  FILE *fo = std::fopen(argv[2], "wb");
  if (!fo) return 5;
  if (std::fwrite(out.data(), 4, out.size(), fo) != out.size()) return 6;
  std::fclose(fo);
  return 0;
}
""" % (N_IN, N_OUT, N_IN, N_OUT)


@dataclass
class Case:
    kind: int
    M: np.ndarray  # world_to_light, (3, 3) float32
    inv_tan: float
    sx: float
    sy: float
    image: np.ndarray  # (H, W, 3) float32, row 0 = the top
    wrap: int
    filt: int
    x: np.ndarray  # (n, 10) float32
    tag: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # (edge inputs: what each row is about)

    def row(self):
        """the `light_maps` row of pbrt_amd.api (the image number is not used by the hook)"""
        return [self.kind, 1, *self.M.reshape(-1), self.inv_tan, self.sx, self.sy]

    def with_filter(self, filt):
        return Case(self.kind, self.M, self.inv_tan, self.sx, self.sy, self.image, self.wrap, filt, self.x, self.tag)


def build(tmp_path):
    """-> the program's path, built under tmp_path"""
    tmp_path = str(tmp_path)
    os.makedirs(os.path.join(tmp_path, "stub", "hip"), exist_ok=True)
    with open(os.path.join(tmp_path, "stub", "hip", "hip_runtime.h"), "w") as f:
        f.write(STUB)
    src, exe = os.path.join(tmp_path, "light_map_host.cpp"), os.path.join(tmp_path, "light_map_host")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes", "-I", os.path.join(tmp_path, "stub"), "-I",
                    os.path.join(ROOT, "pbrt_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def run(exe, case, tmp_path):
    """case -> (n, 11) float32: ok, wi, tmax, scale, s, t, rgb"""
    fi, fo, fr = (os.path.join(str(tmp_path), f) for f in ("in.bin", "out.bin", "rec.bin"))
    np.ascontiguousarray(case.x, F32).reshape(-1, N_IN).tofile(fi)
    H, W = case.image.shape[:2]
    np.concatenate([np.array([case.kind, *case.M.reshape(-1), case.inv_tan, case.sx, case.sy, W, H, case.wrap, case.filt], F32),
                    np.ascontiguousarray(case.image, F32).reshape(-1)]).tofile(fr)
    subprocess.run([exe, fi, fo, fr], check=True)
    return np.fromfile(fo, F32).reshape(-1, N_OUT)


def smooth_image(width=16, height=8):
    """a smooth generated image, everywhere >= 0.05"""
    r, c = np.mgrid[0:height, 0:width].astype(np.float64)
    u, v = (c + 0.5) / width, (r + 0.5) / height
    rgb = np.stack([0.55 + 0.45 * np.sin(2 * np.pi * u) * np.cos(np.pi * v), 0.5 + 0.4 * np.cos(2 * np.pi * (u + v)), 0.35 + 0.3 * np.sin(2 * np.pi * (2 * u - v) + 0.7)], -1)
    assert rgb.min() >= 0.05
    return rgb.astype(F32)


def random_rotation(r):
    """a rotation matrix, float32 (orthonormal to a few 1e-8: far inside scene creation's 1e-4)"""
    q = r.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).astype(F32)


def _rows_from_directions(r, d_world):
    """rows of 10 whose direction FROM the light TO the shading point is d_world (unit, float64): p in [-2, 2]^3, po = p + d t inside the same
    cube with t >= 0.1, nf with cos(nf, wi) in [0.05, 1], nL of 1 .. 8"""
    n = len(d_world)
    p = r.uniform(-2, 2, (n, 3))
    with np.errstate(all="ignore"):
        room = np.where(d_world > 0, (2.0 - p) / d_world, np.where(d_world < 0, (-2.0 - p) / d_world, np.inf)).min(1)
    tight = room < 0.2
    p[tight] *= 0.5  # (towards the centre: at least 1 of room in every direction)
    with np.errstate(all="ignore"):
        room = np.where(d_world > 0, (2.0 - p) / d_world, np.where(d_world < 0, (-2.0 - p) / d_world, np.inf)).min(1)
    t = r.uniform(0.1, np.maximum(room, 0.1001))
    po = p + d_world * t[:, None]
    nf = _about(-d_world, r.uniform(0.05, 1.0, n), r.uniform(0, 2 * np.pi, n))
    x = np.concatenate([po, nf, p, r.integers(1, 9, (n, 1)).astype(np.float64)], 1).astype(F32)
    v = x[:, 3:6].astype(np.float64)
    x[:, 3:6] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)  # (unit again AS FLOAT32: what the kernel sees)
    return x


N_GROUPS = 8
ASPECTS = (0.5, 1.0, 2.0, 0.5, 1.0, 2.0, 1.0, 2.0)


def domain_cases(kind, n=1 << 16, seed=2306, filt=BILINEAR):
    """DESIGN.md 3.23's measured domain: N_GROUPS cases of n / N_GROUPS rows each, every case under a random rotation and the smooth 16 x 8
    image.  Projection (wrap clamp): fov in [20, 120] degrees, aspect 1/2, 1 or 2, directions uniform on the screen from 10 % outside the
    window to its centre -- none of them aimed at an edge.  Goniometric (wrap repeat): directions uniform over the sphere but for the caps
    within sin(theta) < 0.05 of the poles."""
    r = np.random.default_rng(seed + kind)
    cases = []
    m = n // N_GROUPS
    for g in range(N_GROUPS):
        M = random_rotation(r)
        if kind == PROJECTION:
            fov, aspect = r.uniform(20.0, 120.0), ASPECTS[g]
            inv_tan = F32(1.0 / np.tan(np.radians(fov) / 2))
            sx, sy = (F32(aspect), F32(1)) if aspect > 1 else (F32(1), F32(1 / aspect))
            px, py = r.uniform(-1.1, 1.1, m) * float(sx), r.uniform(-1.1, 1.1, m) * float(sy)
            w = np.stack([px / float(inv_tan), py / float(inv_tan), np.ones(m)], 1)
            w /= np.linalg.norm(w, axis=1, keepdims=True)
        else:
            inv_tan = sx = sy = F32(0)
            c = r.uniform(-1, 1, m) * np.sqrt(1 - 0.05 ** 2)
            phi = r.uniform(0, 2 * np.pi, m)
            st = np.sqrt(1 - c * c)
            w = np.stack([st * np.cos(phi), c, st * np.sin(phi)], 1)
        d_world = w @ M.astype(np.float64)  # (M^T w: the rows of M are the light's axes)
        cases.append(Case(kind, M, float(inv_tan), float(sx), float(sy), smooth_image(), CLAMP if kind == PROJECTION else REPEAT, filt, _rows_from_directions(r, d_world)))
    return cases


def header_f32(x, M):
    """wi, w and dist2 of rows x in the header's own float32 operations (IEEE, so numpy's are the same): what an edge input is built from"""
    x, M = np.asarray(x, F32), np.asarray(M, F32).reshape(3, 3)
    dv = x[:, 6:9] - x[:, 0:3]
    d2 = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
    with np.errstate(all="ignore"):
        dist = np.sqrt(d2)
        wi = dv / dist[:, None]
    d = -wi
    w = np.stack([(M[k, 0] * d[:, 0] + M[k, 1] * d[:, 1]) + M[k, 2] * d[:, 2] for k in range(3)], 1)
    return wi, w, d2, dist


def point_scale_f32(x):
    """the point light's (cs / dist2) nL of rows x in float32, operation for operation sample_light's"""
    wi, _, d2, _ = header_f32(x, np.eye(3))
    nf = np.asarray(x, F32)[:, 3:6]
    cs = (wi[:, 0] * nf[:, 0] + wi[:, 1] * nf[:, 1]) + wi[:, 2] * nf[:, 2]
    with np.errstate(all="ignore"):
        return (cs / d2) * np.asarray(x, F32)[:, 9]


def _scaled_rows(r, v, M, n):
    """n rows whose p - po is v (float32) times a power of two -- the SAME unit direction in float32, bit for bit -- with p = 0, a normal
    within 60 degrees of wi and nL of 1 .. 8"""
    v = np.asarray(v, F32)
    k = F32(2.0) ** r.integers(-3, 2, n).astype(F32)
    po = -(v[None, :] * k[:, None])
    wi64 = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64))
    nf = _about(np.tile(wi64, (n, 1)), r.uniform(0.5, 1.0, n), r.uniform(0, 2 * np.pi, n))
    x = np.concatenate([po, nf, np.zeros((n, 3)), r.integers(1, 9, (n, 1))], 1).astype(F32)
    return x


# what an edge input is about: test_light_map_host.py says what each kind must give
EDGE_KINDS = ("px_at_plus_sx", "px_at_minus_sx", "py_at_plus_sy", "px_one_ulp_beyond", "py_one_ulp_beyond", "wz_at_min", "wz_one_ulp_above", "pole_plus", "pole_minus",
              "seam_zero", "seam_below", "po_is_p", "black_texel", "ones")


def edge_cases(seed=91, groups=12, rows=24):
    """-> cases whose `tag` holds indices into EDGE_KINDS.  Every case is built ON the float32 values the header computes for its rows: a
    group of rows shares ONE float32 direction (p - po scaled by powers of two), and the record's window is moved onto that direction's own
    px / py, or the record's rotation onto its w.z (see EDGE_KINDS and test_light_map_host.py)."""
    r = np.random.default_rng(seed)
    one_tex = np.ones((1, 1, 3), F32)
    ident = np.eye(3, dtype=F32)
    cases = []

    def tagged(name, n):
        return np.full(n, EDGE_KINDS.index(name), np.int64)

    for g in range(groups):
        # a direction well inside a projection's frustum under a random rotation
        M = random_rotation(r)
        inv_tan = F32(r.uniform(0.8, 3.0))
        w = np.array([r.uniform(0.2, 0.8) * r.choice([-1, 1]), r.uniform(0.2, 0.8) * r.choice([-1, 1]), 1.0])
        v = (-(w / np.linalg.norm(w)) @ M.astype(np.float64)).astype(F32)  # p - po = -d
        x = _scaled_rows(r, v, M, rows)
        _, wf, _, _ = header_f32(x, M)
        assert (wf == wf[0]).all()  # (one float32 direction for the whole group)
        px, py = (wf[0, 0] / wf[0, 2]) * inv_tan, (wf[0, 1] / wf[0, 2]) * inv_tan
        big = F32(8.0)
        for name, sx, sy in (("px_at_plus_sx" if px > 0 else "px_at_minus_sx", abs(px), big), ("py_at_plus_sy", big, abs(py)),
                             ("px_one_ulp_beyond", np.nextafter(abs(px), F32(0)), big), ("py_one_ulp_beyond", big, np.nextafter(abs(py), F32(0)))):
            if name == "py_at_plus_sy" and py < 0:
                continue  # (the lower edge is covered by px's two signs: the comparison is the same text)
            cases.append(Case(PROJECTION, M, float(inv_tan), float(sx), float(sy), smooth_image(), CLAMP, BILINEAR, x, tagged(name, rows)))
        # w.z AT the least depth and one ulp above it: the light's z axis scaled within scene creation's tolerance so that the product lands there
        vz = np.array([r.uniform(-1, 1), r.uniform(-1, 1), 0.0])
        vz = vz / np.linalg.norm(vz) * np.sqrt(1 - 1e-6)
        v = np.array([-vz[0], -vz[1], -1e-3], F32)
        x = _scaled_rows(r, v, ident, rows)
        wi, _, _, _ = header_f32(x, ident)
        dz = -wi[0, 2]
        for name, target in (("wz_at_min", MIN_Z), ("wz_one_ulp_above", np.nextafter(MIN_Z, F32(1)))):
            c0 = F32(target / dz)
            found = [c for c in (np.nextafter(c0, F32(0)), c0, np.nextafter(c0, F32(2))) if F32(c * dz) == target and abs(float(c) ** 2 - 1) < 5e-5]
            if not found:
                continue
            Mz = ident.copy()
            Mz[2, 2] = found[0]
            cases.append(Case(PROJECTION, Mz, 1.0, 4000.0, 4000.0, one_tex, CLAMP, POINT, x, tagged(name, rows)))
    # the goniometric map's poles, its seam, po = p, a black texel, an image of ones
    for sign, name in ((1.0, "pole_plus"), (-1.0, "pole_minus")):
        x = _scaled_rows(r, np.array([0, -sign * 0.75, 0], F32), ident, rows)  # d = -wi = +-y
        cases.append(Case(GONIOMETRIC, ident, 0.0, 0.0, 0.0, smooth_image(), REPEAT, BILINEAR, x, tagged(name, rows)))
    for g in range(groups):
        a, b = r.uniform(0.1, 1.0), r.uniform(-1.0, 1.0)
        x = _scaled_rows(r, np.array([-a, -b, 0], F32), ident, rows)  # d = (+a, b, 0): phi = 0 exactly
        cases.append(Case(GONIOMETRIC, ident, 0.0, 0.0, 0.0, smooth_image(), REPEAT, BILINEAR, x, tagged("seam_zero", rows)))
        x = _scaled_rows(r, np.array([-a, -b, 1e-7 * a], F32), ident, rows)  # d.z a hair below 0: phi a hair below 2 pi
        cases.append(Case(GONIOMETRIC, ident, 0.0, 0.0, 0.0, smooth_image(), REPEAT, BILINEAR, x, tagged("seam_below", rows)))
    for kind in (PROJECTION, GONIOMETRIC):
        window = (1.0, 1.0, 1.0) if kind == PROJECTION else (0.0, 0.0, 0.0)
        for c in domain_cases(kind, 8 * 64, seed + 5):
            x = c.x.copy()
            x[:, 0:3] = x[:, 6:9]
            cases.append(Case(kind, c.M, *window, one_tex, CLAMP, POINT, x, tagged("po_is_p", len(x))))
        # a 2 x 2 point-sampled image whose top-left texel is black: the directions that land there give no sample
        quad = np.array([[[0, 0, 0], [0.5, 1, 2]], [[1, 1, 1], [2, 0.5, 0]]], F32)
        for c in domain_cases(kind, 8 * 64, seed + 6):
            cases.append(Case(kind, c.M, c.inv_tan, c.sx, c.sy, quad, c.wrap, POINT, c.x, tagged("black_texel", len(c.x))))
        for c in domain_cases(kind, 8 * 64, seed + 7):
            cases.append(Case(kind, c.M, c.inv_tan, c.sx, c.sy, one_tex, c.wrap, POINT, c.x, tagged("ones", len(c.x))))
    return cases
