"""pbrt_amd/csrc/spot_light.hpp compiled FOR THE HOST into a stand-alone program (plain g++ with -ffp-contract=off, nothing of HIP): the
header's text, and spot_eval.inc around it, exactly as kernels_blocks.hip's spot_eval_kernel compiles them for the device.  The program's
<hip/hip_runtime.h> is a stub of a few lines in which __device__ and __forceinline__ mean nothing and float4 is four floats.  Shared by
tests/test_spot_host.py (the header against float64) and tests/test_spot_gpu.py (the device against this program, bit for bit), with the
inputs both use."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IN, N_OUT = 15, 7  # include/pbrt_hip_debug.h PBRT_HIP_SPOT_EVAL_IN / _OUT
F32 = np.float32

STUB = """#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#define __host__
#define __device__
#define __forceinline__ inline
struct float4 { float x, y, z, w; };
"""

MAIN = """#include <cstdio>
#include <vector>
#include "spot_light.hpp"
using namespace pbrt_hip;
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *fi = std::fopen(argv[1], "rb");
  if (!fi) return 3;
  std::fseek(fi, 0, SEEK_END);
  const long bytes = std::ftell(fi);
  std::fseek(fi, 0, SEEK_SET);
  const size_t n = (size_t)bytes / (4 * %d);
  std::vector<float> in(n * %d), out(n * %d);
  if (std::fread(in.data(), 4, in.size(), fi) != in.size()) return 4;
  std::fclose(fi);
  for (size_t i = 0; i < n; i++) {
    const float *x = in.data() + i * %d;
    float *y = out.data() + i * %d;
#include "spot_eval.inc"
  }
  FILE *fo = std::fopen(argv[2], "wb");
  if (!fo) return 5;
  if (std::fwrite(out.data(), 4, out.size(), fo) != out.size()) return 6;
  std::fclose(fo);
  return 0;
}
""" % (N_IN, N_IN, N_OUT, N_IN, N_OUT)


def build(tmp_path):
    """-> the program's path, built under tmp_path"""
    tmp_path = str(tmp_path)
    os.makedirs(os.path.join(tmp_path, "stub", "hip"), exist_ok=True)
    with open(os.path.join(tmp_path, "stub", "hip", "hip_runtime.h"), "w") as f:
        f.write(STUB)
    src, exe = os.path.join(tmp_path, "spot_host.cpp"), os.path.join(tmp_path, "spot_host")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes", "-I", os.path.join(tmp_path, "stub"), "-I",
                    os.path.join(ROOT, "pbrt_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def run(exe, x, tmp_path):
    """x (n, 15) float32 -> (n, 7) float32"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, N_IN)
    fi, fo = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    x.tofile(fi)
    subprocess.run([exe, fi, fo], check=True)
    return np.fromfile(fo, np.float32).reshape(-1, N_OUT)


def _frame(n):
    big_x = np.abs(n[:, 0]) > np.abs(n[:, 1])
    with np.errstate(all="ignore"):
        a = np.stack([-n[:, 2], np.zeros(len(n)), n[:, 0]], 1) / np.sqrt(n[:, 0] ** 2 + n[:, 2] ** 2)[:, None]
        b = np.stack([np.zeros(len(n)), n[:, 2], -n[:, 1]], 1) / np.sqrt(n[:, 1] ** 2 + n[:, 2] ** 2)[:, None]
    v2 = np.where(big_x[:, None], a, b)
    return v2, np.cross(n, v2)


def _about(n, cos_t, phi):
    """unit vectors whose cosine to the unit vectors n is cos_t, at azimuth phi"""
    v2, v3 = _frame(n)
    st = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    w = v2 * (st * np.cos(phi))[:, None] + v3 * (st * np.sin(phi))[:, None] + n * cos_t[:, None]
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def domain_inputs(n=1 << 16, seed=2205):
    """DESIGN.md 3.22's measured domain, float32 rows of 15: po and p in [-2, 2]^3 at least 0.1 apart, nf with cos(nf, wi) in [0.05, 1],
    cos_total in [-0.9, 0.9], a falloff band cos_start - cos_total in [0.02, 0.5] (cos_start <= 0.98), the axis placed so that ct is uniform
    from 0.1 below cos_total to 0.1 above cos_start (within [-1, 1]): a third of the inputs outside the cone, inside it, and in the band,
    none of them aimed at an edge -- ct is continuous, so an input within 4 ulp of a cosine is a one-in-a-million event --, nL of 1 .. 8"""
    r = np.random.default_rng(seed)
    po, p = r.uniform(-2, 2, (n, 3)), r.uniform(-2, 2, (n, 3))
    close = np.linalg.norm(p - po, axis=1) < 0.1
    p[close] += 0.5
    wi = (p - po) / np.linalg.norm(p - po, axis=1, keepdims=True)
    nf = _about(wi, r.uniform(0.05, 1.0, n), r.uniform(0, 2 * np.pi, n))
    cos_total = r.uniform(-0.9, 0.9, n)
    cos_start = np.minimum(cos_total + r.uniform(0.02, 0.5, n), 0.98)
    ct = np.clip(r.uniform(cos_total - 0.1, cos_start + 0.1), -1.0, 1.0)
    axis = _about(-wi, ct, r.uniform(0, 2 * np.pi, n))
    x = np.concatenate([po, nf, p, axis, cos_total[:, None], cos_start[:, None], r.integers(1, 9, (n, 1)).astype(np.float64)], 1).astype(np.float32)
    for k in (3, 9):  # (the vectors unit again AS FLOAT32: what the kernel sees)
        v = x[:, k:k + 3].astype(np.float64)
        x[:, k:k + 3] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    assert (x[:, 12] <= x[:, 13]).all()
    return x


def ct_f32(x):
    """ct = -(wi . axis) of rows x in the header's own float32 operations (IEEE, so numpy's are the same): what an edge input is built from"""
    x = np.asarray(x, np.float32)
    dv = x[:, 6:9] - x[:, 0:3]
    d2 = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
    with np.errstate(all="ignore"):
        wi = dv / np.sqrt(d2)[:, None]
    a = x[:, 9:12]
    return -((wi[:, 0] * a[:, 0] + wi[:, 1] * a[:, 1]) + wi[:, 2] * a[:, 2])


# what an edge input is about: test_spot_host.py says what each kind must give
EDGE_KINDS = ("at_total_soft", "at_total_hard", "at_start", "just_below_total", "whole_sphere", "start_is_one", "on_axis_start_is_one", "po_is_p")


def edge_inputs(n=4096, seed=77):
    """-> (x [n, 15] float32, kind [n] indices into EDGE_KINDS).  The domain's geometry with the cone moved ONTO the input's own float32 ct:
    ct exactly at cos_total (a soft edge: delta = 0; a hard edge cos_total = cos_start: inside), exactly at cos_start, one ulp below
    cos_total; cos_total = cos_start = -1 about an axis-aligned axis (|wi . a| <= 1 exactly there: the falloff is 1 everywhere); cos_start =
    1 off the axis (always in the band or outside) and ON it (an axis-aligned axis along wi: ct = 1 exactly, full intensity); po = p"""
    r = np.random.default_rng(seed)
    x = domain_inputs(n, seed)
    kind = r.integers(0, len(EDGE_KINDS), n)
    one = np.float32(1.0)
    eye = np.eye(3, dtype=np.float32)
    sign = np.where(r.uniform(size=n) < 0.5, -one, one)[:, None]
    k = lambda name: kind == EDGE_KINDS.index(name)  # noqa: E731
    m = k("whole_sphere")
    x[m, 9:12] = (eye[r.integers(0, 3, n)] * sign)[m]
    x[m, 12] = x[m, 13] = -one
    m = k("on_axis_start_is_one")  # p straight along an axis from po, the cone's axis pointing back along it
    ax = r.integers(0, 3, n)
    step = (eye[ax] * sign * r.uniform(0.25, 3.0, (n, 1)).astype(np.float32))
    x[m, 6:9] = (x[:, 0:3] + step)[m]
    step = x[:, 6:9] - x[:, 0:3]  # (as float32 subtracts: still along the one axis)
    x[m, 9:12] = (-np.sign(step) * (eye[ax] != 0))[m]
    x[m, 3:6] = (np.sign(step) * (eye[ax] != 0))[m]  # nf = wi
    x[m, 13] = one
    x[m, 12] = r.uniform(-0.9, 0.9, n).astype(np.float32)[m]
    m = k("start_is_one")
    x[m, 13] = one
    ct = ct_f32(x)
    # (float32's ct AT or a hair beyond +-1: no cosine can sit on it with room for a band above it)
    moved = k("at_total_soft") | k("at_total_hard") | k("at_start") | k("just_below_total")
    kind[moved & ~(np.abs(ct) < one)] = EDGE_KINDS.index("po_is_p")
    m = k("at_total_soft")
    x[m, 12] = ct[m]
    x[m, 13] = np.maximum(x[m, 13], np.nextafter(ct[m], one))
    m = k("at_total_hard")
    x[m, 12] = x[m, 13] = ct[m]
    m = k("at_start")
    x[m, 13] = ct[m]
    x[m, 12] = np.minimum(x[m, 12], ct[m])
    m = k("just_below_total")
    x[m, 12] = np.nextafter(ct[m], one)
    x[m, 13] = np.maximum(x[m, 13], x[m, 12])
    m = k("po_is_p")
    x[m, 6:9] = x[m, 0:3]
    assert (x[:, 12] <= x[:, 13]).all() and (np.abs(x[:, 12:14]) <= 1).all()
    return x, kind
