"""pbrt_amd/csrc/sphere_light.hpp compiled FOR THE HOST into a stand-alone program (plain g++ with -ffp-contract=off, nothing of HIP): the
header's text, and sphere_light_eval.inc around it, exactly as kernels_blocks.hip's sphere_light_eval_kernel compiles them for the device.
The program's <hip/hip_runtime.h> is a stub of a few lines in which __device__ and __forceinline__ mean nothing and float4 is four floats.
Shared by tests/test_sphere_light_host.py (the header against float64) and tests/test_sphere_light_gpu.py (the device against this program,
bit for bit), with the inputs both use: 2^16 of the measured domain and 4096 edge inputs, 69 632 in all."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IN, N_OUT = 13, 8  # include/pbrt_hip_debug.h PBRT_HIP_SPHERE_LIGHT_EVAL_IN / _OUT
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
#include "sphere_light.hpp"
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
#include "sphere_light_eval.inc"
  }
  FILE *fo = std::fopen(argv[2], "wb");
  if (!fo) return 5;
  if (std::fwrite(out.data(), 4, out.size(), fo) != out.size()) return 6;
  std::fclose(fo);
  return 0;
}
""" % (N_IN, N_IN, N_OUT, N_IN, N_OUT)


# the second program: cosine_about (kernel_math.hpp) beside the direction rebuilt from sphere_light.hpp's COPIES of its disk map and frame.
# Per row n xyz (unit), u1, u2 -> cosine_about's wi, then (v2 dx + v3 dy) + n z with z as cosine_about forms it
COPY_MAIN = """#include <cstdio>
#include <vector>
#include "sphere_light.hpp"
using namespace pbrt_hip;
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *fi = std::fopen(argv[1], "rb");
  if (!fi) return 3;
  std::fseek(fi, 0, SEEK_END);
  const size_t n = (size_t)std::ftell(fi) / 20;
  std::fseek(fi, 0, SEEK_SET);
  std::vector<float> in(n * 5), out(n * 6);
  if (std::fread(in.data(), 4, in.size(), fi) != in.size()) return 4;
  std::fclose(fi);
  for (size_t i = 0; i < n; i++) {
    const float *x = in.data() + i * 5;
    float *y = out.data() + i * 6;
    const V3 nn = mk(x[0], x[1], x[2]);
    V3 a;
    cosine_about(nn, x[3], x[4], a);
    float dx, dy;
    sphere_light::disk(x[3], x[4], dx, dy);
    V3 v2, v3;
    sphere_light::frame(nn, v2, v3);
    const float zz = (1.0f - dx * dx) - dy * dy;
    const float z = sqrtf(zz > 0.f ? zz : 0.f);
    const V3 b = (v2 * dx + v3 * dy) + nn * z;
    y[0] = a.x; y[1] = a.y; y[2] = a.z; y[3] = b.x; y[4] = b.y; y[5] = b.z;
  }
  FILE *fo = std::fopen(argv[2], "wb");
  if (!fo) return 5;
  if (std::fwrite(out.data(), 4, out.size(), fo) != out.size()) return 6;
  std::fclose(fo);
  return 0;
}
"""


def build(tmp_path, main=None, name="sphere_light_host"):
    """-> the program's path, built under tmp_path"""
    tmp_path = str(tmp_path)
    os.makedirs(os.path.join(tmp_path, "stub", "hip"), exist_ok=True)
    with open(os.path.join(tmp_path, "stub", "hip", "hip_runtime.h"), "w") as f:
        f.write(STUB)
    src, exe = os.path.join(tmp_path, name + ".cpp"), os.path.join(tmp_path, name)
    with open(src, "w") as f:
        f.write(main or MAIN)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes", "-I", os.path.join(tmp_path, "stub"), "-I",
                    os.path.join(ROOT, "pbrt_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def run(exe, x, tmp_path, n_in=N_IN, n_out=N_OUT):
    """x (n, 13) float32 -> (n, 8) float32 (the copy check: 5 -> 6)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, n_in)
    fi, fo = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    x.tofile(fi)
    subprocess.run([exe, fi, fo], check=True)
    return np.fromfile(fo, np.float32).reshape(-1, n_out)


def _hemisphere_about(w, r):
    """unit vectors uniform on the hemisphere about the unit vectors w"""
    v = r.normal(size=w.shape)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.where(((v * w).sum(1) < 0)[:, None], -v, v)


def domain_inputs(n=1 << 16, seed=2508):
    """DESIGN.md 3.25's measured domain, float32 rows of 13: po and c in [-2, 2]^3 (at least 0.05 apart), r with r / d log-uniform in
    [1e-4, 0.99], nf uniform on the hemisphere about the direction to the centre, (u1, u2) uniform in [0, 1)^2, nL of 1 .. 8"""
    r = np.random.default_rng(seed)
    po, c = r.uniform(-2, 2, (n, 3)), r.uniform(-2, 2, (n, 3))
    close = np.linalg.norm(c - po, axis=1) < 0.05
    c[close] += 0.5
    x = np.zeros((n, N_IN), np.float32)
    x[:, 0:3], x[:, 6:9] = po, c
    d = np.linalg.norm(x[:, 6:9].astype(np.float64) - x[:, 0:3].astype(np.float64), axis=1)  # (of the float32 points: what the kernel sees)
    x[:, 9] = d * np.exp(r.uniform(np.log(1e-4), np.log(0.99), n))
    w = (x[:, 6:9].astype(np.float64) - x[:, 0:3].astype(np.float64)) / d[:, None]
    nf = _hemisphere_about(w, r).astype(np.float32).astype(np.float64)
    x[:, 3:6] = nf / np.linalg.norm(nf, axis=1, keepdims=True)
    x[:, 10:12] = np.minimum(r.uniform(0, 1, (n, 2)).astype(np.float32), np.float32(1) - np.finfo(np.float32).eps)
    x[:, 12] = r.integers(1, 9, n)
    return x


# what an edge input is about: tests/test_sphere_light_host.py says what each kind must give
EDGE_KINDS = ("on_surface", "inside", "at_centre", "u_corners", "tiny")


def edge_inputs(n=4096, seed=91):
    """-> (x [n, 13] float32, kind [n] indices into EDGE_KINDS).  The domain's geometry with po moved ONTO the sphere (its float32 nearest:
    outside or not by rounding), INSIDE it, to its CENTRE; (u1, u2) from {0, 1/2, 1 - 2^-24}^2; and a sphere of r / d = 1e-6"""
    r = np.random.default_rng(seed)
    x = domain_inputs(n, seed)
    kind = r.integers(0, len(EDGE_KINDS), n)
    k = lambda name: kind == EDGE_KINDS.index(name)  # noqa: E731
    c, po = x[:, 6:9].astype(np.float64), x[:, 0:3].astype(np.float64)
    w = (po - c) / np.linalg.norm(po - c, axis=1, keepdims=True)
    m = k("on_surface")
    x[m, 0:3] = (c + w * x[:, 9:10].astype(np.float64))[m]
    m = k("inside")
    x[m, 0:3] = (c + w * x[:, 9:10].astype(np.float64) * r.uniform(0.0, 0.999, (n, 1)))[m]
    m = k("at_centre")
    x[m, 0:3] = x[m, 6:9]
    m = k("u_corners")
    corners = np.array([0.0, 0.5, 1.0 - 2.0 ** -24], np.float32)
    x[m, 10:12] = corners[r.integers(0, 3, (n, 2))][m]
    m = k("tiny")
    x[m, 9] = (np.linalg.norm(c - po, axis=1) * 1e-6)[m]
    return x, kind


def all_inputs():
    """the 69 632 rows the device is held to the host on"""
    return np.concatenate([domain_inputs(), edge_inputs()[0]])
