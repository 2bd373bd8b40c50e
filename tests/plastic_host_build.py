"""pbrt_amd/csrc/plastic_bsdf.hpp compiled FOR THE HOST into a stand-alone program (plain g++ with -ffp-contract=off, nothing of HIP): the
header's text, and plastic_eval.inc around it, exactly as kernels_blocks.hip's plastic_eval_kernel compiles them for the device.  The
program's <hip/hip_runtime.h> is a stub of a few lines in which __device__ and __forceinline__ mean nothing and float4 is four floats.
Shared by tests/test_plastic_host.py (the header against float64) and tests/test_plastic_gpu.py (the device against this program, bit for
bit), with the inputs both use."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IN, N_OUT = 18, 10  # include/pbrt_hip_debug.h PBRT_HIP_PLASTIC_EVAL_IN / _OUT

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
#include "plastic_bsdf.hpp"
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
#include "plastic_eval.inc"
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
    src, exe = os.path.join(tmp_path, "plastic_host.cpp"), os.path.join(tmp_path, "plastic_host")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes", "-I", os.path.join(tmp_path, "stub"), "-I",
                    os.path.join(ROOT, "pbrt_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def run(exe, x, tmp_path):
    """x (n, 18) float32 -> (n, 10) float32"""
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
    v2, v3 = _frame(n)
    st = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    w = v2 * (st * np.cos(phi))[:, None] + v3 * (st * np.sin(phi))[:, None] + n * cos_t[:, None]
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def domain_inputs(n=1 << 16, seed=321):
    """DESIGN.md 3.21's measured domain: unit nf anywhere, wo and wi with cos_o, cos_i in [0.05, 1], (u1, u2) in [0, 1), Kd, Ks in [0, 1],
    alpha in [0.05, 1] -- float32 rows of 18"""
    r = np.random.default_rng(seed)
    nf = r.normal(size=(n, 3))
    nf /= np.linalg.norm(nf, axis=1, keepdims=True)
    wo = _about(nf, r.uniform(0.05, 1.0, n), r.uniform(0, 2 * np.pi, n))
    wi = _about(nf, r.uniform(0.05, 1.0, n), r.uniform(0, 2 * np.pi, n))
    u = np.minimum(r.uniform(0, 1, (n, 2)).astype(np.float32), np.float32(1.0 - 2.0 ** -23))
    x = np.concatenate([nf, wo, wi, u, r.uniform(0, 1, (n, 3)), r.uniform(0, 1, (n, 3)), r.uniform(0.05, 1.0, (n, 1))], 1).astype(np.float32)
    # (the vectors unit again AS FLOAT32: what the kernel sees)
    for k in (0, 3, 6):
        v = x[:, k:k + 3].astype(np.float64)
        x[:, k:k + 3] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return x


def edge_inputs(n=4096, seed=654):
    """the ends: u1 at 0, 1/2 - 1 ulp, 1/2, 1/2 + 1 ulp and 1 - eps, alpha at 1e-3 and 1, grazing wo (cos_o down to 1e-4), wi anywhere --
    below the surface included --, axis-aligned normals"""
    r = np.random.default_rng(seed)
    x = domain_inputs(n, seed)
    half = np.float32(0.5)
    ends = np.array([0.0, np.nextafter(half, np.float32(0)), half, np.nextafter(half, np.float32(1)), 1.0 - 2.0 ** -23], np.float32)
    x[:, 9] = ends[r.integers(0, len(ends), n)]
    x[:, 17] = np.where(r.uniform(size=n) < 0.5, np.float32(1e-3), np.float32(1.0))
    x[: n // 4, 17] = r.uniform(1e-3, 1.0, n // 4).astype(np.float32)
    nf = x[:, 0:3].astype(np.float64)
    axis = r.integers(0, 3, n)
    nf[n // 2:] = np.eye(3)[axis[n // 2:]] * np.where(r.uniform(size=(n - n // 2, 1)) < 0.5, -1.0, 1.0)
    wo = _about(nf, 10.0 ** r.uniform(-4, 0, n), r.uniform(0, 2 * np.pi, n))
    wi = _about(nf, r.uniform(-0.2, 1.0, n), r.uniform(0, 2 * np.pi, n))
    x[:, 0:3], x[:, 3:6], x[:, 6:9] = nf.astype(np.float32), wo.astype(np.float32), wi.astype(np.float32)
    return x
