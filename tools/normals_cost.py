"""Frame time of scenes that carry shading normals (render_kernel_n, three more 16-byte loads and the interpolation per
shaded triangle hit, 4 waves per SIMD) beside the SAME scenes flat (render_kernel, 5 waves per SIMD): scenes.icosphere_scene(level 6:
81 920 triangles) at 1024 x 1024, 64 spp, direct lighting, and a 100 000-triangle scenes.random_mesh_scene at 1024 x 1024, 64 spp, depth 8,
whose every corner gets a synthetic normal -- the face normal turned by up to 20 degrees, from a seeded generator --, all in one process on
one GPU.  Prints one line per scene -- median kernel time of the measured frames, Msamples/s, the shader clock the GPU held (bench.py's
ClockSampler), the device bytes -- and the VGPRs, spills and waves per SIMD of the kernels from the code object's notes.

  python tools/normals_cost.py [--steps 5] [--warmup 2] > profiles/normals_vs_flat.txt"""
import argparse
import dataclasses
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_line(lib_path, want):
    """VGPRs / spills / scratch and the waves per SIMD they allow (512 VGPRs per SIMD lane in granules of 8) of the kernel named `want`"""
    from pbrt_amd import isa_id
    syms = sorted(isa_id.kernel_ids_by_symbol(lib_path))
    for sym, name in zip(syms, isa_id._demangle(syms)):
        if isa_id.normalise(name) == want:
            r = isa_id.kernel_resources(lib_path, sym)
            v = r["vgpr_count"] + (r["agpr_count"] or 0)
            return f"{want}: {v} VGPRs, {r['vgpr_spill_count']} spilled, {r['private_segment_fixed_size']} B scratch, {r['sgpr_count']} SGPRs -> up to {512 // ((v + 7) // 8 * 8)} waves per SIMD by registers"
    return f"{want}: not in the library"


def synthetic_normals(sd, seed=11, max_deg=20.0):
    """(n_tris, 9) float32: every corner's normal = the triangle's face normal turned by up to max_deg degrees about a random axis in the
    triangle's plane (a degenerate triangle: zeros, "none")"""
    rng = np.random.default_rng(seed)
    P = sd.P.astype(np.float64)[sd.idx.astype(np.int64)]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = np.cross(e1, e2)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    ok = ln[:, 0] > 0
    n = np.where(ok[:, None], n / np.where(ok[:, None], ln, 1.0), 0.0)
    t = np.where(ok[:, None], e1 / np.maximum(np.linalg.norm(e1, axis=1, keepdims=True), 1e-300), 0.0)
    b = np.cross(n, t)
    out = np.zeros((len(P), 3, 3))
    for v in range(3):
        th = np.radians(max_deg) * rng.random(len(P))[:, None]
        ph = 2 * np.pi * rng.random(len(P))[:, None]
        out[:, v] = np.cos(th) * n + np.sin(th) * (np.cos(ph) * t + np.sin(ph) * b)
    return out.reshape(-1, 9).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--tris", type=int, default=100_000)
    a = ap.parse_args()
    # (the kernels' names are demangled by a child process: before anything initialises the GPU)
    from pbrt_amd import _lib
    lines = [kernel_line(_lib.LIB_PATH, "render_kernel_n<false,0,false,false,false,false>"), kernel_line(_lib.LIB_PATH, "render_kernel_n<false,30,false,false,false,false>"),
             kernel_line(_lib.LIB_PATH, "render_kernel<false,false,false,0,3,false,false>"), kernel_line(_lib.LIB_PATH, "render_kernel<false,false,false,30,3,false,false>")]
    import pbrt_amd
    from bench import ClockSampler
    from pbrt_amd import scenes
    mesh = scenes.random_mesh_scene(a.tris, a.res, a.res)
    cases = [
        ("icosphere smooth", scenes.icosphere_scene(a.level, True, a.res, a.res), dict(integrator=pbrt_amd.INTEGRATOR_DIRECT, max_depth=5)),
        ("icosphere flat", scenes.icosphere_scene(a.level, False, a.res, a.res), dict(integrator=pbrt_amd.INTEGRATOR_DIRECT, max_depth=5)),
        ("mesh smooth", dataclasses.replace(mesh, tri_n=synthetic_normals(mesh)).normalized(), dict(integrator=pbrt_amd.INTEGRATOR_PATH, max_depth=8)),
        ("mesh flat", mesh, dict(integrator=pbrt_amd.INTEGRATOR_PATH, max_depth=8)),
    ]
    print(f"# {pbrt_amd.api.lib().pbrt_hip_version().decode()} build {pbrt_amd.build_id()}; {a.res} x {a.res}, 8 x 8 spp, stratified; scenes.icosphere_scene(level {a.level}) "
          f"under direct lighting, scenes.random_mesh_scene({a.tris}) at max_depth 8 with synthetic normals; {a.warmup} warm-up + {a.steps} measured frames per scene, same process, same GPU")
    for name, sd, kw in cases:
        with pbrt_amd.Scene(sd) as sc:
            ms = []
            for i in range(a.warmup):
                sc.render(seed=i, spp=(8, 8), **kw)
            clocks = ClockSampler(0, period_s=0.05)
            clocks.start()
            for i in range(a.steps):
                ms.append(sc.render(seed=a.warmup + i, spp=(8, 8), **kw)[1]["kernel_ms"])
            clock = clocks.stop()
            med = statistics.median(ms)
            ghz = f"{clock['ghz_median']:.2f} GHz median ({clock['ghz_min']:.2f} .. {clock['ghz_max']:.2f}, {clock['samples']} samples)" if clock else "not readable"
            print(f"{name:17s} kernel_ms median {med:9.3f} (min {min(ms):.3f}, max {max(ms):.3f})  {a.res * a.res * 64 / med / 1e3:9.1f} Msamples/s  shader clock {ghz}  "
                  f"device bytes {sc.info()['device_bytes']}")
    for l in lines:
        print(l)


if __name__ == "__main__":
    main()
