"""Frame time of a scene by the kind of its one light: a point light through the default kernel (render_kernel), the same
scene forced through the GLS instantiations of render_kernel_x by ONE unused glass material -- the kernels that carry the spot branch since
3.22 --, and that point light replaced by a spot light whose cone is the whole sphere (the same film, bit for bit).  (c) - (b) is the
branch; (b) - (a) is the known occupancy price of the GLS kernels, which a scene with a spot light pays.  The scene is the 100 000-triangle
scenes.random_mesh_scene at 1024 x 1024, 64 spp, depth 8, its ceiling emitter dark; all cases in one process on one GPU.  With them
scenes.glass_sphere_scene and scenes.plastic_scene at the same size: scenes that ran the GLS kernels before pay for the added compare of the
light's type word.  Prints one line per case -- median kernel time of the measured frames, Msamples/s, the shader clock the GPU held
(bench.py's ClockSampler) -- and the VGPRs, spills and waves per SIMD of the kernels from the code object's notes.

PBRT_HIP_LIB_DIR=<the parent commit's library> ... --cases glass plastic takes the frames of the commit before 3.22 in the same job, twice
for the spread between two runs (that library lacks the hooks added since; they are left unbound).

  python tools/spot_cost.py [--steps 5] [--warmup 2] [--cases ...] > profiles/spot_vs_point.txt"""
import argparse
import ctypes
import dataclasses
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from textures_cost import kernel_line  # noqa: E402

CASES = ("point", "point_gls", "spot", "glass", "plastic")
LIGHT_P, LIGHT_I = (0.0, 0.0, 1.9), (12.0, 12.0, 12.0)


def case_scene(name, n_tris, res):
    from pbrt_amd import GLASS, LIGHT_POINT, scenes
    if name == "glass":
        return scenes.glass_sphere_scene(res, res)
    if name == "plastic":
        return scenes.plastic_scene(res, res)
    sd = scenes.random_mesh_scene(n_tris, res, res)
    mats = sd.materials.copy()
    mats[:, 4:7] = 0  # (the ceiling emitter dark: the one light is the explicit one)
    kw = dict(lights=np.array([[LIGHT_POINT, *LIGHT_P, *LIGHT_I]], np.float32))
    if name == "point_gls":  # (one more material, used by nothing: the scene's flag is all it sets)
        mats = np.concatenate([mats, [[GLASS, 1, 1, 1, 1, 1, 1]]]).astype(np.float32)
    if name == "spot":
        from pbrt_amd import LIGHT_SPOT
        kw = dict(lights=np.array([[LIGHT_SPOT, *LIGHT_P, *LIGHT_I]], np.float32), spot_cones=np.array([[0, 0, -1, -1, -1]], np.float32))
    return dataclasses.replace(sd, materials=mats, mat_tex=np.zeros(0, np.uint32), **kw).normalized()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--tris", type=int, default=100_000)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=CASES)
    a = ap.parse_args()
    # (the kernels' names are demangled by a child process: before anything initialises the GPU)
    from pbrt_amd import _lib
    lines = [kernel_line(_lib.LIB_PATH, k) for k in ("render_kernel<false,false,false,30,3,false,false>", "render_kernel_x<false,30,false,false,false,false,true>",
                                                     "render_kernel_x<true,30,false,false,false,false,true>", "render_kernel_x<true,30,true,false,true,false,true>")]
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SYMBOLS if not hasattr(probe, n)]:  # (an older library: the hooks it lacks stay unbound)
        del _lib.SYMBOLS[name]
    import pbrt_amd
    from bench import ClockSampler
    print(f"# {pbrt_amd.api.lib().pbrt_hip_version().decode()} build {pbrt_amd.build_id()}; {a.res} x {a.res}, 8 x 8 spp, stratified, path integrator, max_depth 8; "
          f"point / point_gls / spot: scenes.random_mesh_scene({a.tris}) under one light; glass: scenes.glass_sphere_scene; plastic: scenes.plastic_scene; "
          f"{a.warmup} warm-up + {a.steps} measured frames per case, same process, same GPU")
    films = {}
    for name in a.cases:
        with pbrt_amd.Scene(case_scene(name, a.tris, a.res)) as sc:
            kw = dict(integrator=pbrt_amd.INTEGRATOR_PATH, max_depth=8, spp=(8, 8))
            for i in range(a.warmup):
                films[name] = sc.render(seed=i, **kw)[0]
            clocks = ClockSampler(0, period_s=0.05)
            clocks.start()
            ms = [sc.render(seed=a.warmup + i, **kw)[1]["kernel_ms"] for i in range(a.steps)]
            clock = clocks.stop()
            med = statistics.median(ms)
            ghz = f"{clock['ghz_median']:.2f} GHz median ({clock['ghz_min']:.2f} .. {clock['ghz_max']:.2f}, {clock['samples']} samples)" if clock else "not readable"
            print(f"{name:10s} kernel_ms median {med:9.3f} (min {min(ms):.3f}, max {max(ms):.3f})  {a.res * a.res * 64 / med / 1e3:9.1f} Msamples/s  shader clock {ghz}")
    if all(k in films for k in ("point", "point_gls", "spot")):
        same = np.array_equal(films["point"].view(np.uint32), films["spot"].view(np.uint32)) and np.array_equal(films["point"].view(np.uint32), films["point_gls"].view(np.uint32))
        print(f"# the three films of the mesh scene are {'equal bit for bit' if same else 'NOT EQUAL'}")
    for l in lines:
        print(l)


if __name__ == "__main__":
    main()
