"""Frame time of a scene by the kind of its one light, in the manner of tools/spot_cost.py: (a) a point light forced through
the GLS instantiations of render_kernel_x by ONE unused glass material -- the kernels that carry the mapped lights' branch since 3.23 --,
(b) that point light replaced by a goniometric light whose map is one point-sampled texel of ones (the same film, bit for bit), and (c) by a
projector that looks straight down through a bilinear 1024 x 1024 slide.  (b) - (a) is the branch and the lookup of one texel; (c) - (b) is
what a real image costs.  The scene is the 100 000-triangle scenes.random_mesh_scene at 1024 x 1024, 64 spp, depth 8, its ceiling emitter
dark; all cases in one process on one GPU.  With them scenes.glass_sphere_scene, scenes.plastic_scene and scenes.spot_scene at the same size:
scenes that ran the GLS kernels before pay for the added compare of the light's type word and for the registers the branch takes.  Prints
one line per case -- median kernel time of the measured frames, Msamples/s, the shader clock the GPU held (bench.py's ClockSampler) -- and the
VGPRs, spills and waves per SIMD of the kernels from the code object's notes.

PBRT_HIP_LIB_DIR=<the parent commit's library> ... --cases glass plastic spot takes the frames of the commit before 3.23 in the same job,
twice for the spread between two runs (that library lacks the hooks added since; they are left unbound).

  python tools/light_map_cost.py [--steps 5] [--warmup 2] [--cases ...] > profiles/light_map_vs_point.txt"""
import argparse
import ctypes
import dataclasses
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from textures_cost import kernel_line  # noqa: E402

CASES = ("point_gls", "gonio_ones", "projector", "glass", "plastic", "spot")
LIGHT_P, LIGHT_I = (0.0, 0.0, 1.9), (12.0, 12.0, 12.0)
DOWN = [[1, 0, 0], [0, -1, 0], [0, 0, -1]]  # world_to_light of a projector that looks along the world's -z


def big_slide(n=1024):
    """a smooth n x n image in [0.05, 1]: every lookup blends four different texels"""
    v, u = (np.mgrid[0:n, 0:n].astype(np.float32) + 0.5) / n
    return np.stack([0.525 + 0.475 * np.sin(40 * u) * np.cos(28 * v), 0.525 + 0.475 * np.cos(33 * (u + v)), 0.525 + 0.475 * np.sin(25 * (u - 2 * v))], -1).astype(np.float32)


def case_scene(name, n_tris, res):
    from pbrt_amd import GLASS, LIGHT_POINT, api, scenes
    if name in ("glass", "plastic", "spot"):
        return {"glass": scenes.glass_sphere_scene, "plastic": scenes.plastic_scene, "spot": scenes.spot_scene}[name](res, res)
    sd = scenes.random_mesh_scene(n_tris, res, res)
    mats = sd.materials.copy()
    mats[:, 4:7] = 0  # (the ceiling emitter dark: the one light is the explicit one)
    kw = dict(lights=np.array([[LIGHT_POINT, *LIGHT_P, *LIGHT_I]], np.float32))
    if name == "point_gls":  # (one more material, used by nothing: the scene's flag is all it sets)
        mats = np.concatenate([mats, [[GLASS, 1, 1, 1, 1, 1, 1]]]).astype(np.float32)
    if name == "gonio_ones":
        light, row = api.goniometric_light(LIGHT_P, 1, LIGHT_I)
        kw = dict(lights=np.array([light], np.float32), light_maps=np.array([row], np.float32), images=[np.ones((1, 1, 3), np.float32)],
                  textures=np.array([api.image_texture_row(0, "repeat", "point")], np.float32))
    if name == "projector":
        light, row = api.projection_light(LIGHT_P, 1, LIGHT_I, 120.0, 1.0, DOWN)
        kw = dict(lights=np.array([light], np.float32), light_maps=np.array([row], np.float32), images=[big_slide()],
                  textures=np.array([api.image_texture_row(0, "clamp", "bilinear")], np.float32))
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
          f"point_gls / gonio_ones / projector: scenes.random_mesh_scene({a.tris}) under one light; glass: scenes.glass_sphere_scene; plastic: scenes.plastic_scene; "
          f"spot: scenes.spot_scene; {a.warmup} warm-up + {a.steps} measured frames per case, same process, same GPU")
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
    if all(k in films for k in ("point_gls", "gonio_ones")):
        same = np.array_equal(films["point_gls"].view(np.uint32), films["gonio_ones"].view(np.uint32))
        print(f"# the films of point_gls and gonio_ones are {'equal bit for bit' if same else 'NOT EQUAL'}")
    for l in lines:
        print(l)


if __name__ == "__main__":
    main()
