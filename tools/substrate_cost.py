"""Frame time of a scene by its materials' kind, modelled on tools/plastic_cost.py: all matte forced through the GLS
instantiations of render_kernel_x by ONE unused glass material -- the kernels that carry the plastic and, since 3.24, the substrate branch --,
all plastic (Kd the matte one's, Ks 0.25, roughness 0.1) and all substrate (Kd the matte one's, Ks 0.25, both roughnesses 0.1).  The scene is
the 100 000-triangle scenes.random_mesh_scene at 1024 x 1024, 64 spp, depth 8; all cases in one process on one GPU.  With them the scenes
that already ran these kernels, at the same size: scenes.glass_sphere_scene, plastic_scene and spot_scene.  Prints one line per case --
median kernel time of the measured frames, Msamples/s, the shader clock the GPU held (bench.py's ClockSampler) -- and the VGPRs, spills and
waves per SIMD of the kernels from the code object's notes.

--cases glass plastic_scene spot runs on a tree without the substrate material as well: that is how the frames of the commit before 3.24
are taken in the same job, twice each side for the spread between two runs.

  python tools/substrate_cost.py [--steps 5] [--warmup 2] [--cases ...] > profiles/substrate_vs_plastic.txt"""
import argparse
import dataclasses
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from textures_cost import kernel_line  # noqa: E402

CASES = ("matte_gls", "plastic", "substrate", "glass", "plastic_scene", "spot")
NEIGHBOURS = {"glass": "glass_sphere_scene", "plastic_scene": "plastic_scene", "spot": "spot_scene"}


def case_scene(name, n_tris, res):
    import pbrt_amd
    from pbrt_amd import GLASS, MATTE, scenes
    if name in NEIGHBOURS:
        return getattr(scenes, NEIGHBOURS[name])(res, res)
    sd = scenes.random_mesh_scene(n_tris, res, res)
    mats = sd.materials.copy()
    mats[:, 0] = MATTE
    eta = np.zeros(0, np.float32)
    if name == "matte_gls":  # (one more material, used by nothing: the scene's flag is all it sets)
        mats = np.concatenate([mats, [[GLASS, 1, 1, 1, 1, 1, 1]]]).astype(np.float32)
    else:
        plain = ~(mats[:, 4:7] > 0).any(1)
        mats[plain, 0] = pbrt_amd.PLASTIC if name == "plastic" else pbrt_amd.SUBSTRATE
        mats[plain, 4:7] = 0.25
        eta = np.full(len(mats), pbrt_amd.api.roughness_to_alpha(0.1), np.float32)
    return dataclasses.replace(sd, materials=mats, mat_eta=eta, mat_tex=np.zeros(0, np.uint32)).normalized()


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
    import pbrt_amd
    from bench import ClockSampler
    print(f"# {pbrt_amd.api.lib().pbrt_hip_version().decode()} build {pbrt_amd.build_id()}; {a.res} x {a.res}, 8 x 8 spp, stratified, path integrator, max_depth 8; "
          f"matte_gls / plastic / substrate: scenes.random_mesh_scene({a.tris}); glass / plastic_scene / spot: scenes.{{glass_sphere,plastic,spot}}_scene; "
          f"{a.warmup} warm-up + {a.steps} measured frames per case, same process, same GPU")
    for name in a.cases:
        with pbrt_amd.Scene(case_scene(name, a.tris, a.res)) as sc:
            kw = dict(integrator=pbrt_amd.INTEGRATOR_PATH, max_depth=8, spp=(8, 8))
            for i in range(a.warmup):
                sc.render(seed=i, **kw)
            clocks = ClockSampler(0, period_s=0.05)
            clocks.start()
            ms = [sc.render(seed=a.warmup + i, **kw)[1]["kernel_ms"] for i in range(a.steps)]
            clock = clocks.stop()
            med = statistics.median(ms)
            ghz = f"{clock['ghz_median']:.2f} GHz median ({clock['ghz_min']:.2f} .. {clock['ghz_max']:.2f}, {clock['samples']} samples)" if clock else "not readable"
            print(f"{name:14s} kernel_ms median {med:9.3f} (min {min(ms):.3f}, max {max(ms):.3f})  {a.res * a.res * 64 / med / 1e3:9.1f} Msamples/s  shader clock {ghz}")
    for l in lines:
        print(l)


if __name__ == "__main__":
    main()
