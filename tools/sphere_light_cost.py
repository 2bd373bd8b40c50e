"""Frame time of a scene lit by a sphere lamp against the same scene lit by an emissive quad of the same area at the same place (DESIGN.md
3.25): scenes.random_mesh_scene at 100 000 triangles, 1024 x 1024, 64 spp, depth 8, its ceiling emitter dark; `quad` = a square emitter
facing down (two emissive triangles in the light table), the scene forced through the GLS instantiations of render_kernel_x by ONE unused
glass material, `lamp` = a sphere of the same area at the same centre with a sphere light that names it (which takes the GLS instantiations
by itself, and the ones with spheres).  With them scenes.glass_sphere_scene, scenes.plastic_scene and scenes.spot_scene at the same size:
scenes that ran the GLS kernels before pay for whatever the sphere light's branches cost them.  Prints one line per case -- median kernel
time of the measured frames, Msamples/s -- and the VGPRs, spills and waves per SIMD of the kernels from the code object's notes.

--tree DIR imports pbrt_amd from another checkout (the parent commit's own tree with its own library) in the same job, for the frames of
the commit before 3.25; that tree has no sphere light, so only --cases glass plastic spot_scene run there.

  python tools/sphere_light_cost.py [--steps 5] [--warmup 2] [--cases ...] [--tree DIR] > profiles/sphere_light_vs_quad.txt"""
import argparse
import dataclasses
import math
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("quad", "lamp", "glass", "plastic", "spot_scene")
CENTRE, SIDE, LE = (0.0, 0.0, 1.5), 0.5, (20.0, 20.0, 20.0)
RADIUS = SIDE / math.sqrt(4.0 * math.pi)  # 4 pi r^2 = SIDE^2


def case_scene(name, n_tris, res):
    from pbrt_amd import GLASS, MATTE, scenes
    if name in ("glass", "plastic", "spot_scene"):
        return {"glass": scenes.glass_sphere_scene, "plastic": scenes.plastic_scene, "spot_scene": scenes.spot_scene}[name](res, res)
    sd = scenes.random_mesh_scene(n_tris, res, res)
    mats = sd.materials.copy()
    mats[:, 4:7] = 0  # (the ceiling emitter dark: the one light is the quad or the lamp)
    emitter = len(mats)
    mats = np.concatenate([mats, [[MATTE, 0, 0, 0, *LE]]]).astype(np.float32)
    kw = {}
    if name == "quad":
        h, (cx, cy, cz) = SIDE / 2, CENTRE
        base = len(sd.P)
        quad = np.array([[cx - h, cy - h, cz], [cx - h, cy + h, cz], [cx + h, cy + h, cz], [cx + h, cy - h, cz]], np.float32)  # normal -z
        kw = dict(P=np.concatenate([sd.P, quad]), idx=np.concatenate([sd.idx, np.array([[base, base + 1, base + 2], [base, base + 2, base + 3]], np.uint32)]),
                  mat_id=np.concatenate([sd.mat_id, np.array([emitter, emitter], np.uint16)]))
        mats = np.concatenate([mats, [[GLASS, 1, 1, 1, 1, 1, 1]]]).astype(np.float32)  # (used by nothing: the scene's flag is all it sets)
    else:
        from pbrt_amd import LIGHT_SPHERE
        kw = dict(spheres=np.array([[*CENTRE, RADIUS, emitter]], np.float32), lights=np.array([[LIGHT_SPHERE, 0, 0, 0, *LE]], np.float32))
    return dataclasses.replace(sd, materials=mats, mat_tex=np.zeros(0, np.uint32), **kw).normalized()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--tris", type=int, default=100_000)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=CASES)
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(1, os.path.join(os.path.abspath(a.tree), "tools"))
    from textures_cost import kernel_line
    # (the kernels' names are demangled by a child process: before anything initialises the GPU)
    from pbrt_amd import _lib
    lines = [kernel_line(_lib.LIB_PATH, k) for k in ("render_kernel<false,false,false,30,3,false,false>", "render_kernel_x<false,30,false,false,false,false,true>",
                                                     "render_kernel_x<true,30,false,false,false,false,true>", "render_kernel_x<true,30,true,false,true,false,true>")]
    import pbrt_amd
    print(f"# {pbrt_amd.api.lib().pbrt_hip_version().decode()} build {pbrt_amd.build_id()}; {a.res} x {a.res}, 8 x 8 spp, stratified, path integrator, max_depth 8; "
          f"quad / lamp: scenes.random_mesh_scene({a.tris}), emitter dark, under a {SIDE} x {SIDE} emissive quad / a sphere lamp of radius {RADIUS:.4f} (the same area) at "
          f"{CENTRE}; glass / plastic / spot_scene: scenes.glass_sphere_scene / plastic_scene / spot_scene; {a.warmup} warm-up + {a.steps} measured frames per case, same process, same GPU")
    for name in a.cases:
        with pbrt_amd.Scene(case_scene(name, a.tris, a.res)) as sc:
            kw = dict(integrator=pbrt_amd.INTEGRATOR_PATH, max_depth=8, spp=(8, 8))
            for i in range(a.warmup):
                film = sc.render(seed=i, **kw)[0]
            ms = [sc.render(seed=a.warmup + i, **kw)[1]["kernel_ms"] for i in range(a.steps)]
            med = statistics.median(ms)
            print(f"{name:10s} kernel_ms median {med:9.3f} (min {min(ms):.3f}, max {max(ms):.3f})  {a.res * a.res * 64 / med / 1e3:9.1f} Msamples/s  "
                  f"mean Y {float(film[..., 1].sum() / film[..., 3].sum()):.4f}", flush=True)
    for l in lines:
        print(l)


if __name__ == "__main__":
    main()
