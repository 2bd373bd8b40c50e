"""Frame time of a matte scene by where its Kd comes from: a constant (the default kernel, render_kernel), a
checkerboard, and images -- 1024 x 1024 point-sampled, 1024 x 1024 bilinear, 4096 x 4096 bilinear (268 MB of texels: out of every cache) --
through the TEX instantiation of render_kernel_x.  The scene is the 100 000-triangle scenes.random_mesh_scene at 1024 x 1024, 64 spp, depth
8, every material matte, corner (u, v) drawn from a seeded generator; all cases in one process on one GPU.  Prints one line per case --
median kernel time of the measured frames, Msamples/s, the shader clock the GPU held (bench.py's ClockSampler), the device bytes -- and the
VGPRs, spills and waves per SIMD of the kernels from the code object's notes.

--cases constant checker runs on a tree without image textures as well: that is how the checkerboard frame of the commit before 3.20 is
taken on the same machine (what the type branch costs a scene that has no image), twice for the spread between two runs.

  python tools/textures_cost.py [--steps 5] [--warmup 2] [--cases ...] > profiles/textures_vs_checker.txt"""
import argparse
import dataclasses
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = ("constant", "checker", "image1k_point", "image1k_bilinear", "image4k_bilinear")


def kernel_line(lib_path, want):
    """VGPRs / spills / scratch and the waves per SIMD they allow (512 VGPRs per SIMD lane in granules of 8) of the kernel named `want`"""
    from pbrt_amd import isa_id
    syms = sorted(isa_id.kernel_ids_by_symbol(lib_path))
    for sym, name in zip(syms, isa_id._demangle(syms)):
        if isa_id.normalise(name) == want:
            r = isa_id.kernel_resources(lib_path, sym)
            v = r["vgpr_count"] + (r["agpr_count"] or 0)
            return f"{want}: {v} VGPRs, {r['vgpr_spill_count']} spilled, {r['private_segment_fixed_size']} B scratch, {r['sgpr_count']} SGPRs -> up to {512 // ((v + 7) // 8 * 8)} waves per SIMD by registers, machine-code id {isa_id.kernel_ids_by_symbol(lib_path)[sym]}"
    return f"{want}: not in the library"


def matte_mesh(n_tris, res):
    """scenes.random_mesh_scene with every mirror turned matte and random corner (u, v) in [0, 1]^2"""
    from pbrt_amd import MATTE, scenes
    sd = scenes.random_mesh_scene(n_tris, res, res)
    mats = sd.materials.copy()
    mats[:, 0] = MATTE
    uv = np.random.default_rng(21).random((len(sd.idx), 6)).astype(np.float32)
    return dataclasses.replace(sd, materials=mats, tri_uv=uv).normalized()


def textured(sd, row, images=None):
    """Kd of every material that does not emit from the one texture `row`"""
    plain = ~(sd.materials[:, 4:7] > 0).any(1)
    kw = dict(textures=np.array([row], np.float32), mat_tex=plain.astype(np.uint32))
    if images is not None:
        kw["images"] = images
    return dataclasses.replace(sd, **kw).normalized()


def case_scene(name, mesh):
    if name == "constant":
        return mesh
    if name == "checker":
        return textured(mesh, [0, .1, .2, .3, .8, .7, .6, 64.0, 64.0, 0.25, -0.5])
    from pbrt_amd import api
    size = 4096 if name.startswith("image4k") else 1024
    image = np.random.default_rng(size).random((size, size, 3), dtype=np.float32)
    return textured(mesh, api.image_texture_row(0, "repeat", "point" if name.endswith("point") else "bilinear", (4.0, 4.0, 0.25, -0.5)), [image])


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
    lines = [kernel_line(_lib.LIB_PATH, k) for k in ("render_kernel<false,false,false,0,3,false,false>", "render_kernel<false,false,false,30,3,false,false>",
                                                     "render_kernel_x<false,0,false,true,false,false,false>", "render_kernel_x<false,30,false,true,false,false,false>")]
    import pbrt_amd
    from bench import ClockSampler
    mesh = matte_mesh(a.tris, a.res)
    print(f"# {pbrt_amd.api.lib().pbrt_hip_version().decode()} build {pbrt_amd.build_id()}; scenes.random_mesh_scene({a.tris}), every material matte, {a.res} x {a.res}, "
          f"8 x 8 spp, stratified, path integrator, max_depth 8; {a.warmup} warm-up + {a.steps} measured frames per case, same process, same GPU")
    for name in a.cases:
        with pbrt_amd.Scene(case_scene(name, mesh)) as sc:
            kw = dict(integrator=pbrt_amd.INTEGRATOR_PATH, max_depth=8, spp=(8, 8))
            for i in range(a.warmup):
                sc.render(seed=i, **kw)
            clocks = ClockSampler(0, period_s=0.05)
            clocks.start()
            ms = [sc.render(seed=a.warmup + i, **kw)[1]["kernel_ms"] for i in range(a.steps)]
            clock = clocks.stop()
            med = statistics.median(ms)
            ghz = f"{clock['ghz_median']:.2f} GHz median ({clock['ghz_min']:.2f} .. {clock['ghz_max']:.2f}, {clock['samples']} samples)" if clock else "not readable"
            print(f"{name:17s} kernel_ms median {med:9.3f} (min {min(ms):.3f}, max {max(ms):.3f})  {a.res * a.res * 64 / med / 1e3:9.1f} Msamples/s  shader clock {ghz}  "
                  f"device bytes {sc.info()['device_bytes']}")
    for l in lines:
        print(l)


if __name__ == "__main__":
    main()
