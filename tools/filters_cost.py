"""Frame time of the weighted pixel filters (the WIDE render kernels' `if (R.filter_table)` finish, a table weight per pixel
of the footprint into the fixed-point film) beside the box filter of the same radii and the default filter, on ONE scene in one process on
one GPU: scenes.random_mesh_scene at 100 000 triangles, 1024 x 1024, 64 spp, depth 8.  Prints one line per case -- the kernel times of
the measured frames (median, min, max), Msamples/s, the shader clock the GPU held (bench.py's ClockSampler) -- then the VGPRs and spills of the kernels from the code object's notes.

profiles/filters_vs_box.txt also holds the A-B that decided the form of the add (a build with lane-private destination slots against the
plain form that ships: the slots lost and were removed).

  python tools/filters_cost.py [--steps 3] [--warmup 1] [--only gaussian,"box 2x2"]"""
import argparse
import dataclasses
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from normals_cost import kernel_line  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--tris", type=int, default=100_000)
    ap.add_argument("--only", default="", help="comma-separated case names (default: all)")
    a = ap.parse_args()
    # (the kernels' names are demangled by a child process: before anything initialises the GPU)
    from pbrt_amd import _lib
    lines = [kernel_line(_lib.LIB_PATH, "render_kernel<false,false,false,0,3,true,false>"), kernel_line(_lib.LIB_PATH, "render_kernel<false,false,false,30,3,true,false>"),
             kernel_line(_lib.LIB_PATH, "render_kernel<false,false,false,30,3,false,false>")]
    import pbrt_amd
    from bench import ClockSampler
    from pbrt_amd import scenes
    mesh = scenes.random_mesh_scene(a.tris, a.res, a.res)

    def filtered(kind):
        return dataclasses.replace(mesh, pixel_filter=kind).normalized()
    cases = [
        ("gaussian", filtered("gaussian"), (2.0, 2.0)), ("box 2x2", mesh, (2.0, 2.0)), ("default box", mesh, (0.5, 0.5)),
        ("mitchell", filtered("mitchell"), (2.0, 2.0)), ("triangle", filtered("triangle"), (2.0, 2.0)), ("sinc 4x4", filtered("sinc"), (4.0, 4.0)), ("box 4x4", mesh, (4.0, 4.0)),
    ]
    only = [c for c in a.only.split(",") if c]
    cases = [c for c in cases if not only or c[0] in only]
    print(f"# {pbrt_amd.api.lib().pbrt_hip_version().decode()} build {pbrt_amd.build_id()} ({os.path.relpath(_lib.LIB_PATH)}); scenes.random_mesh_scene({a.tris}), {a.res} x {a.res}, "
          f"8 x 8 spp, stratified, path integrator, max_depth 8; {a.warmup} warm-up + {a.steps} measured frames per case, same process, same GPU")
    for name, sd, radii in cases:
        with pbrt_amd.Scene(sd) as sc:
            kw = dict(integrator=pbrt_amd.INTEGRATOR_PATH, max_depth=8, spp=(8, 8), filter_width=radii)
            ms = []
            for i in range(a.warmup):
                sc.render(seed=i, **kw)
            clocks = ClockSampler(0, period_s=0.05)
            clocks.start()
            for i in range(a.steps):
                ms.append(sc.render(seed=a.warmup + i, **kw)[1]["kernel_ms"])
            clock = clocks.stop()
            med = statistics.median(ms)
            ghz = f"{clock['ghz_median']:.2f} GHz median ({clock['ghz_min']:.2f} .. {clock['ghz_max']:.2f}, {clock['samples']} samples)" if clock else "not readable"
            print(f"{name:12s} radii {radii[0]:g} x {radii[1]:g}  kernel_ms {' '.join(f'{m:.3f}' for m in ms)}  median {med:9.3f} (min {min(ms):.3f}, max {max(ms):.3f})  "
                  f"{a.res * a.res * 64 / med / 1e3:9.1f} Msamples/s  shader clock {ghz}")
    for l in lines:
        print(l)


if __name__ == "__main__":
    main()
