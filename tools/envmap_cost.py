"""Throughput of scenes.envmap_scene under an environment map (render_kernel_env, the map importance-sampled with two binary
searches per light sample) beside the same scene under a CONSTANT sky of the map's mean radiance (render_kernel_x with GLS: the scene has
a glass sphere): 1024 x 1024, 256 spp, depth 8, the map procedural_sky(2048, 1024), both in one process on one GPU.  Prints one line per
scene -- median kernel time of the measured frames, Msamples/s, the shader clock the GPU held (bench.py's ClockSampler) -- and the VGPRs,
spills and waves per SIMD of the two kernels from the code object's notes (pbrt_amd/isa_id.py kernel_resources).

  python tools/envmap_cost.py [--steps 5] [--warmup 2] > profiles/envmap_vs_constant.txt"""
import argparse
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--map", type=int, nargs=2, default=(2048, 1024), metavar=("W", "H"))
    a = ap.parse_args()
    # (the kernels' names are demangled by a child process: before anything initialises the GPU)
    from pbrt_amd import _lib
    lines = [kernel_line(_lib.LIB_PATH, "render_kernel_env<true,0,false,false,false>"), kernel_line(_lib.LIB_PATH, "render_kernel_x<true,0,false,false,false,false,true>")]
    import pbrt_amd
    from bench import ClockSampler
    from pbrt_amd import scenes
    sky = scenes.procedural_sky(*a.map)
    kw = dict(max_depth=8, spp=(16, 16), integrator=pbrt_amd.INTEGRATOR_PATH, sampler="stratified")
    print(f"# {pbrt_amd.api.lib().pbrt_hip_version().decode()} build {pbrt_amd.build_id()}; scenes.envmap_scene {a.res} x {a.res}, 16 x 16 spp, max_depth 8, integrator 0, "
          f"stratified; map {a.map[0]} x {a.map[1]} (max / mean {sky.max() / sky.mean():.0f}); {a.warmup} warm-up + {a.steps} measured frames per scene, same process, same GPU")
    for name, constant in (("map", False), ("constant", True)):
        with pbrt_amd.Scene(scenes.envmap_scene(a.res, a.res, sky=sky, constant=constant)) as sc:
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
            print(f"{name:8s} kernel_ms median {med:9.3f} (min {min(ms):.3f}, max {max(ms):.3f})  {a.res * a.res * 256 / med / 1e3:9.1f} Msamples/s  shader clock {ghz}  "
                  f"device bytes {sc.info()['device_bytes']}")
    for l in lines:
        print(l)


if __name__ == "__main__":
    main()
