"""Throughput of scenes.glass_sphere_scene (the GLS instantiations of render_kernel_x) beside the same scene with the two
glass materials replaced by mirrors (render_kernel, the default path): 1024 x 1024, 256 spp, depth 16, both in one process on one GPU.
Prints one line per scene: median kernel time of the measured frames, Msamples/s, and the shader clock the GPU held during them (bench.py's
ClockSampler: the device's pp_dpm_sclk read from a host thread).

  python tools/glass_vs_mirror.py [--steps 5] [--warmup 2] > profiles/glass_vs_mirror.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=1024)
    a = ap.parse_args()
    import pbrt_amd
    from bench import ClockSampler
    from pbrt_amd import scenes
    print(f"# {pbrt_amd.api.lib().pbrt_hip_version().decode()} build {pbrt_amd.build_id()}; {a.res} x {a.res}, 16 x 16 spp, max_depth 16, integrator 0, "
          f"stratified; {a.warmup} warm-up + {a.steps} measured frames per scene, same process, same GPU")
    for name, glass in (("glass", True), ("mirror", False)):
        with pbrt_amd.Scene(scenes.glass_sphere_scene(a.res, a.res, glass=glass)) as sc:
            ms = []
            for i in range(a.warmup):
                sc.render(max_depth=16, spp=(16, 16), seed=i)
            clocks = ClockSampler(0, period_s=0.05)
            clocks.start()
            for i in range(a.steps):
                ms.append(sc.render(max_depth=16, spp=(16, 16), seed=a.warmup + i)[1]["kernel_ms"])
            clock = clocks.stop()
            med = statistics.median(ms)
            ghz = f"{clock['ghz_median']:.2f} GHz median ({clock['ghz_min']:.2f} .. {clock['ghz_max']:.2f}, {clock['samples']} samples)" if clock else "not readable"
            print(f"{name:6s} kernel_ms median {med:9.3f} (min {min(ms):.3f}, max {max(ms):.3f})  {a.res * a.res * 256 / med / 1e3:9.1f} Msamples/s  shader clock {ghz}")


if __name__ == "__main__":
    main()
