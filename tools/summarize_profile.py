#!/usr/bin/env python3
"""Condenses what tools/measure_round.sh left under gpurun_out/ into the small files kept under profiles/.

  python tools/summarize_profile.py <round-tag> <workload> [<workload> ...]

Per workload: <tag>_<wl>_kernel_stats.csv (rocprofv3 --kernel-trace --stats of bench.py), <tag>_<wl>_pmc_counters.txt
(the PMC passes of the low-spp probe), <tag>_<wl>_summary.json = pmc_<wl>.json (kernel time per frame, FETCH_SIZE /
WRITE_SIZE per frame from the two dedicated passes, and the VALU-issue model of tools/valu_model.py: what bench.py's
`roofline` reads), and <tag>_<wl>_bench.json for every bench line found.
"""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "render_kernel<false, false"
FRAMES_TRACE, FRAMES_PMC = 3, 1  # --steps 2 --warmup 1 / --steps 1 --warmup 0


def one(pattern):
    f = glob.glob(pattern, recursive=True)
    return max(f, key=os.path.getmtime) if f else None  # (a re-run of one workload leaves the older files beside the new ones)


def latest_calibration(P, G):
    """{ratio_112MB, ratio_1536MB, source} from the newest fetch_size_calibration.txt (gpurun_out/*/ of this job, else the committed one)"""
    import re
    fresh = sorted(glob.glob(os.path.join(G, "*", "fetch_size_calibration.txt")), key=os.path.getmtime)[::-1]
    for f in fresh + sorted(glob.glob(os.path.join(P, "*fetch_size_calibration.txt")))[::-1]:
        for line in open(f):
            m = re.match(r"FETCH_SIZE_BYTES_PER_KNOWN_BYTE 112MB ([0-9.]+) 1536MB ([0-9.]+)", line)
            if m:
                return {"ratio_112MB": float(m.group(1)), "ratio_1536MB": float(m.group(2)), "source": os.path.relpath(f, ROOT)}
    return None


def main():
    tag = sys.argv[1]
    G, P = os.path.join(ROOT, "gpurun_out"), os.path.join(ROOT, "profiles")
    os.makedirs(P, exist_ok=True)
    for wl in sys.argv[2:]:
        summary = {"workload": wl, "round": tag}
        stats = one(os.path.join(G, f"prof_{tag}_{wl}_trace", "**", "*kernel_stats.csv"))
        if stats:
            rows = list(csv.DictReader(open(stats)))
            with open(os.path.join(P, f"{tag}_{wl}_kernel_stats.csv"), "w", newline="") as f:
                w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
                w.writeheader()
                for r in rows:
                    r["Name"] = r["Name"][:160]
                    w.writerow(r)
            k = [r for r in rows if KERNEL in r["Name"]][0]
            calls = int(k["Calls"])
            summary.update({"kernel": k["Name"], "calls": calls, "frames": FRAMES_TRACE, "launches_per_frame": calls / FRAMES_TRACE,
                            "avg_ms": float(k["TotalDurationNs"]) / 1e6 / FRAMES_TRACE, "min_ms": float(k["MinNs"]) / 1e6, "max_ms": float(k["MaxNs"]) / 1e6,
                            "share_of_gpu_time_pct": float(k["Percentage"]),
                            "source": f"rocprofv3 --kernel-trace --stats -- python3 bench.py --workload {wl} --steps 2 --warmup 1 --no-cpu-baseline; avg_ms = per frame"})
        for name, sub in (("FETCH_SIZE", "fetch"), ("WRITE_SIZE", "write")):
            f = one(os.path.join(G, f"prof_{tag}_{wl}_{sub}", "**", "*counter_collection.csv"))
            if not f:
                continue
            cr = list(csv.DictReader(open(f)))
            vals = [float(r["Counter_Value"]) for r in cr if KERNEL in r["Kernel_Name"] and r["Counter_Name"] == name]
            summary[name + "_KB_per_launch"] = sum(vals) / FRAMES_PMC
            kr = [r for r in cr if KERNEL in r["Kernel_Name"]][0]
            # (rocprofv3's VGPR_Count / LDS_Block_Size columns are an allocation granule field and the STATIC LDS: kept under their own
            # names; "vgpr" / "lds_bytes" below come from the code object's notes and the launch's stack plan -- VERDICT r05 weak 2c)
            summary.update({"rocprof_vgpr_field": int(kr["VGPR_Count"]), "rocprof_sgpr_field": int(kr["SGPR_Count"]), "rocprof_lds_block_size": int(kr["LDS_Block_Size"]),
                            "grid": int(kr["Grid_Size"]), "workgroup": int(kr["Workgroup_Size"])})
        if "FETCH_SIZE_KB_per_launch" in summary and "WRITE_SIZE_KB_per_launch" in summary:
            # MI355X_MICROARCH.md "HBM": FETCH_SIZE = TCC_EA0_RDREQ x 64 B in KB, L2-miss requests including Infinity-Cache hits; it reads
            # exactly half of the bytes of a WIDE COALESCED 16 B/lane stream; other access shapes (ours: divergent 16-B loads) are
            # uncalibrated, so both the raw and the doubled figure are kept.
            summary["traffic_bytes_raw"] = (summary["FETCH_SIZE_KB_per_launch"] + summary["WRITE_SIZE_KB_per_launch"]) * 1024
            summary["traffic_bytes_fetch_doubled"] = (2 * summary["FETCH_SIZE_KB_per_launch"] + summary["WRITE_SIZE_KB_per_launch"]) * 1024
            summary["pmc_source"] = ("separate passes: rocprofv3 --pmc FETCH_SIZE --kernel-trace / --pmc WRITE_SIZE --kernel-trace -- python3 bench.py "
                                     f"--workload {wl} --steps 1 --warmup 0 --no-cpu-baseline --no-counters")
        pmc = os.path.join(G, f"pmc_{tag}_{wl}", "summary.txt")
        if os.path.exists(pmc):
            shutil.copy(pmc, os.path.join(P, f"{tag}_{wl}_pmc_counters.txt"))
            model = json.loads(subprocess.run([sys.executable, os.path.join(ROOT, "tools", "valu_model.py"), pmc], capture_output=True, text=True, check=True).stdout)
            summary.update(model)
            summary["valu_source"] = f"tools/pmc_passes.sh on tools/pmc_probe.py {wl} (low-spp frame) -> profiles/{tag}_{wl}_pmc_counters.txt -> tools/valu_model.py"
            # the TREE the per-ray counters belong to (pmc_probe.py's own walk counters): bench.py withholds the profile when the live
            # production walk does other work per ray (a builder edit leaves the render kernel's machine code alone)
            c = dict((k, float(v)) for k, v in (l.split() for l in open(pmc)))
            if "TREE_FETCHES_PER_RAY" in c:
                summary["tree"] = {"kernel_fetches_per_ray": c["TREE_FETCHES_PER_RAY"], "kernel_tris_per_ray": c["TREE_TRIS_PER_RAY"], "quad_nodes": int(c["TREE_QUAD_NODES"]),
                                   "quad_stack_need": int(c["TREE_STACK_NEED"]), "spp": int(c["PROBE_SPP"])}
                summary["lds_dynamic_bytes"] = int(c["LAUNCH_LDS_ROWS"]) * 256
                summary["waves_per_cu"] = int(c["LAUNCH_WAVES_PER_CU"])
        # the library the counters were taken on (bench.py withholds figures priced with another build's profile)
        for line_file in (os.path.join(G, f"prof_{tag}_{wl}_trace.json"), os.path.join(G, f"bench_{wl}_{tag}.json")):
            try:
                cfg = json.load(open(line_file))["config"]
                summary["build_id"] = cfg["library_build_id"]
                # the tree the per-ray counters belong to (tools/measure_round.sh: PROBE_BUILDER = bench.py's default builder)
                summary["builder"] = cfg.get("accelerator", {}).get("builder", "gpu")
                break
            except (OSError, ValueError, KeyError):
                continue
        # ... and, what the validity of the profile is decided by: the machine code of the kernel the counters belong to
        # (pbrt_amd/isa_id.py; computed from the library beside this script -- on the GPU box the one that was measured)
        try:
            sys.path.insert(0, ROOT)
            from pbrt_amd import build, isa_id
            if summary.get("kernel"):
                summary["kernel_isa_id"] = isa_id.kernel_id(build.LIB_PATH, summary["kernel"])
                summary["compiler"] = build.compiler_version().splitlines()[0]
                # the mangled symbol: bench.py looks the kernel up by it (no demangler, so no child process from a GPU-initialised process)
                summary["kernel_symbol"] = isa_id.kernel_symbol(build.LIB_PATH, summary["kernel"])
                res = isa_id.kernel_resources(build.LIB_PATH, summary["kernel_symbol"]) if summary["kernel_symbol"] else None
                if res:  # what the compiler allocated (code-object notes) + the launch's dynamic LDS (the walk's stack)
                    summary.update({"vgpr": res["vgpr_count"], "sgpr": res["sgpr_count"], "vgpr_spill": res["vgpr_spill_count"], "scratch_bytes": res["private_segment_fixed_size"],
                                    "lds_bytes": (res["group_segment_fixed_size"] or 0) + summary.get("lds_dynamic_bytes", 0),
                                    "resources_source": "code-object notes (NT_AMDGPU_METADATA) + the launch's dynamic LDS (pbrt_hip_render_stack_layout: stack rows x 256 B + path-record bytes)"})
        except Exception as e:  # noqa: BLE001
            summary["kernel_isa_id_error"] = repr(e)[:200]
        # FETCH_SIZE calibrated for this access shape (tools/fetch_size_calibration.sh): known bytes per counted byte of
        # 64-byte records gathered at random, from the table that is in the workload's regime (in / past the Infinity Cache)
        cal = latest_calibration(P, G)
        if cal and cal["source"].startswith("gpurun_out"):  # this job's own calibration: kept under profiles/ beside what it calibrates
            kept = os.path.join(P, f"{tag}_fetch_size_calibration.txt")
            shutil.copy(os.path.join(ROOT, cal["source"]), kept)
            cal["source"] = os.path.relpath(kept, ROOT)
        if cal and "FETCH_SIZE_KB_per_launch" in summary:
            ratio = cal["ratio_1536MB"] if wl == "big" else cal["ratio_112MB"]
            summary["fetch_size_calibration"] = {"factor": 1.0 / ratio, "fetch_size_bytes_per_known_byte": ratio, "table": "1536 MB (past the Infinity Cache)" if wl == "big" else "112 MB (inside the Infinity Cache)",
                                                 "source": cal["source"]}
            summary["traffic_bytes_calibrated"] = (summary["FETCH_SIZE_KB_per_launch"] / ratio + summary.get("WRITE_SIZE_KB_per_launch", 0.0)) * 1024
        with open(os.path.join(P, f"{tag}_{wl}_summary.json"), "w") as f:
            json.dump(summary, f, indent=1)
        shutil.copy(os.path.join(P, f"{tag}_{wl}_summary.json"), os.path.join(P, f"pmc_{wl}.json"))
        print(wl, {k: summary.get(k) for k in ("avg_ms", "traffic_bytes_raw", "valu_busy_frac_at_profile_clock", "lane_utilisation", "valu_issue_cycles_per_ray")})
    for f in glob.glob(os.path.join(G, f"bench_*_{tag}.json")):
        wl = os.path.basename(f)[len("bench_"):-len(f"_{tag}.json")]  # "c3", "c3_gpubuilder", ...
        if os.path.getsize(f):
            shutil.copy(f, os.path.join(P, f"{tag}_{wl}_bench.json"))


if __name__ == "__main__":
    main()
