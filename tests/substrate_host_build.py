"""pbrt_amd/csrc/substrate_bsdf.hpp compiled FOR THE HOST into a stand-alone program (plain g++ with -ffp-contract=off, nothing of HIP): the
header's text, and substrate_eval.inc around it, exactly as kernels_blocks.hip's substrate_eval_kernel compiles them for the device.  The
stub of <hip/hip_runtime.h>, the way the program is run and the input generators are tests/plastic_host_build.py's: the layout is plastic's
(18 floats in, 10 out).  Shared by tests/test_substrate_host.py (the header against float64) and tests/test_substrate_gpu.py (the device
against this program, bit for bit)."""
import os
import subprocess

import plastic_host_build as phb
from plastic_host_build import N_IN, N_OUT, ROOT, STUB, domain_inputs, edge_inputs, run  # noqa: F401  (the generators and run: for the tests)

MAIN = phb.MAIN.replace("plastic_bsdf.hpp", "substrate_bsdf.hpp").replace("plastic_eval.inc", "substrate_eval.inc")
assert "substrate_bsdf.hpp" in MAIN and "substrate_eval.inc" in MAIN and "plastic" not in MAIN


def build(tmp_path):
    """-> the program's path, built under tmp_path"""
    tmp_path = str(tmp_path)
    os.makedirs(os.path.join(tmp_path, "stub", "hip"), exist_ok=True)
    with open(os.path.join(tmp_path, "stub", "hip", "hip_runtime.h"), "w") as f:
        f.write(STUB)
    src, exe = os.path.join(tmp_path, "substrate_host.cpp"), os.path.join(tmp_path, "substrate_host")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-attributes", "-I", os.path.join(tmp_path, "stub"), "-I",
                    os.path.join(ROOT, "pbrt_amd", "csrc"), src, "-o", exe], check=True)
    return exe
