"""Records tests/golden/device_trees.json: the tree the device builder makes of each SMALL_SCENES scene under the builders "gpu"
and "gpu-plain", as util.device_tree_record describes it (tests/test_gpu_parity.py::test_device_built_trees_are_the_recorded_ones
compares).  Needs a GPU.  Run from the repo root, on the commit whose trees are to be kept:
  python tests/golden/make_golden_device_trees.py [output.json]
Two runs in separate processes must write the same file (the builder is deterministic); record only then."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["PBRT_HIP_DEBUG_KNOBS"] = "1"  # the suite's own settings (tests/conftest.py): re-insertion from 8 triangles on
os.environ["PBRT_HIP_REINSERT_MIN_TRIS"] = "8"

import pbrt_amd  # noqa: E402
from util import SMALL_SCENES, device_tree_record  # noqa: E402

NAMES = ["mesh1k", "mesh20k", "cornell", "ties", "deep", "check_sphere", "spheres2k"]
out = {}
for name in NAMES:
    sd = SMALL_SCENES[name]()
    for builder in ("gpu", "gpu-plain"):
        with pbrt_amd.Scene(sd, builder=builder) as sc:
            out[f"{name}/{builder}"] = device_tree_record(sc)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_trees.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"wrote {len(out)} trees to {path}")
