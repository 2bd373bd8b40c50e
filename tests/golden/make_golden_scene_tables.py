"""Records tests/golden/scene_tables.npz: the words of every array and scalar that pbrt_hip_scene_tables_host reports for the three
descriptions of tests/scene_tables_cases.py (tests/test_scene_tables_host.py compares).  No GPU needed.  The file holds what the commit BEFORE
scene_tables.hpp computed: it was recorded with PBRT_HIP_LIB_DIR naming a library built from that commit, with the hook added at the end of its
capi_scene.cpp around its own gather_inputs.  Run from the repo root:
  PBRT_HIP_LIB_DIR=<library directory> python tests/golden/make_golden_scene_tables.py [output.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import scene_tables_cases as cases  # noqa: E402

out = {f"{name}/{key}": words for name, make in cases.CASES.items() for key, words in cases.tables(make()).items()}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "scene_tables.npz")
np.savez_compressed(path, **out)
print(f"wrote {len(out)} arrays, {sum(v.size for v in out.values())} words, to {path}")
