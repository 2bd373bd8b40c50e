"""The inputs of the builder-stage tests (test_build_stages_host.py, test_build_stages_gpu.py), generated from seeds, and their stage-1
reference (build_ref.build_stage1), computed once per process and left unchanged.  Coordinates stay within [2^-20, 2^20] in magnitude
apart from exact zeros."""
import functools

import numpy as np

import build_ref
import util


def soup(n, seed):
    """n random triangles: centres uniform in [1, 3]^3, corners within 0.6 n^(-1/3) of them (as large as their spacing)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(1.0, 3.0, (n, 1, 3))
    P = (c + rng.uniform(-1.0, 1.0, (n, 3, 3)) * 0.6 * n ** (-1.0 / 3.0)).astype(np.float32).reshape(-1, 3)
    return P, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def _copies():
    P, idx = soup(300, 77)
    return P, np.concatenate([np.tile(idx[:1], (1000, 1)), idx]).astype(np.uint32)


def _flat(axes):
    P, idx = soup(600, 31)
    P = P.copy()
    P[:, list(axes)] = np.float32(1.5)
    return P, idx


def _scene(sd):
    P, idx = util.with_sphere_proxies(sd)
    return np.asarray(P, np.float32).reshape(-1, 3) + np.float32(0.0), np.asarray(idx, np.uint32).reshape(-1, 3)  # (-0 + 0 = +0)


# name -> (maker, what the case is there to reach)
CASES = {
    "n2": (lambda: soup(2, 2), "the smallest tree: one interior node"),
    "n3": (lambda: soup(3, 3), "a leaf beside an interior child"),
    "n7": (lambda: soup(7, 7), "the largest tree re-insertion skips (n < 8)"),
    "n8": (lambda: soup(8, 8), "the first size re-insertion runs on under the suite's PBRT_HIP_REINSERT_MIN_TRIS=8"),
    "n255": (lambda: soup(255, 255), "one ragged 256-thread block: the LDS-aggregated path of sah_bounds_kernel / sah_bins_kernel with idle lanes"),
    "n256": (lambda: soup(256, 256), "a block that is exactly one segment"),
    "n257": (lambda: soup(257, 257), "a second block of one triangle: the global-atomic path beside the LDS path on the same level"),
    "n513": (lambda: soup(513, 513), "blocks partly inside a segment: mixed levels"),
    "n1023": (lambda: soup(1023, 1023), "the last size of the greedy collapse"),
    "n1024": (lambda: soup(1024, 1024), "the first size of the dynamic programme"),
    "n2049": (lambda: soup(2049, 2049), "a second block of centroid_bounds_kernel (2048 triangles each) holding one triangle"),
    "n5000": (lambda: soup(5000, 5000), "three blocks of centroid_bounds_kernel, the last one ragged"),
    "n20000": (lambda: soup(20000, 20000), "several re-insertion passes and thousands of moves"),
    "undone": (lambda: soup(2000, 100000), "a last pass that raises the summed area and is undone (found by a search of seeds with the host run)"),
    "ties": (lambda: _scene(util.tie_scene()), "equal plane costs and equal Morton keys (every triangle twice, degenerate triangles)"),
    "copies": (_copies, "1000 copies of one triangle: no plane exists, segments are halved"),
    "deep": (lambda: _scene(util.deep_tree_scene(k=400)), "a level >= 40: the forced halving of sah_split_kernel; the visit cap of the re-insertion search is reached"),
    "flat1": (lambda: _flat((2,)), "a soup flat in one axis: the axis tie rule with a zero extent"),
    "flat2": (lambda: _flat((1, 2)), "a soup flat in two axes: ext[1] > ext[2] false, collinear triangles"),
    "spheres": (lambda: _scene(util.sphere_cloud_scene()), "with_sphere_proxies(spheres2k): degenerate proxy triangles"),
}


@functools.lru_cache(maxsize=None)
def mesh(name):
    P, idx = CASES[name][0]()
    P.setflags(write=False)
    idx.setflags(write=False)
    return P, idx


@functools.lru_cache(maxsize=None)
def reference(name):
    """build_ref.build_stage1 of the case (shared: callers copy what they change)"""
    return build_ref.build_stage1(*mesh(name))
