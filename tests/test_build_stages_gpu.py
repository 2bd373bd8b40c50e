"""The device tree builder (pbrt_amd/csrc/bvh_gpu.hip) stage by stage against references, through the observer of
pbrt_hip_gpu_build_stages_device: stage 1 bit for bit against its numpy restatement (build_ref.py); the passes of stage 2 word for word
against the host run of the same functions ON THE DEVICE'S OWN stage-1 tree; the tail of stage 2 against its restatement; the collapse
against the host's collapse of the device's stage-2 tree, its tables against the float64 recurrence and the tree it emits against the
float64 optimum.  Every equality is on raw words; the one tolerance here is build_ref.dp_bound, derived at build_ref.DP_C."""
import math

import numpy as np
import pytest

import build_cases
import build_ref
import util
from pbrt_amd.api import collapse_host, gpu_build_stages, reinsert_links_host

pytestmark = pytest.mark.gpu
ALL = list(build_cases.CASES)
TREE_KEYS = ("child", "parent_internal", "parent_leaf", "boxes", "order")
_built = {}


def _n(name):
    return len(build_cases.mesh(name)[1])


def stages(name):
    """the device build of a case, once per session (read-only to the tests)"""
    if name not in _built:
        _built[name] = gpu_build_stages(*build_cases.mesh(name))
    return _built[name]


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)


def assert_trees_equal(got, want, what):
    for k in TREE_KEYS:
        assert np.array_equal(words(got[k]), words(want[k])), f"{what}: {k} differs in {np.count_nonzero(words(got[k]) != words(want[k]))} words"


@pytest.mark.parametrize("name", ALL)
def test_stage1_equals_the_restatement_bit_for_bit(gpu, name):
    d, r = stages(name), build_cases.reference(name)
    assert np.array_equal(d["morton_keys"], r["morton_keys"]), "Morton keys"
    assert_trees_equal(d["built"], r, "after sah_build")


def _compare_passes_with_host(d):
    """the device's link form after the passes and its counts == the host run (reinsert_links_host) on the device's own stage-1 tree"""
    b, links, st = d["built"], d["links"], d["reinsert"]
    h = reinsert_links_host(b["child"], b["boxes"], b["order"])
    assert h["valid"]
    assert np.array_equal(links["par"], h["par"]), "par"
    assert np.array_equal(words(links["boxes"]), words(h["boxes"])), "bx"
    # (the observer copies before ri_order_kernel, the host run returns after order_children: the same pairs, and in the host's order
    # once the rule is applied to the device's)
    assert np.array_equal(np.sort(links["kid"], 1), np.sort(h["kid"], 1)), "kid"
    assert np.array_equal(build_ref.order_children(links["kid"], links["boxes"]), h["kid"]), "kid, children ordered"
    assert st["undone"] == h["undone"]
    assert st["passes"] == h["passes"] - h["undone"], "passes kept"
    assert st["moves"] == h["applied"] and st["visits"] == h["visits"]
    unit = math.ldexp(1.0, -h["fixed_exp"])
    assert st["cost_before"] == h["fixed_before"] * unit and st["cost_after"] == h["fixed_after"] * unit, "the fixed-point sums"
    return h


@pytest.mark.parametrize("name", [k for k in ALL if k not in ("n2", "n3", "n7")])
def test_stage2_passes_equal_the_host_run(gpu, name):
    d = stages(name)
    assert d["links"] is not None, "re-insertion runs from 8 triangles on under the suite's PBRT_HIP_REINSERT_MIN_TRIS"
    h = _compare_passes_with_host(d)
    if name == "n20000":
        assert h["passes"] >= 3 and h["applied"] >= 2000, "several passes, thousands of moves"
    if name == "undone":
        assert h["undone"] == 1, "the undo path: the device restores the links and boxes it saved before the pass"
    if name == "deep":  # (the 1000 copies of one triangle stop at 48 visits: equal boxes prune at once)
        assert h["max_visits"] >= 512, "the visit cap of the search is reached"


def test_stage2_full_refit_equals_the_host_run(gpu, monkeypatch):
    """PBRT_HIP_REINSERT_FULL_REFIT: every box every pass (ri_refit_kernel) instead of the dirty chains (ri_mark_kernel, ri_refit_dirty_kernel)"""
    monkeypatch.setenv("PBRT_HIP_REINSERT_FULL_REFIT", "1")
    full = gpu_build_stages(*build_cases.mesh("n5000"))
    _compare_passes_with_host(full)
    assert_trees_equal(full["optimised"], stages("n5000")["optimised"], "full refit against the dirty chains")


@pytest.mark.parametrize("name", ["n2", "n3", "n7"])
def test_small_trees_skip_stage2(gpu, name):
    d = stages(name)
    assert d["links"] is None and d["reinsert"] is None
    assert_trees_equal(d["optimised"], d["built"], "a tree below 8 triangles is left as built")


@pytest.mark.parametrize("name", [k for k in ALL if k not in ("n2", "n3", "n7")])
def test_stage2_tail_equals_the_restatement(gpu, name):
    d = stages(name)
    want = build_ref.reinsert_tail(d["links"]["par"], d["links"]["kid"], d["links"]["boxes"], d["built"]["order"])
    assert_trees_equal(d["optimised"], want, "after reinsert")
    build_ref.check_binary_tree(d["optimised"])


@pytest.mark.parametrize("name", ALL)
def test_stage3_quads_equal_the_host_collapse(gpu, name):
    """greedy below 1024 triangles, the dynamic programme from there on: the same rule forced on the host, on the device's stage-2 tree"""
    d = stages(name)
    t = d["optimised"]
    dp = _n(name) >= 1024
    assert (d["dp"] is not None) == dp
    quads, need = collapse_host(t["child"], t["boxes"], t["order"], "dp" if dp else "greedy")
    assert len(d["quads"]) == len(quads) and d["stack_need"] == need
    assert np.array_equal(util.sorted_quad_rows(d["quads"]), util.sorted_quad_rows(quads))


@pytest.mark.parametrize("name", [k for k in ALL if _n(k) >= 1024])
def test_stage3_tables_and_emitted_tree_against_float64(gpu, name):
    """Every exported F(v, k, d), Fl and G within build_ref.dp_bound(m) = m x 10 x 2^-24 (relative; m = nodes in v's subtree; derivation at
    build_ref.DP_C: seven roundings of area_on_grid and at most two additions per interior node) of the float64 recurrence, and the float64
    expected work of the quad tree the device EMITTED within the same bound of G64(root): the collapse followed the programme's choices."""
    d = stages(name)
    t, n = d["optimised"], _n(name)
    ref = build_ref.dp_tables_f64(t["child"], t["boxes"])
    m = ref["nodes"]
    got = {"F": d["dp"]["F"], "Fl": d["dp"]["Fl"], "G": d["dp"]["G"]}
    want = {"F": ref["F"][:n - 1], "Fl": ref["F"][n - 1:, 0, :], "G": ref["G"]}
    bound = {"F": build_ref.dp_bound(m[:n - 1])[:, None, None], "Fl": build_ref.dp_bound(m[n - 1:])[:, None], "G": build_ref.dp_bound(m[:n - 1])}
    for k in got:
        rel = np.abs(got[k].astype(np.float64) - want[k]) / want[k]
        print(f"{name} {k}: worst relative error / bound = {float((rel / bound[k]).max()):.3g}")
        assert np.all(rel <= bound[k]), k
    work, reached = build_ref.quad_tree_work_f64(d["quads"], t["child"], t["boxes"])
    g64 = ref["G"][0]
    print(f"{name}: emitted tree's work {work:.12g}, optimum {g64:.12g}, relative excess {(work - g64) / g64:.3g}, bound {float(build_ref.dp_bound(2 * n - 1)):.3g}")
    assert reached == len(d["quads"])
    assert g64 * (1 - 1e-12) <= work <= g64 * (1 + build_ref.dp_bound(2 * n - 1))


def test_hook_builds_what_a_scene_builds(gpu):
    """the hook's final quads and leaf order == Scene(..., builder="gpu").export_quads() of a scene holding the same soup"""
    sd = util.tie_scene()
    sc = gpu.Scene(sd, builder="gpu")
    quads, order = sc.export_quads()
    d = stages("ties")
    assert np.array_equal(order, d["optimised"]["order"])
    assert len(quads) == len(d["quads"]) and sc.info()["quad_stack_need"] == d["stack_need"]
    assert np.array_equal(util.sorted_quad_rows(quads), util.sorted_quad_rows(d["quads"]))
