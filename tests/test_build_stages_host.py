"""The device tree builder's stages against their references, the part that needs no GPU: the stage-1 restatement (build_ref.py) is a
valid tree and survives its own float64 side check; the host runs of stage 2 and stage 3 on that tree (pbrt_hip_reinsert_links_host,
pbrt_hip_collapse_host -- the same functions the device calls, reinsert_core.hpp and quad_encode.hpp) keep their promises; the hooks
refuse what they must.  tests/test_build_stages_gpu.py compares the device with all of this."""
import ctypes as C
import sys

import numpy as np
import pytest

import build_cases
import build_ref
from pbrt_amd import _lib
from pbrt_amd.api import collapse_host, reinsert_links_host
from test_host import _check_quads

ALL = list(build_cases.CASES)


def _n(name):
    return len(build_cases.mesh(name)[1])


@pytest.mark.parametrize("name", ALL)
def test_reference_tree_is_a_valid_binary_tree(name):
    r = build_cases.reference(name)
    build_ref.check_binary_tree(r)
    assert len(r["splits"]) == _n(name) - 1 and r["morton_keys"].max() < 1 << 30


def test_cases_reach_what_they_are_there_for():
    """asserted from the REFERENCE: the forced halving (a level >= 40), halving for want of a plane, the axis tie rule"""
    deep = build_cases.reference("deep")
    assert deep["max_level"] >= build_ref.MEDIAN_LEVEL
    assert any(s["level"] >= build_ref.MEDIAN_LEVEL and s["best"] >= 0 for s in deep["splits"]), "a plane existed and the level overrode it"
    copies = build_cases.reference("copies")
    assert sum(s["best"] < 0 for s in copies["splits"]) >= 900, "1000 equal triangles: no plane"
    assert any(s["best"] < 0 for s in build_cases.reference("ties")["splits"])
    for name in ("flat1", "flat2"):
        P, idx = build_cases.mesh(name)
        ext = np.ptp(P, 0)
        assert (ext == 0).sum() == (1 if name == "flat1" else 2)


@pytest.mark.parametrize("name", ALL)
def test_reference_plane_choices_against_float64(name):
    """build_ref.check_plane_choices (the derivation of the 2^-20 margin is at build_ref.PLANE_MARGIN): the chosen plane's float64 cost is
    within the margin of the least; it IS the float64 argmin except at nodes where two costs lie within the margin, and those are at most
    1 % of the case's split nodes (`ties` is exempt from the cap and checked for the lowest index among equal costs)."""
    r = build_cases.reference(name)
    chk = build_ref.check_plane_choices(r["splits"])
    assert not chk["over_margin"] and not chk["unexplained"], chk
    if name == "ties":
        assert not build_ref.check_lowest_index_among_equal(r["splits"])
    else:
        assert len(chk["not_argmin"]) <= 0.01 * chk["split_nodes"], (len(chk["not_argmin"]), chk["split_nodes"])
    if name != "deep":  # (its coordinates shrink to 2^-149: products of extents underflow there and the derivation does not cover them)
        assert chk["underflowed"] == 0


def _tree_args(r):
    return r["child"], r["boxes"], r["order"]


def _cost(kid_boxes):
    """summed half surface area of the interior nodes, float64 from the float32 boxes"""
    d = kid_boxes[:, 3:].astype(np.float64) - kid_boxes[:, :3].astype(np.float64)
    return float(((d[:, 0] * d[:, 1] + d[:, 0] * d[:, 2]) + d[:, 1] * d[:, 2]).sum())


@pytest.mark.parametrize("name", [k for k in ALL if k not in ("n2", "n3")])
def test_host_reinsertion_of_the_reference_tree(name):
    r = build_cases.reference(name)
    n = _n(name)
    a = reinsert_links_host(*_tree_args(r))
    b = reinsert_links_host(*_tree_args(r))
    assert a["valid"], "LinkTree::valid"
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32) if k == "boxes" else a[k], np.asarray(b[k]).view(np.uint32) if k == "boxes" else b[k]), k
    assert a["fixed_after"] <= a["fixed_before"], "the cost does not rise (the device's fixed-point sums)"
    assert _cost(a["boxes"][:n - 1]) <= _cost(r["boxes"][:n - 1]) * (1 + 1e-12)
    assert np.array_equal(a["boxes"][n - 1:].view(np.uint32), r["boxes"][n - 1:].view(np.uint32)), "leaves keep their boxes and ids"
    assert a["passes"] >= 1 and a["applied"] <= a["found"]
    if name == "undone":
        assert a["undone"] == 1
    if name == "deep":  # (the 1000 copies of one triangle stop at 48 visits: equal boxes prune at once)
        assert a["max_visits"] >= 512, "the visit cap of the search is reached"
    # the tail of stage 2 restated over the result: a valid tree again, over the same triangles
    t = build_ref.reinsert_tail(a["par"], a["kid"], a["boxes"], r["order"])
    build_ref.check_binary_tree(t)


@pytest.mark.parametrize("name", ALL)
def test_host_collapse_of_the_reference_tree(name):
    """_check_quads on both rules; from 1024 triangles on (where the builder uses the dynamic programme) dp's float64 expected work is at most
    greedy's, and within build_ref.dp_bound (its derivation: build_ref.DP_C) of the float64 optimum G64(root)."""
    sys.setrecursionlimit(10000)
    r = build_cases.reference(name)
    P, idx = build_cases.mesh(name)
    n = _n(name)
    work = {}
    for rule in ("greedy", "dp"):
        quads, need = collapse_host(*_tree_args(r), rule)
        _check_quads(quads, need, P, idx.astype(np.int64), r["order"])
        work[rule], reached = build_ref.quad_tree_work_f64(quads, r["child"], r["boxes"])
        assert reached == len(quads)
    if n >= 1024:
        dp = build_ref.dp_tables_f64(r["child"], r["boxes"])
        g64 = dp["G"][0]
        print(f"{name}: work greedy {work['greedy']:.9g} dp {work['dp']:.9g} optimum {g64:.9g} rel {(work['dp'] - g64) / g64:.3g} bound {build_ref.dp_bound(2 * n - 1):.3g}")
        assert work["dp"] <= work["greedy"]
        assert g64 * (1 - 1e-12) <= work["dp"] <= g64 * (1 + build_ref.dp_bound(2 * n - 1))


def test_hooks_refuse_bad_arguments():
    """a null array, n_tris < 2, an index beyond n_verts (the device hook refuses it before it looks for a device), a child word out of range"""
    l = _lib.lib()
    INVALID = -1  # PBRT_HIP_ERR_INVALID
    r = build_cases.reference("n8")
    n = 8
    child, boxes, order = (np.ascontiguousarray(r[k]) for k in ("child", "boxes", "order"))
    u32p, fp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_float)))
    nq, need = C.c_uint32(), C.c_uint32()
    quads = np.zeros((n, 16), np.uint32)

    def reinsert(n_, child_, boxes_, order_):
        return l.pbrt_hip_reinsert_links_host(n_, child_, boxes_, order_, None, None, None, None, None, None)

    def collapse(n_, child_, boxes_, order_, rule=2):
        return l.pbrt_hip_collapse_host(n_, child_, boxes_, order_, rule, u32p(quads), n, C.byref(nq), C.byref(need))

    for call in (reinsert, collapse):
        assert call(n, u32p(child), fp(boxes), u32p(order)) == 0
        assert call(n, None, fp(boxes), u32p(order)) == INVALID
        assert call(n, u32p(child), None, u32p(order)) == INVALID
        assert call(n, u32p(child), fp(boxes), None) == INVALID
        assert call(1, u32p(child), fp(boxes), u32p(order)) == INVALID
        assert call(0, u32p(child), fp(boxes), u32p(order)) == INVALID
        for word in (n - 1, 0x80000000 | n, 0, int(child[1, 0])):  # an interior node / a leaf slot out of range, the root, a node used twice
            bad = child.copy()
            bad[0, 0] = word
            assert call(n, u32p(bad), fp(boxes), u32p(order)) == INVALID, hex(word)
        bad = order.copy()
        bad[3] = n
        assert call(n, u32p(child), fp(boxes), u32p(bad)) == INVALID
        bad = boxes.copy()
        bad[2, 1] = np.nan
        assert call(n, u32p(child), fp(bad), u32p(order)) == INVALID
    assert collapse(n, u32p(child), fp(boxes), u32p(order), rule=0) == INVALID
    assert l.pbrt_hip_collapse_host(n, u32p(child), fp(boxes), u32p(order), 2, u32p(quads), n, None, C.byref(need)) == INVALID
    # the device hook: refused at the boundary, before a device is looked for
    P, idx = (np.ascontiguousarray(a) for a in build_cases.mesh("n8"))
    st = _lib.BuildStages()
    dev = lambda P_, nv, idx_, nt, flags=1, out=C.byref(st): l.pbrt_hip_gpu_build_stages_device(0, P_, nv, idx_, nt, flags, out)
    assert dev(None, len(P), u32p(idx), n) == INVALID
    assert dev(fp(P), len(P), None, n) == INVALID
    assert dev(fp(P), len(P), u32p(idx), n, out=None) == INVALID
    assert dev(fp(P), len(P), u32p(idx), 1) == INVALID
    assert dev(fp(P), len(P) - 1, u32p(idx), n) == INVALID
    assert dev(fp(P), len(P), u32p(idx), n, flags=2) == INVALID
    bad = P.copy()
    bad[5, 0] = np.inf
    assert dev(fp(bad), len(P), u32p(idx), n) == INVALID
