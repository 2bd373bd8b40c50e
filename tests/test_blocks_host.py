"""The kernels' building blocks against float64, on the CPU: the oracle's restatements (oracle_math.hpp, oracle.cpp, oracle_scene.hpp) through
orc_blocks_eval over the input sets of tests/blocks_ref.py and tests/walk_ref.py (the walk's node step and triangle test), under the bounds written
there and in DESIGN.md 3.4 / 3.5 / 3.6; the power heuristic's weights and sample_light likewise.  The device runs the same
sets through pbrt_hip_blocks_eval_device in tests/test_blocks_gpu.py, bit-equal to what is checked here.  Parity between oracle and kernels
cannot see a wrong coefficient or a wrong range threshold -- both restate the same fixed order of fp32 operations -- and a render sees one
only once it moves an image: these tests do, element by element."""
import ctypes as C

import numpy as np
import pytest

import blocks_ref as br
from pbrt_amd import _lib, api


@pytest.mark.parametrize("op", list(br.POLY_BOUND))
def test_polynomials_against_float64(oracle, op):
    """poly_sin, poly_cos, poly_atan_pos, poly_acos and the octant reduction of sin / cos over [0, 2 pi]: every 64th float32 pattern of the
    domain and every pattern within 4096 of 0, of the domain's ends, of the range thresholds and of the multiples of pi / 4.  The bound is
    DESIGN.md 3.6's table -- the error measured here + 0.5 ulp --, and the measured figure itself is pinned to 1 %: a change of the
    arithmetic that moves it has to move the table."""
    x, aux = br.inputs(op)
    got = oracle.blocks_eval(op, x)
    worst, at = br.check(op, x, aux, got)
    print(f"{op}: {len(x)} inputs, largest error {worst:.4g} {br.POLY_BOUND[op][0]} at x = {at!r} (bound {br.POLY_BOUND[op][1]})")
    assert abs(worst / br.POLY_MEASURED[op] - 1.0) < 0.01, (op, worst, br.POLY_MEASURED[op])


@pytest.mark.parametrize("op", ["SPHERE_UV", "FRESNEL", "COSINE_ABOUT"])
def test_composite_blocks_against_float64(oracle, op):
    """sphere_uv (the seam, the poles, the axes, a clamped |nz|), the Fresnel term (grazing and normal incidence, the critical angle pattern by
    pattern, matched indices) and cosine sampling about a normal (the disk's centre, rim and wedge diagonals; normals on the frame's
    branch): bounds propagated in float64 per element from the polynomials', none taken from the outputs; each below 1e-5 on 99 % of the
    elements, so that a bound blown up at a singular point cannot carry the test."""
    x, aux = br.inputs(op)
    figures = br.check(op, x, aux, oracle.blocks_eval(op, x))
    print(f"{op}: {len(x)} inputs, largest error / bound and shares of the bounds below 1e-5: {figures}")


def test_fresnel_clamps_a_cosine_above_one(oracle):
    """1 - ci^2 is negative for a cosine that rounding carried above 1; the clamp in front of it keeps ct = 1 and F in [0, 1]"""
    x = br.fresnel_above_one_inputs()
    br.check_fresnel_above_one(x, oracle.blocks_eval("FRESNEL", x))


def test_sphere_test_alone_against_float64(oracle):
    """sphere_hit without a tree around it, over the ladder of distance / radius of util.SPHERE_LADDER: what test_oracle_selfcheck.py's
    test_sphere_hits_against_float64 checks of the walks, of the function -- a failure there and not here is the walk's."""
    x, parts = br.inputs("SPHERE_HIT")
    for rung, m in br.check("SPHERE_HIT", x, parts, oracle.blocks_eval("SPHERE_HIT", x)).items():
        print(f"D, r = {rung}: max |dt| {m['max_dt']:.3g}, max |dt| / bound {m['max_ratio']:.3f}, off the surface {m['off_surface_radii']:.3g} r, robust {m['robust']}")


def test_node_step_against_float64(oracle):
    """One step of the production walk (oracle/quad_walk.cpp quad_step, what walk(), orc_quad_path_check and the op all call) against the
    float64 statement of tests/walk_ref.py over about 2^18 (node, ray) pairs: no false negative, the near planes outside the true ones and no
    further than the roundings and the margin put them (QUAD_C = 9), no hit beyond that model, the slot entered, the unused slots, a ray
    that meets a real node's exact child box let in.  Prints the largest observed fractions of the bounds."""
    x, aux = br.inputs("QUAD_STEP")
    got = oracle.blocks_eval("QUAD_STEP", x)
    figures = br.wr.check_quad_step(x, aux, got, oracle.blocks_eval("QUAD_STEP_PK", x))
    print("QUAD_STEP:", figures)
    assert figures["pairs"] >= 250_000 and figures["on the domain"] >= 0.9 * figures["pairs"] and figures["must hit"] >= 100_000
    assert 0.25 <= figures["largest fraction of the inward bound"] <= 1.0 and 0.25 <= figures["largest fraction of the outward bound"] <= 1.0


@pytest.mark.parametrize("size", br.wr.TRI_SIZES)
def test_triangle_test_against_float64(oracle, size):
    """Moeller-Trumbore + the |det| cut + the own-box rule (Scene::tri_hit) over the ladder aspect x distance / size x |d| of one size, 2^14
    rays a rung, against float64 with a running error bound per ray (tests/walk_ref.py): on the ASSERTED rungs at least half of the rays
    are robust by float64 alone, hit-or-miss equals float64's on every robust ray and |dt|, |du|, |dv| stay within their bounds; on ALL rays
    an accepted hit lies at or beyond its own box's entry and its ray meets that box.  Prints DESIGN.md 3.5's table, the rungs that are
    measured and not asserted included."""
    x, parts = br.wr.tri_hit_inputs(size)
    table = br.wr.check_tri_hit(parts, x, oracle.blocks_eval("TRI_HIT", x))
    assert sum(m["asserted"] for m in table.values()) >= (2 if size < 1 else 9)
    for (aspect, dist, _, dlen), m in table.items():
        print(f"aspect {aspect:g} dist/size {dist:g} size {size:g} |d| {dlen:g}: {'asserted' if m['asserted'] else 'NOT ASSERTED'} robust {m['robust']:.3f} "
              f"max |dt| {m['max_dt']:.3g} |duv| {m['max_duv']:.3g} err/bound t {m['ratio_t']:.3f} u {m['ratio_u']:.3f} v {m['ratio_v']:.3f} "
              f"equal {m['equal']:.4f} (robust: {m['robust_equal']}) lost to the det cut {m['lost_to_cut']:.3f}")


def test_flat_triangles_and_exact_rays(oracle):
    """triangles flat in an axis plane and slivers rotated in it: every ray robustly inside in u, v and t is a hit, whatever the condition
    number (no holes, at unit level); rays whose arithmetic is exact: the edges and vertices count, u + v = 1 included, and a ray through
    a corner of the triangle's own box is let in"""
    x, aux = br.inputs("TRI_HIT")
    print("TRI_HIT:", br.check("TRI_HIT", x, aux, oracle.blocks_eval("TRI_HIT", x)))


@pytest.mark.parametrize("op", ["MIS_W_LIGHT", "MIS_W_BSDF"])
def test_mis_weights_against_float64(oracle, op):
    """The power heuristic's two weights over pl = 2^-70 ... 2^70 against every pb a bounce ray can carry and smaller: never
    NaN; within four roundings of 1 / (1 + (pb / pl)^2) and 1 / (1 + (pl / pb)^2) wherever no square leaves float32's normal range; from
    pl = 2^64 upwards, where pl^2 is +inf, the light's weight within that bound of 1 and the bounce ray's at most a denormal step above its
    value; in the 0 / 0 corner (both squares zero: densities no render reaches, pb >= 2^-24 / pi) a finite weight in [0, 1].  The plain
    quotient is inf / inf = NaN from pl = 2^64: a tiny emitter far away or seen at a grazing angle zeroed its whole sample."""
    x, aux = br.inputs(op)
    print(f"{op}: {len(x)} inputs:", br.check(op, x, aux, oracle.blocks_eval(op, x)))


def test_direct_light_estimate_against_float64(oracle):
    """sample_light element by element against the float64 estimator written from the text: point, distant, constant-sky
    and emissive-triangle lights, each with mis 0 and 1, over the ladders of blocks_ref.light_inputs (distances 2^-10 ... 2^10, areas 2^-40 ...
    2^20, cosines down to 2^-20, nL up to 1000, the sample on a vertex, the shaded point on the light, the light behind the surface, the
    triangle seen from behind).  The decision equals float64's wherever float64 settles it beyond the float32 rounding of its own operands
    -- the share it does not settle is computed from the reference alone, printed, and at most 2 % of a kind's set outside the rungs built to
    sit on the edge --; Ld, wi and tmax of an accepted element lie within (roundings counted x U) x the element's condition; Ld is never NaN;
    where pl >= 2^64 the estimate with mis = 1 is the one with mis = 0.  The largest error / bound is printed beside LIGHT_MEASURED."""
    x, aux = br.inputs("LIGHT")
    shares = br.light_margin_shares(aux, br.light_reference(x))   # of the reference alone, before anything is evaluated
    print("LIGHT: share of the elements float64 does not settle, outside the edge rungs:", shares)
    assert max(shares.values()) <= 0.02
    figures = br.check("LIGHT", x, aux, oracle.blocks_eval("LIGHT", x))
    print(f"LIGHT: {len(x)} inputs:", figures, "recorded:", br.LIGHT_MEASURED)
    assert max(figures[k] for k in br.LIGHT_MEASURED) <= 1.0


def test_oracle_hook_refuses_what_it_does_not_know(oracle):
    """orc_blocks_eval refuses what it does not know, and an op's outputs have the documented shapes"""
    with pytest.raises(KeyError):
        oracle.blocks_eval("TAN", np.zeros(1, np.float32))
    a = np.zeros(64, np.float32)
    assert len(oracle.BLOCK_OPS) == 15 and oracle.lib().orc_blocks_eval(15, 1, a.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)) == -1  # (COUNT itself)
    assert oracle.lib().orc_blocks_eval(99, 1, C.c_void_p(0), C.c_void_p(0)) == -1
    assert oracle.lib().orc_blocks_eval(0, 1, C.c_void_p(0), C.c_void_p(0)) == -1
    for op, (code, w_in, w_out) in oracle.BLOCK_OPS.items():
        assert api.BLOCK_OPS[op] == (code, w_in, w_out)
        assert oracle.blocks_eval(op, np.full((3, w_in), 0.5, np.float32)).shape == (3, w_out)
    assert tuple(oracle.BLOCK_OPS) == br.ALL_OPS


def test_device_hook_refuses_bad_arguments_before_it_touches_a_device():
    """pbrt_hip_blocks_eval_device: PBRT_HIP_ERR_INVALID for an unknown op, a negative n, a null array -- decided before any HIP call, so
    this runs without a GPU; n = 0 is nothing to do"""
    f = _lib.lib().pbrt_hip_blocks_eval_device
    a = np.zeros(64, np.float32)
    p = a.ctypes.data_as(C.POINTER(C.c_float))
    assert len(api.BLOCK_OPS) == 15 and f(0, 15, 1, p, p) == -1 and f(0, 0xffffffff, 1, p, p) == -1
    assert f(0, 0, -1, p, p) == -1
    assert f(0, 0, 1, None, p) == -1 and f(0, 0, 1, p, None) == -1
    assert b"blocks_eval_device" in _lib.lib().pbrt_hip_last_error()
    assert f(0, 0, 0, p, p) == 0
