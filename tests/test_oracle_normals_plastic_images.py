"""The oracle's shading normals, plastic (3.21) and image lookup (3.20) without a GPU, held to things that are not the
oracle: its hooks against the host compile of plastic_bsdf.hpp and the product's host image hook bit for bit and against normals_ref's
float64 with its first-order bounds; its films against the float64 references (tests/plastic_ref.py), the closed forms
tests/test_normals_gpu.py and tests/test_image_texture_gpu.py hold the kernels to, the identity "a point-sampled 2 x 2 image is the
checkerboard", and small determinate scenes that tell one statement of the three sections from its nearest wrong neighbour; every scene it
refuses.  What the HIP path adds to this is tests/test_normals_plastic_parity_gpu.py: the kernels' films equal the oracle's word for word."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import image_ref as ir
import normals_ref as nr
import plastic_host_build as hb
import plastic_ref as pr
from image_ref import BILINEAR, BLACK, CLAMP, POINT, REPEAT
from oracle import binding as orc
from pbrt_amd import (GLASS, INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_DISTANT, LIGHT_INFINITE, LIGHT_POINT, MATTE, MIRROR, PLASTIC,
                      SceneData, _lib, api, film_to_rgb, look_at, scenes)
from test_envmap_host import random_map
from util import assert_bit_equal, bits, checker_plane_scene, lit_plane_scene, meets_random_scene_bar, quad_mesh, twin_agreement

SAMPLERS = ("stratified", "sobol", "sobol_nd", "halton")
BAR = dict(rtol=3e-6, atol=1e-7)  # tests/test_normals_gpu.py's bar for the closed forms


def _rgb(film):
    return film_to_rgb(film).astype(np.float64)


def _render(sd, **kw):
    return orc.OracleScene(sd).render(**kw)[0]


# ---- the hooks ----

def test_plastic_words_equal_the_host_compile(tmp_path):
    """orc_plastic_eval (oracle/oracle.cpp: restated from DESIGN.md 3.21) against plastic_bsdf.hpp compiled for the host, over the measured
    domain and the edge inputs: f, pdf_b, the sampled direction and its weight -- 0 words differ"""
    exe = hb.build(tmp_path)
    x = np.concatenate([hb.domain_inputs(), hb.edge_inputs()])
    assert len(x) == (1 << 16) + 4096
    got, want = orc.plastic_eval(x), hb.run(exe, x, tmp_path)
    assert (got[:, 7:] != 0).any(1).mean() > 0.5  # (most samples live: the comparison is not one of zeros)
    assert_bit_equal(got, want, "orc_plastic_eval vs the host compile of plastic_bsdf.hpp")


def test_image_lookup_equals_the_host_hook():
    """orc_image_lookup_eval against pbrt_hip_image_lookup_eval_host over the images and inputs of tests/test_image_texture_host.py: dyadic,
    random with random mappings, the non-finite ones, both filters, three wraps; and two records in one pool -- 0 words differ"""
    ident = (1.0, 1.0, 0.0, 0.0)
    n = 0
    for k, (w, h) in enumerate(ir.SIZES):
        img = ir.random_image(w, h, 100 + k)
        for wrap in (REPEAT, CLAMP, BLACK):
            for filt in (POINT, BILINEAR):
                for uv, mapping in ((ir.dyadic_inputs(rows=9), ident), ir.random_inputs(20_000, 7 * k + wrap), (ir.non_finite_inputs(), ident)):
                    rec = [(img, wrap, filt, mapping)]
                    got, want = orc.image_lookup_eval(rec, 0, uv), api.image_lookup_eval_host(rec, 0, uv)
                    assert np.isfinite(got).all()
                    assert_bit_equal(got, want, f"image {w} x {h}, wrap {wrap}, filter {filt}, mapping {mapping}")
                    n += len(uv)
    a, b = ir.random_image(3, 5, 1), ir.random_image(17, 4, 2)
    uv, mapping = ir.random_inputs(5000, 3)
    recs = [(a, REPEAT, POINT, mapping), (b, CLAMP, BILINEAR, mapping), (a, BLACK, BILINEAR, mapping)]
    for which in range(3):
        assert_bit_equal(orc.image_lookup_eval(recs, which, uv), api.image_lookup_eval_host(recs, which, uv), f"record {which} of three in one pool")
    assert not np.array_equal(orc.image_lookup_eval(recs, 1, uv), orc.image_lookup_eval(recs, 0, uv))
    assert n > 500_000
    with pytest.raises(ValueError):
        orc.image_lookup_eval([(a, 3, POINT, ident)], 0, uv)  # an unknown wrap


def test_image_lookup_orientation_and_accumulation_order():
    """What no random image tells apart from its neighbours at a glance: t = 0 is the BOTTOM row (row H - 1 of the array), and the bilinear
    sum runs j outer, i inner -- the other order rounds differently on a good share of random inputs between four unequal texels"""
    img = np.zeros((2, 1, 3), np.float32)
    img[0], img[1] = (1, 2, 3), (4, 5, 6)  # array row 0 = the image's top
    got = orc.image_lookup_eval([(img, CLAMP, POINT, (1, 1, 0, 0))], 0, [[0.5, 0.1], [0.5, 0.9]])
    assert np.array_equal(got, [[4, 5, 6], [1, 2, 3]])
    quad = np.zeros((2, 2, 3), np.float32)
    quad[1, 0], quad[1, 1], quad[0, 0], quad[0, 1] = 0.7, 0.3, 0.9, 0.55  # bottom row first: texel (i, j) = quad[1 - j, i]
    rng = np.random.default_rng(4)
    uv = (0.25 + 0.5 * rng.random((4096, 2))).astype(np.float32)  # between the four texel centres
    got = orc.image_lookup_eval([(quad, CLAMP, BILINEAR, (1, 1, 0, 0))], 0, uv)[:, 0]
    s, t = uv[:, 0] * np.float32(2) - np.float32(0.5), uv[:, 1] * np.float32(2) - np.float32(0.5)
    dx, dy = s - np.floor(s), t - np.floor(t)
    w = {(i, j): (dx if i else 1 - dx) * (dy if j else 1 - dy) for i in (0, 1) for j in (0, 1)}
    tex = {(i, j): quad[1 - j, i, 0] for i in (0, 1) for j in (0, 1)}
    j_outer = np.float32(0)
    for j in (0, 1):
        for i in (0, 1):
            j_outer = j_outer + tex[i, j] * w[i, j]
    i_outer = np.float32(0)
    for i in (0, 1):
        for j in (0, 1):
            i_outer = i_outer + tex[i, j] * w[i, j]
    assert j_outer.dtype == np.float32 and (j_outer != i_outer).sum() > 100  # (the two orders are told apart by these inputs)
    assert np.array_equal(got, j_outer)


def test_shading_normal_against_float64():
    """orc_shading_normal_eval over the input set of tests/test_normals_gpu.py::test_hook_against_float64, against normals_ref's float64
    with its first-order bounds, on the same robust subset -- which the reference alone decides, and whose share is at least that test's"""
    x, _ = nr.hook_inputs()
    ref = nr.shading_normal_f64(x)
    rb = ref["robust"]
    assert rb.mean() >= 0.90
    out = orc.shading_normal_eval(x)
    nsf, fell = out[:, :3].astype(np.float64), out[:, 3]
    assert set(np.unique(fell)) <= {0.0, 1.0} and not fell[rb].any()
    err = np.abs(nsf - ref["nsf"])
    assert (ref["bound"][rb] > 0).all()
    ratio = err[rb] / ref["bound"][rb]
    print(f"robust {rb.mean():.4f}; largest error / bound {ratio.max():.3f}; largest error {err[rb].max():.3g}")
    assert not (err[rb] > 0.5).any() and (ratio <= 1.0).all(), float(ratio.max())
    fb = ref["fell_back"]
    assert fell[fb].all() and fb.sum() >= 1024
    ng = x[:, 9:12]
    sure = fb & (np.abs(ref["c_wo"]) > nr.ROBUST_FACTOR * ref["c_wo_err"])
    assert sure.sum() >= 900
    assert_bit_equal(out[sure, :3], np.where(ref["flip_wo"][:, None], -ng, ng)[sure], "fallback")
    assert ((bits(out[fb, :3]) == bits(ng[fb])).all(1) | (bits(out[fb, :3]) == bits(-ng[fb])).all(1)).all()
    assert np.allclose(np.linalg.norm(nsf[~fb], axis=1), 1.0, atol=1e-5)
    assert orc.shading_normal_eval(np.zeros((0, 17), np.float32)).shape == (0, 4)


# ---- plastic films against the float64 reference ----

def _pref(sd, **kw):
    if kw.get("sampler") == "sobol_nd":
        kw = dict(kw, sobol_matrices=api.sobol_matrices())
    return pr.render(sd, **kw)


def _plastic_plane(res, eye, lights, kd=(0.3, 0.4, 0.5), ks=(0.5, 0.4, 0.3), roughness=0.2, fov=40.0, half=4.0):
    """tests/test_plastic_gpu.py's plane: a plastic quad z = 0 seen from `eye`"""
    row, alpha = api.plastic_material(kd, ks, roughness)
    h = half
    return SceneData(P=np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], np.float32), idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                     mat_id=np.zeros(2, np.uint16), materials=np.array([row], np.float32), mat_eta=np.array([alpha], np.float32),
                     lights=np.array(lights, np.float32), cam_to_world=look_at(eye, (0, 0, 0), (0, 0, 1))[1], fov=fov, xres=res, yres=res).normalized()


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_plastic_one_bounce_frames_match_the_reference(sampler):
    """tests/test_plastic_gpu.py's one-bounce frames (a plastic quad under one point light, under one distant light, direct lighting) at
    the bar it holds the kernel to: weights equal, 99 % of the pixels within 1e-4, PSNR >= 90 dB"""
    d = np.array([0.3, -0.2, 0.93])
    for name, light in (("point", [LIGHT_POINT, 0.5, -0.4, 1.5, 6, 6, 6]), ("distant", [LIGHT_DISTANT, *(d / np.linalg.norm(d)), 2, 2, 2])):
        sd = _plastic_plane(32, (0.2, -2.5, 1.2), [light])
        kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(2, 2), seed=11, sampler=sampler)
        film = _render(sd, **kw)
        ps, share, weights = twin_agreement(_pref(sd, **kw), film)
        print(f"{name} light, {sampler}: PSNR {ps:.1f} dB, {100 * share:.2f} % of the pixels within 1e-4")
        assert film[..., 1].mean() > 0.05
        assert weights and share >= 0.99 and ps >= 90.0, (name, sampler, ps, share)


PATH_CASES = [dict(integrator=i, sampler=s) for i in (INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS) for s in ("stratified", "halton")]
PATH_CASES += [dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol_nd", filter_width=(1.5, 0.75)), dict(integrator=INTEGRATOR_PATH, sampler="sobol", max_sample_luminance=1.0)]


@pytest.fixture(scope="module")
def plastic_box():
    sd = scenes.plastic_scene(32, 32)
    return sd, orc.OracleScene(sd)


@pytest.mark.parametrize("case", PATH_CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_plastic_whole_paths_match_the_reference(plastic_box, case):
    """scenes.plastic_scene(32, 32) at depth 5 under integrators 0, 1 and 2, the wide box filter and the luminance clamp, held to
    util.meets_random_scene_bar: the cases and the bar of tests/test_plastic_gpu.py::test_whole_paths_match_the_reference"""
    sd, o = plastic_box
    kw = dict(case, max_depth=5, spp=(4, 4), seed=5)
    film = o.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_pref(sd, **kw), film, kw)
    print(f"{case}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert ok, (case, ps, off)


@pytest.mark.parametrize("wrong", [dict(g_one=True), dict(lobe_pick=1.0 / 3.0)], ids=["G=1", "lobe-at-1/3"])
def test_a_wrong_plastic_reference_fails_the_same_bar(plastic_box, wrong):
    sd, o = plastic_box
    kw = dict(integrator=INTEGRATOR_PATH, sampler="stratified", max_depth=5, spp=(4, 4), seed=5)
    ok, ps, off = meets_random_scene_bar(_pref(sd, **kw, **wrong), o.render(**kw)[0], kw)
    print(f"{wrong}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert not ok


def _sky_only_plastic(le=(0.5, 0.25, 1.0), extra_light=None):
    """a plastic plane under a constant infinite light (and, extra_light, a second light that lights nothing: nL = 2)"""
    lights = [[LIGHT_INFINITE, 0, 0, 0, *le]] + ([extra_light] if extra_light else [])
    return _plastic_plane(16, (1.0, -2.0, 3.0), lights, half=50.0)


def test_plastic_under_a_constant_sky_keeps_the_constant_weight_pair():
    """A plastic plane alone under a constant infinite light, integrator 2 (DESIGN.md 3.21 "Light sample"): the light sample keeps the weight
    1 / (1 + nL^2) and the bounce ray that escapes nL^2 / (nL^2 + 1), whatever the BSDF.  Against the float64 reference, which has the
    rule, at the fixed cases' bar, with nL = 1 and nL = 2 (a distant light from below the plane beside the sky); and the rule is SEEN: the
    reference's own mean under integrator 0 is met within 5 standard errors, which the power heuristic on the light sample alone misses"""
    for extra in (None, [LIGHT_DISTANT, 0.0, 0.6, -0.8, 3, 3, 3]):
        sd = _sky_only_plastic(extra_light=extra)
        for sampler in ("stratified", "halton"):
            kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=3, spp=(4, 4), seed=7, sampler=sampler)
            film = _render(sd, **kw)
            ps, share, weights = twin_agreement(_pref(sd, **kw), film)
            print(f"sky alone, nL {1 + (extra is not None)}, {sampler}: PSNR {ps:.1f} dB, {100 * share:.2f} % within 1e-4")
            assert weights and share >= 0.99 and ps >= 90.0, (extra, sampler, ps, share)
    # unbiasedness: integrators 0 and 2 estimate the same image.  One bounce, 256 spp; the spread from the oracle's own per-pixel values
    sd = _sky_only_plastic()
    o = orc.OracleScene(sd)
    kw = dict(max_depth=1, spp=(16, 16), seed=3, sampler="stratified")
    a, b = (_rgb(o.render(integrator=i, **kw)[0])[..., 1] for i in (INTEGRATOR_PATH, INTEGRATOR_PATH_MIS))
    se = np.sqrt((a.var(ddof=1) + b.var(ddof=1)) / a.size)
    print(f"sky alone: integrator 0 mean {a.mean():.6f}, integrator 2 mean {b.mean():.6f}, 5 se {5 * se:.2e}")
    assert a.mean() > 0.05 and abs(a.mean() - b.mean()) <= 5 * se, (a.mean(), b.mean(), se)


def _floor_under_an_emitter():
    """a plastic floor lit only by an emissive triangle pair above it, the camera looking down at the floor: under integrator 2 what a
    bounce ray finds on the emitter is weighted through the stored pdf_b"""
    row, alpha = api.plastic_material((0.3, 0.4, 0.5), (0.6, 0.5, 0.4), 0.3, remap=False)
    floor = ((-3, -3, 0), (3, -3, 0), (3, 3, 0), (-3, 3, 0))
    lamp = ((-0.7, -0.7, 1.2), (-0.7, 0.7, 1.2), (0.7, 0.7, 1.2), (0.7, -0.7, 1.2))  # wound to face down
    P, idx, mat_id = quad_mesh([(floor, 0), (lamp, 1)])
    return SceneData(P=P, idx=idx, mat_id=mat_id, materials=np.array([row, [MATTE, 0, 0, 0, 5, 4, 3]], np.float32), mat_eta=np.array([alpha, 0], np.float32),
                     cam_to_world=look_at((2.5, -2.5, 0.9), (0, 0, 0), (0, 0, 1))[1], fov=50.0, xres=24, yres=24).normalized()


def test_plastic_floor_under_an_emitter_uses_the_stored_density():
    """The `pb` path of 3.21: integrator 2 against the float64 reference at the fixed cases' bar, depth 1 (the light sample and the bounce
    ray's emitter hit, nothing else) and depth 4"""
    sd = _floor_under_an_emitter()
    assert orc.OracleScene(sd).light_count() == 2  # the lamp's two triangles; the plastic floor's Ks is no emission
    for depth, sampler in ((1, "stratified"), (1, "sobol_nd"), (4, "halton")):
        kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=depth, spp=(4, 4), seed=2, sampler=sampler)
        film = _render(sd, **kw)
        ps, share, weights = twin_agreement(_pref(sd, **kw), film)
        print(f"floor under an emitter, depth {depth}, {sampler}: PSNR {ps:.1f} dB, {100 * share:.2f} % within 1e-4")
        assert film[..., 1].mean() > 0.02
        assert weights and share >= 0.99 and ps >= 90.0, (depth, sampler, ps, share)


# ---- normals: the closed forms of tests/test_normals_gpu.py ----

SETTINGS = [dict(integrator=i, max_depth=d, sampler=s) for i in (INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS) for d in (1, 5) for s in ("stratified", "halton")]
WL = np.array([0.6, 0.0, 0.8])
PLANE_CASES = {
    "towards the light": (nr.tilted(30.0, 0.0), WL),
    "away from the light": (nr.tilted(30.0, 180.0), WL),
    "handed in negated": (-nr.tilted(30.0, 0.0), WL),
    "handed in seven times as long": (7.0 * nr.tilted(30.0, 180.0), WL),
    "light above the shading hemisphere, below the plane": (nr.tilted(40.0, 0.0), np.array([0.9, 0.0, -0.1]) / np.hypot(0.9, 0.1)),
    "light above the plane, below the shading hemisphere": (nr.tilted(40.0, 180.0), np.array([0.95, 0.0, 0.2]) / np.hypot(0.95, 0.2)),
}


@pytest.mark.parametrize("case", list(PLANE_CASES))
def test_one_normal_for_the_whole_plane(case):
    """rho / pi L max(0, n* . wl) to 3e-6, exactly 0 where the light is above one of the two hemispheres only (the light sample taken with
    nsf AND counted only on the geometric front side): test_normals_gpu.py's cases, settings and bar"""
    n_star, wl = PLANE_CASES[case]
    sd, _ = lit_plane_scene("distant", 16)
    sd.lights[0, 1:4] = wl
    nr.with_normal(sd, n_star)
    n_unit = sd.tri_n[0, :3].astype(np.float64)
    n_unit /= np.linalg.norm(n_unit)
    if n_unit[2] < 0:
        n_unit = -n_unit
    wl32 = sd.lights[0, 1:4].astype(np.float64)
    lit = wl32[2] > 0 and n_unit @ wl32 > 0
    want = nr.lambert_distant(sd.materials[0, 1:4], (3.0, 2.0, 1.0), n_unit, wl32) if lit else np.zeros(3)
    assert lit == ("hemisphere" not in case)
    o = orc.OracleScene(sd)
    for kw in SETTINGS:
        rgb = _rgb(o.render(spp=(2, 2), seed=9, **kw)[0])
        if lit:
            assert np.allclose(rgb, want, **BAR), (case, kw, rgb.min((0, 1)), rgb.max((0, 1)), want)
        else:
            assert (rgb == 0).all(), (case, kw, rgb.max())
    if case == "towards the light":
        assert not np.allclose(want, lit_plane_scene("distant", 16)[1], rtol=1e-2)


@pytest.mark.parametrize("theta", [20.0, 40.0, 70.0])
def test_clipped_cosine_lobe(theta):
    """a constant sky over a plane whose shading normal is tilted by theta: every sample expects rho Le (1 + cos theta) / 2 -- the light
    sample under integrator 0, light sample and bounce ray sharing it under integrator 2 (without the rule at the bounce: more)"""
    sd, full = lit_plane_scene("infinite", 16)
    nr.with_normal(sd, nr.tilted(theta, 75.0))
    p = nr.clipped_lobe_fraction(theta)
    o = orc.OracleScene(sd)
    rgb = _rgb(o.render(integrator=INTEGRATOR_PATH, max_depth=1, spp=(8, 8), seed=3)[0])
    n = 16 * 16 * 64
    m = rgb.mean((0, 1)) / full
    assert (np.abs(m - p) <= 5 * np.sqrt(p * (1 - p) / n) + 1e-6).all(), (theta, m, p)
    assert np.allclose(rgb / full, (rgb / full)[..., :1], rtol=1e-5)
    rgb = _rgb(o.render(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(8, 8), seed=3)[0])
    px = rgb[..., 1].reshape(-1) / full[1]
    se = px.std(ddof=1) / np.sqrt(px.size)
    print(f"theta {theta}: integrator 2 mean / (rho Le) = {px.mean():.5f}, expected {p:.5f}, standard error {se:.5f}")
    assert abs(px.mean() - p) <= 5 * se + 1e-3 * p, (theta, px.mean(), p, se)


def test_mirror_reflects_about_the_shading_normal():
    """Kr Le where the reflection about n* leaves on the geometric front side, exactly 0 where not"""
    sd, _ = lit_plane_scene("infinite", 16)
    sd.materials = np.array([[MIRROR, 0.9, 0.9, 0.9, 0, 0, 0]], np.float32)
    nr.with_normal(sd, nr.tilted(40.0, 30.0))
    n32 = sd.tri_n[0, :3].astype(np.float64)
    n32 /= np.linalg.norm(n32)
    o, d = nr.pixel_corner_rays(sd)
    up = nr.reflect(-d, n32)[..., 2] > 0
    agree = (up == up[0]).all(0)
    assert agree.mean() >= 0.8 and up[0][agree].any() and (~up[0][agree]).any()
    want = np.where(up[0][..., None], 0.9 * np.array([0.5, 0.25, 1.0]), 0.0)
    osc = orc.OracleScene(sd)
    for kw in (dict(integrator=INTEGRATOR_PATH, max_depth=5), dict(integrator=INTEGRATOR_PATH_MIS, max_depth=1, sampler="halton")):
        rgb = _rgb(osc.render(spp=(2, 2), seed=2, **kw)[0])
        assert np.allclose(rgb[agree], want[agree], **BAR), kw
        assert (rgb[agree & ~up[0]] == 0).all()


def test_glass_keeps_the_geometric_normal():
    """3.18: a glass triangle ignores its normals.  A glass pane with strongly tilted corner normals in front of a lit matte wall renders
    the film of the pane without normals, bit for bit (the wall and the floor carry zero normals: flat)"""
    pane = ((-1.0, 0.0, -1.0), (1.0, 0.0, -1.0), (1.0, 0.2, 1.0), (-1.0, 0.2, 1.0))
    wall = ((-3, 2, -3), (3, 2, -3), (3, 2, 3), (-3, 2, 3))
    P, idx, mat_id = quad_mesh([(pane, 1), (wall, 0)])
    sd = SceneData(P=P, idx=idx, mat_id=mat_id, materials=np.array([[MATTE, .6, .5, .4, 0, 0, 0], [GLASS, .9, .9, .9, .9, .8, .95]], np.float32),
                   mat_eta=np.array([1.5, 1.5], np.float32), lights=np.array([[LIGHT_POINT, 0.5, -1.0, 1.5, 30, 30, 30], [LIGHT_INFINITE, 0, 0, 0, .3, .3, .3]], np.float32),
                   cam_to_world=look_at((0.3, -3.0, 0.4), (0, 0, 0), (0, 0, 1))[1], fov=45.0, xres=24, yres=24).normalized()
    tri_n = np.zeros((4, 9), np.float32)
    tri_n[:2] = np.tile(nr.tilted(50.0, 20.0)[[0, 2, 1]] * [1, -1, 1], 3)  # about the pane's -y normal, tilted by 50 degrees
    with_n = dataclasses.replace(sd, tri_n=tri_n).normalized()
    for kw in (dict(integrator=INTEGRATOR_PATH, sampler="stratified"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="halton")):
        kw = dict(kw, max_depth=6, spp=(2, 2), seed=4)
        plain = _render(sd, **kw)
        assert plain[..., 1].std() > 0.01
        assert_bit_equal(_render(with_n, **kw), plain, f"glass with normals vs without, {kw}")
    # ... while the same normals on a MIRROR pane are seen
    mirror = dataclasses.replace(with_n, materials=np.array([[MATTE, .6, .5, .4, 0, 0, 0], [MIRROR, .9, .9, .9, 0, 0, 0]], np.float32)).normalized()
    flat = dataclasses.replace(mirror, tri_n=np.zeros((0, 9), np.float32)).normalized()
    assert not np.array_equal(_render(mirror, **kw), _render(flat, **kw))


@pytest.mark.parametrize("kind", ["distant", "infinite", "mesh"])
def test_zero_normals_give_the_plain_film(kind):
    """all corner normals zero = "none": the oracle's film of the scene without the record, bit for bit"""
    plain = lit_plane_scene(kind, 16)[0] if kind != "mesh" else scenes.cornell_scene(24, 24)
    sd = dataclasses.replace(plain, tri_n=np.zeros((len(plain.idx), 9), np.float32)).normalized()
    assert len(sd.tri_n) == len(sd.idx) and len(plain.tri_n) == 0
    for kw in SETTINGS[::3]:
        assert_bit_equal(_render(sd, spp=(2, 2), seed=5, **kw), _render(plain, spp=(2, 2), seed=5, **kw), f"{kind} {kw}")


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_PATH_MIS])
@pytest.mark.parametrize("name", ["cornell", "glass_sphere", "envmap"])
def test_face_normals_change_nothing_but_rounding(name, integrator):
    """every triangle carries its own float64 face normal rounded to fp32: the oracle with the record against the oracle without it, at
    twin_agreement's bar for rounding-only differences (tests/test_normals_gpu.py holds the kernel to the same)"""
    plain = {"cornell": scenes.cornell_scene, "glass_sphere": scenes.glass_sphere_scene, "envmap": scenes.envmap_scene}[name](32, 32)
    sd = dataclasses.replace(plain, tri_n=nr.face_normals(plain)).normalized()
    kw = dict(integrator=integrator, max_depth=5, spp=(4, 4), seed=7)
    ps, share, weights = twin_agreement(_render(plain, **kw), _render(sd, **kw))
    print(f"{name} integrator {integrator}: PSNR {ps:.1f} dB, {100 * share:.2f} % of the pixels within 1e-4")
    assert weights and share >= 0.99 and ps >= 90.0, (name, integrator, ps, share)


# ---- images: films ----

def _mesh_scene():
    """a small textured mesh scene: Cornell's box with two checkerboards over random corner (u, v), and a checkered sphere"""
    rng = np.random.default_rng(21)
    sd = scenes.cornell_scene(24, 21)
    plain = (sd.materials[:, 0] == MATTE) & ~(sd.materials[:, 4:7] > 0).any(1)
    tex = np.array([[0, .1, .2, .3, .8, .7, .6, 5.0, 3.0, 0.25, -0.5], [0, .9, .1, .1, .1, .9, .2, -2.5, 4.0, 0.1, 0.3]], np.float32)
    mat_tex = np.where(plain, 1 + np.arange(len(plain)) % 2, 0).astype(np.uint32)
    return dataclasses.replace(sd, textures=tex, mat_tex=mat_tex, tri_uv=rng.uniform(-1.5, 2.5, (len(sd.idx), 6)).astype(np.float32),
                               spheres=np.array([[0.0, 0.0, 0.3, 0.3, int(np.flatnonzero(plain)[0])]], np.float32)).normalized()


def test_2x2_point_images_render_the_checkerboard_film():
    """DESIGN.md 3.20's identity on the oracle: checkerboards replaced by their 2 x 2 point-sampled images -- two images in one pool, on
    triangles and on a sphere -- give the checkerboard film bit for bit; the texture is seen"""
    for make in (lambda: checker_plane_scene(32)[0], _mesh_scene):
        sd = make()
        isd = ir.with_checkers_as_images(sd)
        assert len(isd.images) == len(sd.textures) >= 1 and (isd.textures[:, 0] == 4).all()
        for kw in (dict(integrator=INTEGRATOR_PATH, sampler="stratified"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol_nd")):
            kw = dict(kw, max_depth=5, spp=(2, 2), seed=3)
            checker = _render(sd, **kw)
            assert_bit_equal(_render(isd, **kw), checker, f"2 x 2 images vs checkerboards, {kw}")
            bare = dataclasses.replace(sd, mat_tex=np.zeros(len(sd.materials), np.uint32)).normalized()
            assert not np.array_equal(_render(bare, **kw), checker)


LIGHT = np.array([3.0, 2.0, 1.0]) * 0.8 / np.pi  # lit_plane_scene("distant"): L cos / pi


def _plane_with_image(image, wrap, filt, mapping, res=64):
    sd, _ = lit_plane_scene("distant", res)
    sd.mat_tex = np.array([1], np.uint32)
    sd.textures = np.array([api.image_texture_row(0, wrap, filt, mapping)], np.float32)
    sd.images = [image]
    sd.tri_uv = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32)
    return sd.normalized()


@pytest.fixture(scope="module")
def plane_uv():
    """(u, v) of the plane under the rays through the pixel centres and corners: (5, 64, 64, 2), float64 (test_image_texture_gpu._plane_uv)"""
    o_sc = orc.OracleScene(lit_plane_scene("distant", 64)[0])
    offsets = [(0.5, 0.5), (0, 0), (1, 0), (0, 1), (1, 1)]
    out = np.zeros((5, 64, 64, 2))
    for k, (ox, oy) in enumerate(offsets):
        for py in range(64):
            for px in range(64):
                o, d = o_sc.camera_ray(px + ox, py + oy)
                t = -o[2] / d[2]
                out[k, py, px] = ((o[0] + t * d[0]) + 50) / 100, ((o[1] + t * d[1]) + 50) / 100
    return out


def test_bilinear_ramp_on_the_lit_plane(plane_uv):
    """tests/test_image_texture_gpu.py::test_bilinear_lookup_on_the_lit_plane on the oracle: an 8 x 8 image whose red is a linear ramp in u
    and green one in v, clamp, the visible part between the outer texel centres -- every channel of every pixel within 3e-6 of the range the
    closed-form ramp takes over the pixel's corner rays.  (A row flip mirrors the green ramp; the other accumulation order does not show
    here: test_image_lookup_orientation_and_accumulation_order.)"""
    i = (np.arange(8) + 0.5) / 8
    img = np.zeros((8, 8, 3), np.float32)
    img[..., 0] = (0.1 + 0.8 * i)[None, :]
    img[..., 1] = (0.2 + 0.6 * i)[::-1][:, None]
    img[..., 2] = 0.4
    mapping = (4.0, 4.0, -1.5, -1.5)
    s, t = 4.0 * plane_uv[1:, ..., 0] - 1.5, 4.0 * plane_uv[1:, ..., 1] - 1.5
    assert s.min() > 1 / 16 and s.max() < 15 / 16 and t.min() > 1 / 16 and t.max() < 15 / 16
    assert s.max() - s.min() > 0.05 and t.max() - t.min() > 0.05
    rgb = _rgb(_render(_plane_with_image(img, CLAMP, BILINEAR, mapping), integrator=INTEGRATOR_DIRECT, max_depth=1, spp=(1, 1), seed=3))
    for ch, ramp in ((0, (0.1 + 0.8 * s) * LIGHT[0]), (1, (0.2 + 0.6 * t) * LIGHT[1]), (2, np.full_like(s, 0.4) * LIGHT[2])):
        lo, hi = ramp.min(0), ramp.max(0)
        assert ((rgb[..., ch] >= lo - 3e-6) & (rgb[..., ch] <= hi + 3e-6)).all(), (ch, np.maximum(lo - rgb[..., ch], rgb[..., ch] - hi).max())
    assert rgb[..., 0].max() - rgb[..., 0].min() > 0.02 and rgb[..., 1].max() - rgb[..., 1].min() > 0.005


@pytest.mark.parametrize("wrap", [REPEAT, CLAMP, BLACK], ids=["repeat", "clamp", "black"])
def test_point_lookup_on_the_lit_plane(plane_uv, wrap):
    """a random 4 x 3 image on the lit plane at 1 spp: where the pixel's five rays agree on a texel the pixel is THAT texel's colour x
    L cos / pi to 3e-6 (float64 restatement, image_ref.point), every other pixel some texel's (black: or 0)"""
    img = ir.random_image(4, 3, 12)
    mapping = (12.0, 12.0, -5.1, -5.5)
    rgb = _rgb(_render(_plane_with_image(img, wrap, POINT, mapping), integrator=INTEGRATOR_DIRECT, max_depth=1, spp=(1, 1), seed=3))
    texel = [ir.point(img, wrap, (12.0 * uv[..., 0] - 5.1).ravel(), (12.0 * uv[..., 1] - 5.5).ravel()).reshape(64, 64, 3) for uv in plane_uv]
    uncrossed = np.all([(t == texel[0]).all(-1) for t in texel[1:]], 0)
    assert uncrossed.mean() >= 0.9
    assert (np.abs(rgb - texel[0] * LIGHT).max(-1) < 3e-6)[uncrossed].all()
    palette = [c for c in img.reshape(-1, 3).astype(np.float64)] + ([np.zeros(3)] if wrap == BLACK else [])
    assert (np.min([np.abs(rgb - c * LIGHT).max(-1) for c in palette], 0) < 3e-6).all()
    assert len({tuple(c) for c in np.round(texel[0][uncrossed], 6)}) >= 4


# ---- what the oracle does not render it refuses ----

def _create(sd, mutate=None):
    """orc_scene_create on sd's description after `mutate(desc)`; -> the handle's truth (the scene is destroyed again)"""
    l = orc.lib()
    desc = orc.SceneDesc()
    keep = api.fill_desc(desc, sd.normalized(), orc.Material, orc.Light, orc.Sphere, orc.Texture)
    if mutate:
        mutate(desc)
    h = l.orc_scene_create(C.byref(desc))
    del keep
    if h:
        l.orc_scene_destroy(h)
    return bool(h)


def _set_slot_word(desc, slot, word, value):
    C.cast(desc.textures, C.POINTER(C.c_uint32))[16 * slot + word] = value


def test_oracle_refuses_what_it_does_not_render():
    box = scenes.cornell_scene(8, 8)
    assert _create(box)

    def mat_type_4(desc):
        desc.mats[0].type = 4
    assert not _create(box, mat_type_4)  # a material type above 3
    plastic = scenes.plastic_scene(8, 8)
    assert (plastic.materials[:, 0] == PLASTIC).any() and _create(plastic)
    # an unknown slot type; the pixel filter's slot (no test hands the oracle one: refused, not ignored)
    tex = np.array([[0, .1, .2, .3, .8, .7, .6, 5.0, 3.0, 0.25, -0.5]], np.float32)
    tsd = dataclasses.replace(box, textures=tex, mat_tex=np.zeros(len(box.materials), np.uint32)).normalized()
    assert _create(tsd)
    assert not _create(tsd, lambda desc: _set_slot_word(desc, 0, 0, 5))
    assert not _create(tsd, lambda desc: _set_slot_word(desc, 0, 0, 3))
    with pytest.raises(ValueError, match="pixel filter"):
        orc.OracleScene(dataclasses.replace(box, pixel_filter="gaussian").normalized())
    # normals: accepted; a slot whose n_tris is not the scene's; a second slot
    nsd = dataclasses.replace(tsd, tri_n=nr.face_normals(tsd)).normalized()
    assert _create(nsd)  # (slot 0 the checkerboard, slot 1 the normals)
    assert not _create(nsd, lambda desc: _set_slot_word(desc, 1, 1, len(nsd.idx) - 1))

    def second_normals(desc):
        C.memmove(C.addressof(desc.textures[0]), C.addressof(desc.textures[1]), 64)
    assert not _create(nsd, second_normals)
    # a matte kd_tex that names a slot of type 1, 2 or 3
    first_matte = int(np.flatnonzero((box.materials[:, 0] == MATTE) & ~(box.materials[:, 4:7] > 0).any(1))[0])

    def kd_from(slot):
        def mutate(desc):
            desc.mats[first_matte].kd_tex = slot
        return mutate
    assert _create(dataclasses.replace(nsd, tri_uv=np.zeros((len(nsd.idx), 6), np.float32)).normalized(), kd_from(1))  # (the checkerboard: fine)
    assert not _create(nsd, kd_from(2))  # the normals' slot
    env = dataclasses.replace(scenes.envmap_scene(8, 8, sky=random_map(2, 4, 1)), textures=tex, mat_tex=np.zeros(3, np.uint32)).normalized()
    assert _create(env) and not _create(env, kd_from(2))  # the map's slot (test_oracle_glass_env.py has it too)

    def kd_from_filter(desc):
        _set_slot_word(desc, 0, 0, 3)
        desc.mats[first_matte].kd_tex = 1
    assert not _create(tsd, kd_from_filter)
    assert not _create(tsd, kd_from(2))  # ... and a slot beyond the table
    # plastic beside a map slot or a normals slot, as the product refuses it
    def plastic_mat(desc):
        desc.mats[0].type = 3
        desc.mats[0].le[:] = [.5, .5, .5]
        desc.mats[0].kd_tex = int(np.array([0.3], np.float32).view(np.uint32)[0])
    assert _create(tsd, plastic_mat) and not _create(nsd, plastic_mat) and not _create(env, plastic_mat)
    for bad in (dataclasses.replace(plastic, tri_n=nr.face_normals(plastic)).normalized(),):
        with pytest.raises(ValueError, match="plastic beside"):
            orc.OracleScene(bad)
        with pytest.raises(_lib.PbrtHipError, match="plastic"):  # (the product's own refusal of the same scene, before any device work)
            api.Scene(bad)
