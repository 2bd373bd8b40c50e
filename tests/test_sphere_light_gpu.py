"""Sphere lights on the device: sphere_light.hpp bit for bit against its host compile; one lamp over a matte floor against
the closed form Kd L (r / d)^2 cos theta_c down to r / d = 0.01 (the ratio test: a deficit is the shadow ray stopped by the light's own
sphere); films against the float64 reference of tests/sphere_light_ref.py (same random numbers) with controls that must fail; MIS against
plain light sampling; an unlisted emissive sphere against the oracle, bit for bit; routing, two ranks, the command lines; twelve random
scenes.  Films of 32 x 32 at 16 samples or smaller (the two ranks: 96 x 16)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import render_variant_table as rvt
import sphere_light_host_build as hb
import sphere_light_random as rnd
import sphere_light_ref as ref
from pbrt_amd import (INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_DISTANT, LIGHT_INFINITE, LIGHT_POINT, LIGHT_SPHERE, MATTE, SceneData, _lib, api,
                      look_at, scenes)
from util import assert_bit_equal, meets_random_scene_bar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = ("stratified", "sobol", "sobol_nd", "halton")
WIDE = (1.5, 0.75)
XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])


def _ref(sd, **kw):
    if kw.get("sampler") == "sobol_nd":
        kw = dict(kw, sobol_matrices=api.sobol_matrices())
    return ref.render(sd, **kw)


def _held(sd, kw, film, what, **ref_kw):
    ok, ps, off = meets_random_scene_bar(_ref(sd, **kw, **ref_kw), film, kw)
    print(f"{what}: PSNR {ps:.1f} dB, {off} of {film.shape[0] * film.shape[1]} pixels off at 1e-4")
    return ok


# ---- 1. the header on the device ----

def test_device_equals_the_host_compile_bit_for_bit(gpu, tmp_path):
    exe = hb.build(tmp_path)
    x = hb.all_inputs()
    assert len(x) == 69632
    assert_bit_equal(api.sphere_light_eval(x), hb.run(exe, x, tmp_path), "pbrt_hip_sphere_light_eval_device vs the host compile of sphere_light.hpp")


# ---- 2. the closed form and the ratio test ----

KD, LE, HEIGHT, RES = 0.6, (5.0, 4.0, 3.0), 10.0, 8


def _lamp_over_floor(ratio, fov=1.0, res=RES, height=HEIGHT, le=LE):
    """one lamp of radius ratio x height straight above the origin of a matte floor, seen from the side in a view of `fov` degrees that the
    floor fills; nothing else in the scene"""
    h = 50.0
    sd = SceneData(P=np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], np.float32), idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32), mat_id=np.zeros(2, np.uint16),
                   materials=np.array([[MATTE, KD, KD, KD, 0, 0, 0], [MATTE, 0, 0, 0, *le]], np.float32), spheres=np.array([[0, 0, height, ratio * height, 1]], np.float32),
                   cam_to_world=look_at((0.0, -24.0, 18.0), (0, 0, 0), (0, 0, 1))[1], fov=fov, xres=res, yres=res).normalized()
    sd.lights = np.array([api.sphere_light(sd, 0)], np.float32)
    return sd


def _closed_form_film(sd, sub=8):
    """[h, w, 3] rgb: the mean over each pixel's area (sub x sub points) of Kd L (r / d)^2 cos theta_c at the floor point the camera ray meets,
    taken from the point the estimate is made at -- kSpawnEps = 1e-4 above the floor"""
    res = int(sd.xres)
    c2w = sd.cam_to_world.astype(np.float64)
    th = float(np.float32(np.tan(float(sd.fov) * np.pi / 360.0)))
    f = (np.arange(res * sub) + 0.5) / (res * sub) * 2 - 1
    d = np.stack([*np.meshgrid(f * th, -f * th, indexing="xy"), np.ones((res * sub, res * sub))], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    t = -o[2] / d[..., 2]
    assert (t > 0).all()
    po = o + d * t[..., None] + np.array([0.0, 0.0, 1e-4])
    c, r = sd.spheres[0, :3].astype(np.float64), float(sd.spheres[0, 3])
    wc = c - po
    dist = np.linalg.norm(wc, axis=-1)
    assert (wc[..., 2] / dist > r / dist).all()  # the whole lamp above every point's horizon
    v = ref.closed_form(1.0, 1.0, r, dist, wc[..., 2] / dist)
    v = v.reshape(res, sub, res, sub).mean((1, 3))
    return v[..., None] * (KD * np.array(LE))


def _ratio_case(gpu, ratio):
    """-> (worst |film - closed form| over the pixels in standard errors, the film's mean Y over the closed form's: 1 - the deficit)"""
    sd = _lamp_over_floor(ratio)
    kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(4, 4), seed=3, sampler="stratified")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
    samples = []
    ref.render(sd, **kw, samples=samples)
    y = np.stack(samples) @ XYZ[1]
    se = y.std(0, ddof=1) / np.sqrt(len(samples))
    want = _closed_form_film(sd) @ XYZ[1]
    got = film[..., 1] / film[..., 3]
    z = np.abs(got - want) / se
    print(f"r/d {ratio:g}: worst pixel {z.max():.2f} standard errors, mean film / closed form {got.mean() / want.mean():.6f}, relative se {float((se / want).mean()):.2e}")
    return float(z.max()), float(got.mean() / want.mean())


@pytest.mark.parametrize("ratio", [0.5, 0.1, 0.03, 0.01])
def test_a_lamp_over_a_floor_meets_the_closed_form(gpu, ratio):
    z, share = _ratio_case(gpu, ratio)
    assert z <= 5.0, (ratio, z, share)


def test_the_ratio_test_below_the_asserted_range(gpu):
    """r / d = 3e-3 and 1e-3, MEASURED: the figures are DESIGN.md 3.25's floor (printed; what is asserted is that light arrives at all and
    nothing arrives that the closed form does not have -- within one part in a thousand)"""
    for ratio in (3e-3, 1e-3):
        z, share = _ratio_case(gpu, ratio)
        assert 0.5 < share < 1.001, (ratio, z, share)


# ---- 3. films against the float64 reference ----

CASES = [dict(integrator=INTEGRATOR_PATH, sampler="stratified"), dict(integrator=INTEGRATOR_DIRECT, sampler="halton"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol_nd"),
         dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="stratified", filter_width=WIDE),
         dict(integrator=INTEGRATOR_PATH, sampler="sobol", max_sample_luminance=0.1)]


@pytest.fixture(scope="module")
def lamp_box():
    return scenes.sphere_light_scene(32, 32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_films_match_the_reference(gpu, lamp_box, case):
    kw = dict(case, max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(lamp_box) as sc:
        film = sc.render(**kw)[0]
        assert sc.info()["n_lights"] == 2
    assert film[..., 1].max() > 0.5 and _held(lamp_box, kw, film, str(case)), case


def _mixed_scene():
    """the pick li and the order of the chain: a point light, the lamp, a distant light, a constant infinite light, a spot light and the emissive
    triangles of cornell_scene's ceiling light in one light table; the lamp hangs above the short block"""
    sd = scenes.cornell_scene(32, 32)
    lamp_mat = len(sd.materials)
    sd = dataclasses.replace(sd, materials=np.concatenate([sd.materials, np.array([[MATTE, 0, 0, 0, 9, 7, 4]], np.float32)]),
                             spheres=np.array([[0.45, -0.45, 0.1, 0.12, lamp_mat]], np.float32), mat_tex=np.zeros(0, np.uint32)).normalized()
    d = np.array([0.2, -0.7, 0.6])
    s1, c1 = api.spot_light((-0.6, -0.5, 0.9), (-0.35, 0.3, 0.2), (3, 3, 4), 25.0, 8.0)
    lights = [[LIGHT_POINT, 0.0, -0.8, -0.5, .3, .3, .3], api.sphere_light(sd, 0), [LIGHT_DISTANT, *(d / np.linalg.norm(d)), .2, .2, .25], [LIGHT_INFINITE, 0, 0, 0, .1, .12, .15], s1]
    return dataclasses.replace(sd, lights=np.array(lights, np.float32), spot_cones=np.array([c1], np.float32)).normalized()


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_PATH_MIS])
def test_mixed_lights_match_the_reference(gpu, integrator):
    sd = _mixed_scene()
    assert len(sd.idx) <= 40
    kw = dict(integrator=integrator, max_depth=5, spp=(4, 4), seed=12, sampler="stratified")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        assert sc.info()["n_lights"] == 7  # five explicit lights and the ceiling's two triangles
    assert _held(sd, kw, film, f"mixed lights, integrator {integrator}")
    assert not _held(sd, kw, film, "... against the area density", wrong="area")


def _plastic_floor_scene():
    """a plastic floor under the lamp: sample_light_general's sphere branch and the density a plastic bounce keeps for the hit side"""
    sd = _lamp_over_floor(0.25, fov=30.0, res=32, height=1.0)
    row, alpha = api.plastic_material((0.3, 0.3, 0.3), (0.4, 0.4, 0.4), 0.15)
    sd.materials = np.array([row, sd.materials[1].tolist()], np.float32)
    sd.mat_eta = np.array([alpha, 1.5], np.float32)
    sd.cam_to_world = look_at((0.0, -2.4, 1.1), (0, 0, 0.2), (0, 0, 1))[1]
    return sd.normalized()


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS])
def test_a_plastic_floor_under_the_lamp_matches_the_reference(gpu, integrator):
    sd = _plastic_floor_scene()
    kw = dict(integrator=integrator, max_depth=4, spp=(4, 4), seed=8, sampler="halton")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
    assert film[..., 1].max() > 0.5 and _held(sd, kw, film, f"plastic floor, integrator {integrator}")
    if integrator == INTEGRATOR_PATH_MIS:
        assert not _held(sd, kw, film, "... against a hit-side weight of 1", wrong="hit_weight")


# ---- 4. controls that must fail the same bar ----

def test_the_area_density_fails_the_bar(gpu, lamp_box):
    kw = dict(integrator=INTEGRATOR_PATH, sampler="stratified", max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(lamp_box) as sc:
        film = sc.render(**kw)[0]
    assert not _held(lamp_box, kw, film, "area density", wrong="area")


def test_a_hit_side_weight_of_one_fails_the_bar(gpu, lamp_box):
    kw = dict(integrator=INTEGRATOR_PATH_MIS, sampler="stratified", max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(lamp_box) as sc:
        film = sc.render(**kw)[0]
    assert not _held(lamp_box, kw, film, "hit-side weight 1", wrong="hit_weight")


def test_one_minus_cos_by_subtraction_fails_the_bar_at_a_small_lamp(gpu):
    sd = _lamp_over_floor(1e-3, fov=20.0, res=16, le=(5e6, 4e6, 3e6))  # (a film of order 1: the bar's 120 dB are counted from a peak of 1)
    kw = dict(integrator=INTEGRATOR_DIRECT, sampler="stratified", max_depth=5, spp=(2, 2), seed=2)
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
    assert film[..., 1].min() > 0.5 and _held(sd, kw, film, "r / d = 1e-3")
    assert not _held(sd, kw, film, "... against 1 - cos by subtraction", wrong="omc_subtract")


# ---- 5. MIS against plain light sampling ----

def test_mis_agrees_with_light_sampling_under_a_large_near_lamp(gpu):
    """r / d = 0.8: the lamp fills most of the hemisphere and the BSDF-sampled half carries most of the MIS estimate.  Integrators 0 and 2
    estimate the same radiance; the films agree within 5 standard errors (the reference's per-sample values, the two runs' added)"""
    sd = _lamp_over_floor(0.8, fov=6.0, res=8, height=1.0)
    sd.cam_to_world = look_at((0.0, -2.4, 0.45), (0, 0, 0), (0, 0, 1))[1]  # (every ray passes under the lamp and meets the floor)
    sd = sd.normalized()
    films, ses = [], []
    with gpu.Scene(sd) as sc:
        for integrator in (INTEGRATOR_PATH, INTEGRATOR_PATH_MIS):
            kw = dict(integrator=integrator, max_depth=1, spp=(4, 4), seed=7, sampler="stratified")
            film = sc.render(**kw)[0]
            samples = []
            twin = ref.render(sd, **kw, samples=samples)
            assert meets_random_scene_bar(twin, film, kw)[0]
            y = np.stack(samples) @ XYZ[1]
            films.append(film[..., 1] / film[..., 3])
            ses.append(y.std(0, ddof=1) / np.sqrt(len(samples)))
    se = np.sqrt(ses[0] ** 2 + ses[1] ** 2)
    z = np.abs(films[0] - films[1]) / se
    print(f"worst pixel {z.max():.2f} standard errors; relative se {float((se / films[0]).mean()):.3f}; the two films differ by {float(np.abs(films[0] / films[1] - 1).max()):.3f} at most")
    assert films[0].min() > 0.1 and not np.array_equal(films[0], films[1]) and z.max() <= 5.0


# ---- 6. what does not change ----

def _glass_scene_with_an_emissive_sphere():
    sd = scenes.glass_sphere_scene(32, 32)
    mats = sd.materials.copy()
    mats[5] = [MATTE, 0, 0, 0, 4, 3, 2]  # the hovering sphere: an emitter, where it was glass (the cube stays glass: the GLS kernels)
    return dataclasses.replace(sd, materials=mats).normalized()


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS])
def test_an_unlisted_emissive_sphere_renders_as_the_oracle_does(gpu, oracle, integrator):
    sd = _glass_scene_with_an_emissive_sphere()
    assert not len(sd.lights) and (sd.materials[int(sd.spheres[0, 4]), 4:7] > 0).all()
    orc = oracle.OracleScene(sd)
    with gpu.Scene(sd) as sc:
        for sampler in SAMPLERS:
            kw = dict(integrator=integrator, max_depth=5, spp=(2, 2), seed=9, sampler=sampler)
            film = sc.render(**kw)[0]
            assert film[..., 1].mean() > 0.01
            assert_bit_equal(film, orc.render(**kw)[0], f"{kw}: an unlisted emissive sphere vs the oracle")
        kw = dict(integrator=integrator, max_depth=5, spp=(2, 2), seed=9, sampler="halton")
        assert_bit_equal(sc.render_acc(WIDE, **kw)[0], orc.render_acc(WIDE, **kw)[0], "accumulators under the wide box")
    orc.close()


def test_an_unlisted_sphere_beside_a_listed_lamp_adds_nothing_under_mis(gpu):
    """two emissive spheres over a floor, ONE of them a light: under MIS a BSDF-sampled ray that lands on the other adds nothing -- what the
    reference does, and not what a reference that lists both does"""
    sd = _lamp_over_floor(0.3, fov=30.0, res=16, height=1.0)
    sd.cam_to_world = look_at((0.0, -2.4, 0.6), (0.3, 0, 0), (0, 0, 1))[1]
    sd.materials = np.concatenate([sd.materials, np.array([[MATTE, 0, 0, 0, 2, 6, 8]], np.float32)])
    sd.spheres = np.concatenate([sd.spheres, np.array([[0.9, 0.1, 0.5, 0.3, 2]], np.float32)])
    sd.mat_tex = np.zeros(0, np.uint32)
    sd = sd.normalized()
    kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=3, spp=(4, 4), seed=4, sampler="stratified")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        assert sc.info()["n_lights"] == 1
    assert _held(sd, kw, film, "one lamp listed")
    both = dataclasses.replace(sd, lights=np.array([api.sphere_light(sd, 0), api.sphere_light(sd, 1)], np.float32)).normalized()
    assert not meets_random_scene_bar(_ref(both, **kw), film, kw)[0]
    with gpu.Scene(both) as sc:
        lit = sc.render(**kw)[0]
        assert sc.info()["n_lights"] == 2
    assert _held(both, kw, lit, "both lamps listed") and lit[..., 1].sum() > film[..., 1].sum()


@pytest.mark.parametrize("max_depth", [0, 1])
def test_depth_0_and_1(gpu, lamp_box, max_depth):
    for integrator in (INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS):
        kw = dict(integrator=integrator, max_depth=max_depth, spp=(2, 2), seed=1, sampler="sobol")
        with gpu.Scene(lamp_box) as sc:
            film = sc.render(**kw)[0]
        assert _held(lamp_box, kw, film, f"max_depth {max_depth}, integrator {integrator}")
        assert film[..., 1].max() > 1.0  # the lamps themselves, seen by the camera
        if max_depth == 0:  # ... and nothing else
            assert (film[..., 1] > 0).mean() < 0.05


# ---- 7. routing and refusals ----

def test_a_matte_scene_with_a_lamp_takes_a_gls_row(gpu):
    sd = _lamp_over_floor(0.2, fov=30.0, res=32, height=1.0)
    assert (sd.materials[:, 0] == MATTE).all()
    want = dict(spheres=True, wide=False, table_sampler=False, mis=False, textured=False, glass=bool((sd.lights[:, 0] == LIGHT_SPHERE).any()), env=False, normals=False,
                counters=rvt.COUNT_NONE)
    rows = [r for r in rvt.table() if all(getattr(r, k) == v for k, v in want.items())]
    assert len(rows) == 1 and rows[0].code == 0 and rows[0].family == "x" and rows[0].glass
    kw = dict(integrator=INTEGRATOR_PATH, max_depth=5, spp=(2, 2), seed=1, sampler="stratified")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        assert film[..., 1].max() > 0.05 and _held(sd, kw, film, "a matte scene with a lamp")
        for flags in (True, "walk"):  # the counting instantiations do not exist for a GLS scene
            with pytest.raises(_lib.PbrtHipError) as e:
                sc.render(counters=flags, **kw)
            assert e.value.code == -4, str(e.value)
    # the same scene without the light row takes the counters: it is the light that moved it
    with gpu.Scene(dataclasses.replace(sd, lights=np.zeros((0, 7), np.float32))) as sc:
        assert sc.render(counters=True, **kw)[1]["camera_rays"] == 32 * 32 * 4


@pytest.mark.parametrize("beside", ["envmap", "normals"])
def test_a_lamp_beside_a_map_or_normals_is_refused(gpu, beside):
    sd = _lamp_over_floor(0.2)
    kw = dict(envmap=np.full((2, 4, 3), 0.5, np.float32)) if beside == "envmap" else dict(tri_n=np.tile(np.array([0, 0, 1], np.float32), (len(sd.idx), 3)))
    with pytest.raises(_lib.PbrtHipError) as e:
        gpu.Scene(dataclasses.replace(sd, **kw))
    assert e.value.code == -4 and "sphere light" in str(e.value)


# ---- 8. two ranks ----

def test_two_ranks_add_up(gpu):
    sd = scenes.sphere_light_scene(96, 16)
    kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(2, 2), seed=6, sampler="halton")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        parts = [sc.render(rank=r, world_size=2, **kw)[0] for r in range(2)]
        acc = sc.render_acc(WIDE, **kw)[0]
        acc_parts = [sc.render_acc(WIDE, rank=r, world_size=2, **kw)[0] for r in range(2)]
    assert all(p[..., 3].any() for p in parts) and all(a[..., 3].any() for a in acc_parts)  # (two super-tiles: each rank has one)
    assert_bit_equal(parts[0] + parts[1], film, "two ranks' films")
    assert_bit_equal(acc_parts[0] + acc_parts[1], acc, "two ranks' accumulators")


# ---- 9. through every layer ----

def test_the_command_lines_render_the_scene_file(gpu, tmp_path):
    from pbrt_amd import loader
    from pbrt_amd.build import CLI_PATH
    text = open(os.path.join(ROOT, "scenes", "sphere_light_cornell.pbrt")).read().replace("[256]", "[32]").replace('"integer pixelsamples" 64', '"integer pixelsamples" 16')
    ls = loader.load_string(text)
    assert (ls.scene.lights[:, 0] == LIGHT_SPHERE).sum() == 2 and not ls.warnings
    with gpu.Scene(ls.scene) as sc, gpu.Scene(scenes.sphere_light_scene(32, 32)) as gen:
        kw = dict(ls.render_kwargs(), seed=4)
        assert_bit_equal(gen.render(**kw)[0], sc.render(**kw)[0], "scenes.sphere_light_scene vs scenes/sphere_light_cornell.pbrt")
    scene = tmp_path / "lamps.pbrt"
    scene.write_text(text)
    for argv in ([CLI_PATH], [sys.executable, "-m", "pbrt_amd.cli"]):
        out = tmp_path / ("native.png" if argv[0] == CLI_PATH else "python.png")
        r = subprocess.run(argv + ["-v", "-o", str(out), str(scene)], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0 and "unknown" not in r.stderr, (argv, r.stderr)
        img = gpu.read_image(out)
        assert img.shape == (32, 32, 3) and img.std() > 0.02 and img.max() > 0.3


# ---- 10. random scenes ----

@pytest.mark.parametrize("seed", rnd.seeds())
def test_random_scenes_match_the_reference(gpu, seed):
    sd, kw = rnd.case(seed)
    assert (sd.lights[:, 0] == LIGHT_SPHERE).sum() >= 1 and sd.xres <= 32 and sd.yres <= 32
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
    assert _held(sd, kw, film, f"seed {seed}: {len(sd.idx)} triangles, {len(sd.spheres)} spheres, {int((sd.lights[:, 0] == LIGHT_SPHERE).sum())} lamps, {kw}"), seed
