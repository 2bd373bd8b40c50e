"""Spot lights on the device: spot_light.hpp bit for bit against its host compile; a whole-sphere spot light against the point
light it then is, and through it against the oracle, bit for bit; films against the float64 reference of tests/spot_ref.py (same random
numbers) with controls that must fail; the cone's geometry on a floor; routing, refusals, two ranks and a scene of every kind of light.
Films of 32 x 32 (the two ranks: 96 x 16), scenes of at most 40 triangles."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import render_variant_table as rvt
import spot_host_build as hb
import spot_ref as ref
from pbrt_amd import (INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_DISTANT, LIGHT_INFINITE, LIGHT_POINT, LIGHT_SPOT, MATTE, SceneData,
                      _lib, api, look_at, scenes)
from util import assert_bit_equal, meets_random_scene_bar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = ("stratified", "sobol", "sobol_nd", "halton")
WIDE = (1.5, 0.75)


def _ref(sd, **kw):
    if kw.get("sampler") == "sobol_nd":
        kw = dict(kw, sobol_matrices=api.sobol_matrices())
    return ref.render(sd, **kw)


# ---- 1. the header on the device ----

def test_device_equals_the_host_compile_bit_for_bit(gpu, tmp_path):
    exe = hb.build(tmp_path)
    x = np.concatenate([hb.domain_inputs(), hb.edge_inputs()[0]])
    assert len(x) == (1 << 16) + 4096
    assert_bit_equal(api.spot_eval_device(x), hb.run(exe, x, tmp_path), "pbrt_hip_spot_eval_device vs the host compile of spot_light.hpp")


# ---- 2. the bridge to the oracle: a spot light whose cone is the whole sphere IS the point light ----

BRIDGE_P, BRIDGE_I = (0.1, -0.2, 0.9), (3.0, 2.8, 2.5)


def _without_emitter(sd, lights, cones=()):
    """`sd` without its two emitter triangles (the sixth quad of the Cornell-style generators), lit by `lights` instead"""
    keep = np.ones(len(sd.idx), bool)
    keep[10:12] = False
    assert (sd.materials[sd.mat_id[~keep], 0] == MATTE).all() and (sd.materials[sd.mat_id[~keep], 4:7] > 0).all()  # (what is dropped is the emitter)
    return dataclasses.replace(sd, idx=sd.idx[keep], mat_id=sd.mat_id[keep], lights=np.array(lights, np.float32), spot_cones=np.array(cones, np.float32).reshape(-1, 5)).normalized()


def _bridge_pair(name):
    base = scenes.cornell_scene(32, 32) if name == "cornell" else scenes.plastic_scene(32, 32)
    point = _without_emitter(base, [[LIGHT_POINT, *BRIDGE_P, *BRIDGE_I]])
    spot = _without_emitter(base, [[LIGHT_SPOT, *BRIDGE_P, *BRIDGE_I]], [[0, 0, -1, -1, -1]])  # (an axis-aligned axis: |wi . a| <= 1 exactly)
    return point, spot


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS])
@pytest.mark.parametrize("name", ["cornell", "plastic"])
def test_a_whole_sphere_spot_light_is_the_point_light(gpu, oracle, name, integrator):
    """fall = 1 multiplies last and is exact: the film of the spot scene (the GLS kernels, sample_light_spot / sample_light_general's spot
    branch) equals the point light's (cornell: render_kernel's sample_light) and the oracle's, word for word"""
    point, spot = _bridge_pair(name)
    orc = oracle.OracleScene(point)
    with gpu.Scene(point) as a, gpu.Scene(spot) as b:
        for sampler in SAMPLERS:
            kw = dict(integrator=integrator, max_depth=5, spp=(2, 2), seed=9, sampler=sampler)
            film = b.render(**kw)[0]
            assert film[..., 1].mean() > 0.01
            assert_bit_equal(film, a.render(**kw)[0], f"{name}, {kw}: spot vs point")
            assert_bit_equal(film, orc.render(**kw)[0], f"{name}, {kw}: spot vs the oracle's point light")
        # the wide box through the accumulators, and the luminance clamp
        kw = dict(integrator=integrator, max_depth=5, spp=(2, 2), seed=9, sampler="halton")
        acc = b.render_acc(WIDE, **kw)[0]
        assert_bit_equal(acc, a.render_acc(WIDE, **kw)[0], f"{name}: accumulators under the wide box, spot vs point")
        assert_bit_equal(acc, orc.render_acc(WIDE, **kw)[0], f"{name}: accumulators under the wide box, spot vs the oracle")
        kw = dict(kw, max_sample_luminance=0.05)
        film = b.render(**kw)[0]
        assert_bit_equal(film, a.render(**kw)[0], f"{name}: clamped, spot vs point")
        assert_bit_equal(film, orc.render(**kw)[0], f"{name}: clamped, spot vs the oracle")
    orc.close()


# ---- 3. films against the float64 reference ----

CASES = [dict(integrator=INTEGRATOR_PATH, sampler="stratified"), dict(integrator=INTEGRATOR_DIRECT, sampler="halton"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol_nd"),
         dict(integrator=INTEGRATOR_PATH_MIS, sampler="stratified", filter_width=WIDE), dict(integrator=INTEGRATOR_PATH, sampler="sobol", max_sample_luminance=0.1)]


@pytest.fixture(scope="module")
def spot_box():
    return scenes.spot_scene(32, 32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_films_match_the_reference(gpu, spot_box, case):
    kw = dict(case, max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(spot_box) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(spot_box, **kw), film, kw)
    print(f"{case}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert film[..., 1].max() > 0.5 and ok, (case, ps, off)


@pytest.mark.parametrize("wrong", ["square", "axis", "none"])
def test_a_wrong_reference_fails_the_same_bar(gpu, spot_box, wrong):
    """delta^2 in delta^4's place, the axis negated, the falloff dropped"""
    kw = dict(integrator=INTEGRATOR_PATH, sampler="stratified", max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(spot_box) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(spot_box, **kw, wrong=wrong), film, kw)
    print(f"{wrong}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert not ok


# ---- 4. the cone on a floor ----

def test_the_cone_on_a_floor(gpu):
    """One spot light 2 above a matte floor, aimed straight down, half angle 30 degrees with the falloff over the outer 10, direct lighting:
    a pixel whose floor point lies outside the cone by more than one pixel's angle is exactly 0, one inside the full-intensity cone by more
    than that equals the point light's pixel bit for bit"""
    cone, delta = 30.0, 10.0
    h = 20.0
    floor = dict(P=np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], np.float32), idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32), mat_id=np.zeros(2, np.uint16),
                 materials=np.array([[MATTE, .6, .6, .6, 0, 0, 0]], np.float32), cam_to_world=look_at((0.3, -4.0, 3.0), (0, 0, 0), (0, 0, 1))[1], fov=40.0, xres=32, yres=32)
    light, cone_row = api.spot_light((0, 0, 2), (0, 0, -1), (4, 4, 4), cone, delta)
    spot = SceneData(lights=np.array([light], np.float32), spot_cones=np.array([cone_row], np.float32), **floor).normalized()
    point = SceneData(lights=np.array([[LIGHT_POINT, 0, 0, 2, 4, 4, 4]], np.float32), **floor).normalized()
    kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(2, 2), seed=3, sampler="stratified")
    with gpu.Scene(spot) as a, gpu.Scene(point) as b:
        fs, fp = a.render(**kw)[0], b.render(**kw)[0]
    # the floor points of the pixels' centres (camera rays as DESIGN.md 3.2 forms them) and their angles to the axis, float64
    c2w = spot.cam_to_world.astype(np.float64)
    th = np.tan(np.radians(spot.fov) / 2)
    px = (np.arange(32) + 0.5) / 32 * 2 - 1
    d = np.stack([*np.meshgrid(px * th, -px * th, indexing="xy"), np.ones((32, 32))], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    t = -o[2] / d[..., 2]
    assert (t > 0).all()  # every pixel sees the floor
    q = o + d * t[..., None] - np.array([0.0, 0.0, 2.0])
    ang = np.degrees(np.arccos(-q[..., 2] / np.linalg.norm(q, axis=-1)))
    pad = np.pad(ang, 1, mode="edge")
    margin = np.max([np.abs(pad[1 + dy:33 + dy, 1 + dx:33 + dx] - ang) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)  # one pixel's angle
    outside, inside = ang > cone + margin, ang < cone - delta - margin
    assert outside.sum() > 100 and inside.sum() > 20, (int(outside.sum()), int(inside.sum()))
    assert (fs[outside][:, :3] == 0).all()
    assert (fp[inside][:, 1] > 0).all()
    assert_bit_equal(fs[inside], fp[inside], "inside the full-intensity cone: the point light's pixels")
    band = (ang > cone - delta + margin) & (ang < cone - margin)
    assert band.sum() > 20 and (fs[band][:, 1] < fp[band][:, 1]).all() and (fs[band][:, 1] > 0).all()


# ---- 5. routing and refusals ----

def _matte_spot_scene():
    sd = scenes.cornell_scene(32, 32)
    light, cone = api.spot_light((0.2, -0.3, 0.9), (0, 0.1, -1), (5, 5, 5), 40.0, 8.0)
    return _without_emitter(sd, [light], [cone])


def test_a_matte_scene_with_a_spot_light_takes_a_gls_row(gpu):
    sd = _matte_spot_scene()
    assert (sd.materials[:, 0] == MATTE).all() and not len(sd.spheres)
    # what capi_render.cpp fills: the scene's `glass` switch is set by a glass or plastic material OR a spot light
    want = dict(spheres=False, wide=False, table_sampler=False, mis=False, textured=False, glass=bool((sd.lights[:, 0] == LIGHT_SPOT).any()), env=False, normals=False,
                counters=rvt.COUNT_NONE)
    rows = [r for r in rvt.table() if all(getattr(r, k) == v for k, v in want.items())]
    assert len(rows) == 1 and rows[0].code == 0 and rows[0].family == "x" and rows[0].glass
    kw = dict(integrator=INTEGRATOR_PATH, max_depth=5, spp=(2, 2), seed=1, sampler="stratified")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        ok, ps, off = meets_random_scene_bar(_ref(sd, **kw), film, kw)
        assert film[..., 1].max() > 0.05 and ok, (ps, off)
        for flags in (True, "walk"):  # the device's answer to the same question: the counting instantiations do not exist for a GLS scene
            with pytest.raises(_lib.PbrtHipError) as e:
                sc.render(counters=flags, **kw)
            assert e.value.code == -4, str(e.value)
    # the same scene under a point light takes the counters: it is the spot light that moved it
    with gpu.Scene(dataclasses.replace(sd, lights=np.array([[LIGHT_POINT, 0.2, -0.3, 0.9, 5, 5, 5]], np.float32), spot_cones=np.zeros((0, 5), np.float32))) as sc:
        assert sc.render(counters=True, **kw)[1]["camera_rays"] == 32 * 32 * 4


@pytest.mark.parametrize("beside", ["envmap", "normals"])
def test_a_spot_light_beside_a_map_or_normals_is_refused(gpu, beside):
    sd = _matte_spot_scene()
    kw = dict(envmap=np.full((2, 4, 3), 0.5, np.float32)) if beside == "envmap" else dict(tri_n=np.tile(np.array([0, 0, 1], np.float32), (len(sd.idx), 3)))
    with pytest.raises(_lib.PbrtHipError) as e:
        gpu.Scene(dataclasses.replace(sd, **kw))
    assert e.value.code == -4 and "spot" in str(e.value)


# ---- 6. two ranks ----

def test_two_ranks_add_up(gpu):
    sd = scenes.spot_scene(96, 16)
    kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(2, 2), seed=6, sampler="halton")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        parts = [sc.render(rank=r, world_size=2, **kw)[0] for r in range(2)]
        acc = sc.render_acc(WIDE, **kw)[0]
        acc_parts = [sc.render_acc(WIDE, rank=r, world_size=2, **kw)[0] for r in range(2)]
    assert all(p[..., 3].any() for p in parts) and all(a[..., 3].any() for a in acc_parts)  # (two super-tiles: each rank has one)
    assert_bit_equal(parts[0] + parts[1], film, "two ranks' films")
    assert_bit_equal(acc_parts[0] + acc_parts[1], acc, "two ranks' accumulators")


# ---- 7. a spot light beside every other kind of light ----

@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_PATH_MIS])
def test_mixed_lights_match_the_reference(gpu, integrator):
    """the pick li and the order of the chain: a point light, a spot light, a distant light, a constant infinite light, a second spot light
    and the emissive triangles of cornell_scene's ceiling light in one light table"""
    sd = scenes.cornell_scene(32, 32)
    d = np.array([0.2, -0.7, 0.6])
    s1, c1 = api.spot_light((-0.6, -0.5, 0.9), (-0.35, 0.3, 0.2), (3, 3, 4), 25.0, 8.0)
    s2, c2 = api.spot_light((0.7, -0.6, 0.8), (0.35, -0.25, -0.4), (4, 3, 2), 18.0, 5.0)
    lights = [[LIGHT_POINT, 0.0, -0.8, -0.5, .3, .3, .3], s1, [LIGHT_DISTANT, *(d / np.linalg.norm(d)), .2, .2, .25], [LIGHT_INFINITE, 0, 0, 0, .1, .12, .15], s2]
    sd = dataclasses.replace(sd, lights=np.array(lights, np.float32), spot_cones=np.array([c1, c2], np.float32)).normalized()
    assert len(sd.idx) <= 40
    kw = dict(integrator=integrator, max_depth=5, spp=(4, 4), seed=12, sampler="stratified")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        assert sc.info()["n_lights"] == 7
    ok, ps, off = meets_random_scene_bar(_ref(sd, **kw), film, kw)
    print(f"integrator {integrator}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert ok, (ps, off)
    bad, _, _ = meets_random_scene_bar(_ref(sd, **kw, wrong="none"), film, kw)
    assert not bad


# ---- 8. through every layer ----

def test_the_command_lines_render_the_scene_file(gpu, tmp_path):
    from pbrt_amd import loader
    from pbrt_amd.build import CLI_PATH
    text = open(os.path.join(ROOT, "scenes", "spot_cornell.pbrt")).read().replace("[256]", "[32]").replace('"integer pixelsamples" 64', '"integer pixelsamples" 16')
    ls = loader.load_string(text)
    assert (ls.scene.lights[:, 0] == LIGHT_SPOT).sum() == 2 and not ls.warnings
    with gpu.Scene(ls.scene) as sc, gpu.Scene(scenes.spot_scene(32, 32)) as gen:
        kw = dict(ls.render_kwargs(), seed=4)
        assert_bit_equal(gen.render(**kw)[0], sc.render(**kw)[0], "scenes.spot_scene vs scenes/spot_cornell.pbrt")
    scene = tmp_path / "spot.pbrt"
    scene.write_text(text)
    for argv in ([CLI_PATH], [sys.executable, "-m", "pbrt_amd.cli"]):
        out = tmp_path / ("native.png" if argv[0] == CLI_PATH else "python.png")
        r = subprocess.run(argv + ["-v", "-o", str(out), str(scene)], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0 and "unknown" not in r.stderr, (argv, r.stderr)
        img = gpu.read_image(out)
        assert img.shape == (32, 32, 3) and img.std() > 0.02 and img.max() > 0.3
