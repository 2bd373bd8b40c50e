"""Projection and goniometric lights on the device: light_map.hpp bit for bit against its host compile; a goniometric light
with an image of ones against the point light it then is, and through it against the oracle, bit for bit; a slide on a floor; films against
the float64 reference of tests/light_map_ref.py (same random numbers) with controls that must fail; routing, refusals, two ranks and the
command lines.  Films of 32 x 32 (the two ranks: 96 x 16), scenes of at most 40 triangles."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import light_map_host_build as hb
import light_map_ref as ref
import render_variant_table as rvt
from pbrt_amd import (INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_DISTANT, LIGHT_INFINITE, LIGHT_MAPPED, LIGHT_POINT, MATTE, SceneData, _lib, api,
                      look_at, scenes)
from util import assert_bit_equal, meets_random_scene_bar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = ("stratified", "sobol", "sobol_nd", "halton")
WIDE = (1.5, 0.75)
ONES = np.ones((1, 1, 3), np.float32)


def _ref(sd, **kw):
    if kw.get("sampler") == "sobol_nd":
        kw = dict(kw, sobol_matrices=api.sobol_matrices())
    return ref.render(sd, **kw)


def _with_lights(sd, lights, maps=(), images=(), rows=(), cones=()):
    return dataclasses.replace(sd, lights=np.array(lights, np.float32), light_maps=np.array(maps, np.float32).reshape(-1, 14), images=list(images),
                               textures=np.array(rows, np.float32).reshape(-1, 11), spot_cones=np.array(cones, np.float32).reshape(-1, 5)).normalized()


def _without_emitter(sd):
    """`sd` without its two emitter triangles (the sixth quad of the Cornell-style generators)"""
    keep = np.ones(len(sd.idx), bool)
    keep[10:12] = False
    assert (sd.materials[sd.mat_id[~keep], 0] == MATTE).all() and (sd.materials[sd.mat_id[~keep], 4:7] > 0).all()  # (what is dropped is the emitter)
    return dataclasses.replace(sd, idx=sd.idx[keep], mat_id=sd.mat_id[keep])


# ---- 5. the header on the device ----

def test_device_equals_the_host_compile_bit_for_bit(gpu, tmp_path):
    exe = hb.build(tmp_path)
    cases = hb.domain_cases(hb.PROJECTION) + hb.domain_cases(hb.GONIOMETRIC) + hb.edge_cases()
    assert sum(len(c.x) for c in cases) > (2 << 16) + 3000
    for i, c in enumerate(cases):
        got = api.light_map_eval_device(c.x, c.image, c.row(), wrap=c.wrap, filter=c.filt)
        assert_bit_equal(got, hb.run(exe, c, tmp_path), f"case {i} (kind {c.kind}): pbrt_hip_light_map_eval_device vs the host compile of light_map.hpp")


# ---- 6. the bridge to the oracle: a goniometric light with an image of ones IS the point light ----

BRIDGE_P, BRIDGE_I = (0.1, -0.2, 0.9), (3.0, 2.8, 2.5)


def _bridge_pair(name):
    base = _without_emitter(scenes.cornell_scene(32, 32) if name == "cornell" else scenes.plastic_scene(32, 32))
    point = _with_lights(base, [[LIGHT_POINT, *BRIDGE_P, *BRIDGE_I]])
    light, row = api.goniometric_light(BRIDGE_P, 1, BRIDGE_I)
    mapped = _with_lights(base, [light], [row], [ONES], [api.image_texture_row(0, "repeat", "point")])
    return point, mapped


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS])
@pytest.mark.parametrize("name", ["cornell", "plastic"])
def test_a_goniometric_light_of_ones_is_the_point_light(gpu, oracle, name, integrator):
    """rgb = 1 multiplies last and is exact: the film of the mapped scene (the GLS kernels, sample_light_mapped / sample_light_general's
    mapped branch) equals the point light's (cornell: render_kernel's sample_light) and the oracle's, word for word"""
    point, mapped = _bridge_pair(name)
    orc = oracle.OracleScene(point)
    with gpu.Scene(point) as a, gpu.Scene(mapped) as b:
        for sampler in SAMPLERS:
            kw = dict(integrator=integrator, max_depth=5, spp=(2, 2), seed=9, sampler=sampler)
            film = b.render(**kw)[0]
            assert film[..., 1].mean() > 0.01
            assert_bit_equal(film, a.render(**kw)[0], f"{name}, {kw}: mapped vs point")
            assert_bit_equal(film, orc.render(**kw)[0], f"{name}, {kw}: mapped vs the oracle's point light")
        # the wide box through the accumulators, and the luminance clamp
        kw = dict(integrator=integrator, max_depth=5, spp=(2, 2), seed=9, sampler="halton")
        acc = b.render_acc(WIDE, **kw)[0]
        assert_bit_equal(acc, a.render_acc(WIDE, **kw)[0], f"{name}: accumulators under the wide box, mapped vs point")
        assert_bit_equal(acc, orc.render_acc(WIDE, **kw)[0], f"{name}: accumulators under the wide box, mapped vs the oracle")
        kw = dict(kw, max_sample_luminance=0.05)
        film = b.render(**kw)[0]
        assert_bit_equal(film, a.render(**kw)[0], f"{name}: clamped, mapped vs point")
        assert_bit_equal(film, orc.render(**kw)[0], f"{name}: clamped, mapped vs the oracle")
    orc.close()


# ---- 7. the slide on a floor ----

DOWN = [[1, 0, 0], [0, -1, 0], [0, 0, -1]]  # world_to_light of a projector that looks straight down: its +x is the world's +x, its +y the world's -y
FLOOR_FOV = 60.0


def _floor():
    h = 20.0
    return dict(P=np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], np.float32), idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32), mat_id=np.zeros(2, np.uint16),
                materials=np.array([[MATTE, .6, .6, .6, 0, 0, 0]], np.float32), cam_to_world=look_at((0.3, -4.0, 3.0), (0, 0, 0), (0, 0, 1))[1], fov=40.0, xres=32, yres=32)


def _floor_screen():
    """(px, py, margin_x, margin_y) [32, 32]: the projector's screen coordinates of the floor points under the pixels' centres (camera rays as
    DESIGN.md 3.2 forms them), float64, and how far they move over one pixel"""
    c2w = look_at((0.3, -4.0, 3.0), (0, 0, 0), (0, 0, 1))[1].astype(np.float64)
    th = np.tan(np.radians(40.0) / 2)
    g = (np.arange(32) + 0.5) / 32 * 2 - 1
    d = np.stack([*np.meshgrid(g * th, -g * th, indexing="xy"), np.ones((32, 32))], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    t = -o[2] / d[..., 2]
    assert (t > 0).all()  # every pixel sees the floor
    q = o + d * t[..., None] - np.array([0.0, 0.0, 2.0])
    w = q @ np.array(DOWN, np.float64).T
    inv_tan = 1.0 / np.tan(np.radians(FLOOR_FOV) / 2)
    px, py = w[..., 0] / w[..., 2] * inv_tan, w[..., 1] / w[..., 2] * inv_tan

    def margin(v):
        pad = np.pad(v, 1, mode="edge")
        return np.max([np.abs(pad[1 + dy:33 + dy, 1 + dx:33 + dx] - v) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    return px, py, margin(px), margin(py)


def test_the_slide_on_a_floor(gpu):
    """One projector 2 above a matte floor, aimed straight down, fov 60, direct lighting.  With an image of ones: a pixel inside the window
    by more than a pixel's extent equals the point light's bit for bit, one outside by more than that is exactly 0.  With a 2 x 2
    point-sampled image of texels that are powers of two (or 0) per channel: each quadrant of the lit square equals the film of the point
    light whose I is multiplied by the quadrant's texel -- a power of two scales exactly --, and the file's top right texel lies at the
    light's +x, +y."""
    kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(2, 2), seed=3, sampler="stratified")
    I = np.array([4.0, 4.0, 4.0])
    light, row = api.projection_light((0, 0, 2), 1, I, FLOOR_FOV, 1.0, DOWN)

    def point_film(scale):
        with gpu.Scene(SceneData(lights=np.array([[LIGHT_POINT, 0, 0, 2, *(I * scale)]], np.float32), **_floor()).normalized()) as sc:
            return sc.render(**kw)[0]
    px, py, mx, my = _floor_screen()
    inside = (np.abs(px) < 1 - mx) & (np.abs(py) < 1 - my)
    outside = (np.abs(px) > 1 + mx) | (np.abs(py) > 1 + my)
    assert inside.sum() > 40 and outside.sum() > 100, (int(inside.sum()), int(outside.sum()))
    ones = SceneData(lights=np.array([light], np.float32), light_maps=np.array([row], np.float32), images=[ONES],
                     textures=np.array([api.image_texture_row(0, "clamp", "point")], np.float32), **_floor()).normalized()
    with gpu.Scene(ones) as sc:
        f1 = sc.render(**kw)[0]
    fp = point_film(np.ones(3))
    assert (fp[inside][:, 1] > 0).all() and (f1[outside][:, :3] == 0).all()
    assert_bit_equal(f1[inside], fp[inside], "inside the window: the point light's pixels")
    # row 0 of the image is its top: t > 1/2, the light's +y; column 1 is s > 1/2, the light's +x
    quad = np.array([[[0.5, 1, 2], [2, 0.5, 0]], [[1, 2, 0.5], [0, 0, 0]]], np.float32)
    slide = dataclasses.replace(ones, images=[quad]).normalized()
    with gpu.Scene(slide) as sc:
        fq = sc.render(**kw)[0]
    for r, c in ((0, 0), (0, 1), (1, 0), (1, 1)):
        m = inside & ((px > mx) if c == 1 else (px < -mx)) & ((py > my) if r == 0 else (py < -my))
        assert m.sum() > 8, (r, c, int(m.sum()))
        assert_bit_equal(fq[m], point_film(quad[r, c].astype(np.float64))[m], f"the quadrant of texel ({r}, {c})")
        assert (fq[m][:, 1] > 0).all() == bool(quad[r, c].any())
    assert (fq[outside][:, :3] == 0).all()


# ---- 8. films against the float64 reference ----

CASES = [dict(integrator=INTEGRATOR_PATH, sampler="stratified"), dict(integrator=INTEGRATOR_DIRECT, sampler="halton"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol_nd"),
         dict(integrator=INTEGRATOR_PATH_MIS, sampler="stratified", filter_width=WIDE), dict(integrator=INTEGRATOR_PATH, sampler="sobol", max_sample_luminance=0.1)]
CONTROL_KW = dict(integrator=INTEGRATOR_PATH, sampler="stratified", max_depth=5, spp=(4, 4), seed=5)


@pytest.fixture(scope="module")
def projector_box():
    return scenes.projector_scene(32, 32)


@pytest.fixture(scope="module")
def projector_film(projector_box):
    import pbrt_amd
    with pbrt_amd.Scene(projector_box) as sc:
        return sc.render(**CONTROL_KW)[0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_films_match_the_reference(gpu, projector_box, case):
    kw = dict(case, max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(projector_box) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(projector_box, **kw), film, kw)
    print(f"{case}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert film[..., 1].max() > 0.3 and ok, (case, ps, off)


@pytest.mark.parametrize("wrong", ["flip_t", "no_swap", "no_inv_tan", "other_light"])
def test_a_wrong_reference_fails_the_same_bar(gpu, projector_box, projector_film, wrong):
    """t flipped, the goniometric swap of y and z dropped, inv_tan dropped, the image multiplied into the light behind the one that names it"""
    ok, ps, off = meets_random_scene_bar(_ref(projector_box, **CONTROL_KW, wrong=wrong), projector_film, CONTROL_KW)
    print(f"{wrong}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert not ok


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_PATH_MIS])
def test_mixed_lights_match_the_reference(gpu, integrator):
    """the pick li and the order of the chain: a point light, a projection light, a distant light, a constant infinite light, a spot light, a
    goniometric light and the emissive triangles of cornell_scene's ceiling light in one light table"""
    sd = scenes.cornell_scene(32, 32)
    d = np.array([0.2, -0.7, 0.6])
    frame = [[-1, 0, 0], [0, 0, 1], [0, 1, 0]]
    slide, gonio = scenes.procedural_slide(), scenes.procedural_gonio()
    pl, pm = api.projection_light((0.0, -0.9, 0.0), 1, (6, 6, 6), 50.0, slide.shape[1] / slide.shape[0], frame)
    gl, gm = api.goniometric_light((-0.4, 0.2, 0.5), 2, (1.5, 1.2, 1.0), frame)
    s1, c1 = api.spot_light((0.7, -0.6, 0.8), (0.35, -0.25, -0.4), (4, 3, 2), 18.0, 5.0)
    lights = [[LIGHT_POINT, 0.0, -0.8, -0.5, .3, .3, .3], pl, [LIGHT_DISTANT, *(d / np.linalg.norm(d)), .2, .2, .25], [LIGHT_INFINITE, 0, 0, 0, .1, .12, .15], s1, gl]
    sd = _with_lights(sd, lights, [pm, gm], [slide, gonio], [api.image_texture_row(0, "clamp"), api.image_texture_row(1, "repeat")], [c1])
    assert len(sd.idx) <= 40
    kw = dict(integrator=integrator, max_depth=5, spp=(4, 4), seed=12, sampler="stratified")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        assert sc.info()["n_lights"] == 8
    ok, ps, off = meets_random_scene_bar(_ref(sd, **kw), film, kw)
    print(f"integrator {integrator}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert ok, (ps, off)
    bad, _, _ = meets_random_scene_bar(_ref(sd, **kw, wrong="other_light"), film, kw)
    assert not bad


# ---- 9. routing and refusals ----

def _matte_mapped_scene():
    light, row = api.projection_light((0.0, -0.9, 0.1), 1, (8, 8, 8), 50.0, 4 / 3, [[-1, 0, 0], [0, 0, 1], [0, 1, 0]])
    return _with_lights(_without_emitter(scenes.cornell_scene(32, 32)), [light], [row], [scenes.procedural_slide()], [api.image_texture_row(0, "clamp")])


def test_a_matte_scene_with_a_mapped_light_takes_a_gls_row(gpu):
    sd = _matte_mapped_scene()
    assert (sd.materials[:, 0] == MATTE).all() and not len(sd.spheres) and not sd.mat_tex.any()
    # what capi_render.cpp fills: the scene's `glass` switch is set by a glass or plastic material, a spot light OR a mapped light; the
    # light's image makes no TEX scene of it
    want = dict(spheres=False, wide=False, table_sampler=False, mis=False, textured=False, glass=bool((sd.lights[:, 0] == LIGHT_MAPPED).any()), env=False, normals=False,
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
    # the same scene under a point light takes the counters: it is the mapped light that moved it
    with gpu.Scene(_with_lights(sd, [[LIGHT_POINT, 0.0, -0.9, 0.1, 8, 8, 8]])) as sc:
        assert sc.render(counters=True, **kw)[1]["camera_rays"] == 32 * 32 * 4


@pytest.mark.parametrize("beside", ["envmap", "normals"])
def test_a_mapped_light_beside_a_map_or_normals_is_refused(gpu, beside):
    sd = _matte_mapped_scene()
    kw = dict(envmap=np.full((2, 4, 3), 0.5, np.float32)) if beside == "envmap" else dict(tri_n=np.tile(np.array([0, 0, 1], np.float32), (len(sd.idx), 3)))
    with pytest.raises(_lib.PbrtHipError) as e:
        gpu.Scene(dataclasses.replace(sd, **kw))
    assert e.value.code == -4 and "light map" in str(e.value)


def test_two_ranks_add_up(gpu):
    sd = scenes.projector_scene(96, 16)
    kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(2, 2), seed=6, sampler="halton")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        parts = [sc.render(rank=r, world_size=2, **kw)[0] for r in range(2)]
        acc = sc.render_acc(WIDE, **kw)[0]
        acc_parts = [sc.render_acc(WIDE, rank=r, world_size=2, **kw)[0] for r in range(2)]
    assert all(p[..., 3].any() for p in parts) and all(a[..., 3].any() for a in acc_parts)  # (two super-tiles: each rank has one)
    assert_bit_equal(parts[0] + parts[1], film, "two ranks' films")
    assert_bit_equal(acc_parts[0] + acc_parts[1], acc, "two ranks' accumulators")


def test_the_command_lines_render_the_scene_file(gpu, tmp_path):
    from pbrt_amd import loader
    from pbrt_amd.build import CLI_PATH
    text = open(os.path.join(ROOT, "scenes", "projector_cornell.pbrt")).read().replace("[256]", "[32]").replace('"integer pixelsamples" 64', '"integer pixelsamples" 16')
    text = text.replace('"textures/', '"' + os.path.join(ROOT, "scenes", "textures") + "/")  # (the copy of the file lies elsewhere)
    ls = loader.load_string(text)
    assert (ls.scene.lights[:, 0] == LIGHT_MAPPED).sum() == 2 and not ls.warnings
    with gpu.Scene(ls.scene) as sc, gpu.Scene(scenes.projector_scene(32, 32)) as gen:
        kw = dict(ls.render_kwargs(), seed=4)
        assert_bit_equal(gen.render(**kw)[0], sc.render(**kw)[0], "scenes.projector_scene vs scenes/projector_cornell.pbrt")
    scene = tmp_path / "projector.pbrt"
    scene.write_text(text)
    for argv in ([CLI_PATH], [sys.executable, "-m", "pbrt_amd.cli"]):
        out = tmp_path / ("native.png" if argv[0] == CLI_PATH else "python.png")
        r = subprocess.run(argv + ["-v", "-o", str(out), str(scene)], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0 and "unknown" not in r.stderr, (argv, r.stderr)
        img = gpu.read_image(out)
        assert img.shape == (32, 32, 3) and img.std() > 0.02 and img.max() > 0.3
