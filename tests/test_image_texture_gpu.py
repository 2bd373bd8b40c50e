"""Image textures for Kd on the device: the lookup kernel against the host run of the same header bit for bit; the
identity -- a scene whose checkerboards are replaced by their 2 x 2 point-sampled repeat images renders the checkerboard scene's film, the
HIP one and the oracle's, word for word -- through every group of TEX instantiations; closed forms for the point and the bilinear lookup on
a lit plane; the refusals that need a device."""
import dataclasses

import numpy as np
import pytest

from pbrt_amd import (GLASS, INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_ENVMAP, LIGHT_INFINITE, LIGHT_POINT, MATTE, MIRROR, SceneData, _lib,
                      api, look_at, scenes)

import image_ref as ref
from image_ref import BILINEAR, BLACK, CLAMP, POINT, REPEAT
from util import assert_bit_equal, checker_plane_scene, deep_tree_scene, lit_plane_scene

pytestmark = pytest.mark.gpu


# ---- the device hook computes the host hook's bits ----

def test_device_lookup_equals_host_lookup(gpu):
    """two images in one call (a wrong pool offset shows in the second), every size, wrap and filter; dyadic, random and non-finite inputs"""
    images = [ref.random_image(w, h, 100 + k) for k, (w, h) in enumerate(ref.SIZES)]
    dy = ref.dyadic_inputs(rows=9)
    for k, img in enumerate(images):
        other = images[(k + 1) % len(images)]
        for wrap in (REPEAT, CLAMP, BLACK):
            for filt in (POINT, BILINEAR):
                rnd, mapping = ref.random_inputs(50_000, 31 * k + 3 * wrap + filt)
                for uv, m in ((dy, (1.0, 1.0, 0.0, 0.0)), (rnd, mapping), (ref.non_finite_inputs(), (1.0, 1.0, 0.0, 0.0))):
                    recs = [(other, CLAMP, BILINEAR, (0.5, 2.0, 0.1, 0.2)), (img, wrap, filt, m)]
                    for which in (1, 0) if k == 0 else (1,):
                        dev = api.image_lookup_eval_device(recs, which, uv)
                        host = api.image_lookup_eval_host(recs, which, uv)
                        assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), (img.shape, wrap, filt, which, m)


# ---- the identity, as films ----

def _mesh_scene(res=32):
    """300 random triangles with two checkerboards on two of the four materials (a mirror among them), two textured spheres, a point light
    and a sky; random corner (u, v)"""
    rng = np.random.default_rng(77)
    c = rng.uniform(-1, 1, (300, 1, 3))
    P = (c + rng.uniform(-0.4, 0.4, (300, 3, 3))).reshape(-1, 3).astype(np.float32)
    mats = np.array([[MATTE, .5, .5, .5, 0, 0, 0], [MATTE, .7, .6, .5, 0, 0, 0], [MIRROR, .9, .9, .9, 0, 0, 0], [MATTE, .4, .5, .6, 0, 0, 0]], np.float32)
    tex = np.array([[0, .1, .2, .3, .8, .7, .6, 5.0, 3.0, 0.25, -0.5], [0, .9, .3, .2, .2, .4, .9, -2.5, 7.0, -0.125, 1.75]], np.float32)
    return SceneData(P=P, idx=np.arange(900, dtype=np.uint32).reshape(-1, 3), mat_id=(np.arange(300) % 4).astype(np.uint16), materials=mats,
                     mat_tex=np.array([1, 2, 0, 0], np.uint32), textures=tex, tri_uv=rng.uniform(-1.5, 2.5, (300, 6)).astype(np.float32),
                     spheres=np.array([[0.3, -0.9, 0.2, 0.35, 0], [-0.6, -0.8, -0.3, 0.3, 1]], np.float32),
                     lights=np.array([[LIGHT_POINT, 1.5, -2.0, 2.5, 9, 8, 7], [LIGHT_INFINITE, 0, 0, 0, .3, .35, .45]], np.float32),
                     cam_to_world=look_at((0.2, -3.6, 1.2), (0, 0, 0), (0, 0, 1))[1], fov=45.0, xres=res, yres=res - 3).normalized()


def _with_glass(sd):
    m = sd.materials.copy()
    m[3] = [GLASS, .9, .9, .9, .95, .9, .8]
    return dataclasses.replace(sd, materials=m, mat_eta=np.full(len(m), 1.5, np.float32)).normalized()


def _with_map(sd):
    from test_envmap_host import random_map, random_rotation
    return dataclasses.replace(sd, lights=np.concatenate([sd.lights, np.array([[LIGHT_ENVMAP, 0, 0, 0, .8, .9, 1.1]], np.float32)]), envmap=random_map(8, 16, 41),
                               envmap_world_to_light=random_rotation(17).astype(np.float32)).normalized()


def _with_normals(sd):
    rng = np.random.default_rng(3)
    e1, e2 = sd.P[sd.idx[:, 1]] - sd.P[sd.idx[:, 0]], sd.P[sd.idx[:, 2]] - sd.P[sd.idx[:, 0]]
    ng = np.cross(e1, e2).astype(np.float64)
    ng[np.linalg.norm(ng, axis=1) == 0] = (0, 0, 1)  # (a triangle that fp32 collapsed: any normal)
    tri_n = (ng[:, None, :] / np.linalg.norm(ng, axis=1)[:, None, None] + rng.uniform(-0.3, 0.3, (len(sd.idx), 3, 3))).reshape(-1, 9)
    return dataclasses.replace(sd, tri_n=tri_n.astype(np.float32)).normalized()


def _deep(res=24):
    rng = np.random.default_rng(9)
    sd = deep_tree_scene(res, res - 3, k=400)
    return dataclasses.replace(sd, textures=np.array([[0, .1, .2, .3, .8, .7, .6, 5.0, 3.0, 0.25, -0.5]], np.float32), mat_tex=np.array([1], np.uint32),
                               tri_uv=rng.uniform(-1.5, 2.5, (len(sd.idx), 6)).astype(np.float32),
                               lights=np.concatenate([sd.lights, np.array([[LIGHT_POINT, 1.5, -2.0, 2.5, 9, 8, 7]], np.float32)])).normalized()


def _c0(res=32):
    """BASELINE's C0, scenes/c0_check_sphere.pbrt with its checkerboard ground, at res x res"""
    import os
    from pbrt_amd import loader
    ls = loader.load_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "c0_check_sphere.pbrt"))
    assert (ls.scene.textures[:, 0] == 0).all() and ls.scene.mat_tex.max() == 1
    return dataclasses.replace(ls.scene, xres=res, yres=res).normalized()


PATH = dict(integrator=INTEGRATOR_PATH, max_depth=5, spp=(2, 2), seed=3)
# (name, scene, how the films are made, render arguments, builder): one case per group of instantiations that has TEX
CASES = {
    "plane": (lambda: checker_plane_scene(32)[0], "film", PATH, None),
    "mesh": (_mesh_scene, "film", PATH, None),
    "c0": (lambda: _c0(), "film", PATH, None),
    "direct": (_mesh_scene, "film", dict(PATH, integrator=INTEGRATOR_DIRECT), None),
    "mis": (_mesh_scene, "film", dict(PATH, integrator=INTEGRATOR_PATH_MIS), None),
    "sobol_nd": (_mesh_scene, "film", dict(PATH, sampler="sobol_nd"), None),
    "halton_mis": (_mesh_scene, "film", dict(PATH, sampler="halton", integrator=INTEGRATOR_PATH_MIS), None),
    "wide_box": (_mesh_scene, (1.5, 0.75), PATH, None),
    "wide_box_sobol_nd": (_mesh_scene, (1.5, 0.75), dict(PATH, sampler="sobol_nd"), None),
    "gaussian": (lambda: dataclasses.replace(_mesh_scene(), pixel_filter="gaussian").normalized(), (0.0, 0.0), PATH, None),
    "glass": (lambda: _with_glass(_mesh_scene()), "film", PATH, None),
    "map": (lambda: _with_map(_mesh_scene()), "film", PATH, None),
    "map_mis": (lambda: _with_map(_mesh_scene()), "film", dict(PATH, integrator=INTEGRATOR_PATH_MIS, sampler="halton"), None),
    "normals": (lambda: _with_normals(_mesh_scene()), "film", PATH, None),
    "normals_map": (lambda: _with_map(_with_normals(_mesh_scene())), "film", PATH, None),
    "deep": (_deep, "film", PATH, "host"),
    "deep_map": (lambda: _with_map(_deep()), "film", PATH, "host"),
    "deep_normals": (lambda: _with_normals(_deep()), "film", PATH, "host"),
}


def _render(scene, how, kw):
    return scene.render(**kw)[0] if how == "film" else scene.render_acc(how, **kw)[0]


@pytest.mark.parametrize("case", list(CASES))
def test_2x2_point_images_render_the_checkerboard_film(gpu, oracle, case):
    make, how, kw, builder = CASES[case]
    sd = make()
    isd = ref.with_checkers_as_images(sd)
    assert len(isd.images) == len(sd.textures) >= 1 and (isd.textures[:, 0] == 4).all() and np.array_equal(isd.mat_tex, sd.mat_tex)
    # (the oracle is not handed the weighted filters' record: there the checkerboard scene's HIP film, which tests/test_filters_gpu.py
    # holds to its own restatement, is the reference)
    want = _render(oracle.OracleScene(sd), how, kw) if sd.pixel_filter is None else None
    with gpu.Scene(sd, builder=builder) as sc:
        checker = _render(sc, how, kw)
        if case.startswith("deep"):  # the overflow variant of the walk's stack, or the case does not reach the instantiations it is there for
            import ctypes as C
            rows, waves, beyond = C.c_uint32(), C.c_uint32(), C.c_uint32()
            assert _lib.lib().pbrt_hip_render_stack_plan(sc.info()["quad_stack_need"], C.byref(rows), C.byref(waves), C.byref(beyond)) == 0 and beyond.value > 0
    with gpu.Scene(isd, builder=builder) as sc:
        image = _render(sc, how, kw)
    if how == "film":
        assert_bit_equal(image, checker, f"{case}: the 2 x 2 images against the checkerboards (HIP)")
        if want is not None:
            assert_bit_equal(checker, want, f"{case}: the checkerboard scene against the oracle")
            assert_bit_equal(image, want, f"{case}: the 2 x 2 images against the oracle's film of the checkerboards")
            assert_bit_equal(image, oracle.OracleScene(isd).render(**kw)[0], f"{case}: the 2 x 2 images against the oracle's film of the images")
    else:
        assert want is None or np.array_equal(checker, want), f"{case}: the checkerboard scene against the oracle (accumulators)"
        assert np.array_equal(image, checker) and np.abs(image[..., 3]).sum() > 0, f"{case}: the 2 x 2 images against the checkerboards (accumulators)"
    # the texture is seen: the same scene without textures is another film
    with gpu.Scene(dataclasses.replace(sd, mat_tex=np.zeros(len(sd.materials), np.uint32)).normalized(), builder=builder) as sc:
        assert not np.array_equal(_render(sc, how, kw), image), f"{case}: the scene without its textures gives the same film"


def test_identity_on_every_visible_device(gpu, oracle):
    """the in-library multi-GPU path: the texel pool travels to every clone"""
    sd = _mesh_scene()
    isd = ref.with_checkers_as_images(sd)
    want = oracle.OracleScene(sd).render(**PATH)[0]
    with api.MultiScene(isd) as ms:
        assert ms.n_gpus == gpu.device_count()
        film, _ = ms.render(**PATH)
    assert_bit_equal(film, want, f"2 x 2 images on {gpu.device_count()} GPUs against the oracle's film of the checkerboards")
    film, _ = api.render_multi(isd, **PATH)
    assert_bit_equal(film, want, "pbrt_hip_render_multi")


def test_device_bytes_count_the_texel_pool(gpu):
    sd, _ = checker_plane_scene(16)
    isd = ref.with_checkers_as_images(sd)
    big = dataclasses.replace(isd, images=[ref.random_image(64, 32, 1)]).normalized()
    with gpu.Scene(isd) as a, gpu.Scene(big) as b:
        assert b.info()["device_bytes"] - a.info()["device_bytes"] == 16 * (64 * 32 - 4)


# ---- closed forms on the lit plane ----

LIGHT = np.array([3.0, 2.0, 1.0]) * 0.8 / np.pi  # util.lit_plane_scene("distant"): L cos / pi


def _plane_with_image(image, wrap, filt, mapping, res=64):
    sd, _ = lit_plane_scene("distant", res)
    sd.mat_tex = np.array([1], np.uint32)
    sd.textures = np.array([api.image_texture_row(0, wrap, filt, mapping)], np.float32)
    sd.images = [image]
    sd.tri_uv = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32)  # (as util.checker_plane_scene: u = (x + 50) / 100, v = (y + 50) / 100)
    return sd.normalized()


def _plane_uv(oracle, res, offsets):
    """(u, v) of the plane under the rays through pixel + offset, for every pixel: (len(offsets), res, res, 2), float64"""
    o_sc = oracle.OracleScene(lit_plane_scene("distant", res)[0])  # (the camera alone: these closed forms do not go through the oracle's image lookup)
    out = np.zeros((len(offsets), res, res, 2))
    for k, (ox, oy) in enumerate(offsets):
        for py in range(res):
            for px in range(res):
                o, d = o_sc.camera_ray(px + ox, py + oy)
                t = -o[2] / d[2]
                out[k, py, px] = ((o[0] + t * d[0]) + 50) / 100, ((o[1] + t * d[1]) + 50) / 100
    return out


@pytest.fixture(scope="module")
def plane_uv(oracle):
    return _plane_uv(oracle, 64, [(0.5, 0.5), (0, 0), (1, 0), (0, 1), (1, 1)])


# "borders": texel borders where checker_plane_scene's cell borders fall (su = 7 / 4, sv = 7 / 3, the deltas scaled alike): the frame holds
# the image's last column and row and what lies beyond them.  "finer": two columns, two rows and what lies beyond the last column.
PLANE_MAPPINGS = {"borders": (7.0 / 4, 7.0 / 3, 0.25 / 4, -0.5 / 3), "finer": (12.0, 12.0, -5.1, -5.5)}


@pytest.mark.parametrize("which", list(PLANE_MAPPINGS))
@pytest.mark.parametrize("wrap", [REPEAT, CLAMP, BLACK], ids=["repeat", "clamp", "black"])
def test_point_lookup_on_the_lit_plane(gpu, plane_uv, wrap, which):
    """a random 4 x 3 image on util.lit_plane_scene("distant"), 1 spp: every pixel is some texel's colour x L cos / pi to 3e-6 (black: or
    0), and at least 0.9 of them the texel under the pixel centre's ray -- which the geometry allows: the numpy expectation alone says how
    many pixels a border crosses"""
    img = ref.random_image(4, 3, 12)
    mapping = PLANE_MAPPINGS[which]
    with gpu.Scene(_plane_with_image(img, wrap, POINT, mapping)) as sc:
        rgb = gpu.film_to_rgb(sc.render(integrator=INTEGRATOR_DIRECT, max_depth=1, spp=(1, 1), seed=3)[0]).astype(np.float64)
    su, sv, du, dv = mapping
    texel = [ref.point(img, wrap, (su * uv[..., 0] + du).ravel(), (sv * uv[..., 1] + dv).ravel()).reshape(64, 64, 3) for uv in plane_uv]
    uncrossed = np.all([(t == texel[0]).all(-1) for t in texel[1:]], 0)
    assert uncrossed.mean() >= 0.9, uncrossed.mean()  # the geometry allows it
    palette = [c for c in img.reshape(-1, 3).astype(np.float64)] + ([np.zeros(3)] if wrap == BLACK else [])
    nearest = np.min([np.abs(rgb - c * LIGHT).max(-1) for c in palette], 0)
    assert (nearest < 3e-6).all(), ("a pixel that is no texel's colour", nearest.max())
    agree = (np.abs(rgb - texel[0] * LIGHT).max(-1) < 3e-6).mean()
    assert agree >= 0.9, agree
    shown = {tuple(c) for c in np.round(texel[0].reshape(-1, 3), 6)}
    # what the frame holds: "borders" one texel and the wrap's own region beyond it (clamp: the same texel again); "finer" four texels and
    # beyond them the first column again (repeat), the last one (clamp) or black
    assert len(shown) >= {REPEAT: 2, CLAMP: 1, BLACK: 2}[wrap] if which == "borders" else len(shown) == {REPEAT: 6, CLAMP: 4, BLACK: 5}[wrap], len(shown)


def test_bilinear_lookup_on_the_lit_plane(gpu, plane_uv):
    """an 8 x 8 image, red a linear ramp in u, green a linear ramp in v, blue constant, clamp; the mapping keeps the visible part between the
    outer texel centres, where bilinear interpolation reproduces a linear ramp exactly: at 1 spp every channel of every pixel lies within
    3e-6 of the range the closed-form ramp takes over the pixel's four corner rays"""
    i = (np.arange(8) + 0.5) / 8
    img = np.zeros((8, 8, 3), np.float32)
    img[..., 0] = (0.1 + 0.8 * i)[None, :]        # red: along u
    img[..., 1] = (0.2 + 0.6 * i)[::-1][:, None]  # green: along v, row 0 of the array is the TOP (v near 1)
    img[..., 2] = 0.4
    mapping = (4.0, 4.0, -1.5, -1.5)
    s, t = 4.0 * plane_uv[1:, ..., 0] - 1.5, 4.0 * plane_uv[1:, ..., 1] - 1.5
    assert s.min() > 1 / 16 and s.max() < 15 / 16 and t.min() > 1 / 16 and t.max() < 15 / 16  # between the outer texel centres
    assert s.max() - s.min() > 0.05 and t.max() - t.min() > 0.05  # ... and the ramps are seen
    with gpu.Scene(_plane_with_image(img, CLAMP, BILINEAR, mapping)) as sc:
        rgb = gpu.film_to_rgb(sc.render(integrator=INTEGRATOR_DIRECT, max_depth=1, spp=(1, 1), seed=3)[0]).astype(np.float64)
    # (the image's texels are fp32 roundings of the ramp: 6e-8 of the 3e-6)
    for ch, ramp in ((0, (0.1 + 0.8 * s) * LIGHT[0]), (1, (0.2 + 0.6 * t) * LIGHT[1]), (2, np.full_like(s, 0.4) * LIGHT[2])):
        lo, hi = ramp.min(0), ramp.max(0)
        assert ((rgb[..., ch] >= lo - 3e-6) & (rgb[..., ch] <= hi + 3e-6)).all(), (ch, np.maximum(lo - rgb[..., ch], rgb[..., ch] - hi).max())
    assert rgb[..., 0].max() - rgb[..., 0].min() > 0.02 and rgb[..., 1].max() - rgb[..., 1].min() > 0.005


# ---- refusals that need a device ----

def test_counter_flags_are_refused_for_an_image_textured_scene(gpu):
    sd, _ = checker_plane_scene(16)
    with gpu.Scene(ref.with_checkers_as_images(sd)) as sc:
        for bad in (dict(counters=True), dict(counters="walk")):
            with pytest.raises(_lib.PbrtHipError) as e:
                sc.render(max_depth=3, spp=(1, 1), seed=1, **bad)
            assert e.value.code == -4 and "textured" in str(e.value)


def test_demo_scenes_render(gpu):
    """scenes/textured_cornell.pbrt and its twin in arrays hold the same image (to the PNG's 8 bits) and records and render alike, and the planks are seen: the mean colour in their place is another film"""
    import os
    from pbrt_amd import loader
    ls = loader.load_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "textured_cornell.pbrt"))
    sd = dataclasses.replace(ls.scene, xres=48, yres=48).normalized()
    kw = dict(ls.render_kwargs(), spp=(2, 2), seed=1)
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
    twin = scenes.textured_cornell_scene(48, 48)
    assert np.abs(twin.images[0] - sd.images[0]).max() < 0.01 and np.array_equal(twin.textures, sd.textures)  # (the PNG's 8 bits between them)
    with gpu.Scene(twin) as sc:
        assert np.abs(gpu.film_to_rgb(sc.render(**kw)[0]) - gpu.film_to_rgb(film)).mean() < 0.02
    flat = dataclasses.replace(sd, mat_tex=np.zeros(len(sd.materials), np.uint32)).normalized()
    with gpu.Scene(flat) as sc:
        plain = sc.render(**kw)[0]
    assert np.isfinite(film).all() and not np.array_equal(film, plain)
