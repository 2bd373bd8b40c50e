"""Glass and the environment map (3.17) inside the bit-exact contract: the HIP film against the CPU oracle's, word for
word -- every comparison with the oracle is assert_bit_equal (np.array_equal for accumulators), none has a tolerance.  (A few edge tests
also make sure their SCENE shows what it was built for -- the pane darkens the floor, the lamp is in the frame, the camera sees the polar
row --: checks of the set-up with generous margins, not parity bounds.)  Three parts: the instantiation grid (one small scene per geometry class, crossed with
integrator, sampler, textures and film path, so that the `GLS` instantiations of render_kernel_x and those of render_kernel_env each produce
pixels a test looks at), one small test per edge of the two features, and random scenes (util.random_glass_env_case; widened by
tools/soak.sh).  The library has no hook that names the kernel a render launched, so the grid asserts what the issue allows instead: the
same scene with its glass turned into mirrors, or its map into the constant sky of the map's mean, gives ANOTHER film -- the glass / map code
ran and is seen --, for every render of the grid: each sampler, the wide filter's accumulators and the clamped film.  (The scene without
primitives cannot show glass, whatever is rendered: no ray meets a surface.  There the scene's glass flag alone selects the instantiation,
capi_render.cpp render_launch, the comparison with the oracle says that the `GLS` kernel leaves an empty scene alone, and only the map's negative
control applies.)"""
import dataclasses
import os

import numpy as np
import pytest

from pbrt_amd import (GLASS, INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_ENVMAP, LIGHT_INFINITE, LIGHT_POINT, MATTE, MIRROR,
                      SceneData, look_at, scenes)
from test_envmap_host import random_map, random_rotation, sun_map
from util import (GRID_MATS, M_GLASS, M_LAMP, M_MATTE, M_MIRROR, assert_bit_equal, case_holds_glass, case_holds_map, deep_tree_scene,
                  meets_random_scene_bar, random_glass_env_case, sphere_cloud_scene, twin_render)
from util import cube_faces as _cube, glass_room_scene as _room, quad_corners as _quad

pytestmark = pytest.mark.gpu

SAMPLERS = ("stratified", "sobol", "sobol_nd", "halton")
WIDE = (1.5, 0.75)
GRID_MAP, GRID_ROTATION = random_map(8, 16, 41), random_rotation(17).astype(np.float32)


# ---- the instantiation grid ----

GRID_ETA = np.array([1.5, 1.5, 1.5, 1.5], np.float32)
GRID_LIGHTS = np.array([[LIGHT_POINT, 1.5, -2.0, 2.5, 9, 8, 7], [LIGHT_INFINITE, 0, 0, 0, .3, .35, .45]], np.float32)


def _grid_scene(kind, res=24):
    """one fixed small scene per geometry class, each holding a glass material, a mirror and a matte"""
    rng = np.random.default_rng(5)
    cam = look_at((0.2, -3.6, 1.2), (0, 0, 0), (0, 0, 1))[1]
    common = dict(materials=GRID_MATS, mat_eta=GRID_ETA, lights=GRID_LIGHTS, cam_to_world=cam, fov=45.0, xres=res, yres=res - 3)
    if kind == "tris17":  # 14 random triangles, a floor, an emitter above
        c = rng.uniform(-1, 1, (14, 1, 3))
        P = (c + rng.uniform(-0.6, 0.6, (14, 3, 3))).reshape(-1, 3)
        fl, fi = _quad((-3, -3, -1.2), (3, -3, -1.2), (3, 3, -1.2), (-3, 3, -1.2))
        P = np.concatenate([P, fl, [(-0.5, -0.5, 2.0), (-0.5, 0.5, 2.0), (0.5, 0.0, 2.0)]]).astype(np.float32)
        idx = np.concatenate([np.arange(42).reshape(-1, 3), np.array(fi) + 42, [[46, 47, 48]]]).astype(np.uint32)
        mat_id = np.array([M_GLASS, M_MIRROR, M_MATTE] * 4 + [M_GLASS, M_GLASS] + [M_MATTE, M_MATTE, M_LAMP], np.uint16)
        assert len(idx) == 17
        return SceneData(P=P, idx=idx, mat_id=mat_id, **common).normalized()
    if kind in ("deep", "deep_sph"):  # the deep stacks (the overflow variant of the walk's stack); deep_sph: with three spheres, SPH beside it
        sd = deep_tree_scene(res, res - 3, k=400)
        sph = np.array([[0.15, 0.05, 0.8, 0.08, M_GLASS], [0.45, 0.1, 0.7, 0.07, M_MIRROR], [0.3, -0.05, 0.9, 0.06, M_MATTE]], np.float32)
        return dataclasses.replace(sd, materials=GRID_MATS, mat_eta=GRID_ETA, mat_tex=np.zeros(0, np.uint32), mat_id=(np.arange(400) % 3).astype(np.uint16),
                                   spheres=sph if kind == "deep_sph" else sd.spheres, lights=np.concatenate([sd.lights, GRID_LIGHTS[:1]])).normalized()
    if kind == "spheres":  # SPH: 200 spheres, 64 triangles and the ceiling lamp of the random-mesh scene WITHOUT its box (the sky shows); every
        sd = sphere_cloud_scene(200, res, res - 3)  # fifth material is a mirror already, the next one becomes glass
        mats, eta = sd.materials.copy(), np.full(len(sd.materials), 1.5, np.float32)
        for i in range(1, 250, 5):
            mats[i] = [GLASS, .9, .9, .9, .95, .9, .8]
            eta[i] = (1.33, 1.5, 2.4)[i % 3]
        keep = np.r_[0:64, 76:78]  # (12 box triangles follow the 64 random ones)
        return dataclasses.replace(sd, materials=mats, mat_eta=eta, idx=sd.idx[keep], mat_id=sd.mat_id[keep], lights=GRID_LIGHTS).normalized()
    if kind == "tri1":  # one glass triangle in front of the camera
        return SceneData(P=np.array([(-1.5, 0, -1), (1.5, 0.3, -1), (0, -0.2, 1.5)], np.float32), idx=np.array([[0, 1, 2]], np.uint32),
                         mat_id=np.array([M_GLASS], np.uint16), **common).normalized()
    assert kind == "empty"
    return SceneData(**common).normalized()


GRID_KINDS = ("tris17", "deep", "spheres", "deep_sph", "tri1", "empty")


def _builder(kind):
    """the deep scenes on the host builder's tree (whose depth the scene was made for), the others on the library's default"""
    return "host" if kind.startswith("deep") else None


def _check_stack_variant(sc, kind):
    """The walk's stack variant is chosen from the tree's stack bound (device_types.h render_stack_plan, asked through the library's own
    pbrt_hip_render_stack_plan: entries beyond the LDS rows = the overflow variant): the two deep scenes must take it and the others must
    not, or the grid does not reach the instantiations it is there for"""
    import ctypes as C
    from pbrt_amd import _lib
    need = sc.info()["quad_stack_need"]
    rows, waves, beyond = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert _lib.lib().pbrt_hip_render_stack_plan(need, C.byref(rows), C.byref(waves), C.byref(beyond)) == 0
    assert (beyond.value > 0) == kind.startswith("deep"), (kind, need, rows.value, beyond.value)


def _textured(sd):
    """a checkerboard as the Kd of every matte material that does not emit, over random corner (u, v)"""
    rng = np.random.default_rng(9)
    plain = (sd.materials[:, 0] == MATTE) & ~(sd.materials[:, 4:7] > 0).any(1)
    return dataclasses.replace(sd, textures=np.array([[0, .1, .2, .3, .8, .7, .6, 5.0, 3.0, 0.25, -0.5]], np.float32), mat_tex=plain.astype(np.uint32),
                               tri_uv=rng.uniform(-1.5, 2.5, (len(sd.idx), 6)).astype(np.float32)).normalized()


def _with_map(sd):
    return dataclasses.replace(sd, lights=np.concatenate([sd.lights, np.array([[LIGHT_ENVMAP, 0, 0, 0, .8, .9, 1.1]], np.float32)]), envmap=GRID_MAP,
                               envmap_world_to_light=GRID_ROTATION).normalized()


def _glass_as_mirror(sd):
    m = sd.materials.copy()
    g = m[:, 0] == GLASS
    m[g, 0], m[g, 4:7] = MIRROR, 0
    return dataclasses.replace(sd, materials=m).normalized()


def _map_as_constant(sd):
    w = np.sin((np.arange(sd.envmap.shape[0]) + 0.5) * np.pi / sd.envmap.shape[0])[:, None, None]
    mean = (sd.envmap.astype(np.float64) * w).sum((0, 1)) / (w.sum() * sd.envmap.shape[1])
    lights = sd.lights.copy()
    k = int(np.flatnonzero(lights[:, 0] == LIGHT_ENVMAP)[0])
    lights[k, 0], lights[k, 4:7] = LIGHT_INFINITE, lights[k, 4:7] * mean
    return dataclasses.replace(sd, lights=lights, envmap=np.zeros((0, 0, 3), np.float32)).normalized()


@pytest.mark.parametrize("textures", [False, True], ids=["plain", "textured"])
@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS])
@pytest.mark.parametrize("kind", GRID_KINDS)
def test_glass_grid(gpu, oracle, kind, integrator, textures):
    """render_kernel_x<..., GLS>: four samplers x {default film, the wide box filter (1.5, 0.75) through the accumulators, luminance clamp 1}"""
    sd = _grid_scene(kind)
    if textures:
        sd = _textured(sd)
    o = oracle.OracleScene(sd)
    base = dict(integrator=integrator, max_depth=6, spp=(2, 2), seed=3)
    films = {}
    with gpu.Scene(sd, builder=_builder(kind)) as sc:
        _check_stack_variant(sc, kind)
        for sampler in SAMPLERS:
            kw = dict(base, sampler=sampler)
            films[sampler, "film"] = sc.render(**kw)[0]
            assert_bit_equal(films[sampler, "film"], o.render(**kw)[0], f"{kind} {kw}")
            films[sampler, "wide"] = sc.render_acc(WIDE, **kw)[0]
            assert np.array_equal(films[sampler, "wide"], o.render_acc(WIDE, **kw)[0]), f"{kind} {kw}: accumulators under box filter {WIDE}"
            kw["max_sample_luminance"] = 1.0
            films[sampler, "clamp"] = sc.render(**kw)[0]
            assert_bit_equal(films[sampler, "clamp"], o.render(**kw)[0], f"{kind} {kw}")
    if kind != "empty":  # the glass is seen in every one of the twelve renders: as mirrors the scene is another film (module docstring)
        with gpu.Scene(_glass_as_mirror(sd), builder=_builder(kind)) as sc:
            for sampler in SAMPLERS:
                kw = dict(base, sampler=sampler)
                assert not np.array_equal(sc.render(**kw)[0], films[sampler, "film"]), f"{kind} {kw}: glass as mirrors gives the same film"
                assert not np.array_equal(sc.render_acc(WIDE, **kw)[0], films[sampler, "wide"]), f"{kind} {kw}: glass as mirrors gives the same accumulators"
                kw["max_sample_luminance"] = 1.0
                assert not np.array_equal(sc.render(**kw)[0], films[sampler, "clamp"]), f"{kind} {kw}: glass as mirrors gives the same clamped film"


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS])
@pytest.mark.parametrize("kind", GRID_KINDS)
def test_map_grid(gpu, oracle, kind, integrator):
    """render_kernel_env: a 16 x 8 HDR map under a random rotation beside the scene's other lights, four samplers x textures off / on"""
    plain = _with_map(_grid_scene(kind))
    base = dict(integrator=integrator, max_depth=6, spp=(2, 2), seed=4)
    for sd in (plain, _textured(plain)):
        o = oracle.OracleScene(sd)
        films = {}
        with gpu.Scene(sd, builder=_builder(kind)) as sc:
            _check_stack_variant(sc, kind)
            for sampler in SAMPLERS:
                kw = dict(base, sampler=sampler)
                films[sampler] = sc.render(**kw)[0]
                assert_bit_equal(films[sampler], o.render(**kw)[0], f"{kind} under the map, textures {sd is not plain}, {kw}")
        with gpu.Scene(_map_as_constant(sd), builder=_builder(kind)) as sc:  # the map is seen in every render: its mean as a constant sky is another film
            for sampler in SAMPLERS:
                kw = dict(base, sampler=sampler)
                assert not np.array_equal(sc.render(**kw)[0], films[sampler]), f"{kind} {kw}, textures {sd is not plain}: the map's mean as a constant gives the same film"


# ---- edges ----

def _check(gpu, oracle, sd, what, builder=None, **kw):
    ref = oracle.OracleScene(sd).render(**kw)[0]
    with gpu.Scene(sd, builder=builder) as sc:
        film = sc.render(**kw)[0]
    assert_bit_equal(film, ref, f"{what} {kw}")
    return film


def _glass_box(res=32, **change):
    sd = scenes.glass_sphere_scene(res, res)
    mats, eta = sd.materials.copy(), sd.mat_eta.copy()
    for k, v in change.items():
        for row in (4, 5):  # the cube's and the ball's glass
            if k == "eta":
                eta[row] = v
            elif k == "kr":
                mats[row, 1:4] = v
            elif k == "kt":
                mats[row, 4:7] = v
    return dataclasses.replace(sd, materials=mats, mat_eta=eta).normalized()


@pytest.mark.parametrize("max_depth", [0, 1, 2, 12])
def test_depths(gpu, oracle, max_depth):
    """the depth rule around glass (a ray at the limit is traced after a specular bounce), and the roulette after it (depth 12)"""
    for integrator in (INTEGRATOR_PATH, INTEGRATOR_PATH_MIS):
        _check(gpu, oracle, _glass_box(), "glass box", integrator=integrator, max_depth=max_depth, spp=(2, 2), seed=max_depth, sampler=SAMPLERS[max_depth % 4])


@pytest.mark.parametrize("eta", [1.0, 16.0])
def test_eta_at_its_limits(gpu, oracle, eta):
    _check(gpu, oracle, _glass_box(eta=eta), f"eta {eta}", max_depth=8, spp=(2, 2), seed=1)
    _check(gpu, oracle, _glass_box(eta=eta), f"eta {eta}", integrator=INTEGRATOR_PATH_MIS, max_depth=8, spp=(2, 2), seed=1, sampler="halton")


@pytest.mark.parametrize("which", ["kt", "kr"])
def test_zero_weight_ends_the_path(gpu, oracle, which):
    """Kt = 0 / Kr = 0: the branch taken leaves beta = 0 and the path stops there -- no further request is made"""
    sd = _glass_box(**{which: 0.0})
    a = _check(gpu, oracle, sd, f"{which} = 0", max_depth=8, spp=(2, 2), seed=2)
    _check(gpu, oracle, sd, f"{which} = 0", max_depth=8, spp=(2, 2), seed=2, sampler="sobol_nd", integrator=INTEGRATOR_PATH_MIS)
    assert not np.array_equal(a, _check(gpu, oracle, _glass_box(), "glass box", max_depth=8, spp=(2, 2), seed=2))


@pytest.mark.parametrize("shape", ["sphere", "cube"])
def test_camera_inside_glass(gpu, oracle, shape):
    """every camera ray starts inside the glass: leaving (r = eta), total internal reflection in the cube's corners"""
    if shape == "sphere":
        sd = _room(spheres=[[0.0, -0.2, 0.1, 0.7, M_GLASS]])
    else:
        sd = _room(extra_parts=_cube((-0.6, -0.8, -0.5), (0.6, 0.4, 0.7), M_GLASS))
    for kw in (dict(integrator=INTEGRATOR_PATH, sampler="stratified"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol")):
        _check(gpu, oracle, sd, f"camera inside a glass {shape}", max_depth=10, spp=(2, 2), seed=8, **kw)


def test_glass_quad_wound_away_from_the_camera(gpu, oracle):
    """the camera looks at the BACK of the quad: cos_o < 0, so the first interface is a leaving one"""
    for flip in (False, True):
        q = ((-0.8, 1.0, -0.6), (0.9, 1.0, -0.6), (0.9, 1.2, 0.9), (-0.8, 1.2, 0.9))
        sd = _room(extra_parts=[(q[::-1] if flip else q, M_GLASS)])
        _check(gpu, oracle, sd, f"glass quad, flipped {flip}", max_depth=6, spp=(2, 2), seed=3, sampler="halton")


def test_glass_pane_occludes_the_shadow_ray(gpu, oracle):
    """a pane between a point light and the floor: glass occludes shadow rays (no caustics by light sampling), the floor under it is dark but
    for what refracts through"""
    pane = ((-1.0, -1.0, 0.5), (1.0, -1.0, 0.5), (1.0, 1.0, 0.5), (-1.0, 1.0, 0.5))
    mats = GRID_MATS.copy()
    mats[M_LAMP, 4:7] = 0
    sd = _room(extra_parts=[(pane, M_GLASS)], lights=[[LIGHT_POINT, 0, 0, 1.5, 20, 20, 20]], eye=(0, -1.9, -0.5), look=(0, 0, -2), mats=mats)
    lit = _check(gpu, oracle, sd, "pane under a point light", integrator=INTEGRATOR_DIRECT, max_depth=1, spp=(2, 2), seed=1)
    bare = dataclasses.replace(sd, idx=sd.idx[:-2], mat_id=sd.mat_id[:-2]).normalized()
    open_ = _check(gpu, oracle, bare, "no pane", integrator=INTEGRATOR_DIRECT, max_depth=1, spp=(2, 2), seed=1)
    assert lit[..., 1].sum() < 0.8 * open_[..., 1].sum()
    _check(gpu, oracle, sd, "pane under a point light", max_depth=6, spp=(2, 2), seed=1, sampler="sobol_nd")


def test_emitter_seen_through_glass_under_mis(gpu, oracle):
    """emission is collected in full after a specular bounce: the ceiling emitter behind a glass pane, integrator 2"""
    pane = ((-1.5, 0.8, -1.5), (1.5, 0.8, -1.5), (1.5, 0.8, 1.95), (-1.5, 0.8, 1.95))
    sd = _room(extra_parts=[(pane, M_GLASS)], eye=(0, -1.5, 0), look=(0, 2, 1.9))
    for sampler in ("stratified", "halton"):
        film = _check(gpu, oracle, sd, "emitter through glass", integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(2, 2), seed=5, sampler=sampler)
    assert film[..., 1].max() > 4 * 4 * 0.5  # (some pixel sees the lamp, Le 5 in green, through the pane)


@pytest.mark.parametrize("name", ["1x1", "7x5", "black", "sun"])
def test_small_maps(gpu, oracle, name):
    sky = {"1x1": random_map(1, 1, 3), "7x5": random_map(5, 7, 2), "black": np.zeros((4, 8, 3), np.float32), "sun": sun_map(8, 16, 2, 5)}[name]
    sd = scenes.envmap_scene(32, 32, sky=sky, world_to_light=random_rotation(4).astype(np.float32), factor=(1.0, 0.9, 0.8))
    for integrator, sampler in ((INTEGRATOR_PATH, "stratified"), (INTEGRATOR_DIRECT, "sobol"), (INTEGRATOR_PATH_MIS, "halton")):
        _check(gpu, oracle, sd, f"map {name}", integrator=integrator, max_depth=5, spp=(2, 2), seed=6, sampler=sampler)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_camera_along_the_maps_axis(gpu, oracle, sign):
    """every camera ray within 1e-4 rad of the light-space +-z axis: sin theta == 0 in fp32, phi from two tiny numbers, the texel of row 0 /
    H - 1; and a matte floor under a map whose polar rows are the bright ones, so that light samples land where the density is 0"""
    m = random_rotation(6).astype(np.float32)
    axis = sign * m[2].astype(np.float64)  # world direction of the light's +-z: M^T (0, 0, +-1)
    sky = random_map(8, 16, 9)
    sky[0] *= 50
    sky[-1] *= 50
    up = (0, 0, 1) if abs(axis[2]) < 0.9 else (1, 0, 0)
    sd = SceneData(materials=GRID_MATS, lights=np.array([[LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32), envmap=sky, envmap_world_to_light=m,
                   cam_to_world=look_at((0, 0, 0), tuple(axis), up)[1], fov=0.01, xres=4, yres=4).normalized()
    _check(gpu, oracle, sd, f"camera along {sign:+.0f} z of the map", max_depth=2, spp=(2, 2), seed=1)
    film = _check(gpu, oracle, sd, f"camera along {sign:+.0f} z of the map", max_depth=2, spp=(1, 1), seed=1, sampler="sobol")
    # one sample per pixel: every pixel is ONE texel of the polar row (any column: phi is anything this close to the pole), nothing else
    want = sky[0 if sign > 0 else 7].astype(np.float64) @ np.array([0.212671, 0.715160, 0.072169])
    assert np.isclose(film[..., 1].astype(np.float64)[..., None], want, rtol=1e-5, atol=0.0).any(-1).all()
    floor = scenes.envmap_scene(32, 32, sky=sky, world_to_light=m)
    for integrator in (INTEGRATOR_PATH, INTEGRATOR_PATH_MIS):
        _check(gpu, oracle, floor, "bright poles", integrator=integrator, max_depth=4, spp=(2, 2), seed=2, sampler="sobol")


def test_map_beside_a_constant_sky_and_a_point_light(gpu, oracle):
    sd = scenes.envmap_scene(32, 32, sky=GRID_MAP, world_to_light=GRID_ROTATION)
    sd = dataclasses.replace(sd, lights=np.concatenate([sd.lights, GRID_LIGHTS[::-1]])).normalized()
    for integrator in (INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS):
        for sampler in ("stratified", "sobol_nd"):
            _check(gpu, oracle, sd, "map + sky + point", integrator=integrator, max_depth=5, spp=(2, 2), seed=7, sampler=sampler)


def test_crop_window_and_shards(gpu, oracle):
    """a crop window; world_size 3 with the shards summed; both builders"""
    sd = scenes.envmap_scene(64, 48, crop=(0.1, 0.83, 0.25, 0.9), sky=GRID_MAP, world_to_light=GRID_ROTATION)
    gl = dataclasses.replace(scenes.glass_sphere_scene(64, 64), crop=(0.1, 0.83, 0.25, 0.9)).normalized()
    for what, s, kw in (("map", sd, dict(integrator=INTEGRATOR_PATH_MIS, sampler="halton")), ("glass", gl, dict(sampler="sobol"))):
        kw = dict(kw, max_depth=5, spp=(2, 2), seed=9)
        ref = oracle.OracleScene(s).render(**kw)[0]
        for builder in ("host", "gpu"):
            with gpu.Scene(s, builder=builder) as sc:
                assert_bit_equal(sc.render(**kw)[0], ref, f"{what}, cropped, builder {builder}")
                assert_bit_equal(sum(sc.render(rank=r, world_size=3, **kw)[0] for r in range(3)), ref, f"{what}, cropped, three shards summed")
    kw = dict(max_depth=4, spp=(2, 2), seed=9)
    with gpu.Scene(gl) as sc:
        parts = sum(sc.render_acc(WIDE, rank=r, world_size=3, **kw)[0] for r in range(3))
    assert np.array_equal(parts, oracle.OracleScene(gl).render_acc(WIDE, **kw)[0])


def _clone_scene(with_map):
    """the room of util.glass_room_scene without the wall the camera faces, on a 192 x 64 film -- three 64 x 64 super-tiles in one row, the
    smallest film on which each of 3 ranks owns a tile and renders it from its own clone --: checkered walls with their corner (u, v), a
    checkered sphere, a glass cube, a mirror sphere and, with_map, the 8 x 16 random map as the light seen through the opening"""
    sd = _room(extra_parts=_cube((-0.9, 0.6, -0.9), (-0.1, 1.3, 0.2), M_GLASS), spheres=[[0.7, 1.1, -0.3, 0.45, M_MATTE], [0.1, 1.6, 0.9, 0.4, M_MIRROR]])
    keep = np.r_[0:6, 8:len(sd.idx)]  # (util.cube_faces: triangles 6 and 7 are the wall y = 2)
    quad_uv = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32)  # (as util.checker_plane_scene)
    sd = dataclasses.replace(sd, idx=sd.idx[keep], mat_id=sd.mat_id[keep], xres=192, yres=64, mat_tex=np.array([1, 0, 0, 0], np.uint32),
                             textures=np.array([[0, .1, .2, .3, .8, .7, .6, 5.0, 3.0, 0.25, -0.5]], np.float32), tri_uv=np.tile(quad_uv, (len(keep) // 2, 1)))
    return _with_map(sd) if with_map else sd.normalized()


def test_clones_carry_every_scene_array(gpu, oracle, monkeypatch):
    """pbrt_hip_render_multi with three ranks on this GPU (PBRT_HIP_MULTI_LOOPBACK): ranks 1 and 2 render from CLONES of the scene, so their
    tiles show whether a clone carries the corner (u, v), the texture table, the glass table and the map's tables.  With the map under the
    default filter (the slabs are gathered); without it under the wide box filter and Halton (the ranks' accumulators are added).  The film
    depends on those arrays: the scene without its textures, and with its glass as mirrors, is another film."""
    for with_map in (True, False):
        sd = _clone_scene(with_map)
        kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(2, 2), seed=11)
        if not with_map:
            kw.update(sampler="halton", filter_width=WIDE)
        ref = oracle.OracleScene(sd).render(**kw)[0]
        with gpu.Scene(sd) as sc:
            film = sc.render(**kw)[0]
        assert_bit_equal(film, ref, f"one scene against the oracle {kw}")
        for what, other in (("without its textures", dataclasses.replace(sd, mat_tex=np.zeros(4, np.uint32)).normalized()), ("with its glass as mirrors", _glass_as_mirror(sd))):
            with gpu.Scene(other) as sc:
                assert not np.array_equal(sc.render(**kw)[0], film), f"the scene {what} gives the same film {kw}"
        with monkeypatch.context() as mp:
            mp.setenv("PBRT_HIP_MULTI_LOOPBACK", "1")
            three, _ = gpu.render_multi(sd, 3, **kw)
        assert_bit_equal(three, film, f"three ranks, two of them on clones {kw}")
        assert_bit_equal(three, ref, f"three ranks against the oracle {kw}")


# ---- random scenes ----

_SOAK_FIRST = int(os.environ.get("PBRT_SOAK_FIRST", "0"))


@pytest.mark.parametrize("seed", range(_SOAK_FIRST, _SOAK_FIRST + int(os.environ.get("PBRT_SOAK_SEEDS", "48"))))
def test_random_glass_and_map_scenes_match_oracle(gpu, oracle, seed):
    """util.random_glass_env_case without its cap on the primitive count (the oracle has a BVH), the builders alternating, a random rank
    split with the shards summed -- the films under the default filter, the accumulators under a wide one"""
    sd, kw = random_glass_env_case(seed, cap=False)
    world = int(np.random.default_rng(92_000 + seed).integers(1, 4))
    o = oracle.OracleScene(sd)
    what = f"random scene {seed}: glass {case_holds_glass(sd)}, map {sd.envmap.shape[:2] if case_holds_map(sd) else None}, {world} ranks, {kw}"
    with gpu.Scene(sd, builder="gpu" if seed % 2 else "host") as sc:
        if kw.get("filter_width"):
            k2 = {k: v for k, v in kw.items() if k != "filter_width"}
            parts = sum(sc.render_acc(kw["filter_width"], rank=r, world_size=world, **k2)[0] for r in range(world))
            assert np.array_equal(parts, o.render_acc(kw["filter_width"], **k2)[0]), what
        else:
            assert_bit_equal(sum(sc.render(rank=r, world_size=world, **kw)[0] for r in range(world)), o.render(**kw)[0], what)


def test_hip_equals_the_twin_on_random_glass_and_map_scenes(gpu):
    """the first 24 cases of util.random_glass_env_case, the HIP film against the float64 twin with no oracle in between:
    util.meets_random_scene_bar, unchanged"""
    done = glass = maps = 0
    seed = 0
    with np.errstate(all="ignore"):
        while done < 24:
            case = random_glass_env_case(seed)
            seed += 1
            if case is None:
                continue
            sd, kw = case
            with gpu.Scene(sd, builder="gpu" if seed % 2 else "host") as sc:
                film = sc.render(**kw)[0]
            ok, ps, off = meets_random_scene_bar(twin_render(sd, kw), film, kw)
            print(f"seed {seed - 1}: PSNR {ps:.1f} dB, {off} pixels off at 1e-4")
            assert ok, (seed - 1, ps, off, kw)
            done, glass, maps = done + 1, glass + case_holds_glass(sd), maps + case_holds_map(sd)
    assert glass >= 8 and maps >= 8, (glass, maps)
