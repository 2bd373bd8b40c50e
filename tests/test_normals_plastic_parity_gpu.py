"""Shading normals, plastic (3.21) and image textures (3.20) inside the bit-exact contract: the HIP film against the CPU
oracle's, word for word -- every comparison with the oracle is assert_bit_equal (np.array_equal for accumulators), none has a tolerance.
In the form of tests/test_glass_env_parity_gpu.py, whose grid scenes these are: two instantiation grids (all 64 instantiations of
render_kernel_n; the 64 `GLS` instantiations of render_kernel_x with plastic in the scene), the image cases, one small test per edge,
and random scenes (util.random_normals_plastic_case).  Films are 24 x 21 at 2 x 2 spp, depth 6.  The library has no hook that names the
kernel a render launched: each render has the negative control that the feature is SEEN (every normal zero, plastic as matte of the same
Kd, each image's mean colour as a constant: another film), and test_the_grids_reach_every_instantiation computes from
tests/render_variant_table.py which family and switches every render of the two grids selects."""
import dataclasses
import os

import numpy as np
import pytest

import image_ref as ir
import render_variant_table as rvt
from image_ref import BILINEAR, BLACK, CLAMP, POINT, REPEAT
from pbrt_amd import (INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_ENVMAP, LIGHT_INFINITE, MATTE, MIRROR, PLASTIC, SceneData, api, look_at)
from test_glass_env_parity_gpu import GRID_LIGHTS, SAMPLERS, WIDE, _builder, _check_stack_variant, _grid_scene, _textured, _with_map
from util import (GRID_MATS, M_LAMP, M_MATTE, M_MIRROR, assert_bit_equal, case_holds_map, case_holds_plastic, glass_room_scene, quad_mesh,
                  random_corner_normals, random_normals_plastic_case)

pytestmark = pytest.mark.gpu

KINDS = ("tris17", "deep", "spheres", "deep_sph")
INTEGRATORS = (INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS)
BASE = dict(max_depth=6, spp=(2, 2))


def _with_normals(sd, seed=1):
    return dataclasses.replace(sd, tri_n=random_corner_normals(sd, seed)).normalized()


def _zero_normals(sd):
    return dataclasses.replace(sd, tri_n=np.zeros_like(sd.tri_n)).normalized()


def _prim_mats(sd):
    return np.concatenate([sd.mat_id.astype(np.int64), sd.spheres[:, 4].astype(np.int64)])


# ---- the NRM grid ----

def _nrm_scene(kind, textures, env):
    sd = _grid_scene(kind)
    if textures:
        sd = _textured(sd)
    if env:
        sd = _with_map(sd)
    return _with_normals(sd)


@pytest.mark.parametrize("textures", [False, True], ids=["plain", "textured"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("kind", KINDS)
def test_normals_grid(gpu, oracle, kind, integrator, textures):
    """render_kernel_n: the grid's map off / on x four samplers x the luminance clamp off / on; control: every normal zero is another film"""
    for env in (False, True):
        sd = _nrm_scene(kind, textures, env)
        assert len(sd.tri_n) == len(sd.idx) and (sd.tri_n != 0).any()
        o = oracle.OracleScene(sd)
        films = {}
        with gpu.Scene(sd, builder=_builder(kind)) as sc:
            _check_stack_variant(sc, kind)
            for sampler in SAMPLERS:
                for clamp in (0.0, 1.0):
                    kw = dict(BASE, integrator=integrator, seed=3 + env, sampler=sampler, max_sample_luminance=clamp)
                    films[sampler, clamp] = sc.render(**kw)[0]
                    assert_bit_equal(films[sampler, clamp], o.render(**kw)[0], f"{kind}, map {env}, textures {textures}, {kw}")
        with gpu.Scene(_zero_normals(sd), builder=_builder(kind)) as sc:
            for (sampler, clamp), film in films.items():
                kw = dict(BASE, integrator=integrator, seed=3 + env, sampler=sampler, max_sample_luminance=clamp)
                assert not np.array_equal(sc.render(**kw)[0], film), f"{kind}, map {env}, {kw}: every normal zero gives the same film"


# ---- the plastic grid ----

PLASTIC_ALPHAS = (1e-3, 0.05, 0.4618, 1.0)
PLASTIC_ROWS = np.array([[PLASTIC, .3, .4, .5, .5, .4, .3], [PLASTIC, .5, .3, .2, .2, .3, .6], [PLASTIC, .2, .5, .3, .6, .6, .6], [PLASTIC, .4, .4, .1, .3, .5, .2],
                         [PLASTIC, .5, .4, .3, 0, 0, 0], [PLASTIC, 0, 0, 0, .7, .6, .5]], np.float32)  # (the last two: Ks = 0, Kd = 0)
PLASTIC_ROW_ALPHA = np.array([*PLASTIC_ALPHAS, 0.05, 0.4618], np.float32)


def _plastic_scene(kind):
    """the grid scene with every third primitive whose material is a matte that does not emit, and every third whose material is a mirror,
    moved to one of six plastic materials appended to the table (the four alphas; one with Ks = 0, one with Kd = 0).  Glass stays."""
    sd = _grid_scene(kind)
    n0 = len(sd.materials)
    mats = np.concatenate([sd.materials, PLASTIC_ROWS]).astype(np.float32)
    eta = np.concatenate([sd.mat_eta if len(sd.mat_eta) else np.full(n0, 1.5, np.float32), PLASTIC_ROW_ALPHA]).astype(np.float32)
    mat_id, spheres = sd.mat_id.copy(), sd.spheres.copy()
    prim = _prim_mats(sd)
    matte = (sd.materials[prim, 0] == MATTE) & ~(sd.materials[prim, 4:7] > 0).any(1)
    mirror = sd.materials[prim, 0] == MIRROR
    turned = 0
    for group in (matte, mirror):
        for k, p in enumerate(np.flatnonzero(group)[::3]):
            m = n0 + (turned + k) % len(PLASTIC_ROWS)
            if p < len(mat_id):
                mat_id[p] = m
            else:
                spheres[p - len(mat_id), 4] = m
        turned += len(np.flatnonzero(group)[::3])
    assert turned >= len(PLASTIC_ROWS) or kind == "tris17", (kind, turned)
    out = dataclasses.replace(sd, materials=mats, mat_eta=eta, mat_id=mat_id, spheres=spheres, mat_tex=np.zeros(len(mats), np.uint32)).normalized()
    assert case_holds_plastic(out) and (out.materials[_prim_mats(out), 0] == 2).any()  # plastic, and glass beside it
    return out


GRID_IMAGES = [ir.random_image(3, 5, 31), ir.random_image(17, 4, 32)]


def _plastic_textured(sd, how):
    """a texture on every matte material that does not emit, over random corner (u, v): `checker`: test_glass_env_parity_gpu's board;
    `image`: the two grid images alternating, bilinear / clamp and point / repeat, with mappings that reach negative s"""
    if how == "plain":
        return sd
    if how == "checker":
        return _textured(sd)
    rng = np.random.default_rng(9)
    plain = np.flatnonzero((sd.materials[:, 0] == MATTE) & ~(sd.materials[:, 4:7] > 0).any(1))
    mat_tex = np.zeros(len(sd.materials), np.uint32)
    mat_tex[plain] = 1 + np.arange(len(plain)) % 2
    rows = [api.image_texture_row(0, CLAMP, BILINEAR, (1.7, -2.3, -0.6, 0.4)), api.image_texture_row(1, REPEAT, POINT, (-3.1, 2.2, 0.3, -0.7))]
    return dataclasses.replace(sd, textures=np.array(rows, np.float32), images=GRID_IMAGES, mat_tex=mat_tex,
                               tri_uv=rng.uniform(-1.5, 2.5, (len(sd.idx), 6)).astype(np.float32)).normalized()


def _plastic_as_matte(sd):
    m = sd.materials.copy()
    p = m[:, 0] == PLASTIC
    m[p, 0], m[p, 4:7] = MATTE, 0
    return dataclasses.replace(sd, materials=m).normalized()


@pytest.mark.parametrize("textures", ["plain", "checker", "image"])
@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("kind", KINDS)
def test_plastic_grid(gpu, oracle, kind, integrator, textures):
    """render_kernel_x<..., GLS> with plastic in the scene: four samplers x {default film, the wide box (1.5, 0.75) through render_acc,
    luminance clamp 1}; control: plastic turned into matte of the same Kd is another film"""
    sd = _plastic_textured(_plastic_scene(kind), textures)
    o = oracle.OracleScene(sd)
    base = dict(BASE, integrator=integrator, seed=5)
    films = {}
    with gpu.Scene(sd, builder=_builder(kind)) as sc:
        _check_stack_variant(sc, kind)
        for sampler in SAMPLERS:
            kw = dict(base, sampler=sampler)
            films[sampler, "film"] = sc.render(**kw)[0]
            assert_bit_equal(films[sampler, "film"], o.render(**kw)[0], f"{kind} {textures} {kw}")
            films[sampler, "wide"] = sc.render_acc(WIDE, **kw)[0]
            assert np.array_equal(films[sampler, "wide"], o.render_acc(WIDE, **kw)[0]), f"{kind} {textures} {kw}: accumulators under box filter {WIDE}"
            kw["max_sample_luminance"] = 1.0
            films[sampler, "clamp"] = sc.render(**kw)[0]
            assert_bit_equal(films[sampler, "clamp"], o.render(**kw)[0], f"{kind} {textures} {kw}")
    with gpu.Scene(_plastic_as_matte(sd), builder=_builder(kind)) as sc:
        for sampler in SAMPLERS:
            kw = dict(base, sampler=sampler)
            assert not np.array_equal(sc.render(**kw)[0], films[sampler, "film"]), f"{kind} {kw}: plastic as matte gives the same film"
            assert not np.array_equal(sc.render_acc(WIDE, **kw)[0], films[sampler, "wide"]), f"{kind} {kw}: plastic as matte gives the same accumulators"
            kw["max_sample_luminance"] = 1.0
            assert not np.array_equal(sc.render(**kw)[0], films[sampler, "clamp"]), f"{kind} {kw}: plastic as matte gives the same clamped film"


# ---- what the grids reach ----

def _variant_row(sd, integrator, sampler, wide):
    """the row of render_variant.hpp's table a render of `sd` selects (capi_render.cpp fills the switches this way: spheres in the scene,
    a textured primitive, a glass or plastic material anywhere in the table, a map, the normals' record)"""
    prim = _prim_mats(sd)
    want = dict(spheres=len(sd.spheres) > 0, wide=wide, table_sampler=sampler in ("sobol_nd", "halton"), mis=integrator == INTEGRATOR_PATH_MIS,
                textured=bool(len(sd.mat_tex)) and bool((sd.mat_tex[prim] != 0).any()), glass=bool((sd.materials[:, 0] >= 2).any()), env=case_holds_map(sd),
                normals=len(sd.tri_n) > 0, counters=rvt.COUNT_NONE)
    rows = [r for r in rvt.table() if all(getattr(r, k) == v for k, v in want.items())]
    assert len(rows) == 1 and rows[0].code == 0, (want, rows)
    return rows[0]


def _family_rows(family, last, **fixed):
    rows = [r for r in rvt.table() if r.family == family and r.code == 0 and r.counters == rvt.COUNT_NONE and all(getattr(r, k) == v for k, v in fixed.items())]
    return {(r.spheres, overflow, r.mis, r.textured, r.table_sampler, getattr(r, last)) for r in rows for overflow in (False, True)}


def test_the_grids_reach_every_instantiation():
    """(spheres, overflow, mis, textured, table_sampler, env | wide) of every render of the two grids, from the table of
    render_variant.hpp: the 64 instantiations of render_kernel_n, the 64 `GLS` ones of render_kernel_x.  (overflow: the deep kinds, which
    _check_stack_variant asserts on the device in every grid test.)"""
    reached = set()
    for kind in KINDS:
        for textures in (False, True):
            for env in (False, True):
                sd = _nrm_scene(kind, textures, env)
                for integrator in INTEGRATORS:
                    for sampler in SAMPLERS:
                        r = _variant_row(sd, integrator, sampler, False)
                        assert r.family == "n"
                        reached.add((r.spheres, kind.startswith("deep"), r.mis, r.textured, r.table_sampler, r.env))
    want = _family_rows("n", "env")
    assert len(want) == 64 and reached == want, (len(reached), sorted(want - reached))
    reached = set()
    for kind in KINDS:
        for textures in ("plain", "checker", "image"):
            sd = _plastic_textured(_plastic_scene(kind), textures)
            for integrator in INTEGRATORS:
                for sampler in SAMPLERS:
                    for wide in (False, True):
                        r = _variant_row(sd, integrator, sampler, wide)
                        assert r.family == "x" and r.glass
                        reached.add((r.spheres, kind.startswith("deep"), r.mis, r.textured, r.table_sampler, r.wide))
    want = _family_rows("x", "wide", glass=True)
    assert len(want) == 64 and reached == want, (len(reached), sorted(want - reached))


# ---- image cases ----

def _two_mattes(sd):
    """a second matte material, which every other primitive of a matte that does not emit moves to: both images of the pool are seen"""
    n0 = len(sd.materials)
    mats = np.concatenate([sd.materials, [[MATTE, .3, .6, .7, 0, 0, 0]]]).astype(np.float32)
    eta = np.concatenate([sd.mat_eta if len(sd.mat_eta) else np.full(n0, 1.5, np.float32), [1.5]]).astype(np.float32)
    mat_id, spheres = sd.mat_id.copy(), sd.spheres.copy()
    prim = _prim_mats(sd)
    for p in np.flatnonzero((sd.materials[prim, 0] == MATTE) & ~(sd.materials[prim, 4:7] > 0).any(1))[::2]:
        if p < len(mat_id):
            mat_id[p] = n0
        else:
            spheres[p - len(mat_id), 4] = n0
    return dataclasses.replace(sd, materials=mats, mat_eta=eta, mat_id=mat_id, spheres=spheres, mat_tex=np.zeros(len(mats), np.uint32)).normalized()


def _with_images(sd, filt, wrap):
    """3 x 5 and 17 x 4 in one pool, on alternating matte materials; the first mapping sends part of the surface to negative s, the second
    mirrors u (random corner (u, v) in [-1.5, 2.5]; a sphere's own (u, v) in [0, 1])"""
    rng = np.random.default_rng(19)
    plain = np.flatnonzero((sd.materials[:, 0] == MATTE) & ~(sd.materials[:, 4:7] > 0).any(1))
    mat_tex = np.zeros(len(sd.materials), np.uint32)
    mat_tex[plain] = 1 + np.arange(len(plain)) % 2
    rows = [api.image_texture_row(0, wrap, filt, (1.7, -2.3, -0.6, 0.4)), api.image_texture_row(1, wrap, filt, (-3.1, 2.2, 0.3, -0.7))]
    return dataclasses.replace(sd, textures=np.array(rows, np.float32), images=GRID_IMAGES, mat_tex=mat_tex,
                               tri_uv=rng.uniform(-1.5, 2.5, (len(sd.idx), 6)).astype(np.float32)).normalized()


def _images_as_constants(sd):
    m = sd.materials.copy()
    for i, t in enumerate(sd.mat_tex):
        if t:
            m[i, 1:4] = sd.images[int(sd.textures[t - 1][1])].reshape(-1, 3).mean(0)
    return dataclasses.replace(sd, materials=m, mat_tex=np.zeros(len(m), np.uint32)).normalized()


IMAGE_SCENES = {
    "tris17 under the map": lambda: _with_map(_two_mattes(_grid_scene("tris17"))),
    "spheres under the map": lambda: _with_map(_grid_scene("spheres")),
    "tris17 with normals": lambda: _with_normals(_two_mattes(_grid_scene("tris17"))),
    "deep": lambda: _two_mattes(_grid_scene("deep")),
}


@pytest.mark.parametrize("wrap", [REPEAT, CLAMP, BLACK], ids=["repeat", "clamp", "black"])
@pytest.mark.parametrize("filt", [BILINEAR, POINT], ids=["bilinear", "point"])
def test_image_cases(gpu, oracle, filt, wrap):
    """two images in one pool through the TEX instantiations of render_kernel_env, render_kernel_n and (the deep tree) render_kernel_x;
    control: each image's mean colour as a constant Kd is another film"""
    for name, make in IMAGE_SCENES.items():
        kind = "deep" if name == "deep" else "tris17"
        sd = _with_images(make(), filt, wrap)
        assert len(np.unique(sd.mat_tex[_prim_mats(sd)])) == 3  # untextured, the first image, the second
        o = oracle.OracleScene(sd)
        with gpu.Scene(sd, builder=_builder(kind)) as sc, gpu.Scene(_images_as_constants(sd), builder=_builder(kind)) as flat:
            _check_stack_variant(sc, kind)
            for integrator, sampler in ((INTEGRATOR_PATH, "stratified"), (INTEGRATOR_PATH_MIS, "halton")):
                kw = dict(BASE, integrator=integrator, seed=6, sampler=sampler)
                film = sc.render(**kw)[0]
                assert_bit_equal(film, o.render(**kw)[0], f"{name}, filter {filt}, wrap {wrap}, {kw}")
                assert not np.array_equal(flat.render(**kw)[0], film), f"{name}, filter {filt}, wrap {wrap}: the images' means give the same film"


# ---- edges ----

def _check(gpu, oracle, sd, what, builder=None, **kw):
    ref = oracle.OracleScene(sd).render(**kw)[0]
    with gpu.Scene(sd, builder=builder) as sc:
        film = sc.render(**kw)[0]
    assert_bit_equal(film, ref, f"{what} {kw}")
    return film


@pytest.mark.parametrize("max_depth", [0, 1, 12])
@pytest.mark.parametrize("feature", ["normals", "plastic"])
def test_depths(gpu, oracle, feature, max_depth):
    """the depth rule (depth 0: no vertex is shaded; 1: one light sample, and under MIS the bounce ray that ends the estimate) and the
    roulette behind it (depth 12)"""
    sd = _with_normals(_grid_scene("tris17")) if feature == "normals" else _plastic_scene("tris17")
    for integrator in INTEGRATORS:
        _check(gpu, oracle, sd, f"{feature}, depth {max_depth}", integrator=integrator, max_depth=max_depth, spp=(2, 2), seed=max_depth, sampler=SAMPLERS[(max_depth + integrator) % 4])


def test_geometric_back_face_with_normals(gpu, oracle):
    """the camera looks at the BACK of a matte and of a mirror quad that carry normals: nf = -ng, and nsf flips with it"""
    matte = ((-1.2, 1.0, -0.6), (-0.1, 1.0, -0.6), (-0.1, 1.2, 0.9), (-1.2, 1.2, 0.9))
    mirror = ((0.1, 1.1, -0.6), (1.2, 1.0, -0.6), (1.2, 1.3, 0.9), (0.1, 1.2, 0.9))
    films = []
    for flip in (False, True):
        sd = glass_room_scene(extra_parts=[(matte[::-1] if flip else matte, M_MATTE), (mirror[::-1] if flip else mirror, M_MIRROR)],
                              lights=[[LIGHT_INFINITE, 0, 0, 0, .2, .2, .2]])
        sd = _with_normals(sd, seed=2)
        for kw in (dict(integrator=INTEGRATOR_PATH, sampler="halton"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="stratified")):
            films.append(_check(gpu, oracle, sd, f"quads with normals, flipped {flip}", max_depth=6, spp=(2, 2), seed=3, **kw))
    assert not np.array_equal(films[0], films[2])


def _plastic_only(lights, le_quad=None):
    """a plastic floor and a plastic sphere on it -- nothing else but, le_quad, an emissive quad above them"""
    floor = ((-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    parts = [(floor, 0)]
    mats = [[PLASTIC, .3, .4, .5, .6, .5, .4], [PLASTIC, .5, .2, .2, .3, .3, .3]]
    if le_quad is not None:
        parts.append((((-0.7, -0.7, 1.6), (-0.7, 0.7, 1.6), (0.7, 0.7, 1.6), (0.7, -0.7, 1.6)), 2))  # wound to face down
        mats.append([MATTE, 0, 0, 0, *le_quad])
    P, idx, mat_id = quad_mesh(parts)
    return SceneData(P=P, idx=idx, mat_id=mat_id, materials=np.array(mats, np.float32), mat_eta=np.array([0.3, 0.05, 0][:len(mats)], np.float32),
                     lights=np.array(lights, np.float32).reshape(-1, 7), spheres=np.array([[0.5, 0.3, 0.4, 0.4, 1]], np.float32),
                     cam_to_world=look_at((2.5, -2.5, 1.1), (0, 0, 0.2), (0, 0, 1))[1], fov=50.0, xres=24, yres=21).normalized()


def test_plastic_alone_under_a_constant_sky(gpu, oracle):
    """integrator 2 with the constant infinite light alone: the constant pair of weights, 1 / (1 + nL^2) at the light sample and
    nL^2 / (nL^2 + 1) where the bounce ray escapes"""
    sd = _plastic_only([[LIGHT_INFINITE, 0, 0, 0, .5, .25, 1.0]])
    for sampler in SAMPLERS:
        film = _check(gpu, oracle, sd, "plastic under the sky alone", integrator=INTEGRATOR_PATH_MIS, max_depth=6, spp=(2, 2), seed=7, sampler=sampler)
        assert film[..., 1].mean() > 0.1


def test_plastic_floor_under_an_emissive_triangle(gpu, oracle):
    """integrator 2 with emissive triangles alone: the light sample weighted against plastic's own density, and what the bounce ray finds
    on the emitter weighted through the stored pdf_b"""
    sd = _plastic_only([], le_quad=(5, 4, 3))
    for max_depth, sampler in ((1, "stratified"), (6, "sobol"), (6, "sobol_nd"), (6, "halton")):
        film = _check(gpu, oracle, sd, "plastic under an emitter", integrator=INTEGRATOR_PATH_MIS, max_depth=max_depth, spp=(2, 2), seed=8, sampler=sampler)
        assert film[..., 1].mean() > 0.02


@pytest.mark.parametrize("feature", ["normals", "plastic"])
def test_two_ranks_add_to_the_whole(gpu, oracle, feature):
    """a 96-pixel-wide film: two 64 x 64 super-tiles, one per rank; the ranks' films add to the oracle's"""
    sd = dataclasses.replace(_grid_scene("tris17"), xres=96, yres=21).normalized()
    sd = _with_normals(_textured(sd)) if feature == "normals" else _plastic_textured(dataclasses.replace(_plastic_scene("tris17"), xres=96, yres=21).normalized(), "image")
    kw = dict(BASE, integrator=INTEGRATOR_PATH_MIS, seed=9, sampler="halton")
    o = oracle.OracleScene(sd)
    ref = o.render(**kw)[0]
    with gpu.Scene(sd) as sc:
        parts = [sc.render(rank=r, world_size=2, **kw)[0] for r in range(2)]
        assert all(p[..., 3].sum() > 0 for p in parts)
        assert_bit_equal(parts[0] + parts[1], ref, f"{feature}: two ranks summed")
        if feature == "plastic":
            acc = sum(sc.render_acc(WIDE, rank=r, world_size=2, **kw)[0] for r in range(2))
            assert np.array_equal(acc, o.render_acc(WIDE, **kw)[0])


# ---- random scenes ----

_SOAK_FIRST = int(os.environ.get("PBRT_SOAK_FIRST", "0"))
_SOAK_SEEDS = int(os.environ.get("PBRT_SOAK_SEEDS", "24"))


@pytest.mark.parametrize("seed", range(_SOAK_FIRST, _SOAK_FIRST + _SOAK_SEEDS))
@pytest.mark.parametrize("feature", ["normals", "plastic"])
def test_random_scenes_match_oracle(gpu, oracle, feature, seed):
    """util.random_normals_plastic_case without its cap on the primitive count, the builders alternating, a random rank split with the
    shards summed -- films under the default filter, accumulators under a wide one"""
    sd, kw = random_normals_plastic_case(seed, feature, cap=False)
    assert not (case_holds_plastic(sd) and (case_holds_map(sd) or len(sd.tri_n)))
    world = int(np.random.default_rng(96_000 + seed).integers(1, 4))
    o = oracle.OracleScene(sd)
    what = f"random scene {seed}, {feature}: plastic {case_holds_plastic(sd)}, normals {len(sd.tri_n)}, images {len(sd.images)}, {world} ranks, {kw}"
    with gpu.Scene(sd, builder="gpu" if seed % 2 else "host") as sc:
        if kw.get("filter_width"):
            k2 = {k: v for k, v in kw.items() if k != "filter_width"}
            parts = sum(sc.render_acc(kw["filter_width"], rank=r, world_size=world, **k2)[0] for r in range(world))
            assert np.array_equal(parts, o.render_acc(kw["filter_width"], **k2)[0]), what
        else:
            assert_bit_equal(sum(sc.render(rank=r, world_size=world, **kw)[0] for r in range(world)), o.render(**kw)[0], what)


def test_random_cases_hold_what_they_are_for():
    """the generator alone: over the 24 seeds enough scenes carry normals, plastic and images, and none pairs plastic with a map or normals"""
    normals = plastic = images = 0
    for seed in range(24):
        for feature in ("normals", "plastic"):
            sd, _ = random_normals_plastic_case(seed, feature, cap=False)
            assert not (case_holds_plastic(sd) and (case_holds_map(sd) or len(sd.tri_n)))
            normals += feature == "normals" and bool((sd.tri_n != 0).any())
            plastic += feature == "plastic" and case_holds_plastic(sd)
            images += len(sd.images) > 0
    assert normals >= 16 and plastic >= 16 and images >= 4, (normals, plastic, images)
