"""The substrate material on the device: substrate_bsdf.hpp bit for bit against its host compile, films against the float64
reference of tests/substrate_ref.py (same random numbers) with two wrong references that must fail, a closed form, the MIS corners, the
neighbours (matte, plastic and glass beside it, depth 0 and 1, two ranks, the command line) and twelve random scenes.  32 x 32 films (the
two ranks: 96 x 16), <= 256 spp.  The oracle does not know substrate (3.24, section 12): the reference and the closed form hold it."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from pbrt_amd import (GLASS, INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_DISTANT, LIGHT_INFINITE, LIGHT_POINT, MATTE, PLASTIC, SUBSTRATE, SceneData,
                      api, look_at, scenes)

import substrate_host_build as hb
import substrate_random
import substrate_ref as ref
from util import assert_bit_equal, meets_random_scene_bar, twin_agreement

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLERS = ("stratified", "sobol", "sobol_nd", "halton")
_M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])


def _ref(sd, **kw):
    if kw.get("sampler") == "sobol_nd":
        kw = dict(kw, sobol_matrices=api.sobol_matrices())
    return ref.render(sd, **kw)


def _rgb(film):
    return (np.asarray(film, np.float64)[..., :3] / np.maximum(film[..., 3:4], 1e-30)) @ np.linalg.inv(_M).T


# ---- 1. the header on the device ----

def test_device_equals_the_host_compile_bit_for_bit(gpu, tmp_path):
    exe = hb.build(tmp_path)
    x = np.concatenate([hb.domain_inputs(), hb.edge_inputs()])
    assert len(x) == (1 << 16) + 4096
    y = hb.run(exe, x, tmp_path)
    assert (y[: 1 << 16, 3] > 0).all()
    assert_bit_equal(api.substrate_eval_device(x), y, "pbrt_hip_substrate_eval_device vs the host compile of substrate_bsdf.hpp")


# ---- 2. determinate pixels ----

def _plane_scene(res, eye, lights, kd=(0.3, 0.4, 0.5), ks=(0.5, 0.4, 0.3), alpha=0.2, fov=40.0, half=4.0, up=(0, 0, 1)):
    h = half
    return SceneData(P=np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], np.float32), idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                     mat_id=np.zeros(2, np.uint16), materials=np.array([[SUBSTRATE, *kd, *ks]], np.float32), mat_eta=np.array([alpha], np.float32),
                     lights=np.array(lights, np.float32), cam_to_world=look_at(eye, (0, 0, 0), up)[1], fov=fov, xres=res, yres=res).normalized()


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_one_bounce_frames_match_the_reference(gpu, sampler):
    """A substrate quad under one point light, and under one distant light, direct lighting, 4 spp: nothing is random but the film points.
    The bar is the one the twin's fixed cases are held to (tests/test_plastic_gpu.py): weights equal, 99 % of the pixels within 1e-4 per
    channel, PSNR >= 90 dB."""
    d = np.array([0.3, -0.2, 0.93])
    for name, light in (("point", [LIGHT_POINT, 0.5, -0.4, 1.5, 6, 6, 6]), ("distant", [LIGHT_DISTANT, *(d / np.linalg.norm(d)), 2, 2, 2])):
        sd = _plane_scene(32, (0.2, -2.5, 1.2), [light])
        kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(2, 2), seed=11, sampler=sampler)
        with gpu.Scene(sd) as sc:
            film = sc.render(**kw)[0]
        ps, share, weights = twin_agreement(_ref(sd, **kw), film)
        print(f"{name} light, {sampler}: PSNR {ps:.1f} dB, {100 * share:.2f} % of the pixels within 1e-4")
        assert film[..., 1].mean() > 0.05
        assert weights and share >= 0.99 and ps >= 90.0, (name, sampler, ps, share)


# ---- 3. whole paths ----

PATH_CASES = [dict(integrator=i, sampler=s) for i in (INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS) for s in ("stratified", "halton")]
PATH_CASES += [dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol_nd", filter_width=(1.5, 0.75)), dict(integrator=INTEGRATOR_PATH, sampler="sobol", max_sample_luminance=1.0)]


@pytest.fixture(scope="module")
def substrate_box():
    return scenes.substrate_scene(32, 32)


@pytest.mark.parametrize("case", PATH_CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_whole_paths_match_the_reference(gpu, substrate_box, case):
    kw = dict(case, max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(substrate_box) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(substrate_box, **kw), film, kw)
    print(f"{case}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert ok, (case, ps, off)


@pytest.mark.parametrize("wrong", [dict(cos_product=True), dict(lobe_pick=1.0 / 3.0)], ids=["cos-product", "lobe-at-1/3"])
def test_a_wrong_reference_fails_the_same_bar(gpu, substrate_box, wrong):
    kw = dict(integrator=INTEGRATOR_PATH, sampler="stratified", max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(substrate_box) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(substrate_box, **kw, **wrong), film, kw)
    print(f"{wrong}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert not ok


# ---- 4. a closed form ----

def _sky_plane(theta, alpha, le, kd, ks):
    t = np.radians(theta)
    eye = (20.0 * np.sin(t), 0.0, 20.0 * np.cos(t))
    return _plane_scene(32, eye, [[LIGHT_INFINITE, 0, 0, 0, le, le, le]], (kd,) * 3, (ks,) * 3, alpha=alpha, fov=1.0, half=400.0, up=(0, 1, 0))


def _per_sample_se(sd, kw, n_frame):
    """the standard error of a frame's mean of n_frame samples, from the REFERENCE's per-sample values at 16 spp"""
    samples = []
    ref.render(sd, **dict(kw, spp=(4, 4)), samples=samples)
    return np.stack(samples)[..., 1].std(ddof=1) / np.sqrt(n_frame)


@pytest.mark.parametrize("alpha", [0.1, 0.5])
@pytest.mark.parametrize("theta", [0.0, 60.0, 80.0])
def test_plane_under_a_constant_sky(gpu, theta, alpha):
    """A substrate plane that fills a 1-degree view under a constant infinite light Le, direct lighting, 256 spp: every pixel's expectation
    is Le x albedo(theta_o, alpha), the albedo by float64 quadrature of f cos at the pixels' own view angles.  Tolerance: 5 standard errors
    of the image mean, from the REFERENCE's per-sample values, plus the 3e-6 of the other plane tests."""
    le, kd, ks = 0.8, 0.5, 0.4
    sd = _sky_plane(theta, alpha, le, kd, ks)
    kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(16, 16), seed=2, sampler="stratified")
    with gpu.Scene(sd) as sc:
        got = _rgb(sc.render(**kw)[0])[..., 1].mean()
    se = _per_sample_se(sd, kw, 256 * 32 * 32)
    # the pixels' view angles: camera rays through the pixel centres, as DESIGN.md 3.2 forms them
    c2w = sd.cam_to_world.astype(np.float64)
    th = np.tan(np.radians(sd.fov) / 2)
    px = (np.arange(32) + 0.5) / 32 * 2 - 1
    dirs = np.stack([*np.meshgrid(px * th, -px * th, indexing="xy"), np.ones((32, 32))], -1) @ c2w[:3, :3].T
    cos_o = -dirs[..., 2] / np.linalg.norm(dirs, axis=-1)
    grid = np.linspace(np.arccos(cos_o.max()), np.arccos(cos_o.min()), 5)
    rho = np.interp(np.arccos(cos_o), grid, [ref.albedo(g, float(np.float32(alpha)), kd, ks) for g in grid]).mean()
    want = le * rho
    print(f"theta {theta} alpha {alpha}: mean {got:.6f}, closed form {want:.6f} (albedo {rho:.5f}), 5 se {5 * se:.2e}")
    assert abs(got - want) <= 5 * se + 3e-6, (got, want, se)


# ---- 5. the MIS corners ----

def test_path_and_mis_agree_under_the_constant_sky(gpu):
    """the substrate-only plane under the constant infinite light alone: the light sample's constant weight 1 / (1 + nL^2) and the escaping
    bounce ray's nL^2 / (nL^2 + 1) add up to what integrator 0's light sample gives alone, in the mean within 5 standard errors"""
    sd = _sky_plane(60.0, 0.1, 0.8, 0.5, 0.4)
    kw = dict(max_depth=5, spp=(16, 16), seed=9, sampler="stratified")
    means, ses = [], []
    with gpu.Scene(sd) as sc:
        for integrator in (INTEGRATOR_PATH, INTEGRATOR_PATH_MIS):
            means.append(_rgb(sc.render(integrator=integrator, **kw)[0])[..., 1].mean())
            ses.append(_per_sample_se(sd, dict(kw, integrator=integrator), 256 * 32 * 32))
    se = float(np.hypot(*ses))
    print(f"integrator 0 {means[0]:.6f}, integrator 2 {means[1]:.6f}, 5 se {5 * se:.2e}")
    assert means[0] > 0.1 and abs(means[0] - means[1]) <= 5 * se + 3e-6, (means, se)


def test_mis_under_an_emissive_quad_matches_the_reference(gpu):
    """a substrate floor under an emissive quad alone, integrator 2: the light sample's power-heuristic weight against THIS BSDF's density,
    and the bounce ray that lands on the emitter weighted with the density the vertex stored"""
    h = 2.0
    P = [[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0], [-0.5, -0.5, 1.2], [-0.5, 0.5, 1.2], [0.5, 0.5, 1.2], [0.5, -0.5, 1.2]]  # (the emitter faces -z)
    sd = SceneData(P=np.array(P, np.float32), idx=np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.uint32), mat_id=np.array([0, 0, 1, 1], np.uint16),
                   materials=np.array([[SUBSTRATE, 0.3, 0.4, 0.5, 0.6, 0.5, 0.4], [MATTE, 0, 0, 0, 6, 5, 4]], np.float32), mat_eta=np.array([0.15, 1.5], np.float32),
                   cam_to_world=look_at((0.3, -3.0, 0.9), (0, 0, 0.2), (0, 0, 1))[1], fov=45.0, xres=32, yres=32).normalized()
    kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(4, 4), seed=3, sampler="stratified")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        assert sc.info()["n_lights"] == 2  # (the emitter's two triangles: the floor's Ks is no emission)
    ok, ps, off = meets_random_scene_bar(_ref(sd, **kw), film, kw)
    print(f"emissive quad, MIS: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert film[..., 1].mean() > 0.05 and ok, (ps, off)


# ---- 6. the neighbours ----

def test_a_substrate_triangle_adds_no_light(gpu):
    """Ks rides where a matte record keeps its emission: it must not enter the light list"""
    sd = _plane_scene(8, (0.2, -2.5, 1.2), [[LIGHT_POINT, 0.5, -0.4, 1.5, 6, 6, 6]], ks=(0.9, 0.9, 0.9))
    with gpu.Scene(sd) as sc:
        assert sc.info()["n_lights"] == 1


def _mixed_scene(keep):
    """substrate_scene with a PLASTIC floor, the SUBSTRATE blue sphere and a GLASS orange sphere; `keep`: the kinds that stay, the others
    become matte of the same first colour"""
    sd = scenes.substrate_scene(32, 32)
    mats, beside = sd.materials.copy(), sd.mat_eta.copy()
    mats[0] = [PLASTIC, 0.4, 0.4, 0.4, 0.3, 0.3, 0.3]
    beside[0] = api.roughness_to_alpha(0.2)
    mats[6] = [GLASS, 1, 1, 1, 0.9, 0.9, 0.9]
    beside[6] = 1.5
    for i in (0, 5, 6):
        if int(mats[i, 0]) not in keep:
            mats[i] = [MATTE, *mats[i, 1:4], 0, 0, 0]
    coated = np.isin(mats[:, 0], (GLASS, PLASTIC, SUBSTRATE)).any()
    return dataclasses.replace(sd, materials=mats, mat_eta=beside if coated else np.zeros(0, np.float32)).normalized()


def test_plastic_substrate_and_glass_in_one_scene(gpu, oracle):
    kw = dict(integrator=INTEGRATOR_PATH_MIS, sampler="halton", max_depth=6, spp=(4, 4), seed=7)
    for keep in ((PLASTIC,), (GLASS,)):  # the sub-scenes the oracle knows stay bit-equal to it
        sd = _mixed_scene(keep)
        with gpu.Scene(sd) as sc:
            assert_bit_equal(sc.render(**kw)[0], oracle.OracleScene(sd).render(**kw)[0], f"the sub-scene of kinds {keep} vs the oracle")
    sd = _mixed_scene((PLASTIC, SUBSTRATE, GLASS))
    assert sorted(set(sd.materials[:, 0].astype(int))) == [MATTE, GLASS, PLASTIC, SUBSTRATE]
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(sd, **kw), film, kw)
    print(f"plastic + substrate + glass: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert ok, (ps, off)


@pytest.mark.parametrize("max_depth", [0, 1])
def test_depth_zero_and_one(gpu, substrate_box, max_depth):
    kw = dict(integrator=INTEGRATOR_PATH, sampler="stratified", max_depth=max_depth, spp=(4, 4), seed=5)
    with gpu.Scene(substrate_box) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(substrate_box, **kw), film, kw)
    print(f"max_depth {max_depth}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert film[..., 1].max() > 1.0 and ok, (max_depth, ps, off)  # (the emitter is in view at either depth)


def test_two_ranks_equal_one(gpu):
    sd = scenes.substrate_scene(96, 16)
    kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(2, 2), seed=6, sampler="halton")
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
        parts = [sc.render(rank=r, world_size=2, **kw)[0] for r in range(2)]
    assert all(p[..., 3].any() for p in parts)  # (two super-tiles: each rank has one)
    assert_bit_equal(parts[0] + parts[1], film, "two ranks' films")
    with gpu.MultiScene(sd, n_gpus=1) as ms:
        assert_bit_equal(ms.render(**kw)[0], film, "in-library multi-GPU with one rank vs single-GPU")


def test_cli_renders_the_scene_file(gpu, tmp_path):
    from pbrt_amd import loader
    from pbrt_amd.build import CLI_PATH
    text = open(os.path.join(ROOT, "scenes", "substrate_spheres.pbrt")).read().replace("[256]", "[64]").replace('"integer pixelsamples" 64', '"integer pixelsamples" 16')
    ls = loader.load_string(text)
    assert (ls.scene.materials[:, 0] == SUBSTRATE).sum() == 3
    with gpu.Scene(ls.scene) as sc, gpu.Scene(scenes.substrate_scene(64, 64)) as gen:
        kw = dict(ls.render_kwargs(), seed=4)
        film = sc.render(**kw)[0]
        assert_bit_equal(gen.render(**kw)[0], film, "scenes.substrate_scene vs scenes/substrate_spheres.pbrt")
    with gpu.Scene(scenes.substrate_scene(64, 64, substrate=False)) as sc:
        matte = sc.render(**kw)[0]
    # substrate is not matte of the same Kd: with Ks 0.5 the coat's highlight is plain to see (DESIGN.md 3.24 states the largest difference)
    diff = np.abs(_rgb(film) - _rgb(matte)).mean(-1).max()
    print(f"largest pixel difference against the matte scene: {diff:.3f}")
    assert diff > 0.5  # (the float64 reference at 32 x 32, 16 spp: 1.03 at the sharp sphere's highlight; asserted at half of that)
    scene, out = tmp_path / "substrate.pbrt", tmp_path / "substrate.png"
    scene.write_text(text)
    r = subprocess.run([CLI_PATH, "-v", "--quick", "-o", str(out), str(scene)], capture_output=True, text=True)
    assert r.returncode == 0 and "wrote" in r.stderr and "not supported" not in r.stderr, r.stderr
    img = gpu.read_image(out)
    assert img.shape == (64, 64, 3) and img.std() > 0.05


# ---- 7. random scenes ----

@pytest.mark.parametrize("seed", range(substrate_random.N_SEEDS))
def test_random_scenes_match_the_reference(gpu, seed):
    sd, kw = substrate_random.random_substrate_case(seed)
    with gpu.Scene(sd) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(sd, **kw), film, kw)
    n_sub = int((sd.materials[sd.mat_id.astype(int), 0] == SUBSTRATE).sum()) + int((sd.materials[sd.spheres[:, 4].astype(int), 0] == SUBSTRATE).sum())
    print(f"seed {seed}: {len(sd.idx)} triangles, {len(sd.spheres)} spheres, {n_sub} substrate primitives, {kw}: PSNR {ps:.1f} dB, {off} of {film.shape[0] * film.shape[1]} pixels off at 1e-4")
    assert n_sub > 0 and ok, (seed, ps, off)
