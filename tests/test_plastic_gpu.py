"""The plastic material on the device: plastic_bsdf.hpp bit for bit against its host compile, films against the float64
reference of tests/plastic_ref.py (same random numbers), a closed form, the two path integrators against each other, and the neighbours
(matte through the GLS kernels, glass against the oracle, one-rank multi-GPU, the command line).  32 x 32 films, <= 256 spp."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from pbrt_amd import GLASS, INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_DISTANT, LIGHT_INFINITE, LIGHT_POINT, PLASTIC, SceneData, api, look_at, scenes

import plastic_host_build as hb
import plastic_ref as ref
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
    assert_bit_equal(api.plastic_eval_device(x), hb.run(exe, x, tmp_path), "pbrt_hip_plastic_eval_device vs the host compile of plastic_bsdf.hpp")


# ---- 2. determinate pixels ----

def _plane_scene(res, eye, lights, kd=(0.3, 0.4, 0.5), ks=(0.5, 0.4, 0.3), roughness=0.2, fov=40.0, half=4.0, up=(0, 0, 1)):
    row, alpha = api.plastic_material(kd, ks, roughness)
    h = half
    return SceneData(P=np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], np.float32), idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                     mat_id=np.zeros(2, np.uint16), materials=np.array([row], np.float32), mat_eta=np.array([alpha], np.float32),
                     lights=np.array(lights, np.float32), cam_to_world=look_at(eye, (0, 0, 0), up)[1], fov=fov, xres=res, yres=res).normalized()


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_one_bounce_frames_match_the_reference(gpu, oracle, sampler):
    """A plastic quad under one point light, and under one distant light, direct lighting, 4 spp: nothing is random but the film points.
    The bar is the one the twin's fixed cases are held to (tests/test_oracle_glass_env.py, tests/test_normals_gpu.py): weights equal, 99 %
    of the pixels within 1e-4 per channel, PSNR >= 90 dB."""
    d = np.array([0.3, -0.2, 0.93])
    for name, light in (("point", [LIGHT_POINT, 0.5, -0.4, 1.5, 6, 6, 6]), ("distant", [LIGHT_DISTANT, *(d / np.linalg.norm(d)), 2, 2, 2])):
        sd = _plane_scene(32, (0.2, -2.5, 1.2), [light])
        kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(2, 2), seed=11, sampler=sampler)
        with gpu.Scene(sd) as sc:
            film = sc.render(**kw)[0]
        assert_bit_equal(film, oracle.OracleScene(sd).render(**kw)[0], f"{name} light, {sampler}: against the oracle")
        ps, share, weights = twin_agreement(_ref(sd, **kw), film)
        print(f"{name} light, {sampler}: PSNR {ps:.1f} dB, {100 * share:.2f} % of the pixels within 1e-4")
        assert film[..., 1].mean() > 0.05
        assert weights and share >= 0.99 and ps >= 90.0, (name, sampler, ps, share)


# ---- 3. whole paths ----

PATH_CASES = [dict(integrator=i, sampler=s) for i in (INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS) for s in ("stratified", "halton")]
PATH_CASES += [dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol_nd", filter_width=(1.5, 0.75)), dict(integrator=INTEGRATOR_PATH, sampler="sobol", max_sample_luminance=1.0)]


@pytest.fixture(scope="module")
def plastic_box():
    return scenes.plastic_scene(32, 32)


@pytest.mark.parametrize("case", PATH_CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_whole_paths_match_the_reference(gpu, oracle, plastic_box, case):
    kw = dict(case, max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(plastic_box) as sc:
        film = sc.render(**kw)[0]
    assert_bit_equal(film, oracle.OracleScene(plastic_box).render(**kw)[0], f"plastic_scene vs the oracle, {kw}")  # (and, beside the bar below, word for word)
    ok, ps, off = meets_random_scene_bar(_ref(plastic_box, **kw), film, kw)
    print(f"{case}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert ok, (case, ps, off)


@pytest.mark.parametrize("wrong", [dict(g_one=True), dict(lobe_pick=1.0 / 3.0)], ids=["G=1", "lobe-at-1/3"])
def test_a_wrong_reference_fails_the_same_bar(gpu, plastic_box, wrong):
    kw = dict(integrator=INTEGRATOR_PATH, sampler="stratified", max_depth=5, spp=(4, 4), seed=5)
    with gpu.Scene(plastic_box) as sc:
        film = sc.render(**kw)[0]
    ok, ps, off = meets_random_scene_bar(_ref(plastic_box, **kw, **wrong), film, kw)
    print(f"{wrong}: PSNR {ps:.1f} dB, {off} of {32 * 32} pixels off at 1e-4")
    assert not ok


# ---- 4. a closed form ----

@pytest.mark.parametrize("alpha", [0.1, 0.5])
@pytest.mark.parametrize("theta", [0.0, 60.0, 80.0])
def test_plane_under_a_constant_sky(gpu, theta, alpha):
    """A plastic plane that fills the view under a constant infinite light Le, direct lighting, 256 spp: every pixel's expectation is
    Le (Kd + Ks rho(theta_o, alpha)), rho by float64 quadrature at the pixels' own view angles (the 1-degree view spans half a degree about
    theta).  Tolerance: 5 standard errors of the image mean, from the REFERENCE's per-sample values, plus the 3e-6 of the other plane tests."""
    le, kd, ks = 0.8, (0.3, 0.3, 0.3), (0.6, 0.6, 0.6)
    t = np.radians(theta)
    eye = (20.0 * np.sin(t), 0.0, 20.0 * np.cos(t))
    sd = _plane_scene(32, eye, [[LIGHT_INFINITE, 0, 0, 0, le, le, le]], kd, ks, roughness=alpha, fov=1.0, half=400.0, up=(0, 1, 0))
    sd.mat_eta = np.array([alpha], np.float32)  # (alpha itself, not a remapped roughness)
    kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(16, 16), seed=2, sampler="stratified")
    with gpu.Scene(sd) as sc:
        got = _rgb(sc.render(**kw)[0])[..., 1].mean()
    samples = []
    ref.render(sd, **dict(kw, spp=(4, 4)), samples=samples)  # 16 samples per pixel price one: the frame's mean has 256 x 1024 of them
    per_sample = np.stack(samples)[..., 1]
    se = per_sample.std(ddof=1) / np.sqrt(256 * 32 * 32)
    # the pixels' view angles: camera rays through the pixel centres, as DESIGN.md 3.2 forms them
    c2w = sd.cam_to_world.astype(np.float64)
    th = np.tan(np.radians(sd.fov) / 2)
    px = (np.arange(32) + 0.5) / 32 * 2 - 1
    dirs = np.stack([*np.meshgrid(px * th, -px * th, indexing="xy"), np.ones((32, 32))], -1) @ c2w[:3, :3].T
    cos_o = -dirs[..., 2] / np.linalg.norm(dirs, axis=-1)
    grid = np.linspace(np.arccos(cos_o.max()), np.arccos(cos_o.min()), 5)
    rho = np.interp(np.arccos(cos_o), grid, [ref.albedo(g, float(np.float32(alpha))) for g in grid]).mean()
    want = le * (kd[1] + ks[1] * rho)
    print(f"theta {theta} alpha {alpha}: mean {got:.6f}, closed form {want:.6f} (rho {rho:.5f}), 5 se {5 * se:.2e}")
    assert abs(got - want) <= 5 * se + 3e-6, (got, want, se)


# ---- 5. integrators 0 and 2 agree ----

def test_path_and_mis_agree(gpu):
    sd = scenes.plastic_scene(32, 32, light_scale=0.25, roughness=(0.05, 0.05, 0.05))
    kw = dict(max_depth=5, spp=(16, 16), seed=8, sampler="stratified")
    films, ses = [], []
    with gpu.Scene(sd) as sc:
        for integrator in (INTEGRATOR_PATH, INTEGRATOR_PATH_MIS):
            films.append(_rgb(sc.render(integrator=integrator, **kw)[0]))
            samples = []
            ref.render(sd, integrator=integrator, **dict(kw, spp=(4, 4)), samples=samples)  # the per-sample spread, from the reference
            s = np.stack(samples).reshape(16, 4, 8, 4, 8, 3).transpose(0, 2, 4, 1, 3, 5).reshape(16 * 64, 4, 4, 3)
            ses.append(s.var(0, ddof=1) / (256 * 64))
    blocks = [f.reshape(4, 8, 4, 8, 3).mean((1, 3)) for f in films]
    z = np.abs(blocks[0] - blocks[1]) / np.sqrt(ses[0] + ses[1] + 1e-30)
    print(f"integrators 0 and 2 over 8 x 8 blocks: largest z {z.max():.2f}")
    assert blocks[0].mean() > 0.05 and z.max() <= 5.0, z.max()


# ---- 6. the neighbours ----

def test_matte_scenes_are_untouched(gpu):
    """plastic_scene with matte in plastic's place renders through render_kernel; with one unused glass material beside it, through the GLS
    instantiations of render_kernel_x, which now carry the plastic branch: the same film, bit for bit"""
    sd = scenes.plastic_scene(32, 32, plastic=False)
    gls = dataclasses.replace(sd, materials=np.concatenate([sd.materials, [[GLASS, 1, 1, 1, 1, 1, 1]]]).astype(np.float32), mat_tex=np.zeros(0, np.uint32)).normalized()
    for kw in (dict(integrator=INTEGRATOR_PATH, sampler="stratified"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="halton")):
        kw = dict(kw, max_depth=5, spp=(4, 4), seed=5)
        with gpu.Scene(sd) as a, gpu.Scene(gls) as b:
            assert_bit_equal(a.render(**kw)[0], b.render(**kw)[0], f"matte through render_kernel vs through the GLS kernels, {kw}")


def test_glass_scene_is_untouched(gpu, oracle):
    """glass_sphere_scene against the oracle, which holds the arithmetic of before this material (tests/test_glass_env_parity_gpu.py)"""
    sd = scenes.glass_sphere_scene(32, 32)
    for kw in (dict(integrator=INTEGRATOR_PATH, sampler="stratified"), dict(integrator=INTEGRATOR_PATH_MIS, sampler="sobol_nd")):
        kw = dict(kw, max_depth=8, spp=(4, 4), seed=3)
        with gpu.Scene(sd) as sc:
            assert_bit_equal(sc.render(**kw)[0], oracle.OracleScene(sd).render(**kw)[0], f"glass_sphere_scene vs the oracle, {kw}")


# ---- 7. / 8. through every layer ----

def test_one_rank_multi_gpu_equals_single(gpu, plastic_box):
    kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(4, 4), seed=5, sampler="halton")
    with gpu.Scene(plastic_box) as sc:
        film = sc.render(**kw)[0]
    with gpu.MultiScene(plastic_box, n_gpus=1) as ms:
        assert_bit_equal(ms.render(**kw)[0], film, "in-library multi-GPU with one rank vs single-GPU")


def test_cli_renders_the_scene_file(gpu, tmp_path):
    from pbrt_amd import loader
    from pbrt_amd.build import CLI_PATH
    text = open(os.path.join(ROOT, "scenes", "plastic_spheres.pbrt")).read().replace("[256]", "[64]").replace('"integer pixelsamples" 64', '"integer pixelsamples" 16')
    ls = loader.load_string(text)
    assert (ls.scene.materials[:, 0] == PLASTIC).sum() == 3
    with gpu.Scene(ls.scene) as sc, gpu.Scene(scenes.plastic_scene(64, 64)) as gen:
        kw = dict(ls.render_kwargs(), seed=4)
        film = sc.render(**kw)[0]
        assert_bit_equal(gen.render(**kw)[0], film, "scenes.plastic_scene vs scenes/plastic_spheres.pbrt")
    with gpu.Scene(scenes.plastic_scene(64, 64, plastic=False)) as sc:
        matte = sc.render(**kw)[0]
    # plastic is not matte of the same Kd: the floor's and the spheres' reflections add up to a tenth of the scale somewhere (the reference's
    # two films differ by 0.108 at their most different pixel; at normal incidence the coat reflects 4 %, so a highlight is faint)
    assert np.abs(_rgb(film) - _rgb(matte)).mean(-1).max() > 0.05
    scene, out = tmp_path / "plastic.pbrt", tmp_path / "plastic.png"
    scene.write_text(text)
    r = subprocess.run([CLI_PATH, "-v", "--quick", "-o", str(out), str(scene)], capture_output=True, text=True)
    assert r.returncode == 0 and "wrote" in r.stderr and "not supported" not in r.stderr, r.stderr
    img = gpu.read_image(out)
    assert img.shape == (64, 64, 3) and img.std() > 0.05
