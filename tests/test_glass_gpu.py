"""The glass material on the GPU.  The oracle's own rendering of glass is compared bit for bit in tests/test_glass_env_parity_gpu.py; nothing here asks it: closed forms (the Fresnel curve,
index-matched glass, the furnace), the independent float64 reference of tests/independent_mc_glass.py, and the library against itself
(scene file = arrays, builders, shards, runs)."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import GLASS, INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_INFINITE, LIGHT_POINT, MATTE, SceneData, _lib, look_at, scenes
from util import assert_bit_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAWN_EPS = 1e-4  # kernels.hip kSpawnEps


def _quad(p0, p1, p2, p3):
    return [p0, p1, p2, p3], [[0, 1, 2], [0, 2, 3]]


# ---- A. the Fresnel curve ----

KR = np.array([0.9, 0.8, 0.7])
FRESNEL_EYE, FRESNEL_TILT, FRESNEL_FOV, FRESNEL_RES, FRESNEL_SPP = np.array([0.0, 0.0, 1.0]), 50.0, 60.0, 64, (32, 32)


def _fresnel_scene(inside):
    """A glass quad at z = 0 (eta 1.5, Kr (0.9, 0.8, 0.7), Kt 1) over a black matte quad at z = -1 under a constant sky of radiance 1; the
    camera at height 1 looks 50 degrees off the downward normal with a 60 degree field of view: the frame's middle column sees the quad at
    20 .. 80 degrees.  inside: the glass quad wound the other way -- its normal points down, so the camera's side is the medium."""
    h = 60.0
    v, t = _quad((-h, -h, 0), (h, -h, 0), (h, h, 0), (-h, h, 0))  # normal +z
    if inside:
        t = [[a, c, b] for a, b, c in t]
    v2, t2 = _quad((-h, -h, -1), (h, -h, -1), (h, h, -1), (-h, h, -1))
    a = np.radians(FRESNEL_TILT)
    look = FRESNEL_EYE + np.array([0.0, np.sin(a), -np.cos(a)])
    return SceneData(P=np.array(v + v2, np.float32), idx=np.array(t + [[4 + i for i in tri] for tri in t2], np.uint32), mat_id=np.array([0, 0, 1, 1], np.uint16),
                     materials=np.array([[GLASS, *KR, 1, 1, 1], [MATTE, 0, 0, 0, 0, 0, 0]], np.float32), mat_eta=np.array([1.5, 1.5], np.float32),
                     lights=np.array([[LIGHT_INFINITE, 0, 0, 0, 1, 1, 1]], np.float32),
                     cam_to_world=look_at(FRESNEL_EYE, look, (0, 0, 1))[1], fov=FRESNEL_FOV, xres=FRESNEL_RES, yres=FRESNEL_RES).normalized()


def _fresnel_cosines(at):
    """cos of the angle between the downward normal and the camera ray through raster point (x, y), float64, from the camera's definition
    (its own arithmetic: nothing of the library's); at: offsets into the pixel, e.g. (0.5, 0.5) = centres"""
    a = np.radians(FRESNEL_TILT)
    fwd = np.array([0.0, np.sin(a), -np.cos(a)])
    right = np.cross(np.array([0.0, 0.0, 1.0]), fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    t = np.tan(np.radians(FRESNEL_FOV) / 2)
    x, y = np.meshgrid(np.arange(FRESNEL_RES) + at[0], np.arange(FRESNEL_RES) + at[1])
    d = ((2 * x / FRESNEL_RES - 1) * t)[..., None] * right + ((1 - 2 * y / FRESNEL_RES) * t)[..., None] * up + fwd
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return -d[..., 2]


def _blocks(a, b=8):
    return a.reshape(a.shape[0] // b, b, a.shape[1] // b, b, *a.shape[2:]).mean((1, 3))


def _fresnel_excess(rgb, eta_i, eta_t, use):
    """-> per block and channel: |block mean - Kr F| - (5 Kr sqrt(F (1 - F) / N) + 0.4 % Kr F), with F the float64 Fresnel reflectance averaged
    over the block's pixel centres and N the block's samples (the binomial's own standard error: nothing taken from the render)"""
    import independent_mc_glass as g
    F = _blocks(g.fr_dielectric(_fresnel_cosines((0.5, 0.5)), eta_i, eta_t))
    n = 64 * FRESNEL_SPP[0] * FRESNEL_SPP[1]
    want = F[..., None] * KR
    bound = 5 * KR * np.sqrt(F * (1 - F) / n)[..., None] + 0.004 * want
    got = _blocks(rgb.astype(np.float64))
    return np.where(use[..., None], np.abs(got - want) - bound, -np.inf), got, want, bound


@pytest.mark.parametrize("sampler", ["stratified", "halton"])
def test_fresnel_curve_off_a_glass_quad(gpu, sampler):
    """A sample is Kr (reflected into the sky) or 0 (refracted into the black floor): an 8 x 8 block mean is a binomial estimate of Kr F(theta)."""
    cos_c = _fresnel_cosines((0.5, 0.5))
    assert np.degrees(np.arccos(cos_c[:, 32])).min() < 21 and np.degrees(np.arccos(cos_c[:, 32])).max() > 79
    with gpu.Scene(_fresnel_scene(False)) as sc:
        film, _ = sc.render(integrator=INTEGRATOR_PATH, max_depth=4, spp=FRESNEL_SPP, seed=5, sampler=sampler)
    rgb = gpu.film_to_rgb(film)
    every = np.ones((8, 8), bool)
    ex, got, want, bound = _fresnel_excess(rgb, 1.0, 1.5, every)
    print(f"fresnel outside {sampler}: largest |got - want| / bound = {(np.abs(got - want) / bound).max():.3f}")
    assert ex.max() <= 0, (float(ex.max()), np.unravel_index(ex.argmax(), ex.shape))
    # negative control: the same film is NOT the curve of water
    ex133, _, _, _ = _fresnel_excess(rgb, 1.0, 1.33, every)
    assert ex133.max() > 0
    # from inside the medium: beyond the critical angle (41.8 degrees) every sample reflects with weight exactly Kr
    with gpu.Scene(_fresnel_scene(True)) as sc:
        film, _ = sc.render(integrator=INTEGRATOR_PATH, max_depth=4, spp=FRESNEL_SPP, seed=5, sampler=sampler)
    rgb = gpu.film_to_rgb(film)
    corner = np.stack([_fresnel_cosines(c) for c in ((0, 0), (1, 0), (0, 1), (1, 1))])
    ang_lo = np.degrees(np.arccos(corner.max(0))).reshape(8, 8, 8, 8).min((1, 3))  # the smallest / largest angle in a block, over pixel corners
    ang_hi = np.degrees(np.arccos(corner.min(0))).reshape(8, 8, 8, 8).max((1, 3))
    crit = np.degrees(np.arcsin(1 / 1.5))
    tir = ang_lo > crit + 0.25
    assert tir.sum() >= 24, tir.sum()
    got = _blocks(rgb.astype(np.float64))
    dev = np.abs(got - KR)[tir].max()
    print(f"fresnel inside {sampler}: total reflection blocks {tir.sum()}, largest |mean - Kr| = {dev:.3g}")
    assert dev <= 1e-6, dev
    # below it the binomial comparison again (blocks that end 4 degrees or more under the critical angle: nearer to it F has a square-root
    # singularity, and its mean over pixel centres is not its mean over the block)
    sub = ang_hi < crit - 4.0
    assert sub.sum() >= 8, sub.sum()
    ex, got, want, bound = _fresnel_excess(rgb, 1.5, 1.0, sub)
    print(f"fresnel inside {sampler}: {sub.sum()} blocks under the critical angle, largest |got - want| / bound = {(np.abs(got - want) / bound)[sub].max():.3f}")
    assert ex.max() <= 0, float(ex.max())


# ---- B. index-matched glass is invisible ----

def _lit_scene(res, with_box):
    """A matte floor with a low pyramid under a point light (the style of tests/util.py's lit scenes), seen from (0, -2.5, 3); with_box: a
    closed glass box of eta 1, Kr = Kt = 1 around the camera."""
    eye, light = np.array([0.0, -2.5, 3.0]), np.array([1.5, 1.0, 4.0])
    V, I, M = [], [], []
    v, t = _quad((-20, -20, 0), (20, -20, 0), (20, 20, 0), (-20, 20, 0))
    V += v; I += t; M += [0, 0]
    apex, b = (0.2, 0.6, 0.35), 0.45
    base = [(0.2 - b, 0.6 - b, 0), (0.2 + b, 0.6 - b, 0), (0.2 + b, 0.6 + b, 0), (0.2 - b, 0.6 + b, 0)]
    n0 = len(V)
    V += base + [apex]
    I += [[n0 + k, n0 + (k + 1) % 4, n0 + 4] for k in range(4)]
    M += [1] * 4
    mats = [[MATTE, 0.6, 0.5, 0.4, 0, 0, 0], [MATTE, 0.7, 0.7, 0.3, 0, 0, 0]]
    half = 0.3
    if with_box:
        import independent_mc_glass as g
        bv, bi = g._cube_mesh(half)
        n0 = len(V)
        V += [tuple(np.float32(p) + np.float32(eye)) for p in bv]
        I += [[n0 + int(a) for a in tri] for tri in bi]
        M += [2] * len(bi)
        mats.append([GLASS, 1, 1, 1, 1, 1, 1])
    sd = SceneData(P=np.array(V, np.float32), idx=np.array(I, np.uint32), mat_id=np.array(M, np.uint16), materials=np.array(mats, np.float32),
                   mat_eta=np.ones(len(mats), np.float32), lights=np.array([[LIGHT_POINT, *light, 40, 40, 40]], np.float32),
                   cam_to_world=look_at(eye, (0, 0.3, 0), (0, 0, 1))[1], fov=40.0, xres=res, yres=res).normalized()
    return sd, eye, light, half, np.array(V, np.float64)[:n0 if with_box else len(V)]


def test_index_matched_glass_is_invisible(gpu):
    res = 128
    plain, eye, light, half, mesh = _lit_scene(res, False)
    boxed = _lit_scene(res, True)[0]
    # the geometry the bound rests on, from the test's own numbers: the light is outside the box; every shadow ray starts on the mesh at
    # y >= -1.8 (the floor nearer than the frame's lower edge is not visible: checked below) and ends at the light's y = 1, so it
    # never comes near the box, which ends at y = -2.2; d_min is the smallest distance from the light to any point of the mesh (its plane
    # z = 0 and the pyramid's apex)
    assert np.abs(light - eye).max() > half and eye[1] + half < -1.8 and light[1] > eye[1] + half
    d_min = min(light[2], np.linalg.norm(light - mesh[8]))
    # ONE sample per pixel: a sample's camera request comes first, so both renders trace the same camera rays; the samples of a pixel share
    # one random stream, so with more of them the glass vertex's extra request would shift the jitter of every later sample
    kw = dict(integrator=INTEGRATOR_DIRECT, spp=(1, 1), seed=3, sampler="stratified")
    with gpu.Scene(plain) as sc:
        a = gpu.film_to_rgb(sc.render(max_depth=1, **kw)[0]).astype(np.float64)
    with gpu.Scene(boxed) as sc:
        b = gpu.film_to_rgb(sc.render(max_depth=2, **kw)[0]).astype(np.float64)  # one interface crossed: one bounce more
    assert a.max() > 0.05 and np.isfinite(b).all()
    # the nearest visible floor point (image rows are lines y = const of the floor: the camera does not roll): the frame's lower edge is 20
    # degrees under the axis, which points atan(3 / 2.8) = 47 degrees under the horizon
    low = np.radians(20.0) + np.arctan2(eye[2], 0.3 - eye[1])
    assert eye[1] + eye[2] / np.tan(low) > -1.8
    # smooth pixels, from the glass-less render alone: no relative step above 5 % in the 3 x 3 neighbourhood
    lum = a.sum(-1)
    pad = np.pad(lum, 1, mode="edge")
    nb = np.stack([pad[1 + dy:1 + dy + res, 1 + dx:1 + dx + res] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    smooth = (nb.max(0) - nb.min(0)) <= 0.05 * nb.max(0)
    excluded = 1 - smooth.mean()
    bound = 8 * SPAWN_EPS / d_min
    rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-30)
    rel = np.where(a == 0, np.where(b == 0, 0.0, np.inf), rel)
    worst = rel[smooth].max()
    print(f"index-matched glass: {100 * excluded:.1f} % of the pixels masked, d_min {d_min:.3f}, bound {bound:.3g}, largest relative difference {worst:.3g}, "
          f"pixels that differ at all {(a != b).any(-1).mean():.3f}")
    assert excluded <= 0.10, excluded
    assert worst <= bound, (worst, bound)


# ---- C. the furnace ----

@pytest.mark.parametrize("eta", [1.5, 2.4])
@pytest.mark.parametrize("kind", ["sphere", "cube"])
def test_furnace(gpu, kind, eta):
    """A glass object alone under a constant sky returns the sky: sees a wrong eta_i^2 / eta_t^2, a spawn point on the wrong side of the
    surface, energy lost at total internal reflection.  The standard error is the reference's own (its furnace run, same roulette rule and
    depth), scaled to the library's samples per block."""
    import independent_mc_glass as g
    _, se_ref, cnt_ref = g.furnace_block_means(kind, eta)
    sd = g.furnace_scene(kind, eta)
    spp = (16, 16)
    n_block = 64 * spp[0] * spp[1]
    se = se_ref * np.sqrt(cnt_ref / n_block)[..., None]
    worst = 0.0
    for builder in (None, "host"):
        with gpu.Scene(sd, builder=builder) as sc:
            for integrator in (INTEGRATOR_PATH, INTEGRATOR_PATH_MIS):
                for sampler in ("stratified", "halton"):
                    film, _ = sc.render(integrator=integrator, max_depth=g.FURNACE_DEPTH, spp=spp, seed=11, sampler=sampler)
                    rgb = gpu.film_to_rgb(film).astype(np.float64)
                    got = _blocks(rgb)
                    z = np.abs(got - g.ENV) / (5 * se + 0.004 * g.ENV)
                    rel = rgb.sum((0, 1)) / (g.ENV * rgb.shape[0] * rgb.shape[1]) - 1
                    worst = max(worst, float(z.max()))
                    print(f"furnace {kind} eta {eta} builder {builder} integrator {integrator} {sampler}: largest |mean - sky| / (5 se + 0.4 %) = {z.max():.3f}, "
                          f"image sum {rel.round(5).tolist()}, darkest block {float((got / g.ENV).min()):.4f}")
                    assert z.max() <= 1.0, (builder, integrator, sampler, float(z.max()))
                    assert np.abs(rel).max() < 6e-3, (builder, integrator, sampler, rel)
    assert worst > 0  # (the object is in the frame: some block is not the sky seen directly)


# ---- D. against the independent reference ----

def test_box_with_glass_sphere_matches_the_independent_reference(gpu):
    import independent_mc_glass as g
    mean, se = g.block_means(64, 64, 8, g.BOX_DEPTH, g.BOX_PATHS)
    with gpu.Scene(g.glass_box_scene(64, 64)) as sc:
        for kw in (dict(), dict(integrator=INTEGRATOR_PATH_MIS), dict(sampler="halton"), dict(sampler="halton", integrator=INTEGRATOR_PATH_MIS)):
            film, _ = sc.render(max_depth=g.BOX_DEPTH, spp=(64, 64), seed=2, **kw)
            z, rel = g.compare_with_blocks(gpu.film_to_rgb(film), mean, se, 8)
            print(f"glass box vs reference {kw}: z {z:.3f}, image sum {rel:+.5f}")
            assert z < 5.0 and abs(rel) < 6e-3, (kw, z, rel)
    # negative control: another index is seen
    with gpu.Scene(g.glass_box_scene(64, 64, eta=1.3)) as sc:
        film, _ = sc.render(max_depth=g.BOX_DEPTH, spp=(64, 64), seed=2)
    z, rel = g.compare_with_blocks(gpu.film_to_rgb(film), mean, se, 8)
    print(f"glass box, eta 1.3 against the reference for 1.5: z {z:.3f}")
    assert z > 6.0, z


# ---- E. through every layer ----

def test_scene_file_cli_builders_shards_and_runs(gpu, tmp_path):
    from pbrt_amd import loader
    from pbrt_amd.build import CLI_PATH
    text = open(os.path.join(ROOT, "scenes", "glass_sphere.pbrt")).read().replace("[256]", "[128]").replace('"integer pixelsamples" 64', '"integer pixelsamples" 16')
    ls = loader.load_string(text)
    assert not ls.warnings and (ls.scene.xres, ls.scene.yres) == (128, 128) and (ls.scene.materials[:, 0] == GLASS).sum() == 2
    kw = dict(ls.render_kwargs(), seed=4)
    with gpu.Scene(ls.scene) as sc:
        film, st = sc.render(**kw)
        again, _ = sc.render(**kw)
        parts = [sc.render(rank=r, world_size=2, **kw)[0] for r in range(2)]
        for flags in (True, "walk"):  # the counting instantiations do not exist for glass
            with pytest.raises(_lib.PbrtHipError) as e:
                sc.render(counters=flags, **dict(kw, sampler="stratified", integrator=INTEGRATOR_PATH))  # (the table samplers and MIS refuse the flags on their own)
            assert e.value.code == -4 and "glass" in str(e.value)
    rgb = gpu.film_to_rgb(film)
    assert np.isfinite(rgb).all() and rgb.mean() > 0.05 and rgb[75:100, 72:97].std() > 0.01  # lit, and something is seen in the sphere
    assert_bit_equal(again, film, "two runs")
    assert_bit_equal(parts[0] + parts[1], film, "two shards assembled")
    with gpu.Scene(scenes.glass_sphere_scene(128, 128)) as sc:
        assert_bit_equal(sc.render(**kw)[0], film, "scenes.glass_sphere_scene vs scenes/glass_sphere.pbrt")
    for builder in ("gpu", "host", "gpu-plain", "host-optimized"):
        with gpu.Scene(ls.scene, builder=builder) as sc:
            assert_bit_equal(sc.render(**kw)[0], film, f"builder {builder}")
    # the same scene with mirrors in place of glass is another image (the GLS branch is what ran)
    with gpu.Scene(scenes.glass_sphere_scene(128, 128, glass=False)) as sc:
        assert not np.array_equal(sc.render(**kw)[0], film)
    # the native command line renders the file
    scene = tmp_path / "glass.pbrt"
    scene.write_text(text)
    out = tmp_path / "glass.png"
    r = subprocess.run([CLI_PATH, "-v", "--quick", "-o", str(out), str(scene)], capture_output=True, text=True)
    assert r.returncode == 0 and "wrote" in r.stderr and "not supported" not in r.stderr, r.stderr
    img = gpu.read_image(out)
    assert img.shape == (128, 128, 3) and img.std() > 0.05
