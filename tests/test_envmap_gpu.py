"""Environment-map infinite lights on the GPU.  The oracle's own rendering of a map is compared bit for bit in tests/test_glass_env_parity_gpu.py; nothing here asks it: the device against
the host bit for bit (pbrt_amd/csrc/envmap_core.hpp is one piece of arithmetic), closed forms (the camera sees the texels, a uniform map is
the constant sky, a one-texel sun), the independent float64 program of tests/independent_envmap.py, the furnace, and the library against
itself (runs, builders, scene file = arrays, shards, render_multi)."""
import os

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import (GLASS, INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_ENVMAP, LIGHT_INFINITE, MATTE, MIRROR, SceneData, _lib, loader,
                      look_at, scenes)
from test_envmap_host import f64_texel, random_map, random_rotation, rot_x, sun_map
from util import assert_bit_equal, lit_plane_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])


def _blocks(a, b=8):
    return a.reshape(a.shape[0] // b, b, a.shape[1] // b, b, *a.shape[2:]).mean((1, 3))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- A. one piece of arithmetic ----

def test_device_hook_equals_host_hook(gpu):
    """Sample, lookup and pdf over 2^20 inputs: the kernel that calls envmap_core.hpp on the device returns the bits the host returns --
    the project's fp32 contract for the piece written once for host and device (the oracle's restatement of it: tests/test_oracle_glass_env.py)."""
    n = 1 << 20
    rgb, m = random_map(16, 32, 31), random_rotation(8).astype(np.float32)
    rng = np.random.default_rng(77)
    u12 = rng.random((n, 2), dtype=np.float32)
    u12[:4] = [[0, 0], [0.99999994, 0.99999994], [0, 0.99999994], [0.5, 0]]
    dirs = rng.normal(size=(n, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    dirs[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    with gpu.Scene(scenes.envmap_scene(8, 8, sky=rgb, world_to_light=m)) as sc:
        dev_s = sc.envmap_eval(u12=u12)
        dev_l = sc.envmap_eval(d=dirs)
        assert sc.info()["device_bytes"] >= 16 * 512 + 4 * 17 + 4 * 16 * 33
    host_s = pbrt_amd.api.envmap_eval_host(rgb, m, u12=u12)
    host_l = pbrt_amd.api.envmap_eval_host(rgb, m, d=dirs)
    for what, dev, host in (("sample", dev_s, host_s), ("lookup", dev_l, host_l)):
        for name, a, b in zip(("d", "texel", "le", "pdf"), dev, host):
            diff = int((_bits(a) != _bits(b)).sum())
            print(f"{what} {name}: {diff} of {a.size} words differ")
            assert diff == 0, (what, name, diff)
    assert len(np.unique(host_s[1])) == 512  # (every texel was drawn)
    with gpu.Scene(scenes.check_sphere_scene(8, 8)) as sc:  # a scene without a map has nothing to evaluate
        with pytest.raises(_lib.PbrtHipError) as e:
            sc.envmap_eval(d=dirs[:4])
        assert e.value.code == -1


# ---- B. the camera sees the map ----

def _camera_dirs(eye, look, res, fov, at):
    """unit direction of the camera ray through raster point (x + at[0], y + at[1]) of every pixel, float64, from the camera's definition"""
    fwd = np.asarray(look, np.float64) - np.asarray(eye, np.float64)
    fwd /= np.linalg.norm(fwd)
    right = np.cross(np.array([0.0, 0.0, 1.0]), fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    t = np.tan(np.radians(fov) / 2)
    x, y = np.meshgrid(np.arange(res) + at[0], np.arange(res) + at[1])
    d = ((2 * x / res - 1) * t)[..., None] * right + ((1 - 2 * y / res) * t)[..., None] * up + fwd
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


@pytest.mark.parametrize("rotated", [False, True])
def test_camera_sees_the_map(gpu, rotated):
    """128 x 128, fov 90, a 32 x 16 random map, a lone triangle behind the camera.  A pixel whose four corners and centre map to one texel (float64,
    the test's own camera arithmetic) holds that texel x c to 3e-6 relative, at 1 and at 4 samples per pixel.  Compared in the film's own
    XYZ (the film stores XYZ; film_to_rgb's matrix is the inverse of rgb -> xyz only to 4e-6, which is not the map's business)."""
    res, fov, h, w = 128, 90.0, 16, 32
    sky = random_map(h, w, 41, hdr=False)
    c = np.array([1.25, 0.5, 2.0], np.float32)
    m = random_rotation(17) if rotated else np.eye(3)
    views = [(0.3, 1, 0.2), (1, 0.2, 0.9), (-0.5, -0.4, -0.8)] if not rotated else [(0.3, 1, 0.2)]
    for look in views:
        sd = SceneData(P=np.array([(-1, -5, -1), (1, -5, -1), (0, -5, 1)], np.float32) - np.float32(30) * np.array(look, np.float32) / np.float32(np.linalg.norm(look)),
                       idx=np.array([(0, 1, 2)], np.uint32), mat_id=np.zeros(1, np.uint16), materials=np.array([[MATTE, .5, .5, .5, 0, 0, 0]], np.float32),
                       lights=np.array([[LIGHT_ENVMAP, 0, 0, 0, *c]], np.float32), envmap=sky, envmap_world_to_light=m,
                       cam_to_world=look_at((0, 0, 0), look, (0, 0, 1))[1], fov=fov, xres=res, yres=res).normalized()
        pts = [f64_texel(_camera_dirs((0, 0, 0), look, res, fov, at).reshape(-1, 3), m, h, w) for at in ((0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0.5))]
        tex = np.stack([r * w + cl for r, cl, _, _ in pts])
        one = (tex == tex[-1]).all(0).reshape(res, res)
        texel = tex[-1].reshape(res, res)
        left_out = 1 - one.mean()
        want_rgb = (sky.reshape(-1, 3)[texel] * c).astype(np.float64)  # (the kernel's product, in fp32)
        want = want_rgb @ RGB_TO_XYZ.T
        print(f"look {look} rotated {rotated}: {100 * left_out:.1f} % of the pixels straddle texels, {len(np.unique(texel[one]))} distinct texels seen")
        assert left_out <= 0.25 and len(np.unique(texel[one])) >= 50
        with gpu.Scene(sd) as sc:
            for spp in ((1, 1), (2, 2)):
                for kw in (dict(integrator=INTEGRATOR_PATH), dict(integrator=INTEGRATOR_PATH_MIS, sampler="halton")):
                    film, _ = sc.render(max_depth=3, spp=spp, seed=3, **kw)
                    assert (film[..., 3] == spp[0] * spp[1]).all()
                    got = film[..., :3].astype(np.float64) / film[..., 3:]
                    rel = np.abs(got / want - 1.0)[one]
                    print(f"  spp {spp} {kw}: largest relative difference {rel.max():.3g}")
                    assert rel.max() <= 3e-6, (look, spp, kw, float(rel.max()))
                    # the other pixels hold a mixture of their corners' neighbourhood: never more than the map's largest texel
                    assert (got <= ((sky * c).astype(np.float64) @ RGB_TO_XYZ.T).max((0, 1)) * (1 + 1e-5)).all()


# ---- C. a uniform map is the constant sky ----

@pytest.mark.parametrize("sampler", ["stratified", "halton"])
@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS])
def test_uniform_map_is_the_constant_sky(gpu, integrator, sampler):
    """A matte plane of albedo rho under a map that is L everywhere: every 8 x 8 block mean is rho L within 5 standard errors + 0.4 %.
    The standard error is the estimator's own, in closed form: a light sample is (rho / pi) L cos / pdf with pdf = 1 / (4 pi) over the
    whole sphere, i.e. X = 4 rho L cos+ of a uniform direction: E X = rho L, E X^2 = 16 rho^2 L^2 / 6, sd X = rho L sqrt(5 / 3); a
    block has 64 spp samples.  (The map is 64 x 32: its density is constant per texel in (u, v), which differs from the uniform sphere
    by sin(row centre) / sin(theta), a few per cent away from the poles.  MIS only lowers the variance.)"""
    sd, _ = lit_plane_scene("infinite", res=64)
    rho = sd.materials[0, 1:4].astype(np.float64)
    L = np.array([0.5, 0.25, 1.0])
    sd.lights = np.array([[LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32)
    sd.envmap = np.broadcast_to(L.astype(np.float32), (32, 64, 3)).copy()
    sd.envmap_world_to_light = random_rotation(5)
    spp = (16, 16)
    se = np.sqrt(5.0 / 3.0) * rho * L / np.sqrt(64 * spp[0] * spp[1])
    with gpu.Scene(sd.normalized()) as sc:
        film, _ = sc.render(integrator=integrator, max_depth=5, spp=spp, seed=9, sampler=sampler)
    got = _blocks(gpu.film_to_rgb(film).astype(np.float64))
    z = np.abs(got - rho * L) / (5 * se + 0.004 * rho * L)
    print(f"uniform map, integrator {integrator} {sampler}: largest |block - rho L| / (5 se + 0.4 %) = {z.max():.3f}; image mean / (rho L) = {(got.mean((0, 1)) / (rho * L)).round(5).tolist()}")
    assert z.max() <= 1.0, float(z.max())


# ---- D. a one-texel sun ----

SUN_ROW, SUN_COL, SUN_L = 9, 17, np.array([500.0, 450.0, 300.0])


def _sun_plane(res, occluder):
    """lit_plane_scene's matte plane and camera under a 64 x 32 map that is black but for texel (9, 17) -- 50.6 .. 56.3 degrees from the zenith,
    well above the horizon --; occluder: a matte square of half-width 0.6 at height 1 whose shadow, along the texel's central direction,
    is centred on the point the camera looks at."""
    sd, _ = lit_plane_scene("infinite", res=res)
    sd.lights = np.array([[LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32)
    sd.envmap = sun_map(32, 64, SUN_ROW, SUN_COL, SUN_L)
    th, ph = (SUN_ROW + 0.5) * np.pi / 32, (SUN_COL + 0.5) * 2 * np.pi / 64
    d = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    centre = np.array([0.2, 0.3, 0.0]) + d / d[2]  # on z = 1
    if occluder:
        q = [(centre[0] - 0.6, centre[1] - 0.6, 1.0), (centre[0] + 0.6, centre[1] - 0.6, 1.0), (centre[0] + 0.6, centre[1] + 0.6, 1.0), (centre[0] - 0.6, centre[1] + 0.6, 1.0)]
        sd.P = np.concatenate([sd.P, np.array(q, np.float32)])
        sd.idx = np.concatenate([sd.idx, np.array([(4, 5, 6), (4, 6, 7)], np.uint32)])
        sd.mat_id = np.zeros(4, np.uint16)
    return sd.normalized(), d, centre


@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_PATH_MIS])
def test_one_texel_sun(gpu, integrator):
    """Every lit pixel of the plane is rho / pi x L_s x the integral of cos theta over the texel's solid angle (float64 quadrature), within 5
    standard errors of the integrand's own spread inside the texel + 0.1 %: a light sample lands uniformly in the texel's (u, v), where it is
    (rho / pi) L_s cos(theta) sin(theta) 2 pi^2 / (W H), so its spread is that of cos sin over the texel's 5.6 degrees of theta -- under 2 %.
    A sampler that does not follow the map would hit the texel once in 2048 tries and be off by orders of magnitude in noise (64 samples
    per pixel: most pixels black, the others 30 times too bright).  Under the occluder the umbra is exactly 0; pixels whose plane point lies
    within 0.3 of the shadow's edge (the penumbra of a 5.6-degree light at height 1 is 0.15 wide), or that see the occluder itself, are left
    out.  With MIS the value is the same within the same bound: the bounce ray that finds the sun carries a weight of a few 1e-6."""
    res, spp, W, H = 64, (8, 8), 64, 32
    n = spp[0] * spp[1]
    t0, t1 = SUN_ROW * np.pi / H, (SUN_ROW + 1) * np.pi / H
    th = t0 + (np.arange(4000) + 0.5) * (t1 - t0) / 4000
    integral = (2 * np.pi / W) * (np.cos(th) * np.sin(th)).mean() * (t1 - t0)
    assert abs(integral - (2 * np.pi / W) * 0.5 * (np.sin(t1) ** 2 - np.sin(t0) ** 2)) < 1e-9
    g = np.cos(th) * np.sin(th)
    for occluder in (False, True):
        sd, d_sun, centre = _sun_plane(res, occluder)
        rho = sd.materials[0, 1:4].astype(np.float64)
        want = rho / np.pi * SUN_L * integral
        se = want * (g.std() / g.mean()) / np.sqrt(n)
        with gpu.Scene(sd) as sc:
            film, _ = sc.render(integrator=integrator, max_depth=1, spp=spp, seed=6, sampler="stratified")
        rgb = gpu.film_to_rgb(film).astype(np.float64)
        # where each pixel's five points meet the plane, from the camera's definition
        eye = np.array([1.0, -2.0, 3.0])
        lit = np.ones((res, res), bool)
        dark = np.ones((res, res), bool)
        for at in ((0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0.5)):
            dirs = _camera_dirs(eye, (0.2, 0.3, 0.0), res, 40.0, at)
            p = eye + dirs * (-eye[2] / dirs[..., 2])[..., None]
            if occluder:
                dist = np.maximum(np.abs(p[..., 0] - 0.2), np.abs(p[..., 1] - 0.3))  # from the shadow's centre, in the max norm
                q = eye + dirs * ((1.0 - eye[2]) / dirs[..., 2])[..., None]         # where the ray crosses the occluder's height
                sees = np.maximum(np.abs(q[..., 0] - centre[0]), np.abs(q[..., 1] - centre[1])) < 0.6 + 0.05
                lit &= (dist > 0.6 + 0.3) & ~sees
                dark &= (dist < 0.6 - 0.3) & ~sees
            else:
                dark &= False
        z = (np.abs(rgb - want) / (5 * se + 0.001 * want))[lit]
        print(f"sun, integrator {integrator}, occluder {occluder}: {lit.sum()} lit pixels, largest |pixel - closed form| / (5 se + 0.1 %) = {z.max():.3f} "
              f"(se / value {float((se / want)[0]):.4f}); {dark.sum()} umbra pixels, largest value {rgb[dark].max(initial=0):.3g}")
        assert lit.sum() >= (1500 if occluder else res * res) and z.max() <= 1.0, float(z.max())
        if occluder:
            assert dark.sum() >= 30 and (rgb[dark] == 0).all()


# ---- E. against the independent program ----

def test_matches_the_independent_program(gpu):
    """Ground, matte sphere and mirror sphere under a smooth sky (max / mean < 2: the reference has no light sampling), depth 5: every 8 x 8
    block within 5 of the reference's own standard errors + 0.4 %, the image sum within 0.5 %; integrators 0 and 2, two samplers, and a
    rotated map.  Negative control: the same film against the reference for the map turned by 90 degrees."""
    import independent_envmap as ie
    res = 64
    sky = ie.smooth_sky()
    for m in (np.eye(3), rot_x(-90.0) @ random_rotation(2)):
        mean, se = ie.block_means(res, sky, m)
        assert (se / mean).max() < 0.02
        with gpu.Scene(ie.scene_data(res, sky, m)) as sc:
            for kw in (dict(integrator=INTEGRATOR_PATH), dict(integrator=INTEGRATOR_PATH_MIS), dict(integrator=INTEGRATOR_PATH_MIS, sampler="halton")):
                # (128 x 128 samples per pixel: the bound holds the REFERENCE's noise alone, so the library's own must be small beside it --
                # without MIS a light sample of a smooth sky is 4 rho L cos+, sd 1.3 x its mean: 0.13 % per block at a million samples)
                film, _ = sc.render(max_depth=ie.DEPTH, spp=(128, 128), seed=12, **kw)
                got = _blocks(gpu.film_to_rgb(film).astype(np.float64))
                zz = np.abs(got - mean) / (5 * se + 0.004 * mean)
                z = zz.max()
                rel = got.sum() / mean.sum() - 1
                print(f"independent program, map {'rotated' if m[0, 0] != 1 else 'as is'} {kw}: largest |block - ref| / (5 se + 0.4 %) = {z:.3f} at block / channel "
                      f"{np.unravel_index(zz.argmax(), zz.shape)} (reference se / mean there {float((se / mean).reshape(-1)[zz.argmax()]):.4f}), image sum {rel:+.5f}")
                assert z <= 1.0 and abs(rel) < 5e-3, (kw, float(z), float(rel))
    other, other_se = ie.block_means(res, sky, rot_x(90.0) @ m, paths=64)
    assert (np.abs(got - other) / (5 * other_se + 0.004 * other)).max() > 1.5


# ---- F. the furnace ----

def test_furnace(gpu):
    """A glass sphere, and a mirror sphere, alone under a uniform map return the map (tests/test_glass_gpu.py's furnace with the constant sky
    replaced by a map of the same radiance; the standard error is the glass reference's own, scaled to the samples per block)."""
    import independent_mc_glass as g
    _, se_ref, cnt_ref = g.furnace_block_means("sphere", 1.5)
    spp = (16, 16)
    se = se_ref * np.sqrt(cnt_ref / (64 * spp[0] * spp[1]))[..., None]
    sd = g.furnace_scene("sphere", 1.5)
    sd.lights = np.array([[LIGHT_ENVMAP, 0, 0, 0, 0.5, 0.5, 0.5]], np.float32)
    sd.envmap = np.broadcast_to((2 * g.ENV).astype(np.float32), (8, 16, 3)).copy()
    sd.envmap_world_to_light = random_rotation(1)
    with gpu.Scene(sd.normalized()) as sc:
        for integrator in (INTEGRATOR_PATH, INTEGRATOR_PATH_MIS):
            film, _ = sc.render(integrator=integrator, max_depth=g.FURNACE_DEPTH, spp=spp, seed=11, sampler="halton")
            got = _blocks(gpu.film_to_rgb(film).astype(np.float64))
            z = np.abs(got - g.ENV) / (5 * se + 0.004 * g.ENV)
            print(f"furnace, glass sphere, integrator {integrator}: largest |mean - map| / (5 se + 0.4 %) = {z.max():.3f}, darkest block {float((got / g.ENV).min()):.4f}")
            assert z.max() <= 1.0 and (got != g.ENV).any()
    sd.materials = np.array([[MIRROR, 1, 1, 1, 0, 0, 0]], np.float32)
    with gpu.Scene(sd.normalized()) as sc:
        film, _ = sc.render(max_depth=4, spp=(2, 2), seed=1)
    rgb = gpu.film_to_rgb(film).astype(np.float64)
    assert np.abs(rgb / g.ENV - 1).max() < 5e-6  # every path ends in the map, whatever it hit first


# ---- G. the library against itself ----

def test_scene_file_builders_shards_and_runs(gpu, monkeypatch):
    text = open(os.path.join(ROOT, "scenes", "envmap_spheres.pbrt")).read().replace("[256]", "[128]").replace('"integer pixelsamples" 64', '"integer pixelsamples" 16')
    ls = loader.load_string(text, base_dir=os.path.join(ROOT, "scenes"))
    assert not ls.warnings and (ls.scene.xres, ls.scene.yres) == (128, 128) and ls.scene.envmap.shape == (32, 64, 3)
    kw = dict(ls.render_kwargs(), seed=4)
    with gpu.Scene(ls.scene) as sc:
        film, st = sc.render(**kw)
        again, _ = sc.render(**kw)
        parts = [sc.render(rank=r, world_size=3, **kw)[0] for r in range(3)]
        plain = dict(kw, sampler="stratified", integrator=INTEGRATOR_PATH)
        for flags in (True, "walk"):  # the counting instantiations do not exist for a map
            with pytest.raises(_lib.PbrtHipError) as e:
                sc.render(counters=flags, **plain)
            assert e.value.code == -4 and "environment map" in str(e.value)
        with pytest.raises(_lib.PbrtHipError) as e:  # nor does the wide box filter: a refused combination, named
            sc.render(**dict(plain, filter_width=(1.5, 1.5)))
        assert e.value.code == -4 and "environment map" in str(e.value) and "box filter" in str(e.value)
        other = sc.render(**dict(kw, integrator=INTEGRATOR_PATH))[0]
    rgb = gpu.film_to_rgb(film)
    assert np.isfinite(rgb).all() and rgb.mean() > 0.05 and rgb[:20].mean() > 0.2 and rgb[60:90, 70:100].std() > 0.01  # sky above, something in the mirror
    assert_bit_equal(again, film, "two runs")
    assert_bit_equal(parts[0] + parts[1] + parts[2], film, "three shards assembled")
    assert abs(gpu.film_to_rgb(other).mean() / rgb.mean() - 1) < 0.03 and not np.array_equal(other, film)  # without MIS: the same picture, other samples
    with gpu.Scene(scenes.envmap_scene(128, 128)) as sc:
        assert_bit_equal(sc.render(**kw)[0], film, "scenes.envmap_scene vs scenes/envmap_spheres.pbrt")
    for builder in ("gpu", "host", "gpu-plain", "host-optimized"):
        with gpu.Scene(ls.scene, builder=builder) as sc:
            assert_bit_equal(sc.render(**kw)[0], film, f"builder {builder}")
    one, _ = gpu.render_multi(ls.scene, 1, **kw)
    assert_bit_equal(one, film, "pbrt_hip_render_multi on one GPU")
    monkeypatch.setenv("PBRT_HIP_MULTI_LOOPBACK", "1")  # three ranks on this GPU: every rank renders from a CLONE of the scene, map and tables included
    three, _ = gpu.render_multi(ls.scene, 3, **kw)
    assert_bit_equal(three, film, "pbrt_hip_render_multi, three ranks")
    # the same scene under a constant sky is another picture (the map is what was rendered) ...
    with gpu.Scene(scenes.envmap_scene(128, 128, constant=True)) as sc:
        const_film, _ = sc.render(**kw)
    assert not np.array_equal(const_film, film)
    # ... and a constant-only scene renders exactly what it rendered without the feature: the oracle's film
    from oracle import binding as ob
    sd = scenes.check_sphere_scene(64, 64)
    okw = dict(max_depth=5, spp=(2, 2), seed=3)
    with gpu.Scene(sd) as sc:
        assert_bit_equal(sc.render(**okw)[0], ob.OracleScene(sd).render(**okw)[0], "constant infinite light vs the oracle")
    # a constant light beside the map adds its radiance where the sky is seen directly
    sd2 = scenes.envmap_scene(128, 128)
    sd2.lights = np.concatenate([sd2.lights, np.array([[LIGHT_INFINITE, 0, 0, 0, 0.5, 0.5, 0.5]], np.float32)])
    with gpu.Scene(sd2.normalized()) as sc:
        both = gpu.film_to_rgb(sc.render(**kw)[0])
    assert np.allclose(both[:16] - rgb[:16], 0.5, atol=2e-3 * rgb[:16].max())
