"""Environment-map infinite lights without a GPU: the importance-sampling tables, the sampler against its own density,
the lookup against float64 numpy, the validation of pbrt_hip_scene_create, the parser, and the ENV instantiations of the code object.
Everything the sampler and the lookup compute here is pbrt_amd/csrc/envmap_core.hpp run on the host (pbrt_hip_envmap_eval_host);
tests/test_envmap_gpu.py shows the device computes the same bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import LIGHT_ENVMAP, LIGHT_INFINITE, MATTE, _lib, api, isa_id, loader, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUM = np.array([0.212671, 0.715160, 0.072169])


def random_map(h, w, seed, hdr=True):
    """a seeded map with every texel positive: 0.1 + 20 x^4 (max / min of a few hundred) or, smooth, 0.5 .. 1.5"""
    rng = np.random.default_rng(seed)
    x = rng.random((h, w, 3))
    return (0.1 + 20.0 * x ** 4 if hdr else 0.5 + x).astype(np.float32)


def sun_map(h=32, w=64, row=9, col=17, value=(500.0, 450.0, 300.0)):
    m = np.zeros((h, w, 3), np.float32)
    m[row, col] = value
    return m


def rot_x(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def random_rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def f64_density(rgb):
    """f / mean(f), f = luminance x sin(row centre), in float64 (a black map: the sine alone)"""
    h = rgb.shape[0]
    f = (rgb.astype(np.float64) @ LUM) * np.sin((np.arange(h) + 0.5) * np.pi / h)[:, None]
    if f.sum() == 0.0:
        f = np.broadcast_to(np.sin((np.arange(h) + 0.5) * np.pi / h)[:, None], f.shape).copy()
    return f / f.mean(), f


@pytest.mark.parametrize("name", ["random 32x16", "random 7x5", "sun", "black"])
def test_tables(name):
    rgb = {"random 32x16": random_map(16, 32, 1), "random 7x5": random_map(5, 7, 2), "sun": sun_map(), "black": np.zeros((4, 8, 3), np.float32)}[name]
    h, w = rgb.shape[:2]
    marg, cond, puv = api.envmap_tables(rgb)
    assert marg.shape == (h + 1,) and cond.shape == (h, w + 1) and puv.shape == (h, w)
    # the marginal and every conditional: monotone, from 0 to exactly 1
    assert marg[0] == 0.0 and marg[-1] == 1.0 and (np.diff(marg) >= 0).all()
    assert (cond[:, 0] == 0.0).all() and (cond[:, -1] == 1.0).all() and (np.diff(cond, axis=1) >= 0).all()
    # p_uv is a density over the unit square: its mean over the texels -- the integral of a piecewise-constant function -- is 1
    assert abs(puv.astype(np.float64).mean() - 1.0) < 1e-6
    # ... proportional to y sin(row centre), to fp32 rounding (one rounding of the float64 value: 2^-24 relative)
    want, f = f64_density(rgb)
    assert np.allclose(puv, want, rtol=1e-7, atol=0.0), float(np.abs(puv / np.where(want > 0, want, 1) - 1).max())
    # ... and the CDFs are those of the same f: a texel's probability is p_uv / (W H)
    rows = f.sum(axis=1)
    assert np.allclose(np.diff(marg.astype(np.float64)), rows / rows.sum(), atol=2e-7)
    lit = rows > 0
    assert np.allclose(np.diff(cond.astype(np.float64), axis=1)[lit], (f / np.where(rows > 0, rows, 1)[:, None])[lit], atol=2e-7)
    if name == "black":  # the uniform fallback: every direction equally likely, p_uv = sin / mean(sin)
        s = np.sin((np.arange(h) + 0.5) * np.pi / h)
        assert np.allclose(puv, (s / s.mean())[:, None], rtol=1e-7) and np.allclose(np.diff(cond, axis=1), 1.0 / w, atol=2e-7)
    if name == "sun":  # everything goes to the one texel
        assert puv[9, 17] == np.float32(h * w) and np.count_nonzero(puv) == 1
        assert marg[9] == 0.0 and marg[10] == 1.0 and cond[9, 17] == 0.0 and cond[9, 18] == 1.0


def f64_texel(d, m, h, w):
    """-> (row, col, distance to the nearest texel border in texel units, sin theta) by numpy's own trig in float64"""
    wv = d.astype(np.float64) @ np.asarray(m, np.float64).T
    wv /= np.linalg.norm(wv, axis=1, keepdims=True)
    phi = np.mod(np.arctan2(wv[:, 1], wv[:, 0]), 2 * np.pi)
    theta = np.arccos(np.clip(wv[:, 2], -1, 1))
    x, y = phi / (2 * np.pi) * w, theta / np.pi * h
    col, row = np.minimum(x.astype(np.int64), w - 1), np.minimum(y.astype(np.int64), h - 1)
    fx, fy = x - np.floor(x), y - np.floor(y)
    border = np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy))
    return row, col, border, np.sin(theta)


def test_sampler_follows_its_density():
    """2^20 samples of a 32 x 16 HDR map: each sample's pdf is the pdf of looking its own direction up again, the texel counts follow
    prob(texel) = p_uv / (W H), directions are unit vectors.
    Chi-square bound: 511 degrees of freedom (512 texels, all of positive probability, the smallest expected count about 8); the statistic
    of a correct sampler has mean 511 and standard deviation sqrt(2 x 511) = 32: the bound is mean + 5 sd = 671 (a one-sided tail of
    about 3e-7 for the seed fixed here; a sampler that ignored the map would score in the millions).
    The pdf comparison: with the identity as world_to_light the second lookup sees the very w the sample was made from, and the two pdfs
    agree to the last bit away from texel borders (where the density is not 0: see below).  Under a rotation w comes back from M M^T w with an error of 1e-7, and the density's
    1 / sqrt(1 - w.z^2) turns that into 1e-7 / sin^2 theta: the rotated run holds the 1e-5 for the samples with sin theta > 0.2 and says
    how many those are."""
    h, w, n = 16, 32, 1 << 20
    rgb = random_map(h, w, 11)
    rng = np.random.default_rng(5)
    u12 = rng.random((n, 2), dtype=np.float32)
    _, _, puv = api.envmap_tables(rgb)
    for m, min_sin in ((np.eye(3), 0.0), (random_rotation(3), 0.2)):
        d, texel, le, pdf = api.envmap_eval_host(rgb, m, u12=u12)
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        assert np.array_equal(le, rgb.reshape(-1, 3)[texel])
        d2, texel2, le2, pdf2 = api.envmap_eval_host(rgb, m, d=d)
        row, col, border, sin_t = f64_texel(d, m, h, w)
        # density 0 only where fp32 cannot tell cos theta from 1 (sin theta = sqrt(1 - w.z^2) = 0: "no contribution"): theta < 3.5e-4,
        # a cap of 3e-8 of the sphere -- a handful of the 2^20 samples, all in the rows at the poles
        dark = pdf == 0
        assert dark.sum() <= 64 and (sin_t[dark] < 5e-4).all(), (int(dark.sum()), float(sin_t[dark].max(initial=0)))
        keep = (border > 1e-4) & (sin_t > min_sin) & ~dark
        left_out = 1.0 - (border > 1e-4).mean()
        print(f"rotation {'identity' if min_sin == 0 else 'random'}: {left_out:.5f} of the samples within 1e-4 of a texel border, {keep.mean():.4f} compared")
        assert left_out <= 0.02
        # the comparison is not empty: borders take at most 2 %, and the caps with sin theta <= 0.2 are 2 % of the sphere's solid angle
        # (1 - sqrt(1 - 0.04)) -- a map would have to put four times its uniform share of power there to bring the kept share under 0.9
        assert keep.mean() >= 0.9, float(keep.mean())
        assert np.array_equal(texel[keep], texel2[keep]) and np.array_equal(texel[keep], (row * w + col)[keep])
        rel = np.abs(pdf2[keep].astype(np.float64) / pdf[keep] - 1.0)
        print(f"  pdf of the sample vs pdf of its direction looked up again: max relative difference {rel.max():.3g}")
        assert rel.max() <= 1e-5
        # the density itself, against float64: p_uv / (2 pi^2 sin theta)
        want = puv.reshape(-1)[texel] / (2 * np.pi ** 2 * sin_t)
        ok = keep & (sin_t > 0.2)
        assert np.abs(pdf[ok] / want[ok] - 1.0).max() < 1e-5
        counts = np.bincount(texel, minlength=h * w).astype(np.float64)
        expect = n * puv.reshape(-1).astype(np.float64) / (h * w)
        chi2 = ((counts - expect) ** 2 / expect).sum()
        print(f"  chi-square over {h * w} texels: {chi2:.1f} (bound 671), smallest expected count {expect.min():.1f}")
        assert expect.min() > 5 and chi2 < 671.0, chi2


def test_sampler_is_monotone():
    """The sampled (row, col) is monotone in (u2, u1) -- rows never decrease with u2, and inside a row columns never decrease with u1 --,
    so the strata of a stratified or low-discrepancy pattern map to contiguous, ordered parts of the map (an alias table would scatter
    them).  Checked on jittered (nx, ny) grids: every stratum's rows lie at or above the previous stratum's."""
    h, w = 16, 32
    rgb = random_map(h, w, 12)
    rng = np.random.default_rng(9)
    for nx, ny in ((1, 1), (2, 2), (1, 2), (2, 1), (4, 4), (8, 2), (3, 7), (16, 16)):
        reps = max(1, 4096 // (nx * ny))
        ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        u1 = ((ix[..., None] + rng.random((nx, ny, reps))) / nx).astype(np.float32).clip(0, np.float32(1) - np.float32(2 ** -24))
        u2 = ((iy[..., None] + rng.random((nx, ny, reps))) / ny).astype(np.float32).clip(0, np.float32(1) - np.float32(2 ** -24))
        _, texel, _, _ = api.envmap_eval_host(rgb, u12=np.stack([u1.reshape(-1), u2.reshape(-1)], axis=1))
        row, col = (texel // w).reshape(nx, ny, reps), (texel % w).reshape(nx, ny, reps)
        for j in range(ny - 1):  # strata of u2 in order
            assert row[:, j].max() <= row[:, j + 1].min(), (nx, ny, j)
        order = np.argsort(u2.reshape(-1), kind="stable")
        assert (np.diff(row.reshape(-1)[order]) >= 0).all()
        for r in np.unique(row):  # inside a row: columns in the order of u1, stratum by stratum
            sel = row.reshape(-1) == r
            o = np.argsort(u1.reshape(-1)[sel], kind="stable")
            assert (np.diff(col.reshape(-1)[sel][o]) >= 0).all(), (nx, ny, int(r))
    # the place inside the texel is linear: the corners of the unit square map to the map's ends
    d, texel, _, _ = api.envmap_eval_host(rgb, u12=np.array([[0, 0], [0.999999, 0.999999]], np.float32))
    assert texel.tolist() == [0, h * w - 1] and d[0, 2] > 0.99999 and d[1, 2] < -0.99999


@pytest.mark.parametrize("name", ["identity", "x by -90", "random"])
def test_lookup_against_float64(name):
    """The texel of a direction: the same as float64 numpy (arctan2, arccos) finds for every direction not within 1e-5 texels of a border."""
    h, w, n = 16, 32, 1 << 16
    m = {"identity": np.eye(3), "x by -90": rot_x(-90.0), "random": random_rotation(7)}[name]
    rgb = random_map(h, w, 13)
    rng = np.random.default_rng(21)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    # the axes and the poles' neighbourhood too
    d[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    _, texel, le, pdf = api.envmap_eval_host(rgb, m, d=d)
    row, col, border, sin_t = f64_texel(d, m, h, w)
    keep = border > 1e-5
    assert keep.mean() > 0.99
    assert np.array_equal(texel[keep], (row * w + col)[keep])
    assert np.array_equal(le, rgb.reshape(-1, 3)[texel]) and (texel < h * w).all()
    _, _, puv = api.envmap_tables(rgb)
    ok = keep & (sin_t > 0.2)
    assert np.abs(pdf[ok] / (puv.reshape(-1)[texel[ok]] / (2 * np.pi ** 2 * sin_t[ok])) - 1.0).max() < 1e-5
    if name == "identity":  # the poles themselves: sin theta = 0 is density 0
        assert pdf[4] == 0.0 and pdf[5] == 0.0 and texel[4] < w and texel[5] >= (h - 1) * w
    if name == "x by -90":  # pbrt's usual y-up -> z-up turn: world +y is the light's -z ... and world -z its -y
        assert texel[2] // w == h - 1 and texel[5] // w in (h // 2 - 1, h // 2)


# ---- validation (pbrt_hip_scene_create, before any device work) ----

def _desc(sd):
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd.normalized(), _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    return desc, keep


def _create_desc(desc):
    h = C.c_void_p()
    code = _lib.lib().pbrt_hip_scene_create(C.byref(desc), -1, C.byref(h))
    msg = _lib.lib().pbrt_hip_last_error().decode()
    if code == 0:
        _lib.lib().pbrt_hip_scene_destroy(h)
    return code, msg


def _env_record(desc, slot=None):
    """the pbrt_hip_envmap that sits in a slot (default: the last) of desc.textures, as a view that writes through"""
    slot = desc.n_textures - 1 if slot is None else slot
    return _lib.EnvMap.from_address(C.addressof(desc.textures.contents) + slot * C.sizeof(_lib.Texture))


def _small_scene(**kw):
    return scenes.envmap_scene(8, 8, sky=random_map(4, 8, 3), **kw)


def test_validation():
    no_device = -2 if pbrt_amd.device_count() == 0 else 0
    desc, keep = _desc(_small_scene())
    assert desc.n_textures == 1 and desc.textures[0].type == 1 and desc.lights[0].type == LIGHT_ENVMAP
    assert np.array([desc.lights[0].pad], np.float32).view(np.uint32)[0] == 1
    assert _create_desc(desc)[0] == no_device  # a valid description is stopped by the missing device alone, if it is missing

    def refused(mutate, status, sd=None):
        desc, keep = _desc(sd if sd is not None else _small_scene())
        mutate(desc)
        code, msg = _create_desc(desc)
        assert code == status and "environment" in msg, (code, msg)
        return msg

    def setf(name, value):
        return lambda desc: setattr(_env_record(desc), name, value)

    refused(setf("width", 0), -1)
    refused(setf("height", 0), -1)
    refused(lambda d: (setf("width", 1 << 13)(d), setf("height", (1 << 11) + 1)(d)), -4)  # 2^24 + 2^13 texels: refused before a texel is read
    refused(setf("rgb", C.POINTER(C.c_float)()), -1)
    for bad in (np.nan, np.inf, -np.inf, -1e-3):
        sky = random_map(4, 8, 3)
        sky[2, 5, 1] = bad
        assert "texel 21" in refused(lambda d: None, -1, scenes.envmap_scene(8, 8, sky=sky))
    for m in (np.eye(3) * 2.0, np.array([[1, 0.01, 0], [0, 1, 0], [0, 0, 1]]), np.array([[1, 0, 0], [0, 1, 0], [0, 0, np.nan]]),
              np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1.001]]), np.zeros((3, 3))):
        refused(lambda d: None, -1, _small_scene(world_to_light=m))
    # orthonormal to 1e-4 passes: fp32 rotations, and a mirroring
    for m in (random_rotation(4), rot_x(-90.0), np.diag([1.0, 1.0, -1.0]), np.eye(3) * (1 + 2e-5)):
        assert _create_desc(_desc(_small_scene(world_to_light=m))[0])[0] == no_device
    # a type-3 light must name a type-1 record
    for number in (0, 2, 77):
        refused(lambda d, number=number: setattr(d.lights[0], "pad", float(np.array([number], np.uint32).view(np.float32)[0])), -1)
    from util import checker_plane_scene
    sd, _ = checker_plane_scene(8)
    sd.lights = np.array([[LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32)  # no map in the scene: pad = 0
    refused(lambda d: None, -1, sd)
    sd, _ = checker_plane_scene(8)
    sd.lights = np.array([[LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32)
    sd.envmap = random_map(4, 8, 3)
    desc, keep = _desc(sd)
    assert desc.n_textures == 2 and desc.textures[0].type == 0 and desc.textures[1].type == 1
    assert _create_desc(desc)[0] == no_device  # a checkerboard and a map side by side
    refused(lambda d: setattr(d.lights[0], "pad", float(np.array([1], np.uint32).view(np.float32)[0])), -1, sd)  # names the checkerboard
    # a matte kd_tex that names the map: image textures for Kd do not exist
    refused(lambda d: setattr(d.mats[0], "kd_tex", 2), -1, sd)
    # more than one map light
    sd2 = _small_scene()
    sd2.lights = np.concatenate([sd2.lights, sd2.lights])
    msg = refused(lambda d: None, -4, sd2)
    assert "more than one" in msg
    # constant infinite lights keep working beside the map
    sd3 = _small_scene()
    sd3.lights = np.concatenate([sd3.lights, np.array([[LIGHT_INFINITE, 0, 0, 0, 0.1, 0.2, 0.3]], np.float32)])
    assert _create_desc(_desc(sd3)[0])[0] == no_device
    # the hooks validate like the library
    for call in (lambda: api.envmap_tables(np.full((2, 2, 3), -1.0, np.float32)), lambda: api.envmap_eval_host(random_map(2, 2, 1), np.eye(3) * 3, d=np.eye(3))):
        with pytest.raises(_lib.PbrtHipError) as e:
            call()
        assert e.value.code == -1 and "environment" in str(e.value)
    assert b"0.7" in _lib.lib().pbrt_hip_version()


def test_envmap_record_is_one_texture_slot(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbrt_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n",sizeof(pbrt_hip_envmap),'
                   "sizeof(pbrt_hip_texture),offsetof(pbrt_hip_envmap,rgb),offsetof(pbrt_hip_envmap,world_to_light));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [64, 64, 16, 24]
    assert C.sizeof(_lib.EnvMap) == 64 and _lib.EnvMap.rgb.offset == 16 and _lib.EnvMap.world_to_light.offset == 24


# ---- parser ----

HEAD = """
LookAt 0 -4 1  0 0 0  0 0 1
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" [16] "integer yresolution" [16]
WorldBegin
"""
TAIL = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0]\nWorldEnd\n'


def test_parser_reads_mapname(tmp_path):
    sky = random_map(6, 12, 5)
    pbrt_amd.write_image(tmp_path / "sky.pfm", sky)
    # a PFM next to the scene file (relative names resolve against its directory, as plymesh does)
    ls = loader.load_string(HEAD + 'LightSource "infinite" "string mapname" "sky.pfm"\n' + TAIL, base_dir=str(tmp_path))
    assert not ls.warnings, ls.warnings
    sd = ls.scene
    assert sd.lights.tolist() == [[LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]]
    assert np.array_equal(sd.envmap, sky) and np.array_equal(sd.envmap_world_to_light, np.eye(3, dtype=np.float32)) and len(sd.textures) == 0
    (tmp_path / "scene.pbrt").write_text(HEAD + 'LightSource "infinite" "string mapname" "sky.pfm"\n' + TAIL)
    assert np.array_equal(loader.load_file(tmp_path / "scene.pbrt").scene.envmap, sky)
    # an absolute name; L and scale multiply the texels (infinite.rs:54): they are the light's factor
    ls = loader.load_string(HEAD + f'LightSource "infinite" "string mapname" "{tmp_path}/sky.pfm" "rgb L" [2 3 4] "rgb scale" [.5 .5 2]\n' + TAIL)
    assert ls.scene.lights.tolist() == [[LIGHT_ENVMAP, 0, 0, 0, 1, 1.5, 8]] and np.array_equal(ls.scene.envmap, sky) and not ls.warnings
    # a PNG: 8 bits, value = byte / 255
    pbrt_amd.write_image(tmp_path / "sky.png", np.clip(sky / sky.max(), 0, 1))
    ls = loader.load_string(HEAD + 'LightSource "infinite" "string mapname" "sky.png"\n' + TAIL, base_dir=str(tmp_path))
    assert ls.scene.envmap.shape == (6, 12, 3) and not ls.warnings
    assert np.array_equal(ls.scene.envmap, pbrt_amd.read_image(tmp_path / "sky.png")) and 0 < ls.scene.envmap.max() <= 1.0
    assert np.array_equal(np.round(ls.scene.envmap * 255), ls.scene.envmap * 255)
    # a missing file: a warning, and the constant L x scale (infinite.rs:56-58)
    ls = loader.load_string(HEAD + 'LightSource "infinite" "string mapname" "nowhere.pfm" "rgb L" [2 3 4] "rgb scale" [.5 .5 2]\n' + TAIL, base_dir=str(tmp_path))
    assert ls.scene.lights.tolist() == [[LIGHT_INFINITE, 0, 0, 0, 1, 1.5, 8]] and ls.scene.envmap.size == 0
    assert [w for w in ls.warnings if "nowhere.pfm" in w and "constant" in w], ls.warnings
    # Rotate before the light lands in world_to_light: the inverse of the CTM's rotation
    ls = loader.load_string(HEAD + 'AttributeBegin Rotate -90 1 0 0 LightSource "infinite" "string mapname" "sky.pfm" AttributeEnd\n' + TAIL, base_dir=str(tmp_path))
    assert not ls.warnings, ls.warnings
    assert np.allclose(ls.scene.envmap_world_to_light, rot_x(90.0), atol=1e-6)
    ls = loader.load_string(HEAD + 'AttributeBegin Rotate 30 1 2 3 Rotate 50 0 1 0 LightSource "infinite" "string mapname" "sky.pfm" AttributeEnd\n' + TAIL, base_dir=str(tmp_path))
    m = ls.scene.envmap_world_to_light.astype(np.float64)
    assert not ls.warnings and np.allclose(m @ m.T, np.eye(3), atol=1e-6) and np.linalg.det(m) > 0.999 and not np.allclose(m, np.eye(3), atol=0.1)
    # a CTM that scales: a warning, and the rotation part
    ls = loader.load_string(HEAD + 'AttributeBegin Rotate -90 1 0 0 Scale 2 3 4 LightSource "infinite" "string mapname" "sky.pfm" AttributeEnd\n' + TAIL, base_dir=str(tmp_path))
    assert [w for w in ls.warnings if "scales or shears" in w], ls.warnings
    assert np.allclose(ls.scene.envmap_world_to_light, rot_x(90.0), atol=1e-6)
    # the map beside a checkerboard: the material keeps its texture, the light finds its map, and the library takes the scene
    text = (HEAD + 'Texture "chk" "spectrum" "checkerboard" "rgb tex1" [.1 .2 .3] "rgb tex2" [.8 .7 .6]\n'
            'LightSource "infinite" "string mapname" "sky.pfm"\nMaterial "matte" "texture Kd" "chk"\n' + TAIL)
    ls = loader.load_string(text, base_dir=str(tmp_path))
    assert len(ls.scene.textures) == 1 and ls.scene.mat_tex.tolist() == [1] and np.array_equal(ls.scene.envmap, sky)
    assert _create_desc(_desc(ls.scene)[0])[0] == (-2 if pbrt_amd.device_count() == 0 else 0)
    # one map per scene: a second one is said and falls back to its constant
    ls = loader.load_string(HEAD + 'LightSource "infinite" "string mapname" "sky.pfm"\nLightSource "infinite" "string mapname" "sky.png" "rgb L" [3 3 3]\n' + TAIL,
                            base_dir=str(tmp_path))
    assert ls.scene.lights[:, 0].tolist() == [LIGHT_ENVMAP, LIGHT_INFINITE] and [w for w in ls.warnings if "one environment map" in w]


def test_scene_file_equals_the_generator():
    """scenes/envmap_spheres.pbrt loads to the arrays scenes.envmap_scene builds (tests/test_envmap_gpu.py compares their films); the
    committed scenes/sky_small.pfm is procedural_sky(64, 32) (to 1e-6: the sky goes through numpy's cos / sin, whose last bit is the
    platform's)."""
    ls = loader.load_file(os.path.join(ROOT, "scenes", "envmap_spheres.pbrt"))
    assert not ls.warnings, ls.warnings
    sd = scenes.envmap_scene()
    for f in ("P", "idx", "mat_id", "materials", "lights", "spheres", "cam_to_world", "mat_eta", "mat_tex", "textures", "envmap_world_to_light"):
        assert np.array_equal(getattr(ls.scene, f), getattr(sd, f)), f
    assert ls.scene.envmap.shape == (32, 64, 3) and np.allclose(ls.scene.envmap, sd.envmap, rtol=1e-6, atol=0)
    assert (ls.scene.fov, ls.scene.xres, ls.scene.yres) == (sd.fov, sd.xres, sd.yres) and ls.max_depth == 8
    sky = sd.envmap
    assert sky.max() / sky.mean() > 100 and (sky[:16] > 0).all()  # a small sun: the case importance sampling is for
    c = scenes.envmap_scene(constant=True)
    assert c.lights[0, 0] == LIGHT_INFINITE and c.envmap.size == 0


def test_env_instantiations_hold_their_register_budget():
    """render_kernel_env exists for both stack variants, with and without spheres, MIS, textures and the table samplers -- 32 kernels in
    a translation unit of their own --, spills nothing, uses no scratch, and fits 4 waves per SIMD, the budget 3.17 took (512 VGPRs
    per SIMD lane on gfx950, handed out in granules of 8: 128 at 4 waves)."""
    syms = sorted(isa_id.kernel_ids_by_symbol(_lib.LIB_PATH))
    names = [isa_id.normalise(d) for d in isa_id._demangle(syms)]
    env = [(n, s) for n, s in zip(names, syms) if re.fullmatch(r"render_kernel_env<(true|false),\d+,(true|false),(true|false),(true|false)>", n)]
    assert len(env) == 32, len(env)  # SPH x STACK x MIS x TEX x SND
    import render_variant_table
    budget = 512 // render_variant_table.waves_per_simd("env")  # (render_variant.hpp)
    assert budget == 128  # 4 waves per SIMD: a whole number of granules
    for stack in ("0", "30"):
        assert [n for n, _ in env if n.split(",")[1] == stack], stack
    for n, s in env:
        r = isa_id.kernel_resources(_lib.LIB_PATH, s)
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
        assert r["vgpr_count"] + (r["agpr_count"] or 0) <= budget, (n, r, budget)


def test_reference_checks_itself():
    """tests/independent_envmap.py against itself (no product involved): its lookup is the float64 lookup of this file, two runs with
    different seeds agree block by block within the bar the GPU test holds the library to, the blocks are resolved, and it tells a map
    from the same map turned by 90 degrees."""
    import independent_envmap as ie
    sky = ie.smooth_sky()
    d = np.random.default_rng(1).normal(size=(4096, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = random_rotation(6)
    row, col, _, _ = f64_texel(d, m, *sky.shape[:2])
    assert np.array_equal(ie.lookup(sky, m, d), sky[row, col])
    m1, s1 = ie.block_means(64, sky, np.eye(3), paths=256, seed=1)
    m2, s2 = ie.block_means(64, sky, np.eye(3), paths=256, seed=2)
    z = np.abs(m1 - m2) / (5 * np.sqrt(s1 ** 2 + s2 ** 2) + 0.004 * m1)
    assert z.max() < 1.0 and abs(m1.sum() / m2.sum() - 1) < 5e-3, (float(z.max()), m1.sum() / m2.sum() - 1)
    assert (s1 / m1).max() < 0.03
    m3, s3 = ie.block_means(64, sky, rot_x(90.0), paths=256, seed=1)
    assert (np.abs(m1 - m3) / (5 * np.sqrt(s1 ** 2 + s3 ** 2) + 0.004 * m1)).max() > 1.5
