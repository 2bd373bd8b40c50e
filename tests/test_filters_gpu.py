"""Weighted pixel filters on the GPU: the accumulators bit for bit against tests/filters_ref.py (the exported table, the restated
film points, the oracle's radiances), ranks that add, the footprint hook, a closed form under all four samplers, a scene file, the refusals."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import filters_ref as fr
import pbrt_amd
from pbrt_amd import LIGHT_INFINITE, SceneData, _lib, api, loader, scenes
from test_filters_host import DEPTH, KIND_PARAMS, SEED, emitters_scene, small_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, LIMIT = -1, -4
F32 = np.float32


@pytest.fixture(scope="module")
def shared(oracle):
    """the scene, its oracle (without a filter) and the cache of restated film points + oracle radiances, shared by the cases"""
    sd, cb = small_scene()
    return {"sd": sd, "cb": cb, "oracle": oracle.OracleScene(sd), "cache": {}, "scenes": {}}


def _scene(shared, gpu, pixel_filter):
    key = tuple(pixel_filter)
    if key not in shared["scenes"]:
        shared["scenes"][key] = gpu.Scene(dataclasses.replace(shared["sd"], pixel_filter=pixel_filter).normalized(), device=0)
    return shared["scenes"][key]


@pytest.fixture(scope="module")
def shared_emitters(oracle):
    """the same for the scene of max_depth 0, whose paths draw nothing: the stratified sampler at any sample count (filters_ref.py)"""
    sd, cb = emitters_scene()
    return {"sd": sd, "cb": cb, "oracle": oracle.OracleScene(sd), "cache": {}, "scenes": {}}


def _check(shared, gpu, kind, params, width, sampler, spp, max_depth=DEPTH):
    k = fr.KINDS[kind]
    radii = fr.radii_of(k, width)
    sc = _scene(shared, gpu, (kind,) + tuple(params))
    got, _ = sc.render_acc(width, max_depth=max_depth, spp=spp, seed=SEED, sampler=sampler)
    tab = pbrt_amd.filter_table((kind,) + tuple(params), width)  # (the exported table: its own test holds it to float64)
    want = fr.reference_acc(shared["oracle"], shared["sd"], shared["cb"], radii, spp, SEED, sampler, max_depth, tab, shared["cache"])
    assert np.abs(want[..., 3]).sum() > 0
    bad = (got != want).any(-1)
    assert not bad.any(), f"{kind} {params} radii {radii} {sampler} spp {spp}: {int(bad.sum())} of {bad.size} pixels differ, first {got[bad][0]} vs {want[bad][0]}"
    return got, sc


# ---- 6. accumulators, bit for bit ----
@pytest.mark.parametrize("sampler,spp", [("sobol", (2, 2)), ("stratified", (1, 1))])
@pytest.mark.parametrize("width", [(0.0, 0.0), (1.5, 3.0), (0.5, 0.5)])
@pytest.mark.parametrize("kind", list(KIND_PARAMS))
def test_accumulators_bit_for_bit(shared, gpu, kind, width, sampler, spp):
    """All four accumulators of every pixel equal the reference's: the kinds' default radii (5 x 5 destinations, the sinc's 9 x 9), (1.5, 3.0)
    (a 7-wide axis) and (0.5, 0.5), the narrow case that is still a wide render.  (The stratified sampler at one sample per pixel:
    filters_ref.py says why.)"""
    _check(shared, gpu, kind, KIND_PARAMS[kind][-1], width, sampler, spp)


@pytest.mark.parametrize("spp", [(2, 2), (8, 8)])
@pytest.mark.parametrize("width", [(0.0, 0.0), (1.5, 3.0), (0.5, 0.5)])
@pytest.mark.parametrize("kind", list(KIND_PARAMS))
def test_accumulators_bit_for_bit_stratified_many_samples(shared_emitters, gpu, kind, width, spp):
    """The stratified sampler with several samples per chunk (strata beyond (0, 0), inv_nx != 1) and, at 64, two chunks of a pixel: at
    max_depth 0 no path draws from the chunk's stream, so every film point is restated (filters_ref.py; the host test holds that restatement
    to the oracle's wide box).  The scene: emitters of different colours -- one beyond the 2^15 clamp -- under a constant sky."""
    _check(shared_emitters, gpu, kind, KIND_PARAMS[kind][-1], width, "stratified", spp, max_depth=0)


def test_accumulators_two_chunks_per_pixel(shared, gpu):
    """64 samples per pixel are two chunks of a pixel, on two lanes"""
    _check(shared, gpu, "mitchell", KIND_PARAMS["mitchell"][0], (0.0, 0.0), "sobol", (8, 8))


def test_accumulators_radius_16(shared, gpu):
    _check(shared, gpu, "gaussian", (0.02, 0.0), (16.0, 16.0), "sobol", (1, 1))
    _check(shared, gpu, "gaussian", (0.02, 0.0), (16.0, 16.0), "stratified", (1, 1))


# ---- 7. ranks add; the device's conversion is the host's ----
def test_ranks_add_and_conversions_agree(shared, gpu):
    import torch
    one, sc = _check(shared, gpu, "gaussian", KIND_PARAMS["gaussian"][0], (0.0, 0.0), "sobol", (2, 2))
    kw = dict(max_depth=DEPTH, spp=(2, 2), seed=SEED, sampler="sobol")
    parts = [sc.render_acc((0.0, 0.0), rank=r, world_size=2, **kw)[0] for r in range(2)]
    assert np.array_equal(parts[0] + parts[1], one)
    # (the scene above is one 64 x 64 super-tile, rank 1 of 2 has no sample of it: a film 96 pixels wide gives either rank its share)
    wide_sd = dataclasses.replace(scenes.cornell_scene(96, 20), crop=(0.05, 0.95, 0.15, 0.85), pixel_filter="gaussian").normalized()
    with gpu.Scene(wide_sd, device=0) as ws:
        whole = ws.render_acc((0.0, 0.0), **kw)[0]
        halves = [ws.render_acc((0.0, 0.0), rank=r, world_size=2, **kw)[0] for r in range(2)]
    assert all(np.abs(h).sum() > 0 for h in halves) and np.array_equal(halves[0] + halves[1], whole)
    host = pbrt_amd.film_from_acc(one, weighted=True)
    d_acc = torch.from_numpy(one).to("cuda:0")
    d_film = torch.zeros(one.shape[:2] + (4,), dtype=torch.float32, device="cuda:0")
    sc.film_from_acc_device(d_acc.data_ptr(), d_film.data_ptr())
    torch.cuda.synchronize()
    dev = d_film.cpu().numpy()
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    assert np.array_equal(host.view(np.uint32), fr.film_from_acc_weighted(one).view(np.uint32))
    film, _ = sc.render(filter_width=(0.0, 0.0), **kw)  # pbrt_hip_render converts on the device as well
    assert np.array_equal(film.view(np.uint32), host.view(np.uint32))


def test_clones_carry_the_filter(gpu, monkeypatch):
    """A weighted filter through pbrt_hip_multi_*: rank 1 renders from a CLONE of the scene, which has the filter's record from the original.
    The whole 72 x 40 film is two super-tiles, one per rank; the ranks' integer accumulators add exactly, so the film is the single scene's
    bit for bit -- at the kind's default radii and at radii of the render's own."""
    monkeypatch.setenv("PBRT_HIP_MULTI_LOOPBACK", "1")
    sd = dataclasses.replace(small_scene()[0], xres=72, yres=40, crop=(0.0, 1.0, 0.0, 1.0), pixel_filter="gaussian").normalized()
    kw = dict(spp=(2, 2), max_depth=DEPTH, seed=SEED)
    with gpu.Scene(sd, device=0) as one, gpu.MultiScene(sd, 2) as two:
        for extra in ({}, {"filter_width": (1.0, 3.0)}):
            want, _ = one.render(**kw, **extra)
            got, per_rank = two.render(**kw, **extra)
            assert len(per_rank) == 2 and all(st["samples"] > 0 for st in per_rank), per_rank
            assert np.abs(want[..., :3]).sum() > 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), extra


# ---- 8. the hook ----
def _adversarial_points(rng, cb, rx, ry, n):
    """film points where a bound or an index can flip: integers and half-integers +- 1 ulp, points with d +- r within an ulp of an integer,
    points on every border of the cropped window"""
    x0, y0, x1, y1 = cb
    lat = np.arange(x0 - 3, x1 + 4, dtype=np.float64)
    pts = []
    for base in (lat, lat + 0.5, lat + 0.5 + rx, lat + 0.5 - rx, lat + 0.5 + ry, lat + 0.5 - ry):
        b = base.astype(F32)
        pts += [b, np.nextafter(b, F32(np.inf)), np.nextafter(b, F32(-np.inf))]
    v = np.concatenate(pts)
    v = v[v >= 0]
    px = rng.choice(v, n)
    py = rng.choice(v, n)
    border = np.array([x0, x1, y0, y1, x0 + 0.5, x1 - 0.5, y0 + 0.5, y1 - 0.5], F32)
    m = n // 4
    px[:m] = rng.choice(border, m)
    py[m:2 * m] = rng.choice(border, m)
    return np.stack([px, py], 1).astype(F32)


@pytest.mark.parametrize("radii", [(2.0, 2.0), (1.5, 3.0), (0.5, 0.5), (4.0, 4.0), (16.0, 16.0), (0.3, 2.5)])
def test_footprint_hook_is_the_restatement(gpu, radii):
    """filter_weight.inc over arrays: the clipped bounds of 10^4 film points and the table indices of 10^5 (point, pixel) pairs equal the float32
    numpy restatement exactly"""
    rng = np.random.default_rng(int(radii[0] * 16 + radii[1] * 256))
    cb = (3, 3, 21, 17)
    rand = np.stack([rng.uniform(cb[0] - 3, cb[2] + 3, 5000), rng.uniform(cb[1] - 3, cb[3] + 3, 5000)], 1).astype(F32)
    pts = np.concatenate([rand, _adversarial_points(rng, cb, radii[0], radii[1], 5000)])
    pp = pts[rng.integers(0, len(pts), 100_000)]
    # pixels around the point: inside the footprint, on its rim and outside
    reach = np.array([int(np.ceil(radii[0])) + 1, int(np.ceil(radii[1])) + 1])
    px = np.floor(pp).astype(np.int64) + rng.integers(-reach, reach + 1, (len(pp), 2))
    bounds, index = api.filter_footprint_eval(radii, cb, pts, pp, px.astype(np.int32))
    want = np.stack(fr.footprint(pts[:, 0], pts[:, 1], radii[0], radii[1], cb), 1)
    assert np.array_equal(bounds.astype(np.int64), want)
    want_idx = fr.table_index(pp[:, 0], pp[:, 1], px[:, 0], px[:, 1], radii[0], radii[1], cb)
    assert np.array_equal(index.astype(np.int64), want_idx)
    assert (want_idx >= 0).mean() > 0.01 and (want_idx < 0).mean() > 0.05 and want_idx.max() <= 255  # (the inputs reach both sides)


# ---- 9. closed form, all four samplers ----
def _sky_scene(pixel_filter):
    return SceneData(lights=np.array([[LIGHT_INFINITE, 0, 0, 0, 1, 1, 1]], np.float32), xres=24, yres=20, crop=(0.125, 0.875, 0.15, 0.85), pixel_filter=pixel_filter).normalized()


@pytest.fixture(scope="module")
def box_round_trip(gpu):
    """the XYZ round trip alone, measured: the largest |rgb - 1| of the BOX filter's films of the constant-sky scene (weights 1, the conversion
    the weighted film goes through) over the four samplers, the radii of the filters under test and a handful of sample counts -- the more
    distinct weights, the better the measurement; one figure, a property of the conversion"""
    worst = 0.0
    with gpu.Scene(_sky_scene(None), device=0) as box:
        for sampler in ("stratified", "sobol", "sobol_nd", "halton"):
            for radii in ((2.0, 2.0), (4.0, 4.0)):
                for spp in ((4, 4), (3, 3), (5, 5), (7, 5), (6, 7), (8, 8)):
                    f = box.render(filter_width=radii, spp=spp, max_depth=3, seed=3, sampler=sampler)[0]
                    worst = max(worst, float(np.abs(pbrt_amd.film_to_rgb(f).astype(np.float64) - 1.0).max()))
    return worst


@pytest.mark.parametrize("sampler", ["stratified", "sobol", "sobol_nd", "halton"])
@pytest.mark.parametrize("kind", ["mitchell", "sinc"])
def test_constant_sky_develops_to_one(gpu, box_round_trip, kind, sampler):
    """No geometry under a constant infinite light L = (1, 1, 1): every sample's radiance is exactly 1, so q_r = q_g = q_b = (int64)((w 1) 2^24)
    = q_w and every pixel has acc_r == acc_g == acc_b == acc_w -- whatever the sampler, negative lobes included.  A pixel with a non-zero weight
    sum then develops to RGB 1.  The figure: the film holds XYZ of (v, v, v) and the weight v, v = (float)acc 2^-24 -- the SAME float in all four
    places, so the rounding of the int64 -> float conversions cancels in the division by the weight, and what is left is the XYZ round trip:
    X_k = three float products and two additions (<= 3 roundings of 2^-24 on each), rgb_c = sum_k b_ck X_k likewise (<= 3 more per term), one
    for the division, with terms of magnitude |b_ck X_k| up to (3.24 x 0.95 + 1.54 x 1.00 + 0.50 x 1.09) v = 5.2 v against a result of v: up to
    (6 x 5.2 + 1) 2^-24 = 2^-19 in the worst case, several 2^-24 in practice.  The issue's 2^-22 is below what the round trip alone does, so --
    as the issue provides -- the round trip is MEASURED on the box filter's film of the same scene (weights 1, the same conversion; the filter's
    radii, the four samplers and a handful of sample counts, so that the weights take more than a few values: box_round_trip) and that
    figure is the bound.  MI355X, this test's output: the box's round trip 1.19e-6 (5 x 2^-22); the weighted films reach 9.5e-7 .. 1.19e-6."""
    sd = _sky_scene(kind)
    kw = dict(max_depth=3, seed=3, sampler=sampler, spp=(4, 4))
    with gpu.Scene(sd, device=0) as sc:
        acc, _ = sc.render_acc((0.0, 0.0), **kw)
        film, _ = sc.render(filter_width=(0.0, 0.0), **kw)
    assert (acc[..., 0] == acc[..., 3]).all() and (acc[..., 1] == acc[..., 3]).all() and (acc[..., 2] == acc[..., 3]).all()
    assert np.array_equal(film.view(np.uint32), pbrt_amd.film_from_acc(acc, weighted=True).view(np.uint32))
    lit = acc[..., 3] != 0
    assert lit.mean() > 0.9 and (acc[..., 3] > 0).mean() > 0.9
    err = np.abs(pbrt_amd.film_to_rgb(film)[lit].astype(np.float64) - 1.0).max()
    bound = max(2.0 ** -22, box_round_trip)
    print(f"{kind} {sampler}: weighted |rgb - 1| max {err:.3e}, box round trip {box_round_trip:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, box_round_trip)


# ---- 10. through a scene file ----
def test_scene_file_renders_like_its_arrays(gpu, tmp_path):
    ls = loader.load_file(os.path.join(ROOT, "scenes", "filtered_cornell.pbrt"))
    sd = dataclasses.replace(ls.scene, xres=48, yres=40).normalized()
    kw = dict(ls.render_kwargs(), spp=(2, 2))
    with gpu.Scene(sd, device=0) as sc:
        film, _ = sc.render(**kw)
        acc, _ = sc.render_acc(kw.pop("filter_width"), **kw)
    assert np.array_equal(film.view(np.uint32), pbrt_amd.film_from_acc(acc, weighted=True).view(np.uint32))
    assert acc[..., 3].min() > 0 and (acc[..., :3] > 0).any()
    # the same scene without its filter is another picture (the box of the same radii blurs)
    with gpu.Scene(dataclasses.replace(sd, pixel_filter=None).normalized(), device=0) as box:
        blurred, _ = box.render(filter_width=(2.0, 2.0), **kw)
    assert not np.allclose(pbrt_amd.film_to_rgb(film), pbrt_amd.film_to_rgb(blurred), atol=1e-3)
    # through the FILE: the native command line hands the parser's own description -- the filter's slot as the parser appended it -- to
    # pbrt_hip_render_multi, and python -m pbrt_amd.cli goes through the loader; either PNG is the film rendered from the arrays, written by the
    # same writer, byte for byte (the accumulators are integer sums: every route adds the same samples)
    small = tmp_path / "small.pbrt"
    text = open(os.path.join(ROOT, "scenes", "filtered_cornell.pbrt")).read().replace("[256]", "[32]").replace('"integer pixelsamples" 16', '"integer pixelsamples" 4')
    small.write_text(text)
    ls32 = loader.load_file(str(small))
    with gpu.Scene(ls32.scene, device=0) as sc:
        film32, _ = sc.render(**ls32.render_kwargs())
    want_png = tmp_path / "want.png"
    pbrt_amd.write_image(str(want_png), pbrt_amd.film_to_rgb(film32, ls32.film_scale))
    want = pbrt_amd.read_image(str(want_png))
    assert want.shape == (32, 32, 3) and want.mean() > 0.02 and len(np.unique(want)) > 50
    from pbrt_amd.build import CLI_PATH
    for name, cmd in (("native", [CLI_PATH]), ("python", [sys.executable, "-m", "pbrt_amd.cli"])):
        out = tmp_path / f"{name}.png"
        r = subprocess.run(cmd + [str(small), "--outfile", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        assert np.array_equal(pbrt_amd.read_image(str(out)), want), name


# ---- 11. refusals ----
def _create(desc_edit=None, sd=None):
    """pbrt_hip_scene_create on a small scene whose description `desc_edit` may change: (code, message)"""
    sd = sd or dataclasses.replace(small_scene()[0], pixel_filter="gaussian").normalized()
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd, _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    if desc_edit:
        keep.append(desc_edit(desc))
    h = C.c_void_p()
    rc = _lib.lib().pbrt_hip_scene_create(C.byref(desc), 0, C.byref(h))
    msg = _lib.lib().pbrt_hip_last_error().decode()
    if rc == 0:
        _lib.lib().pbrt_hip_scene_destroy(h)
    return rc, msg


def _with_slots(records):
    def edit(desc):
        texs = (_lib.Texture * len(records))()
        for i, r in enumerate(records):
            C.memmove(C.byref(texs, 64 * i), C.byref(r), 64)
        desc.textures, desc.n_textures = texs, len(records)
        return texs
    return edit


def _record(kind, p0=0.0, p1=0.0):
    r = _lib.PixelFilter(type=3, kind=kind)
    r.param[:] = [p0, p1]
    return r


def test_scene_creation_refusals(gpu):
    assert _create()[0] == 0
    for records, code, word in [([_record(2, 2.0), _record(1)], LIMIT, "more than one"), ([_record(9)], INVALID, "kind"), ([_record(2, 0.0)], INVALID, "alpha"),
                                ([_record(4, -1.0)], INVALID, "tau"), ([_record(3, float("nan"), 0.3)], INVALID, "finite"), ([_record(2, float("inf"))], INVALID, "finite")]:
        rc, msg = _create(_with_slots(records))
        assert rc == code and "filter" in msg and word in msg, (records, rc, msg)

    def kd_names_the_slot(desc):
        desc.mats[0].kd_tex = 1  # (the filter's record is the one slot of the table)
    rc, msg = _create(kd_names_the_slot)
    assert rc == INVALID and "filter" in msg and "kd_tex" in msg


def _render_refusal(gpu, sd, **kw):
    with gpu.Scene(sd, device=0) as sc:
        with pytest.raises(_lib.PbrtHipError) as e:
            sc.render(**kw)
    return e.value.code, str(e.value)


def test_render_refusals(gpu):
    # the existing refusals of a wide render, unchanged: an environment map, shading normals, the counter flags
    env = dataclasses.replace(scenes.envmap_scene(16, 16), pixel_filter="gaussian").normalized()
    code, msg = _render_refusal(gpu, env, filter_width=(0.5, 0.5))
    assert code == LIMIT and "environment map" in msg and "filter" in msg
    nrm = dataclasses.replace(scenes.smooth_mesh_scene(16, 16), pixel_filter="triangle").normalized()
    code, msg = _render_refusal(gpu, nrm)
    assert code == LIMIT and "normals" in msg and "filter" in msg
    plain = dataclasses.replace(small_scene()[0], pixel_filter="mitchell").normalized()
    for counters in (True, "walk"):
        code, msg = _render_refusal(gpu, plain, counters=counters)
        assert code == INVALID and "filter" in msg
    # the wrap rule: a triangle filter of radius 16 has weights up to 240.25 (ceil: 241) on 33 x 33 pixels; 64 spp x 1089 x 241 = 2^24.0018 wraps,
    # 63 x 1089 x 241 does not -- and without the weight factor 64 x 1089 is far below 2^24
    tri = dataclasses.replace(small_scene()[0], pixel_filter="triangle").normalized()
    code, msg = _render_refusal(gpu, tri, filter_width=(16.0, 16.0), spp=(8, 8))
    assert code == LIMIT and "triangle" in msg and "filter" in msg and "2^24" in msg
    with gpu.Scene(tri, device=0) as sc:
        sc.render_prepare(filter_width=(16.0, 16.0), spp=(9, 7))  # 63 spp: accepted (nothing is launched)
    with gpu.Scene(dataclasses.replace(tri, pixel_filter=None).normalized(), device=0) as sc:
        sc.render_prepare(filter_width=(16.0, 16.0), spp=(8, 8))  # the box of that radius: its weights are 1
