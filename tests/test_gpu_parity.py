"""The parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on the
same seeded inputs.  Bar: BIT-EXACT -- every fp32 operation of the path is +,-,*,/,sqrt or a
comparison, executed in the same order on both sides with FMA contraction off,
so the film, the hit records and the visit counters must be identical, not merely close.
(BASELINE.json asks for PSNR >= 50 dB; identical images are PSNR = inf.)"""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, LIGHT_INFINITE, SceneData, scenes
from util import SMALL_SCENES, assert_bit_equal, random_rays

pytestmark = pytest.mark.gpu


def psnr(a, b):
    a = np.clip(a.astype(np.float64), 0, 1)
    b = np.clip(b.astype(np.float64), 0, 1)
    mse = ((a - b) ** 2).mean()
    return np.inf if mse == 0 else 10 * np.log10(1.0 / mse)


# The BASELINE-size cases run on BOTH builders -- "gpu" is what every default path of the library ships (pbrt_hip_scene_create,
# pbrt_hip_render_multi, the command line, bench.py: built and optimised on the device), "host" the canonical binned-SAH tree -- and
# the oracle's answer for a case is computed once.
BUILDERS = [pytest.param(None, id="default"), "host"]  # None = pbrt_hip_scene_create, the §8(b) entry point: must be the device build
_oracle_cache = {}


def oracle_render(oracle, key, make_sd, **kw):
    k = (key, tuple(sorted((a, str(b)) for a, b in kw.items())))
    if k not in _oracle_cache:
        _oracle_cache[k] = oracle.OracleScene(make_sd()).render(**kw)
    return _oracle_cache[k]


def test_native_library_is_the_one_loaded(gpu):
    """The GPU tests run on the in-tree HIP library, not on a fallback."""
    maps = open("/proc/self/maps").read()
    gpu.api.lib()
    maps = open("/proc/self/maps").read()
    from pbrt_amd import _lib
    assert os.path.realpath(_lib.LIB_PATH) in maps and "/pbrt_amd/lib" in _lib.LIB_PATH  # (lib_<variant>/ for A-B builds)


@pytest.mark.parametrize("builder", [None, "host"])  # None: the library's default (pbrt_hip_scene_create: built and optimised on the device)
@pytest.mark.parametrize("name", ["mesh1k", "mesh20k", "cornell", "check_sphere", "sphere", "ties", "deep"])
def test_intersect_matches_oracle(gpu, oracle, name, builder):
    sd = SMALL_SCENES[name]()
    o, d, tmax = random_rays(200_000 if name != "mesh20k" else 400_000, 21)
    ref = oracle.OracleScene(sd)
    rt, rp, rb1, rb2, rc = ref.intersect(o, d, tmax)
    with gpu.Scene(sd, builder=builder) as sc:  # (device-built: the canonical tree behind the counters is made lazily)
        assert sc.build_info()["gpu_built"] == (builder is None and sc.n_prims >= 2)  # (primitives: triangles + spheres)
        t, prim, b1, b2, cnt = sc.intersect(o, d, tmax, counters=True)
        sc_depth, sc_need = sc.info()["depth"], sc.info()["quad_stack_need"]
        occ = sc.occluded(o, d, tmax)
        t2 = sc.intersect(o, d, tmax)[0]  # the non-counting instantiation
    assert_bit_equal(prim, rp, "prim")
    assert_bit_equal(t, rt, "t")
    assert_bit_equal(b1, rb1, "b1")
    assert_bit_equal(b2, rb2, "b2")
    assert_bit_equal(t2, rt, "t (no counters)")
    assert cnt == rc, f"nodes visited / triangles tested {cnt} vs oracle {rc}"  # identical traversal
    assert_bit_equal(occ, ref.occluded(o, d, tmax), "occluded")
    assert (prim != 0xFFFFFFFF).mean() > (0.05 if name != "deep" else 0.0005)
    if name == "deep":
        assert sc_depth >= 39  # (the canonical tree; the host's 4-wide collapse of it needs more than the 40 LDS entries: overflow variant)
        assert sc_need > 40 or builder is None


@pytest.mark.parametrize("builder", [None, "host", "gpu-plain"])
@pytest.mark.parametrize("name", ["mesh1k", "mesh20k", "cornell", "ties", "deep"])
def test_a_hit_is_a_function_of_ray_and_triangle_alone(gpu, oracle, name, builder):
    """The own-box rule where the tie rule used to end: rays aimed exactly at vertices, at points on edges, along edges and
    axes, IN the plane of the triangle they aim at, with tmax at / a hair off the target (util.adversarial_rays) through the trees of all
    three builders -- hit records and occlusion flags equal to the oracle's BRUTE FORCE over all triangles (no box of any tree between the
    ray and the triangle), bit for bit, and the canonical counters equal to the oracle's BVH.  Until round 5 a walk through wider boxes
    could accept a "hit" outside its triangle's own box that a walk over tight boxes never saw (in the Cornell box 25 of 40 000 of
    these rays: tests/test_oracle_selfcheck.py::test_without_the_own_box_rule_...)."""
    from util import adversarial_rays
    sd = SMALL_SCENES[name]().normalized()
    ref = oracle.OracleScene(sd)
    with gpu.Scene(sd, builder=builder) as sc:
        for seed in range(4):
            o, d, tmax = adversarial_rays(sd, 60_000 if sd.idx.shape[0] < 5000 else 12_000, 100 + seed)
            rt, rp, rb1, rb2, _ = ref.intersect(o, d, tmax, brute_force=True)
            rocc = ref.occluded(o, d, tmax, brute_force=True)
            t, prim, b1, b2, cnt = sc.intersect(o, d, tmax, counters=True)  # the canonical walk (EXACT)
            assert_bit_equal(prim, rp, f"{seed}: prim (canonical walk)")
            assert_bit_equal(t, rt, f"{seed}: t (canonical walk)")
            assert cnt == ref.intersect(o, d, tmax)[4], f"{seed}: counters {cnt}"
            t, prim, b1, b2 = sc.intersect(o, d, tmax)[:4]                  # the production walk over the builder's quantised tree
            assert_bit_equal(prim, rp, f"{seed}: prim")
            assert_bit_equal(t, rt, f"{seed}: t")
            assert_bit_equal(b1, rb1, f"{seed}: b1")
            assert_bit_equal(b2, rb2, f"{seed}: b2")
            assert_bit_equal(sc.occluded(o, d, tmax), rocc, f"{seed}: occluded")
        # ... and the rule's PROMISE node by node on the tree this builder put into HBM (exported as it sits there): every node test on the
        # way from the root to an accepted triangle's leaf slot passes with tfar = the hit's t, in the production step's arithmetic
        # (oracle/quad_walk.cpp child_passes; tests/test_oracle_selfcheck.py::test_every_walk_reaches_... does the same for the host's trees)
        quads, order = sc.export_quads()
    if len(quads) and sd.spheres.shape[0] == 0:
        o, d, tmax, tri = adversarial_rays(sd, 40_000, 7, with_targets=True)
        ok, th = ref.tri_accepts(o, d, tmax, tri)
        keep = ok != 0
        V = sd.P[sd.idx.reshape(-1)]
        fails = oracle.quad_path_check(quads, np.concatenate([V.min(0), V.max(0)]), order, o[keep], d[keep], tri[keep], th[keep])
        assert keep.sum() > (100 if name == "deep" else 1000) and not fails.any(), (int(keep.sum()), int((fails != 0).sum()))  # (the deep scene's triangles are specks)


@pytest.mark.parametrize("builder", [None, "host", "gpu-plain"])
def test_spheres_are_primitives_of_the_tree(gpu, oracle, builder):
    """Round 6: `Shape "sphere"` (check-sphere.pbrt:22) is a primitive of the BVH -- a leaf record of its own kind, tested
    in the leaf pass with the f64 quadratic and the own-box rule -- where every ray used to test every sphere after the walk.  2 000
    overlapping spheres + triangles through all three builders: film, hit records, occlusion flags and the canonical counters equal to the
    oracle's; 10 000 spheres cost a frame at most 2 x the production walk's work of 20 000 random triangles (they cost less)."""
    from util import sphere_cloud_scene
    sd = sphere_cloud_scene(2000)
    kw = dict(max_depth=5, spp=(2, 2), seed=4)
    ref = oracle.OracleScene(sd)
    rfilm, rst = ref.render(**kw)
    o, d, tmax = random_rays(100_000, 5, inside=1.5)
    rt, rp, rb1, rb2, rc = ref.intersect(o, d, tmax)
    with gpu.Scene(sd, builder=builder) as sc:
        assert sc.build_info()["gpu_built"] == (builder != "host")
        film, st = sc.render(counters=True, **kw)
        film2, _ = sc.render(**kw)
        t, prim, b1, b2, cnt = sc.intersect(o, d, tmax, counters=True)
        t2, prim2 = sc.intersect(o, d, tmax)[:2]
        occ = sc.occluded(o, d, tmax)
    assert_bit_equal(film, rfilm, "film (canonical walk)")
    assert_bit_equal(film2, rfilm, "film")
    for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
        assert st[k] == rst[k], k
    assert_bit_equal(prim, rp, "prim"); assert_bit_equal(t, rt, "t"); assert_bit_equal(prim2, rp, "prim (production walk)"); assert_bit_equal(t2, rt, "t (production walk)")
    assert cnt == rc and (rp >= sd.idx.shape[0]).mean() > 0.2
    assert_bit_equal(occ, ref.occluded(o, d, tmax), "occluded")
    if builder is None:
        work = {}
        for name, s2 in (("spheres", sphere_cloud_scene(10_000, 128, 128, n_tris=0)), ("triangles", scenes.random_mesh_scene(20_000, 128, 128))):
            with gpu.Scene(s2) as sc:
                sc.render(**kw)
                _, st = sc.render(**kw)
                _, wk = sc.render(counters="walk", **kw)
            rays = wk["camera_rays"] + wk["bounce_rays"] + wk["shadow_rays"]
            work[name] = (wk["nodes_visited"] / rays, wk["tris_tested"] / rays, st["kernel_ms"])
        assert work["spheres"][0] < 2 * work["triangles"][0] and work["spheres"][1] < 2 * work["triangles"][1], work


@pytest.mark.parametrize("builder", [None, "host"])
def test_flat_slivers_have_no_holes(gpu, oracle, builder):
    """slivers lying flat in axis planes (own boxes of zero thickness, Moeller-Trumbore's t hundreds of ulps off the plane's slab
    distance) -- every ray aimed well inside one hits it, at the oracle's distance bit for bit, and the film of the scene equals the
    oracle's: the own-box rule raises such a candidate to its box's entry, it does not reject it (a rejecting rule lost 7 ... 44 % of them)."""
    from util import flat_sliver_scene
    sd, n = flat_sliver_scene()
    rng = np.random.default_rng(12)
    m = 40_000
    tri = rng.integers(0, n, m)
    b = rng.uniform(0.1, 0.8, (m, 2))
    b[b.sum(1) > 0.9] *= 0.5
    V = sd.P[sd.idx[tri]].astype(np.float64)
    target = V[:, 0] + (V[:, 1] - V[:, 0]) * b[:, :1] + (V[:, 2] - V[:, 0]) * b[:, 1:]
    o = rng.uniform(-3, 3, (m, 3))
    dv = target - o
    o, d = o.astype(np.float32), (dv / np.linalg.norm(dv, axis=1)[:, None]).astype(np.float32)
    tmax = np.full(m, np.inf, np.float32)
    ref = oracle.OracleScene(sd)
    rt, rp, rb1, rb2, _ = ref.intersect(o, d, tmax, brute_force=True)
    kw = dict(max_depth=3, spp=(3, 3), seed=2)
    with gpu.Scene(sd, builder=builder) as sc:
        t, prim, b1, b2 = sc.intersect(o, d, tmax)[:4]
        film, _ = sc.render(**kw)
    grazing = np.abs(d[np.arange(m), tri // 3]) < 1e-3
    assert (prim[~grazing] != 0xFFFFFFFF).all()  # no holes
    assert_bit_equal(prim, rp, "prim"); assert_bit_equal(t, rt, "t"); assert_bit_equal(b1, rb1, "b1"); assert_bit_equal(b2, rb2, "b2")
    assert_bit_equal(film, ref.render(**kw)[0], "film")


def test_hip_image_equals_an_independent_float64_implementation_of_the_spec(gpu):
    """north_star's "PSNR >= 50 dB vs the reference image" against a reference that is NOT the oracle: tests/independent_twin.py -- float64
    numpy written from DESIGN.md section 3's text (brute-force Moeller-Trumbore, numpy's sin / cos, no BVH, no own-box rule), sharing the
    random numbers and no code -- on BASELINE C4's scene at depth 16 (integrators 0 and 2), C0's geometry and C1's scene (spheres), a 300-triangle
    mesh with mirrors and two spheres under all four kinds of light, a 64-spp frame in two chunks, the direct-lighting integrator: the HIP film (pbrt_hip_scene_create: the tree built on the device,
    the quantised production walk; the stratified, padded (0,2) and Halton samplers) against it: PSNR >= 90 dB (measured on the oracle: 105 ... 148), 99 % of the pixels (measured on the oracle: 99.5 ... 100 %) equal to 1e-4 in every channel, the same weights.  The
    oracle passes the same check on the CPU (tests/test_oracle_selfcheck.py)."""
    import independent_twin as tw
    from test_oracle_selfcheck import _twin_cases
    cases = _twin_cases() + [("C4's scene at 96 x 96, 36 spp, depth 16", scenes.cornell_scene(96, 96), dict(integrator=INTEGRATOR_PATH, max_depth=16, spp=(6, 6), seed=0))]
    from test_oracle_selfcheck import _twin_kw
    for name, sd, kw in cases:
        twin = tw.render(sd, **_twin_kw(kw))
        with gpu.Scene(sd) as sc:
            film, _ = sc.render(**kw)
        rel = np.abs(twin[..., :3] - film[..., :3]) / np.maximum(np.abs(film[..., :3]), 1e-3 * film[..., :3].max())
        assert tw.psnr_db(twin, film) >= 90.0 and (rel.max(-1) < 1e-4).mean() >= 0.99, (name, tw.psnr_db(twin, film), (rel.max(-1) < 1e-4).mean())
        assert np.array_equal(twin[..., 3], film[..., 3])
    # ... and BASELINE C0 exactly as it is stated (256 x 256, 4 spp, the scene file through the parser, its checkerboard, its Halton sampler)
    from test_oracle_selfcheck import _c0_against_the_twin

    def hip(sd, kw):
        with gpu.Scene(sd) as sc:
            return sc.render(seed=0, **kw)[0]
    for sampler, twin, film in _c0_against_the_twin(hip):
        rel = np.abs(twin[..., :3] - film[..., :3]) / np.maximum(np.abs(film[..., :3]), 1e-3 * film[..., :3].max())
        assert tw.psnr_db(twin, film) >= 60.0 and (rel.max(-1) < 1e-4).mean() >= 0.9999, (sampler, tw.psnr_db(twin, film), (rel.max(-1) < 1e-4).mean())


def test_hip_equals_the_independent_implementation_on_random_scenes(gpu):
    """tests/test_oracle_selfcheck.py's comparison on the soak's random scenes (util.random_twin_case, seeds 0 ... 119: every kind of light,
    emissive triangles, mirrors, spheres, crop windows, three samplers, three integrators), the HIP film against the float64 twin -- no oracle
    in between: util.meets_random_scene_bar per film (the weights exactly; all but a sample's footprint or two of the pixels to 1e-4 / 1e-3
    relative), at most 3 % of the films below 90 dB (one grazing sample)."""
    import independent_twin as tw
    from util import meets_random_scene_bar, random_twin_case, twin_render
    done, below_90 = 0, []
    with np.errstate(all="ignore"):
        for seed in range(120):
            case = random_twin_case(seed)
            if case is None:
                continue
            sd, kw = case
            with gpu.Scene(sd, builder="gpu" if seed % 2 else "host") as sc:
                film, _ = sc.render(**kw)
            ok, ps, off = meets_random_scene_bar(twin_render(sd, kw), film, kw)
            assert ok, (seed, ps, off, kw)
            done += 1
            if ps < 90.0:
                below_90.append((seed, ps))
    assert done >= 80 and len(below_90) <= 0.03 * done, (done, below_90)


def test_an_empty_crop_window_is_an_empty_film(gpu, oracle, monkeypatch):
    """A crop window that holds no pixel (ceil(res x c0) == ceil(res x c1): Film::new, film.rs:82-137) is a film of no pixels and no rays, on
    both sides and under a wide filter too (its halo is not sampled for nothing) -- it came back as "film_assemble: null argument" until the
    parser fuzz sent three such files through pbrt_hip_render (tools/parser_fuzz.py --hip)."""
    for crop in ((0.5, 0.5, 0.0, 1.0), (0.2, 0.8, 0.3, 0.3), (0.51, 0.52, 0.0, 1.0)):
        sd = scenes.cornell_scene(16, 16, crop=crop)
        for kw in (dict(spp=(2, 1), max_depth=3), dict(spp=(1, 2), max_depth=2, filter_width=(1.5, 2.5)), dict(spp=(1, 1), max_depth=2, sampler="halton", integrator=2)):
            ref, rst = oracle.OracleScene(sd).render(**kw)
            with gpu.Scene(sd) as sc:
                film, st = sc.render(**kw)
                cst = sc.render(counters=True, **kw)[1] if len(kw) == 2 else None  # (the counting instantiations: default filter, stratified sampler)
            assert film.shape == ref.shape and film.size == 0, (crop, film.shape, ref.shape)
            assert rst["camera_rays"] == 0 and st["samples"] == 0 and (cst is None or cst["camera_rays"] == 0), (crop, kw, cst, st)
    # ... a rank's share of it, and the in-library multi-GPU path (two ranks looped back onto this device): empty films, no error
    monkeypatch.setenv("PBRT_HIP_MULTI_LOOPBACK", "1")
    sd = scenes.cornell_scene(16, 16, crop=(0.5, 0.5, 0.0, 1.0))
    with gpu.Scene(sd) as sc:
        for r in range(2):
            assert sc.render(rank=r, world_size=2, spp=(1, 1))[0].size == 0
    with gpu.MultiScene(sd, 2) as ms:
        for kw in (dict(spp=(1, 1)), dict(spp=(1, 1), filter_width=(1.5, 1.5))):
            film, stats = ms.render(**kw)
            assert film.size == 0 and sum(st["samples"] for st in stats) == 0


def test_intersect_edge_cases(gpu, oracle):
    sd = SMALL_SCENES["mesh1k"]()
    with gpu.Scene(sd) as sc:
        e = np.zeros((0, 3), np.float32)
        t, prim, *_ = sc.intersect(e, e, np.zeros(0, np.float32))  # empty batch
        assert len(t) == 0
        o, d, tmax = random_rays(37, 2)  # ragged: not a multiple of the wave / block size
        ref = oracle.OracleScene(sd).intersect(o, d, tmax)
        got = sc.intersect(o, d, tmax)
        assert_bit_equal(got[0], ref[0], "t ragged")
        tz = np.zeros(len(o), np.float32)  # tmax = 0: nothing can be hit
        assert (sc.intersect(o, d, tz)[1] == 0xFFFFFFFF).all() and (sc.occluded(o, d, tz) == 0).all()
        # probe rays that are not numbers: a NaN / infinite origin or direction component, a NaN tmax -- misses on both sides, with the
        # canonical counters (such a ray is not walked: with NaN slabs it would visit the whole tree), the sane rays around them unchanged
        ob, db, tb = o.copy(), d.copy(), tmax.copy()
        ob[3, 1] = np.nan; ob[7, 0] = np.inf; db[11, 2] = np.nan; db[13, 0] = -np.inf; tb[17] = np.nan; db[19] = (np.nan, np.nan, np.nan)
        bad = [3, 7, 11, 13, 17, 19]
        gotb, refb = sc.intersect(ob, db, tb, counters=True), oracle.OracleScene(sd).intersect(ob, db, tb)
        for a, b, what in zip(gotb[:4], refb[:4], ("t", "prim", "b1", "b2")):
            assert_bit_equal(a, b, f"batch with non-finite rays: {what}")
        assert (gotb[1][bad] == 0xFFFFFFFF).all() and np.isinf(gotb[0][bad]).all() and gotb[4] == refb[4]
        keep = np.setdiff1d(np.arange(len(o)), bad)
        assert_bit_equal(gotb[0][keep], got[0][keep], "the sane rays of that batch")
        assert np.array_equal(sc.occluded(ob, db, tb) != 0, oracle.OracleScene(sd).occluded(ob, db, tb) != 0) and (sc.occluded(ob, db, tb)[bad] == 0).all()
    # a scene with no geometry at all
    sd = SceneData(xres=16, yres=16, lights=np.array([[LIGHT_INFINITE, 0, 0, 0, 0.25, 0.5, 1.0]], np.float32))
    with gpu.Scene(sd) as sc:
        assert (sc.intersect(o, d, tmax)[1] == 0xFFFFFFFF).all()
        film, st = sc.render(spp=(2, 1))
        ref, _ = oracle.OracleScene(sd).render(spp=(2, 1))
        assert_bit_equal(film, ref, "empty-scene film")


RENDER_CASES = [
    ("mesh1k", INTEGRATOR_PATH, 8, (2, 2), 3),
    ("mesh20k", INTEGRATOR_PATH, 8, (4, 2), 0),
    ("cornell", INTEGRATOR_PATH, 16, (3, 3), 1),
    ("cornell", INTEGRATOR_PATH, 0, (1, 1), 1),
    ("check_sphere", INTEGRATOR_PATH, 5, (2, 2), 9),
    ("sphere", INTEGRATOR_DIRECT, 5, (4, 4), 0),
    ("check_sphere", INTEGRATOR_DIRECT, 5, (2, 1), 4),
    ("ties", INTEGRATOR_PATH, 8, (3, 2), 5),  # duplicated / coplanar / degenerate geometry: the tie rule decides
    ("deep", INTEGRATOR_PATH, 6, (2, 2), 6),  # a very deep tree: 64-entry exact stack, HBM overflow of the production stack
    ("mesh1k", INTEGRATOR_PATH, 8, (8, 8), 7),  # (sample 35 of pixel (13, 0) draws u32 > 2^32 - 2^9: the 1 - 2^-23 clamp of rng.rs:19)
    ("check_sphere", INTEGRATOR_PATH, 5, (16, 5), 2),
]


@pytest.mark.parametrize("builder", [None, "host"])
@pytest.mark.parametrize("name,integrator,depth,spp,seed", RENDER_CASES)
def test_render_matches_oracle(gpu, oracle, name, integrator, depth, spp, seed, builder):
    sd = SMALL_SCENES[name]()
    ref, rst = oracle_render(oracle, ("small", name), lambda: sd, integrator=integrator, max_depth=depth, spp=spp, seed=seed)
    with gpu.Scene(sd, builder=builder) as sc:
        film, st = sc.render(integrator=integrator, max_depth=depth, spp=spp, seed=seed, counters=True)
        film2, st2 = sc.render(integrator=integrator, max_depth=depth, spp=spp, seed=seed)
    assert_bit_equal(film, ref, f"{name} film")
    assert_bit_equal(film2, ref, f"{name} film (no counters)")
    for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
        assert st[k] == rst[k], f"{k}: {st[k]} vs oracle {rst[k]}"
    assert st2["samples"] == sd.xres * sd.yres * spp[0] * spp[1] and st2["kernel_ms"] > 0
    assert psnr(gpu.film_to_rgb(film), oracle.film_write_rgb(ref)) >= 50.0


def test_item_handout_is_scheduling_only(gpu, oracle, monkeypatch):
    """A pixel's samples run in K <= 16 chunks (work items with their own RNG stream and partial film sum)
    that any lane of any wave may take in any order.  The film must not depend on who takes what: ragged image, three
    ranks, a grid of 5 one-wave workgroups (every lane renders hundreds of items) and one of a single hand-out region,
    all bit-equal to the oracle, with the oracle's canonical counters."""
    sd = scenes.cornell_scene(200, 136)
    ref, rst = oracle.OracleScene(sd).render(max_depth=4, spp=(8, 9), seed=5)
    with gpu.Scene(sd) as sc:
        full, st = sc.render(max_depth=4, spp=(8, 9), seed=5, counters=True)
        acc = np.zeros_like(full)
        for r in range(3):
            part, _ = sc.render(max_depth=4, spp=(8, 9), seed=5, rank=r, world_size=3)
            acc += part
        monkeypatch.setenv("PBRT_HIP_RENDER_WORKGROUPS", "5")
        few, _ = sc.render(max_depth=4, spp=(8, 9), seed=5)
        monkeypatch.setenv("PBRT_HIP_RENDER_WORKGROUPS", "300")
        monkeypatch.setenv("PBRT_HIP_REGIONS", "1")
        one, _ = sc.render(max_depth=4, spp=(8, 9), seed=5)
    assert_bit_equal(full, ref, "film")
    assert_bit_equal(acc, ref, "film, union of 3 ranks")
    assert_bit_equal(few, ref, "film from 5 persistent waves")
    assert_bit_equal(one, ref, "film from one hand-out region")
    for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
        assert st[k] == rst[k], f"{k}: {st[k]} vs oracle {rst[k]}"


def test_partial_sum_cap_renders_in_passes(gpu, oracle, monkeypatch):
    """The partial film sums (16 K bytes per pixel) are capped (2 GiB; capi_render.cpp partials_passes): a frame beyond the cap renders in P
    passes over one buffer, pass p taking the rank's super-tiles p, p + P, ... as rank `rank + world * p` of `world * P`.  With the cap
    turned down to one, two and five super-tiles per pass (12, 6 and 3 passes over this film's 4 x 3 super-tiles), alone and as one of
    three ranks: the one-pass film and the oracle's, bit for bit, and the canonical counters summed over the passes."""
    sd = scenes.cornell_scene(200, 136)
    kw = dict(max_depth=4, spp=(8, 9), seed=5)  # 72 spp: K = 2 chunks, 128 KB of partial sums per super-tile
    ref, rst = oracle.OracleScene(sd).render(**kw)
    with gpu.Scene(sd) as sc:
        for cap_kb in (128, 300, 700):
            monkeypatch.setenv("PBRT_HIP_PARTIALS_CAP_KB", str(cap_kb))
            film, st = sc.render(counters=True, **kw)
            assert_bit_equal(film, ref, f"film in passes of {cap_kb} KB")
            for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
                assert st[k] == rst[k], f"{k} at {cap_kb} KB: {st[k]} vs oracle {rst[k]}"
            assert st["samples"] == 200 * 136 * 72
            acc = np.zeros_like(film)
            for r in range(3):
                acc += sc.render(rank=r, world_size=3, **kw)[0]
            assert_bit_equal(acc, ref, f"union of 3 ranks in passes of {cap_kb} KB")
        monkeypatch.delenv("PBRT_HIP_PARTIALS_CAP_KB")


@pytest.mark.parametrize("spp", [(1, 1), (7, 1), (5, 5), (9, 7), (8, 8), (13, 5), (16, 8), (17, 15), (16, 16), (32, 16), (25, 21)])
def test_sample_chunks(gpu, oracle, spp):
    """K = sample_chunks(spp) chunks per pixel -- 1 below 64 spp, then 2, 4, 8, 16 (at least 32 samples per chunk) -- with
    boundaries floor(c * spp / K): every K, with and without a remainder."""
    sd = scenes.cornell_scene(40, 24) if spp[0] * spp[1] > 64 else SMALL_SCENES["cornell"]()
    ref, _ = oracle.OracleScene(sd).render(max_depth=5, spp=spp, seed=21)
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(max_depth=5, spp=spp, seed=21)
    assert_bit_equal(film, ref, f"cornell at {spp[0]}x{spp[1]} spp")
    assert (film[..., 3] == spp[0] * spp[1]).all()


@pytest.mark.parametrize("name,integrator,depth,spp,seed", [
    ("check_sphere", INTEGRATOR_PATH, 5, (4, 8), 9),   # spheres + mirror + distant / infinite lights
    ("sphere", INTEGRATOR_DIRECT, 5, (8, 4), 0),        # direct lighting
    ("deep", INTEGRATOR_PATH, 6, (8, 4), 6),            # HBM-overflow variant of the walk
    ("ties", INTEGRATOR_PATH, 8, (6, 6), 5),            # duplicated / coplanar / degenerate geometry
    ("cornell", INTEGRATOR_PATH, 16, (6, 5), 3),        # shallow tree: two node steps per scheduling check
])
@pytest.mark.parametrize("sampler", ["stratified", "sobol"])
def test_kernel_variants_and_samplers(gpu, oracle, name, integrator, depth, spp, seed, sampler):
    """Every instantiation of the render kernel (spheres, overflow stack, shallow / deep trees, exact walk) with both
    samplers -- the stratified one of DESIGN.md 3.1 and the padded (0,2)-sequence of 3.10: film and canonical counters
    equal the oracle's."""
    sd = SMALL_SCENES[name]()
    ref, rst = oracle.OracleScene(sd).render(integrator=integrator, max_depth=depth, spp=spp, seed=seed, sampler=sampler)
    with gpu.Scene(sd) as sc:
        film, st = sc.render(integrator=integrator, max_depth=depth, spp=spp, seed=seed, counters=True, sampler=sampler)
        film2, _ = sc.render(integrator=integrator, max_depth=depth, spp=spp, seed=seed, sampler=sampler)
    assert_bit_equal(film, ref, f"{name} film ({sampler}, exact walk)")
    assert_bit_equal(film2, ref, f"{name} film ({sampler})")
    for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
        assert st[k] == rst[k], f"{k}: {st[k]} vs oracle {rst[k]}"


def test_sobol_sampler_converges_faster(gpu, oracle):
    """Sanity of the (0,2)-sequence sampler as a sampler: at equal sample counts the image is closer to a converged
    reference than the stratified one's on a directly lit scene (smooth integrand, where low discrepancy pays)."""
    sd = SMALL_SCENES["sphere"]()
    with gpu.Scene(sd) as sc:
        conv, _ = sc.render(integrator=INTEGRATOR_DIRECT, spp=(32, 32), seed=1)
        a, _ = sc.render(integrator=INTEGRATOR_DIRECT, spp=(4, 4), seed=2)
        b, _ = sc.render(integrator=INTEGRATOR_DIRECT, spp=(4, 4), seed=2, sampler="sobol")
    def mse(f):
        return float(((f[..., :3] / f[..., 3:4] - conv[..., :3] / conv[..., 3:4]) ** 2).mean())
    assert mse(b) < 1.5 * mse(a)  # (never much worse; usually better)


def test_render_limits(gpu):
    """sample counts beyond the 20-bit field, depths beyond the 10-bit field, a box filter radius other than 0.5
    and a second render while one is in flight are refused with an error instead of hanging the device."""
    from pbrt_amd import _lib
    sd = SMALL_SCENES["cornell"]()
    with gpu.Scene(sd) as sc:
        for kw, code in ((dict(spp=(2048, 1024)), -4), (dict(spp=(1, 1), max_depth=1024), -4), (dict(spp=(1, 1), filter_width=(17.0, 0.5)), -4),
                         (dict(spp=(1, 1), filter_width=(-1.0, 0.5)), -1), (dict(spp=(1, 1), filter_width=(1.0, 0.5), counters=True), -1),
                         (dict(spp=(1, 1), max_sample_luminance=-1.0), -1), (dict(spp=(1, 1), sampler=7), -1)):
            with pytest.raises(_lib.PbrtHipError) as e:
                sc.render(**kw)
            assert e.value.code == code, (kw, str(e.value))
        film, _ = sc.render(spp=(1024, 1024 // 1024), max_depth=1023)  # the limits themselves are fine (2^10 samples here)
        assert np.isfinite(film).all()
        import torch
        slab = torch.empty(max(sc.slab_floats() // 4, 1), 4, device="cuda")
        sc.render_device(slab.data_ptr(), torch.cuda.current_stream().cuda_stream, spp=(2, 2))
        with pytest.raises(_lib.PbrtHipError) as e:
            sc.render_device(slab.data_ptr(), torch.cuda.current_stream().cuda_stream, spp=(2, 2))
        assert "in flight" in str(e.value)
        sc.render_wait()
        sc.render_device(slab.data_ptr(), torch.cuda.current_stream().cuda_stream, spp=(2, 2))
        sc.render_wait()


def test_rays_parallel_to_an_axis_are_pruned_like_any_other(gpu, oracle):
    """A direction component that is exactly 0 (a shadow ray towards a sun straight overhead -- pbrt-v3's default distant light points
    along z --, a probe ray along an axis) used to turn every quantised plane's t on that axis into NaN (q x inf - inf): the axis dropped
    out of the slab test and such a ray walked every node its remaining coordinate allowed -- 2 500 x the frame time on 1 M triangles,
    found with the 2^24-triangle scene.  The production walk now multiplies by a huge finite power of two instead (kernels.hip trav_run,
    host_math.hpp inv_parallel_for_extent): same film and hits as the oracle, and about the node fetches of a ray that is not parallel."""
    from pbrt_amd import LIGHT_DISTANT
    fetches = {}
    for name, w in (("overhead", (0.0, 0.0, 1.0)), ("tilted", (0.01, 0.02, 1.0))):
        sd = scenes.random_mesh_scene(20000, 96, 96)
        v = np.array(w) / np.linalg.norm(w)
        sd.lights = np.array([[LIGHT_DISTANT, v[0], v[1], v[2], 3, 3, 3]], np.float32)
        sd = sd.normalized()
        kw = dict(max_depth=3, spp=(2, 2), seed=1)
        ref, rst = oracle.OracleScene(sd).render(**kw)
        with gpu.Scene(sd) as sc:
            film, _ = sc.render(**kw)
            _, wk = sc.render(counters="walk", **kw)
        assert_bit_equal(film, ref, f"sun {name}")
        fetches[name] = wk["nodes_visited"] / (rst["camera_rays"] + rst["bounce_rays"] + rst["shadow_rays"])
    assert fetches["overhead"] < 1.5 * fetches["tilted"], fetches
    # probe rays along the axes and the diagonals of the coordinate planes, from inside and outside the scene
    sd = SMALL_SCENES["mesh20k"]()
    rng = np.random.default_rng(5)
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [0, -1, 1], [-1, 0, 1], [0, -0.0, 1]], np.float32)
    d = np.repeat(dirs, 200, 0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = rng.uniform(-1.6, 1.6, d.shape).astype(np.float32)
    o[::3] = np.round(o[::3] * 4) / 4  # origins on round coordinates: planes of the grid the nodes sit on
    tmax = np.full(len(d), np.inf, np.float32)
    with gpu.Scene(sd) as sc:
        hit = sc.intersect(o, d, tmax)
        occ = sc.occluded(o, d, tmax)
    ref = oracle.OracleScene(sd)
    for a, b, what in zip(hit[:4], ref.intersect(o, d, tmax)[:4], ("t", "prim", "b1", "b2")):
        assert_bit_equal(a, b, f"axis-parallel rays: {what}")
    assert np.array_equal(occ != 0, ref.occluded(o, d, tmax) != 0)


def _torture():
    import importlib.util
    spec = importlib.util.spec_from_file_location("torture_probe", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "torture_probe.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.timeout(900)
def test_work_per_ray_is_bounded_off_the_baseline_track(gpu):
    """the cliff of round 5 (every shadow ray towards a sun straight overhead walked the whole tree: 2 500 x the
    frame time) lived four rounds because the suite's only WORK bound was on BASELINE's own ray mix.  Here the 1 M-triangle scene of C3
    under the sixteen variations of tools/torture_probe.py -- point lights on round coordinates, suns along the axes and a diagonal, a sky,
    all mirrors, cameras looking exactly along an axis, direct lighting, depth 0 and 64 -- must cost at most 1.5 x the default frame's
    64-byte fetches per ray and 1.5 x its triangle tests per ray (production-walk counters: box-independent); the three variants without a
    counting instantiation (MIS, Halton, a wide filter) at most 3 x its kernel time in this same job."""
    tp = _torture()
    base = None
    for name, scene_kw, render_kw in tp.VARIANTS:
        sd = tp.variant_scene(n=1_000_000, res=256, **scene_kw)
        k = dict(max_depth=8, spp=(2, 2), seed=1)
        k.update(render_kw)
        with gpu.Scene(sd) as sc:
            sc.render(**k)
            film, st = sc.render(**k)
            w = tp.walk_work(sc, **k)
        assert np.isfinite(film).all(), name
        if base is None:
            base = (w, st["kernel_ms"])
            assert w[0] < 45.0 and w[1] < 6.0, w  # (C3's own: 38.4 + 4.8 at the frame's 2048^2; this frame's camera rays are fewer)
            continue
        if w is not None:
            assert w[0] <= 1.5 * base[0][0] and w[1] <= 1.5 * base[0][1], (name, w, base[0])
        else:
            assert st["kernel_ms"] <= 3.0 * base[1], (name, st["kernel_ms"], base[1])


# fetches / triangle tests per ray of the production walk on tools/torture_probe.py's stress geometries (256 x 256, 4 spp, depth 8), measured
# in round 6 (profiles/r06_torture_probe.txt) and asserted as CEILINGS with 25 % of room: a builder or kernel change that makes one of them
# worse fails here.  "inherent": slow by the nature of a BVH of boxes without spatial splits -- today's figures, not a target.
TORTURE_CEILINGS = {  # name: (64-byte fetches, triangle tests) per ray, measured (gpurun_out/r06c: the suite's own first run printed them)
    "random soup": (35.33, 4.83),
    "flat grid of quads in z = 0": (3.59, 1.45),
    "20 stacked floors of quads": (15.85, 1.92),
    "needles spanning the scene (inherent)": (7890.3, 6143.3),   # every needle's box is the scene: nothing prunes (spatial splits would)
    "a cluster of 1e-5 triangles in a corner": (33.40, 21.51),
    "20 000 coincident triangles (inherent)": (102.75, 238.76),  # 20 000 equal boxes: a walk that reaches one reaches a leaf chain of them
    "40 concentric spherical shells": (11.49, 3.66),
}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("index", range(7))
def test_stress_geometries_keep_their_work_per_ray(gpu, oracle, index):
    tp = _torture()
    name, make = tp.GEOMETRIES[index]
    sd = tp.with_mesh(*make())
    kw = dict(max_depth=8, spp=(2, 2), seed=1)
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(**kw)
        w = tp.walk_work(sc, **kw)
    x0, y0 = sd.xres // 2, sd.yres // 2
    crop = (0.5, 0.5 + 16 / sd.xres, 0.5, 0.5 + 16 / sd.yres)
    ref, _ = oracle.OracleScene(dataclasses.replace(sd, crop=crop).normalized()).render(**kw)
    assert_bit_equal(film[y0:y0 + 16, x0:x0 + 16], ref, name)
    assert name in TORTURE_CEILINGS, (name, w)
    cf, ct = TORTURE_CEILINGS[name]
    assert w[0] <= 1.25 * cf and w[1] <= 1.25 * ct, (name, w, TORTURE_CEILINGS[name])


def test_maximum_triangle_count_matches_oracle(gpu, oracle):
    """The largest scene the boundary takes -- 2^24 triangles (a leaf reference holds a 24-bit slot) -- built and optimised on the
    device (1.1 s), rendered and intersected: film and 20 000 hit records equal to the oracle's on the same arrays; one triangle more is
    refused with PBRT_HIP_ERR_LIMIT (tools/max_size_check.py is the same as a script; profiles/r05y_max_size_check.txt)."""
    from pbrt_amd import _lib
    sd = scenes.random_mesh_scene((1 << 24) - 14, 64, 48)  # + the box's 12 triangles and the light's 2
    assert sd.idx.shape[0] == 1 << 24
    kw = dict(max_depth=6, spp=(2, 2), seed=7)
    o, d, tmax = random_rays(20000, 3, inside=1.9)
    with gpu.Scene(sd) as sc:
        assert sc.build_info()["gpu_built"]
        film, st = sc.render(**kw)
        hit = sc.intersect(o, d, tmax)
        occ = sc.occluded(o, d, tmax)
    ref = oracle.OracleScene(sd)
    assert_bit_equal(film, ref.render(**kw)[0], "film of the 2^24-triangle scene")
    rhit = ref.intersect(o, d, tmax)
    for a, b, what in zip(hit[:4], rhit[:4], ("t", "prim", "b1", "b2")):
        assert_bit_equal(a, b, f"2^24 triangles: {what}")
    assert (rhit[1] != 0xffffffff).mean() > 0.9 and np.array_equal(occ != 0, ref.occluded(o, d, tmax) != 0)
    del ref
    more = SMALL_SCENES["cornell"]()
    more.P = np.zeros((3, 3), np.float32)
    more.idx = np.zeros(((1 << 24) + 1, 3), np.uint32)
    more.mat_id = np.zeros((1 << 24) + 1, np.uint16)
    with pytest.raises(_lib.PbrtHipError) as e:
        gpu.Scene(more.normalized())
    assert e.value.code == -4 and "2^24" in str(e.value)


@pytest.mark.parametrize("res", [(1, 1), (1, 65), (65, 1), (63, 64), (129, 2), (3, 200)])
def test_tiny_and_thin_films(gpu, oracle, res):
    """Films of one pixel, one row, one column, one pixel short of a super-tile, a few pixels over two: the ragged ends of the 64 x 64
    super-tiles and of the item hand-out, alone and as one of three ranks (some of which own nothing), default and wide filter."""
    sd = scenes.cornell_scene(*res)
    kw = dict(max_depth=4, spp=(3, 2), seed=6)
    o = oracle.OracleScene(sd)
    ref, _ = o.render(**kw)
    with gpu.Scene(sd) as sc:
        film, st = sc.render(counters=True, **kw)
        parts = sum(sc.render(rank=r, world_size=3, **kw)[0] for r in range(3))
        wide, _ = sc.render(filter_width=(1.5, 2.0), **kw)
    assert film.shape == (res[1], res[0], 4) and st["samples"] == res[0] * res[1] * 6
    assert_bit_equal(film, ref, f"{res[0]} x {res[1]} film")
    assert_bit_equal(parts, ref, "three ranks")
    assert_bit_equal(wide, o.render(filter_width=(1.5, 2.0), **kw)[0], "wide box filter")


@pytest.mark.parametrize("case", ["fov 179", "fov 0.01", "scaled", "sheared + mirrored", "far away"])
def test_unusual_cameras(gpu, oracle, case):
    """Cameras off the beaten track: the widest and the narrowest fields of view, a camera-to-world matrix with a scale (ray directions that
    are not unit vectors: `Scale` before `Camera` in a scene file), with a shear and a mirror, and a camera 10^5 scene sizes away."""
    sd = SMALL_SCENES["mesh1k"]()
    c2w = sd.cam_to_world.copy()
    if case == "fov 179":
        sd.fov = 179.0
    elif case == "fov 0.01":
        sd.fov = 0.01
    elif case == "scaled":
        c2w[:3, :3] *= np.float32(2.5)
    elif case == "sheared + mirrored":
        c2w[:3, :3] = c2w[:3, :3] @ np.array([[-1, 0.3, 0], [0, 1, 0.2], [0, 0, 1]], np.float32)
    else:
        c2w[:3, 3] = c2w[:3, 3] + c2w[:3, 2] * np.float32(-3e5)  # back along the viewing direction
        sd.fov = 0.0005
    sd.cam_to_world = c2w
    sd = sd.normalized()
    kw = dict(max_depth=5, spp=(2, 2), seed=4)
    ref, rst = oracle.OracleScene(sd).render(**kw)
    with gpu.Scene(sd) as sc:
        film, st = sc.render(counters=True, **kw)
    assert_bit_equal(film, ref, case)
    for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
        assert st[k] == rst[k], (case, k)
    assert np.isfinite(film).all()


@pytest.mark.parametrize("seed", range(6))
def test_degenerate_scene_features(gpu, oracle, seed):
    """Things scenes should not contain and do: a point light exactly ON a mesh vertex (every shadow ray towards it aims at the corner of a
    triangle's own box, where fp32 Moeller-Trumbore used to accept hits that only some walks saw: the own-box rule), lights with zero and with enormous intensity,
    a distant light whose direction is the zero vector, zero-area emitters, materials with Kd = 0 and Kd > 1 (energy-creating), spheres that
    coincide, contain the camera, are 1e-6 and 1e6 across, hundreds of lights -- film, hit records and occlusion equal to the oracle's, and
    nothing that is not a number in the film (the sample filter of SURVEY A11 drops what the arithmetic cannot hold)."""
    from pbrt_amd import LIGHT_DISTANT, LIGHT_POINT
    rng = np.random.default_rng(1000 + seed)
    sd = SMALL_SCENES["mesh1k"]()
    P, idx = sd.P.copy(), sd.idx.copy()
    lights = [[LIGHT_POINT, *P[[1304, 7, 977, 2100, 55, 1500][seed]], 5, 5, 5],                 # ON a vertex (1304: the recorded case of 3.4)
              [LIGHT_POINT, *rng.uniform(-1, 1, 3), 0, 0, 0],                         # no intensity
              [LIGHT_POINT, *rng.uniform(-1, 1, 3), 1e30, 1e30, 1e30],                # overflows the film's floats
              [LIGHT_DISTANT, 0, 0, 0, 2, 2, 2]]                                       # no direction
    lights += [[LIGHT_POINT, *rng.uniform(-1.5, 1.5, 3), *rng.uniform(0, 0.3, 3)] for _ in range(300 if seed % 2 else 0)]
    mats = sd.materials.copy()
    mats[0, 1:4] = 0.0                      # black
    mats[1 % len(mats), 1:4] = 1.7          # reflects more than arrives
    tri = int(rng.integers(0, len(idx)))
    idx[tri] = idx[tri][[0, 0, 1]]          # a zero-area triangle ...
    mats = np.concatenate([mats, [[0, 0.5, 0.5, 0.5, 4, 4, 4]]]).astype(np.float32)
    mat_id = sd.mat_id.copy()
    mat_id[tri] = len(mats) - 1             # ... that emits
    eye = sd.cam_to_world[:3, 3]
    spheres = [[0.3, 0.2, 0.1, 0.25, 0], [0.3, 0.2, 0.1, 0.25, 1 % len(mats)],        # twice the same sphere: the smaller primitive number wins
               [*rng.uniform(-1, 1, 3), 1e-6, 0], [0, 0, 0, 1e6, 0], [*eye, 0.05, 0]]  # a speck; everything is inside this one; round the camera (seed 3: a black film)
    sd = dataclasses.replace(sd, idx=idx, mat_id=mat_id, materials=mats, mat_tex=np.zeros(len(mats), np.uint32), lights=np.array(lights, np.float32),
                             spheres=np.array(spheres[: 2 + seed % 4], np.float32).reshape(-1, 5)).normalized()
    kw = dict(max_depth=6, spp=(2, 2), seed=seed, integrator=[INTEGRATOR_PATH, INTEGRATOR_DIRECT, 2][seed % 3], sampler=["stratified", "halton"][seed % 2])
    ref, _ = oracle.OracleScene(sd).render(**kw)
    o, d, tmax = random_rays(2000, seed, inside=1.8)
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(**kw)
        hit, occ = sc.intersect(o, d, tmax), sc.occluded(o, d, tmax)
    assert_bit_equal(film, ref, f"degenerate scene {seed}")
    assert np.isfinite(film).all()
    rs = oracle.OracleScene(sd)
    for a, b, what in zip(hit[:4], rs.intersect(o, d, tmax)[:4], ("t", "prim", "b1", "b2")):
        assert_bit_equal(a, b, f"degenerate scene {seed}: {what}")
    assert np.array_equal(occ != 0, rs.occluded(o, d, tmax) != 0)


def test_large_film_matches_oracle(gpu, oracle):
    """A 16 384 x 16 384 film (268 M pixels, 4.3 GB; 65 536 super-tiles; the partial sums in three passes under the 2 GiB cap) at one sample
    per pixel: weight 1 everywhere, finite, and three 16 x 16 windows -- both far corners and one inside -- equal to the oracle's.
    (32 768 x 32 768 renders likewise in 0.4 s of kernel time: profiles/README.md r05y; the suite stays at a size whose host-side checks
    take a second.)"""
    res = 16384
    kw = dict(max_depth=5, spp=(1, 1), seed=3)
    with gpu.Scene(scenes.cornell_scene(res, res)) as sc:
        film, st = sc.render(**kw)
    assert film.shape == (res, res, 4) and st["samples"] == res * res
    assert (film[..., 3] == 1).all() and np.isfinite(film[::7]).all()
    for (x0, y0) in ((0, 0), (res - 16, res - 16), (res // 2 + 5, res // 3)):
        crop = (x0 / res, (x0 + 16) / res, y0 / res, (y0 + 16) / res)
        ref, _ = oracle.OracleScene(scenes.cornell_scene(res, res, crop=crop)).render(**kw)
        assert_bit_equal(film[y0:y0 + 16, x0:x0 + 16], ref, f"window at {x0},{y0} of the 16k film")


def test_maximum_sample_count_matches_oracle(gpu, oracle):
    """The largest sample count the boundary takes -- PBRT_HIP_MAX_SPP = 2^20 = 1024 x 1024 strata -- on a one-pixel crop window of
    the Cornell-style box: 16 chunks of 65 536 samples, the 20-bit sample index full, the longest RNG streams and (Halton) the most
    digits any frame can have (13 in base 3); bit-equal to the oracle, weight 2^20."""
    sd = scenes.cornell_scene(64, 64, crop=(0.5, 0.5 + 1 / 64, 0.25, 0.25 + 1 / 64))
    o = oracle.OracleScene(sd)
    with gpu.Scene(sd) as sc:
        for sampler in ("stratified", "halton"):
            kw = dict(max_depth=5, spp=(1024, 1024), seed=1, sampler=sampler)
            film, st = sc.render(**kw)
            assert film.shape == (1, 1, 4) and film[0, 0, 3] == float(1 << 20) and st["samples"] == 1 << 20
            assert_bit_equal(film, o.render(**kw)[0], f"one pixel at 2^20 spp, {sampler}")


@pytest.mark.parametrize("n_gpus", [1, 2])
def test_multi_gpu_render_in_one_process(gpu, oracle, n_gpus):
    """pbrt_hip_multi_*: the scene replicated device to device, one stream per GPU, ONE RCCL gather (a group call of
    ncclGather on communicators from ncclCommInitAll) and the assembly on GPU 0 -- the film must equal the oracle's and
    the single-GPU path's bit for bit.  n_gpus = 1 needs no collective (RCCL is not even loaded); n_gpus = 2 needs two
    devices."""
    if gpu.device_count() < n_gpus:
        pytest.skip(f"needs {n_gpus} GPUs")
    sd = scenes.cornell_scene(200, 136)  # 4 x 3 super-tiles, ragged edges
    kw = dict(max_depth=4, spp=(3, 2), seed=8)
    ref, _ = oracle.OracleScene(sd).render(**kw)
    with gpu.MultiScene(sd, n_gpus) as ms:
        assert ms.n_gpus == n_gpus
        film, stats = ms.render(**kw)
        again, _ = ms.render(**kw)
        import torch
        w, h = sd.crop_size()
        dev = np.empty((h, w, 4), np.float32)
        torch.cuda.synchronize()
        import ctypes as C
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(dev.ctypes.data_as(C.c_void_p), C.c_void_p(ms.film_device_ptr()), dev.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    assert_bit_equal(film, ref, f"film of {n_gpus} GPU(s) in one process")
    assert_bit_equal(again, ref, "second frame of the same handle")
    assert_bit_equal(dev, ref, "the assembled film on GPU 0")
    assert len(stats) == n_gpus and sum(s["samples"] for s in stats) == 200 * 136 * 6
    one, _ = gpu.render_multi(sd, n_gpus, **kw)  # create + render + destroy in one call (what world_end would do)
    assert_bit_equal(one, ref, "pbrt_hip_render_multi")
    with pytest.raises(gpu.api._lib.PbrtHipError):
        gpu.MultiScene(sd, gpu.device_count() + 1)


@pytest.mark.parametrize("n_ranks", [2, 3, 8])
def test_multi_gpu_code_path_with_more_ranks_than_devices(gpu, oracle, monkeypatch, n_ranks):
    """The in-library multi-GPU path at N > 1 on a box with one GPU (PBRT_HIP_MULTI_LOOPBACK: rank g on device g mod <devices>; the
    frame's one exchange made of device-to-device copies / an adding kernel, because RCCL refuses two ranks on one device).  Everything
    but the ncclGather / ncclReduce calls themselves is the code eight real GPUs run: the scene replicated, the ranks' shares launched on
    their own streams, the gathered layout, the assembly, per-rank statistics, a wide filter's integer sums, a rank without tiles, a
    failing rank.  Films equal the oracle's bit for bit."""
    monkeypatch.setenv("PBRT_HIP_MULTI_LOOPBACK", "1")
    sd = scenes.cornell_scene(200, 136)  # 4 x 3 super-tiles, ragged edges
    kw = dict(max_depth=4, spp=(3, 2), seed=8)
    o = oracle.OracleScene(sd)
    ref, _ = o.render(**kw)
    with gpu.MultiScene(sd, n_ranks) as ms:
        assert ms.n_gpus == n_ranks
        film, stats = ms.render(**kw)
        again, _ = ms.render(**dict(kw, sampler="halton"))
        wide, _ = ms.render(filter_width=(1.5, 0.75), **kw)
        back, _ = ms.render(**kw)  # after a wide frame: the gathered buffer changes its role and back
        monkeypatch.setenv("PBRT_HIP_MULTI_FAIL_RANK", str(n_ranks - 1))
        with pytest.raises(gpu.api._lib.PbrtHipError) as e:
            ms.render(**kw)
        assert "injected" in str(e.value)
        monkeypatch.delenv("PBRT_HIP_MULTI_FAIL_RANK")
        after, _ = ms.render(**kw)  # nobody was left waiting: the handle renders on
    assert_bit_equal(film, ref, f"film of {n_ranks} ranks")
    assert_bit_equal(again, o.render(**dict(kw, sampler="halton"))[0], "Halton frame of the same handle")
    assert_bit_equal(wide, o.render(filter_width=(1.5, 0.75), **kw)[0], f"wide box filter, {n_ranks} ranks' accumulators added")
    assert_bit_equal(back, ref, "default filter after a wide frame")
    assert_bit_equal(after, ref, "frame after a failed launch")
    assert len(stats) == n_ranks and sum(s["samples"] for s in stats) == 200 * 136 * 6
    assert all(s["samples"] > 0 and s["kernel_ms"] > 0 for s in stats)  # 12 super-tiles: every one of up to 8 ranks owns some
    tiny = scenes.cornell_scene(100, 60)  # 2 x 1 super-tiles: ranks 2 .. own nothing and send zeros
    one, st = gpu.render_multi(tiny, n_ranks, **kw)
    assert_bit_equal(one, oracle.OracleScene(tiny).render(**kw)[0], "pbrt_hip_render_multi with idle ranks")
    assert [s["samples"] > 0 for s in st] == [True, True] + [False] * (n_ranks - 2)


def test_render_prepare_leaves_nothing_to_allocate(gpu, oracle):
    """pbrt_hip_render_prepare (what pbrt_hip_multi_render calls for every GPU before the first launch of a frame, so that no
    hipMalloc separates the launches): the scene's device footprint does not change between a prepared render's launch and its
    end, the film is the oracle's, and a description the render would refuse is refused here too."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")  # (the runtime the library itself is linked against: no second one is brought in)

    def free_bytes():
        free, total = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    sd = scenes.random_mesh_scene(1000, 512, 512)
    small, big = dict(max_depth=2, spp=(2, 2), seed=5), dict(max_depth=2, spp=(16, 8), seed=5)  # 1 and 4 chunks per pixel: 4 / 17 MB of partial sums
    grew = {}
    for prepared in (False, True):
        with gpu.Scene(sd, builder="gpu") as sc:
            slab = C.c_void_p()
            assert hip.hipMalloc(C.byref(slab), C.c_size_t(max(sc.slab_floats() * 4, 16))) == 0
            sc.render_device(slab.value, None, **small)  # (the kernel's code object, the runtime's own pools: everything a first launch brings)
            sc.render_wait()
            if prepared:
                sc.render_prepare(**big)
            before = free_bytes()
            sc.render_device(slab.value, None, **big)
            sc.render_wait()
            grew[prepared] = before - free_bytes()
            assert hip.hipFree(slab) == 0
            if prepared:
                with pytest.raises(RuntimeError):
                    sc.render_prepare(max_depth=4, spp=(2048, 1024), seed=5)  # 2^21 samples per pixel
    assert grew[False] > 8 << 20, grew  # (the measurement sees an unprepared render allocate)
    assert grew[True] == 0, f"render_device allocated {grew[True]} bytes after render_prepare"
    sd = SMALL_SCENES["mesh1k"]()
    ref, _ = oracle.OracleScene(sd).render(max_depth=4, spp=(3, 2), seed=5)
    with gpu.Scene(sd, builder="gpu") as sc:
        sc.render_prepare(max_depth=4, spp=(3, 2), seed=5)
        film, _ = sc.render(max_depth=4, spp=(3, 2), seed=5)
    assert_bit_equal(film, ref, "film after a prepared render")


def test_rank_without_tiles(gpu, oracle):
    """A frame of one 64x64 super-tile split over three ranks: ranks 1 and 2 own nothing and must return an empty
    (all-zero) film (found by the randomised tests of round 1: a division by the zero workgroups of such a rank)."""
    sd = scenes.cornell_scene(40, 33)
    ref, _ = oracle.OracleScene(sd).render(max_depth=3, spp=(2, 2), seed=4)
    with gpu.Scene(sd) as sc:
        parts = [sc.render(max_depth=3, spp=(2, 2), seed=4, rank=r, world_size=3) for r in range(3)]
    assert_bit_equal(parts[0][0], ref, "rank 0 holds the whole frame")
    for film, st in parts[1:]:
        assert not film.any() and st["samples"] == 0


def test_golden_fixture(gpu):
    """tests/golden/render_golden.npz: films the oracle produced when the fixtures were made
    (tests/golden/make_golden.py); the HIP path must reproduce them bit for bit."""
    import os
    from util import checker_plane_scene, checker_sphere_scene
    every = dict(SMALL_SCENES, checker=lambda: checker_plane_scene(40)[0], checkersphere=lambda: checker_sphere_scene(48, 40))
    # (render_golden_r05.npz: what round 5 added beside the default path -- samplers 2 / 3, integrator 2, a checkerboard Kd on triangles and on a sphere)
    for fixture, n in (("render_golden.npz", 6), ("render_golden_r05.npz", 11)):
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", fixture))
        assert len(g.files) == n
        for key in g.files:
            name, integ, depth, sx, sy, seed, sampler = key.split("-")
            sd = every[name]()
            with gpu.Scene(sd) as sc:
                film, _ = sc.render(integrator=int(integ), max_depth=int(depth), spp=(int(sx), int(sy)), seed=int(seed), sampler=int(sampler))
            assert_bit_equal(film, g[key], f"{fixture}: {key}")


def test_ranks_partition_and_crop(gpu, oracle):
    sd = scenes.cornell_scene(200, 136)
    ref, _ = oracle.OracleScene(sd).render(max_depth=4, spp=(2, 1), seed=2)
    with gpu.Scene(sd) as sc:
        full, _ = sc.render(max_depth=4, spp=(2, 1), seed=2)
        acc = np.zeros_like(full)
        for r in range(3):
            part, st = sc.render(max_depth=4, spp=(2, 1), seed=2, rank=r, world_size=3)
            assert ((acc[..., 3] == 0) | (part[..., 3] == 0)).all()
            acc += part
    assert_bit_equal(full, ref, "full")
    assert_bit_equal(acc, ref, "union of 3 ranks")
    crop = (0.25, 0.75, 0.5, 1.0)
    sdc = scenes.cornell_scene(64, 64, crop=crop)
    with gpu.Scene(sdc) as sc:
        part, _ = sc.render(max_depth=4, spp=(2, 1), seed=1)
    with gpu.Scene(scenes.cornell_scene(64, 64)) as sc:
        whole, _ = sc.render(max_depth=4, spp=(2, 1), seed=1)
    assert_bit_equal(part, whole[32:64, 16:48], "crop window")


def test_device_slab_path_with_torch(gpu, oracle):
    """render_device + film_assemble_device on torch-owned buffers / torch's stream, and the
    torch-side assembly used by the multi-GPU launcher."""
    import torch
    from pbrt_amd import dist as pdist
    sd = scenes.cornell_scene(200, 136)
    ref, _ = oracle.OracleScene(sd).render(max_depth=3, spp=(2, 2), seed=6)
    with gpu.Scene(sd) as sc:
        slabs = []
        for r in range(2):
            n = sc.slab_floats(r, 2)
            slab = torch.full((n // 4, 4), -1.0, device="cuda")
            sc.render_device(slab.data_ptr(), torch.cuda.current_stream().cuda_stream, max_depth=3, spp=(2, 2), seed=6,
                             rank=r, world_size=2)
            st = sc.render_wait()
            assert st["kernel_ms"] > 0
            slabs.append(slab)
        film = pdist.assemble_film(slabs, sd.xres, sd.yres, sd.crop, 2)
        assert_bit_equal(film.cpu().numpy(), ref, "torch-assembled film")
        film2 = torch.zeros(sd.yres, sd.xres, 4, device="cuda")
        for r in range(2):
            sc.film_assemble_device(slabs[r].data_ptr(), r, 2, film2.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert_bit_equal(film2.cpu().numpy(), ref, "kernel-assembled film")
        f1, _ = pdist.render_sharded(sc, 0, 1, max_depth=3, spp=(2, 2), seed=6)
        assert_bit_equal(f1.cpu().numpy(), ref, "render_sharded world 1")


@pytest.mark.parametrize("builder", BUILDERS)
def test_c2_crop_windows_at_full_spp(gpu, oracle, builder):
    """BASELINE config C2 (100k triangles, 1024x1024, 256 spp, maxdepth 8): two 32x32 windows of
    the frame at the full sample count against the oracle, bit for bit -- films from the production walk of the builder's tree,
    canonical counters (for the device-built tree: through the lazily built canonical tree)."""
    for crop in [(0.5, 0.53125, 0.5, 0.53125), (0.125, 0.15625, 0.8125, 0.84375)]:
        sd = scenes.random_mesh_scene(100_000, 1024, 1024, crop=crop)
        ref, rst = oracle_render(oracle, ("c2", crop), lambda: sd, max_depth=8, spp=(16, 16), seed=0)
        with gpu.Scene(sd, builder=builder) as sc:
            assert sc.build_info()["gpu_built"] == (builder is None)
            plain, _ = sc.render(max_depth=8, spp=(16, 16), seed=0)
            film, st = sc.render(max_depth=8, spp=(16, 16), seed=0, counters=True)
        assert film.shape == (32, 32, 4)
        assert_bit_equal(plain, ref, f"C2 window {crop} ({builder} tree, production walk)")
        assert_bit_equal(film, ref, f"C2 window {crop} ({builder}, canonical walk)")
        assert st["nodes_visited"] == rst["nodes_visited"] and st["tris_tested"] == rst["tris_tested"]


@pytest.mark.parametrize("builder", BUILDERS)
def test_full_size_properties_c2(gpu, oracle, builder):
    """The whole C2 frame at reduced spp: size-independent properties + a window against the oracle."""
    sd = scenes.random_mesh_scene(100_000, 1024, 1024)
    with gpu.Scene(sd, builder=builder) as sc:
        info = sc.info()
        film, st = sc.render(max_depth=8, spp=(2, 2), seed=0)
        again, _ = sc.render(max_depth=8, spp=(2, 2), seed=0)
    assert info["depth"] <= 64 and (info["depth"] > 0) == (builder == "host")  # (a device-built scene has no canonical tree yet)
    assert film.shape == (1024, 1024, 4)
    assert (film[..., 3] == 4).all()                      # every pixel got exactly spp samples
    assert np.isfinite(film).all() and (film[..., 1] >= 0).all()
    assert_bit_equal(film, again, "idempotence")           # no run-to-run nondeterminism
    assert st["samples"] == 1024 * 1024 * 4
    ref, _ = oracle_render(oracle, "c2-full-window", lambda: scenes.random_mesh_scene(100_000, 1024, 1024, crop=(0.25, 0.3125, 0.25, 0.3125)),
                           max_depth=8, spp=(2, 2), seed=0)
    assert_bit_equal(film[256:320, 256:320], ref, "window of the full frame")


def test_full_size_wide_filter_c2_and_c3(gpu, oracle):
    """Box filter radius 1.5 at BASELINE sizes: the whole C2 frame (sobol sampler) and the whole C3 frame
    (1M triangles, 2048x2048) at a reduced sample count -- deterministic although 327 680 lanes add with atomics, weights
    9 x spp (a few per thousand more: film points that round up to the next pixel), eight ranks' accumulators adding to one
    rank's, and a window of the frame equal to the oracle's render of that crop window (whose sample bounds reach into the
    same neighbours), sampler 2 on the same scene likewise."""
    for n_tris, res, sampler, crop, sl in ((100_000, 1024, "sobol", (0.25, 0.28125, 0.5, 0.53125), (slice(512, 544), slice(256, 288))),
                                          (1_000_000, 2048, "stratified", (0.5, 0.515625, 0.25, 0.265625), (slice(512, 544), slice(1024, 1056)))):
        sd = scenes.random_mesh_scene(n_tris, res, res)
        kw = dict(max_depth=8, spp=(2, 2), seed=0, sampler=sampler)
        with gpu.Scene(sd, builder="gpu") as sc:
            film, st = sc.render(filter_width=(1.5, 1.5), **kw)
            again, _ = sc.render(filter_width=(1.5, 1.5), **kw)
            if n_tris == 100_000:
                acc, _ = sc.render_acc((1.5, 1.5), **kw)
                parts = sum(sc.render_acc((1.5, 1.5), rank=r, world_size=8, **kw)[0] for r in range(8))
                assert np.array_equal(parts, acc), "eight ranks' accumulators add to one rank's"
                nd, _ = sc.render(**dict(kw, sampler="sobol_nd"))
        assert film.shape == (res, res, 4) and np.isfinite(film).all()
        assert_bit_equal(film, again, "wide filter: run-to-run determinism")
        assert abs(film[..., 3].mean() - 36.0) < 0.05 and film[..., 3].min() >= 36.0
        assert st["samples"] == (res + 2) * (res + 2) * 4  # the sample bounds reach one pixel beyond the image on every side
        win = scenes.random_mesh_scene(n_tris, res, res, crop=crop)
        o = oracle.OracleScene(win)
        ref, _ = o.render(filter_width=(1.5, 1.5), **kw)
        assert_bit_equal(film[sl], ref, f"window of the full {res}x{res} frame, box filter 1.5")
        if n_tris == 100_000:
            assert_bit_equal(nd[sl], o.render(**dict(kw, sampler="sobol_nd"))[0], "window of the full frame, sampler 2")


@pytest.mark.parametrize("builder", BUILDERS)
def test_c2_full_frame_eight_rank_shares_add_up(gpu, oracle, builder):
    """BASELINE config C2 at its full size and sample count: the frame rendered by one rank equals, bit for bit, the sum
    of the eight shares of an 8-GPU job: sharding and the dynamic, XCD-aware hand-out of work items change no sample.  And a
    window of that full frame equals the oracle's render of the window."""
    sd = scenes.random_mesh_scene(100_000, 1024, 1024)
    with gpu.Scene(sd, builder=builder) as sc:
        full, st = sc.render(max_depth=8, spp=(16, 16), seed=0)
        acc = np.zeros_like(full)
        n = 0
        for r in range(8):
            part, pst = sc.render(max_depth=8, spp=(16, 16), seed=0, rank=r, world_size=8)
            assert ((acc[..., 3] == 0) | (part[..., 3] == 0)).all()  # shares do not overlap
            acc += part
            n += pst["samples"]
    assert n == st["samples"] == 1024 * 1024 * 256
    assert (full[..., 3] == 256).all()
    assert_bit_equal(acc, full, "sum of 8 rank shares vs the single-rank frame")
    crop = (0.5, 0.53125, 0.5, 0.53125)  # (the first window of test_c2_crop_windows_at_full_spp: the oracle's film is shared)
    ref, _ = oracle_render(oracle, ("c2", crop), lambda: scenes.random_mesh_scene(100_000, 1024, 1024, crop=crop), max_depth=8, spp=(16, 16), seed=0)
    assert_bit_equal(full[512:544, 512:544], ref, f"window of the full C2 frame at 256 spp ({builder} tree)")


_c3_window_fetches = {}


@pytest.mark.parametrize("builder", BUILDERS)
def test_c3_scene_window(gpu, oracle, builder):
    """BASELINE config C3's scene (1M triangles, 2048x2048): a 16x16 window at 32x16 = 512 spp, on the tree that ships (built and
    optimised on the device: 12 re-insertion passes over 2M nodes) and on the host's."""
    crop = (0.5, 0.5 + 16 / 2048, 0.5, 0.5 + 16 / 2048)
    sd = scenes.random_mesh_scene(1_000_000, 2048, 2048, crop=crop)
    ref, rst = oracle_render(oracle, "c3-window", lambda: sd, max_depth=8, spp=(32, 16), seed=0)
    with gpu.Scene(sd, builder=builder) as sc:
        bi = sc.build_info()
        assert bi["gpu_built"] == (builder is None) and (bi["reinsert_moves"] > 100_000) == (builder is None)
        plain, wst = sc.render(max_depth=8, spp=(32, 16), seed=0, counters="walk")
        film, st = sc.render(max_depth=8, spp=(32, 16), seed=0, counters=True)
        assert 0 < sc.info()["depth"] <= 64
    assert_bit_equal(plain, ref, f"C3 window ({builder} tree, production walk)")
    assert_bit_equal(film, ref, f"C3 window ({builder}, canonical walk)")
    assert st["nodes_visited"] == rst["nodes_visited"] and st["tris_tested"] == rst["tris_tested"]
    rays = wst["camera_rays"] + wst["bounce_rays"] + wst["shadow_rays"]
    _c3_window_fetches[builder] = wst["nodes_visited"] / rays  # 64-byte fetches per ray of the production walk (this window's ray mix)
    if len(_c3_window_fetches) == 2:  # the optimised device tree is the cheaper one to walk (full frame: 38.4 against 40.2)
        assert _c3_window_fetches[None] < _c3_window_fetches["host"], _c3_window_fetches


def test_c0_scene_file_renders_like_the_oracle(gpu, oracle):
    """BASELINE config C0 end to end: scenes/c0_check_sphere.pbrt through the C++ parser, rendered by the
    HIP path and by the oracle (resolution and sample count reduced so the oracle finishes in seconds)."""
    import os
    from pbrt_amd import loader
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "c0_check_sphere.pbrt")).read()
    text = text.replace("[400]", "[96]").replace('"integer pixelsamples" 128', '"integer pixelsamples" 8')
    ls = loader.load_string(text)
    assert (ls.scene.xres, ls.scene.yres) == (96, 96) and ls.spp == (4, 2)
    ref, _ = oracle.OracleScene(ls.scene).render(seed=0, **ls.render_kwargs())
    with gpu.Scene(ls.scene) as sc:
        film, _ = sc.render(seed=0, **ls.render_kwargs())
    assert_bit_equal(film, ref, "C0 film")
    rgb = gpu.film_to_rgb(film)
    assert rgb[5, 5].mean() > 0.3 and np.isfinite(rgb).all()  # the sky is visible and lit


def test_scene_file_with_plymesh_and_instances_renders_like_the_oracle(gpu, oracle, tmp_path):
    """The data formats on the input side that pbrt-v3 scenes use and the reference stops short of (parser.rs:283-300): a binary PLY
    height field (quads, per-vertex (u, v)) defined once as an object and instanced three times -- moved, scaled, mirrored --, textured with
    a checkerboard, beside a ground plane, an area light and a mirror sphere.  One flattened BVH; HIP film == oracle film bit for bit."""
    from pbrt_amd import loader
    from test_parser import _ply_bytes
    n = 24
    g = np.linspace(-1, 1, n + 1)
    verts = [(float(x), float(y), float(0.15 * np.sin(3 * x) * np.cos(2 * y))) for y in g for x in g]
    uv = [(float(i / n), float(j / n)) for j in range(n + 1) for i in range(n + 1)]
    faces = [(j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i) for j in range(n) for i in range(n)]
    (tmp_path / "bumps.ply").write_bytes(_ply_bytes("binary_little_endian", verts, faces, uv=uv, with_normals=True))
    (tmp_path / "scene.pbrt").write_text("""
LookAt 0 -6 4  0 0 0.3  0 0 1
Camera "perspective" "float fov" 40
Sampler "halton" "integer pixelsamples" 16
Integrator "path" "integer maxdepth" 5
Film "image" "integer xresolution" [72] "integer yresolution" [56]
WorldBegin
LightSource "distant" "point from" [-3 -4 10] "rgb L" [1.5 1.4 1.2]
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [12 12 12]
  Translate 0 0 4
  Shape "trianglemesh" "integer indices" [0 2 1 0 3 2] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0]
AttributeEnd
Texture "checks" "spectrum" "checkerboard" "float uscale" [6] "float vscale" [6] "rgb tex1" [.1 .1 .4] "rgb tex2" [.8 .8 .7]
ObjectBegin "bumps"
  Material "matte" "texture Kd" "checks"
  Shape "plymesh" "string filename" "bumps.ply"
ObjectEnd
Material "matte" "rgb Kd" [.5 .5 .5]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-8 -8 -0.2 8 -8 -0.2 8 8 -0.2 -8 8 -0.2]
AttributeBegin  Translate -2.2 0 0.2  ObjectInstance "bumps"  AttributeEnd
AttributeBegin  Translate 0 0.5 0.6 Rotate 30 0 0 1 Scale 0.7 0.7 2  ObjectInstance "bumps"  AttributeEnd
AttributeBegin  Translate 2.2 0 0.2 Scale -1 1 1  ObjectInstance "bumps"  AttributeEnd
AttributeBegin  Material "mirror"  Translate 0 -1.5 0.4  Shape "sphere" "float radius" 0.5  AttributeEnd
WorldEnd
""")
    ls = loader.load_file(str(tmp_path / "scene.pbrt"))
    assert ls.scene.idx.shape[0] == 2 + 2 + 3 * 2 * n * n and ls.scene.tri_uv.shape[0] == ls.scene.idx.shape[0]
    assert not [w for w in ls.warnings if "point-sampled" not in w], ls.warnings
    ref, rst = oracle.OracleScene(ls.scene).render(seed=3, **ls.render_kwargs())
    with gpu.Scene(ls.scene) as sc:
        film, _ = sc.render(seed=3, **ls.render_kwargs())
    assert_bit_equal(film, ref, "instanced PLY scene")
    rgb = gpu.film_to_rgb(film)
    assert np.isfinite(rgb).all() and rgb.mean() > 0.05


def test_c0_as_baseline_states_it(gpu, oracle):
    """BASELINE configs[0] AS WRITTEN: the check-sphere scene (scenes/c0_check_sphere.pbrt = the reference's
    scenes/check-sphere.pbrt:1-37) at 256x256, 4 samples per pixel (2x2 strata, stratified sampler), whole frame, through the C++
    parser on both sides: HIP film == oracle film bit for bit, with the file's own default sampler name ("halton") as well."""
    import os
    from pbrt_amd import loader
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "c0_check_sphere.pbrt")).read()
    text = text.replace("[400]", "[256]")
    assert 'Sampler "halton" "integer pixelsamples" 128' in text
    for sampler, line in (("stratified", 'Sampler "stratified" "integer xsamples" 2 "integer ysamples" 2'), ("halton", 'Sampler "halton" "integer pixelsamples" 4')):
        ls = loader.load_string(text.replace('Sampler "halton" "integer pixelsamples" 128', line))
        assert (ls.scene.xres, ls.scene.yres) == (256, 256) and ls.spp == (2, 2) and ls.integrator == INTEGRATOR_PATH_MIS  # (no Integrator line: "path" as pbrt-v3 means it, round 6)
        assert (ls.sampler == 0) == (sampler == "stratified")
        ref, _ = oracle.OracleScene(ls.scene).render(seed=0, **ls.render_kwargs())
        with gpu.Scene(ls.scene) as sc:
            film, st = sc.render(seed=0, **ls.render_kwargs())
        assert film.shape == (256, 256, 4) and st["samples"] == 256 * 256 * 4 and (film[..., 3] == 4).all()
        assert_bit_equal(film, ref, f"C0 film at 256x256, 4 spp, Sampler \"{sampler}\"")


def test_checkerboard_texture(gpu, oracle):
    """DESIGN.md 3.15, the TEX instantiations of the kernel (render_kernel_x): the closed form of tests/util.py on the HIP path itself,
    then films equal to the oracle's bit for bit -- path integrator over a textured plane with a mirror sphere (spheres + texture),
    every sampler, three ranks -- and the combinations that are not instantiated refused loudly."""
    from util import check_checker_plane, checker_plane_scene
    from pbrt_amd import _lib
    def render(sd):
        with gpu.Scene(sd) as sc:
            return gpu.film_to_rgb(sc.render(integrator=INTEGRATOR_DIRECT, max_depth=1, spp=(1, 1), seed=3)[0])
    assert check_checker_plane(render, lambda sd, x, y: oracle.OracleScene(sd).camera_ray(x, y)) > 0.9
    sd, _ = checker_plane_scene(72)
    sd.spheres = np.array([[0.3, 0.2, 0.6, 0.6, 1]], np.float32)
    sd.materials = np.concatenate([sd.materials, [[1, .9, .9, .9, 0, 0, 0]]]).astype(np.float32)
    sd.mat_tex = np.array([1, 0], np.uint32)
    sd.lights = np.concatenate([sd.lights, [[LIGHT_INFINITE, 0, 0, 0, .3, .35, .4]]]).astype(np.float32)
    sd.normalized()
    o = oracle.OracleScene(sd)
    for builder in (None, "host"):
        with gpu.Scene(sd, builder=builder) as sc:
            for sampler in ("stratified", "sobol", "sobol_nd", "halton"):
                kw = dict(max_depth=5, spp=(3, 2), seed=4, sampler=sampler)
                film, _ = sc.render(**kw)
                assert_bit_equal(film, o.render(**kw)[0], f"textured plane + mirror sphere, {sampler}, builder {builder}")
            kw = dict(max_depth=5, spp=(3, 2), seed=4)
            assert_bit_equal(sum(sc.render(rank=r, world_size=3, **kw)[0] for r in range(3)), o.render(**kw)[0], "three ranks")
            for bad in (dict(counters=True), dict(counters="walk")):
                with pytest.raises(_lib.PbrtHipError) as e:
                    sc.render(**dict(kw, **bad))
                assert e.value.code == -4
            for extra in (dict(filter_width=(1.5, 1.5)), dict(filter_width=(2.0, 0.75), sampler="halton", integrator=2)):  # every variant at once
                wkw = dict(kw, **extra)
                assert_bit_equal(sc.render(**wkw)[0], o.render(**wkw)[0], f"textured plane under a wide box filter: {extra}")
    # a textured material without corner (u, v) is an invalid scene, not a silent constant colour
    sd.tri_uv = np.zeros((0, 6), np.float32)
    with pytest.raises(_lib.PbrtHipError) as e:
        gpu.Scene(sd)
    assert e.value.code == -1


@pytest.mark.parametrize("name,depth,spp,seed", [("cornell", 8, (4, 4), 2), ("check_sphere", 5, (3, 2), 9), ("mesh1k", 8, (2, 2), 3), ("mesh20k", 6, (2, 1), 5),
                                                  ("ties", 8, (3, 2), 5), ("deep", 6, (2, 2), 6)])
def test_mis_integrator_matches_oracle(gpu, oracle, name, depth, spp, seed):
    """Integrator 2 (the path integrator with the direct-light estimate multiple-importance-sampled; the MIS
    instantiations of render_kernel_x): films equal to the oracle's bit for bit -- area lights, a constant environment with a
    distant light, spheres, LDS and overflow stacks, every sampler, three ranks; unsupported combinations refused."""
    from pbrt_amd import INTEGRATOR_PATH_MIS, _lib
    sd = SMALL_SCENES[name]()
    o = oracle.OracleScene(sd)
    with gpu.Scene(sd) as sc:
        for sampler in ("stratified", "sobol", "sobol_nd", "halton"):
            kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=depth, spp=spp, seed=seed, sampler=sampler)
            film, _ = sc.render(**kw)
            assert_bit_equal(film, o.render(**kw)[0], f"{name}, MIS, {sampler}")
        kw = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=depth, spp=spp, seed=seed)
        assert_bit_equal(sum(sc.render(rank=r, world_size=3, **kw)[0] for r in range(3)), o.render(**kw)[0], "three ranks")
        plain, _ = sc.render(**dict(kw, integrator=INTEGRATOR_PATH))
        if name in ("cornell", "check_sphere"):
            assert not np.array_equal(plain, film)
        with pytest.raises(_lib.PbrtHipError) as e:
            sc.render(**dict(kw, counters=True))
        assert e.value.code == -4
        wkw = dict(kw, filter_width=(1.5, 1.5), sampler="sobol_nd")
        assert_bit_equal(sc.render(**wkw)[0], o.render(**wkw)[0], f"{name}, MIS + sampler 2 under a wide box filter")


def test_far_tiny_emitter_matches_oracle_and_twin(gpu, oracle):
    """tests/test_oracle_selfcheck.py test_far_tiny_emitter_keeps_its_samples_and_equals_the_twin on the HIP path: an emitter whose
    light-sampling density squared is +inf in float32 (the light's weight is its limit, 1) -- the film bit-equal to the
    oracle's and equal to the float64 twin's at the bar of the fixed MIS cases"""
    import independent_twin as tw
    from util import FAR_TINY_EMITTER_KW as kw, far_tiny_emitter_scene
    sd = far_tiny_emitter_scene()
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(**kw)
    assert_bit_equal(film, oracle.OracleScene(sd).render(**kw)[0], "far tiny emitter, MIS")
    twin = tw.render(sd, **kw)
    rel = np.abs(twin[..., :3] - film[..., :3]) / np.maximum(np.abs(film[..., :3]), 1e-3 * film[..., :3].max())
    assert tw.psnr_db(twin, film) >= 90.0 and (rel.max(-1) < 1e-4).mean() >= 0.99, (tw.psnr_db(twin, film), (rel.max(-1) < 1e-4).mean())
    assert np.array_equal(twin[..., 3], film[..., 3])


def test_mis_closes_the_heavy_tail_of_the_emitting_box_on_the_gpu(gpu):
    """tests/test_oracle_selfcheck.py's closed form for integrator 2 on the HIP path itself: inside the emitting, reflecting CUBE --
    where light sampling alone leaves a heavy tail -- every pixel is Le sum rho^i to 0.1 % at 6 x 24^2 x 64 samples."""
    from pbrt_amd import INTEGRATOR_PATH_MIS
    from util import furnace_expectation, furnace_scene
    for rho, depth in ((0.5, 3), (0.8, 8)):
        want = furnace_expectation(rho, depth)
        with gpu.Scene(furnace_scene(rho, shape="cube", res=24)) as sc:
            rgb = [gpu.film_to_rgb(sc.render(integrator=INTEGRATOR_PATH_MIS, max_depth=depth, spp=(8, 8), seed=s)[0]) for s in range(6)]
        assert abs(float(np.mean([r.mean() for r in rgb])) - want) < 1e-3 * want
        assert rgb[0][..., 0].std() < 0.05 * want and rgb[0].max() < 1.25 * want


def test_cli_renders_c0(gpu, tmp_path):
    import os
    from pbrt_amd import cli
    scene = tmp_path / "s.pbrt"
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "c0_check_sphere.pbrt")).read()
    scene.write_text(text.replace("[400]", "[64]"))
    out = tmp_path / "o.png"
    assert cli.main(["-q", "--quick", "-o", str(out), str(scene)]) == 0
    from PIL import Image
    img = np.asarray(Image.open(out))
    assert img.shape == (64, 64, 3) and img.std() > 10


def test_native_cli_renders_c0(gpu, tmp_path):
    """pbrt_amd/lib/pbrt: the C++ command line (csrc/pbrt_main.cpp, flags of src/bin/pbrt.rs:24-44)."""
    import os
    import subprocess
    from pbrt_amd.build import CLI_PATH
    scene = tmp_path / "s.pbrt"
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "c0_check_sphere.pbrt")).read()
    scene.write_text(text.replace("[400]", "[64]"))
    out = tmp_path / "o.pfm"
    r = subprocess.run([CLI_PATH, "-v", "--quick", "-n", "4", "-o", str(out), str(scene)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "checkerboard" in r.stderr and "wrote" in r.stderr  # -v shows the parser's warning and the summary
    img = gpu.read_image(out)
    assert img.shape == (64, 64, 3) and img.std() > 0.05
    from pbrt_amd import loader
    ls = loader.load_string(scene.read_text())
    with gpu.Scene(ls.scene) as sc:
        kw = dict(ls.render_kwargs(), spp=(ls.spp[0] // 2, ls.spp[1] // 2))  # --quick; Sampler "halton" -> sampler 3
        film, _ = sc.render(**kw)
    assert_bit_equal(img, gpu.film_to_rgb(film, scale=ls.film_scale), "CLI image vs library render")  # PFM is lossless
    # the CLI renders through pbrt_hip_render_multi on every visible GPU; --gpus 1 must give the same image
    out1 = tmp_path / "o1.pfm"
    r = subprocess.run([CLI_PATH, "-q", "--quick", "--gpus", "1", "-o", str(out1), str(scene)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert_bit_equal(gpu.read_image(out1), img, "CLI --gpus 1 vs all GPUs")
    assert subprocess.run([CLI_PATH, "-q", str(tmp_path / "missing.pbrt")], capture_output=True).returncode == 1


@pytest.mark.parametrize("builder", BUILDERS)
def test_full_size_properties_c3(gpu, oracle, builder):
    """BASELINE config C3's full frame (1M triangles, 2048x2048) at 2 spp: every pixel gets exactly spp
    samples, finite, idempotent; three 16x16 windows of that frame against the oracle."""
    sd = scenes.random_mesh_scene(1_000_000, 2048, 2048)
    with gpu.Scene(sd, builder=builder) as sc:
        film, st = sc.render(max_depth=8, spp=(2, 1), seed=0)
        again, wst = sc.render(max_depth=8, spp=(2, 1), seed=0, counters="walk")
        bi = sc.build_info()
    rays = wst["camera_rays"] + wst["bounce_rays"] + wst["shadow_rays"]
    if builder is None:  # pbrt_hip_scene_create + pbrt_hip_render = the documented pair: the optimised device tree, <= 38.5 64-byte fetches per ray
        assert bi["gpu_built"] and bi["reinsert_passes"] > 0 and wst["nodes_visited"] / rays <= 38.5, (bi, wst["nodes_visited"] / rays)
    else:
        assert not bi["gpu_built"] and wst["nodes_visited"] / rays > 38.5
    assert film.shape == (2048, 2048, 4) and (film[..., 3] == 2).all() and np.isfinite(film).all()
    assert_bit_equal(film, again, "idempotence")
    assert st["samples"] == 2048 * 2048 * 2
    for (x0, y0) in [(0, 0), (1024, 1024), (2032, 2032)]:
        crop = (x0 / 2048, (x0 + 16) / 2048, y0 / 2048, (y0 + 16) / 2048)
        ref, _ = oracle_render(oracle, ("c3-full", x0, y0), lambda: scenes.random_mesh_scene(1_000_000, 2048, 2048, crop=crop), max_depth=8, spp=(2, 1), seed=0)
        assert_bit_equal(film[y0:y0 + 16, x0:x0 + 16], ref, f"window at {x0},{y0}")


def test_full_size_properties_c1(gpu, oracle):
    """BASELINE config C1 at its full size and sample count (analytic sphere + point light, 1024x1024, 8x8 = 64 spp,
    direct lighting): weight == spp, finite, idempotent; three 32x32 windows of the frame against the oracle."""
    sd = scenes.sphere_scene(1024, 1024)
    kw = dict(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(8, 8), seed=0)
    with gpu.Scene(sd) as sc:
        film, st = sc.render(**kw)
        again, _ = sc.render(**kw)
    assert film.shape == (1024, 1024, 4) and (film[..., 3] == 64).all() and np.isfinite(film).all() and (film[..., 1] >= 0).all()
    assert_bit_equal(film, again, "idempotence")
    assert st["samples"] == 1024 * 1024 * 64
    assert film[..., 1].max() > 0  # the lit sphere is in the frame
    for (x0, y0) in [(0, 0), (480, 512), (992, 992)]:
        crop = (x0 / 1024, (x0 + 32) / 1024, y0 / 1024, (y0 + 32) / 1024)
        ref, _ = oracle.OracleScene(scenes.sphere_scene(1024, 1024, crop=crop)).render(**kw)
        assert_bit_equal(film[y0:y0 + 32, x0:x0 + 32], ref, f"C1 window at {x0},{y0}")


@pytest.mark.parametrize("builder", BUILDERS)
def test_full_size_properties_c4(gpu, oracle, builder):
    """BASELINE config C4's full 4096x4096 frame (Cornell-style box, path, maxdepth 16) at 2x2 spp: weight == spp,
    finite, idempotent; three 32x32 windows of the frame against the oracle."""
    sd = scenes.cornell_scene(4096, 4096)
    kw = dict(max_depth=16, spp=(2, 2), seed=0)
    with gpu.Scene(sd, builder=builder) as sc:
        film, st = sc.render(**kw)
        again, _ = sc.render(**kw)
    assert film.shape == (4096, 4096, 4) and (film[..., 3] == 4).all() and np.isfinite(film).all() and (film[..., 1] >= 0).all()
    assert_bit_equal(film, again, "idempotence")
    assert st["samples"] == 4096 * 4096 * 4
    for (x0, y0) in [(0, 0), (2048, 1024), (4064, 4064)]:
        crop = (x0 / 4096, (x0 + 32) / 4096, y0 / 4096, (y0 + 32) / 4096)
        ref, _ = oracle_render(oracle, ("c4-full", x0, y0), lambda: scenes.cornell_scene(4096, 4096, crop=crop), **kw)
        assert_bit_equal(film[y0:y0 + 32, x0:x0 + 32], ref, f"C4 window at {x0},{y0}")


@pytest.mark.parametrize("builder", BUILDERS)
def test_c4_window_at_full_spp(gpu, oracle, builder):
    """BASELINE config C4 (Cornell-style box, 4096x4096, 64x64 = 4096 spp, maxdepth 16): an 8x8 window at the
    full sample count, bit for bit (262k paths of depth up to 16 through the longest RNG streams of any config)."""
    crop = (0.5, 0.5 + 8 / 4096, 0.25, 0.25 + 8 / 4096)
    sd = scenes.cornell_scene(4096, 4096, crop=crop)
    ref, rst = oracle_render(oracle, "c4-window", lambda: sd, max_depth=16, spp=(64, 64), seed=0)
    with gpu.Scene(sd, builder=builder) as sc:
        plain, _ = sc.render(max_depth=16, spp=(64, 64), seed=0)
        film, st = sc.render(max_depth=16, spp=(64, 64), seed=0, counters=True)
    assert film.shape == (8, 8, 4) and (film[..., 3] == 4096).all()
    assert_bit_equal(plain, ref, f"C4 window ({builder} tree, production walk)")
    assert_bit_equal(film, ref, "C4 window")
    for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
        assert st[k] == rst[k]


def test_c4_frame_beyond_the_scratch_cap(gpu, oracle, monkeypatch):
    """C4's film at full size (4096 x 4096) with 32 x 16 = 512 spp: 16 chunks per pixel = 4.3 GB of partial sums, over the 2 GiB cap, so
    the frame renders in two passes (capi_render.cpp partials_passes) -- the default behaviour, no knob.  The same frame with the cap lifted (one
    pass, the round-4 code path) is the same film bit for bit, and an 8 x 8 window of it is the oracle's."""
    sd = scenes.cornell_scene(4096, 4096)
    kw = dict(max_depth=16, spp=(32, 16), seed=0)
    with gpu.Scene(sd) as sc:
        two, st = sc.render(**kw)
        monkeypatch.setenv("PBRT_HIP_PARTIALS_CAP_KB", str(8 << 20))
        one, _ = sc.render(**kw)
        monkeypatch.delenv("PBRT_HIP_PARTIALS_CAP_KB")
    assert st["samples"] == 4096 * 4096 * 512
    assert_bit_equal(two, one, "C4 frame: two passes vs one")
    del one
    x0, y0 = 2048, 1024
    crop = (x0 / 4096, (x0 + 8) / 4096, y0 / 4096, (y0 + 8) / 4096)
    ref, _ = oracle_render(oracle, "c4-window-512", lambda: scenes.cornell_scene(4096, 4096, crop=crop), **kw)
    assert_bit_equal(two[y0:y0 + 8, x0:x0 + 8], ref, "C4 frame in passes, window vs oracle")


# ---- closed forms on the HIP path itself: anchors of the path loop that do not route through the oracle ----

def _hip_rgb(gpu, sd, max_depth, spp, seed):
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(max_depth=max_depth, spp=spp, seed=seed)
    return pbrt_amd.film_to_rgb(film)


@pytest.mark.parametrize("rho", [0.5, 0.8])
@pytest.mark.parametrize("max_depth", [1, 3, 8, 40])
def test_furnace_with_reflecting_walls_sums_the_bounce_series_on_the_gpu(gpu, rho, max_depth):
    """The kernel against Le x sum_{i <= maxdepth} rho^i inside a closed emitting, reflecting icosphere (tests/util.py furnace_scene;
    the same check runs on the oracle in tests/test_oracle_selfcheck.py): multi-bounce throughput, Russian-roulette reweighting and
    the maxdepth accounting of render_kernel pinned WITHOUT the oracle.  8 seeds x 48 x 48 x 256 spp."""
    from util import check_furnace
    mean, se, want = check_furnace(lambda sd, d, spp, seed: _hip_rgb(gpu, sd, d, spp, seed), rho, max_depth, seeds=range(40, 48), spp=(16, 16), res=48)
    assert abs(mean - want) < 3.5 * se + 3e-4 * want, (rho, max_depth, mean, se, want)
    assert se < 0.002 * want


@pytest.mark.parametrize("rho,max_depth", [(0.5, 8), (0.8, 3)])
def test_furnace_in_a_box_on_the_gpu(gpu, rho, max_depth):
    """The cube (heavy-tailed light estimate along its edges: tests/util.py furnace_scene): 8 seeds x 64 x 64 x 1024 spp, from above
    with the standard error, from below with a 1 % allowance."""
    from util import check_furnace
    mean, se, want = check_furnace(lambda sd, d, spp, seed: _hip_rgb(gpu, sd, d, spp, seed), rho, max_depth, seeds=range(40, 48), spp=(32, 32), res=64, shape="box")
    assert want * 0.99 - 3.5 * se < mean < want + 3.5 * se, (rho, max_depth, mean, se, want)


@pytest.mark.parametrize("max_depth", [0, 1, 2, 3])
def test_mirror_furnace_is_exact_up_to_three_bounces_on_the_gpu(gpu, max_depth):
    """The kernel's specular chain against Le x sum_{i <= maxdepth} Kr^i in a closed box of emitting mirrors: exact in every pixel."""
    from util import mirror_furnace_scene
    kr, le = 0.75, 2.0
    rgb = _hip_rgb(gpu, mirror_furnace_scene(kr, le, res=48), max_depth, (2, 2), 3)
    want = le * sum(kr ** i for i in range(max_depth + 1))
    # (Moeller-Trumbore is not watertight: one reflected ray in a thousand slips through an edge of the box and brings nothing back --
    # the same ray on both sides; such a pixel is low by a quarter of a term, none may be high)
    exact = np.isclose(rgb, want, rtol=3e-6, atol=0).all(-1)
    assert exact.mean() >= 0.99 and (rgb <= want * (1 + 3e-6)).all(), (max_depth, exact.mean(), rgb.min(), rgb.max(), want)


def test_checkerboard_on_a_sphere(gpu, oracle):
    """Textured spheres ((u, v) from the sphere's own parametrisation, atan / acos as polynomials on both sides): the closed
    form on the HIP path (a uniform sky: every one-cell pixel is its cell's colour, the cell found by numpy in float64), and films equal to
    the oracle's bit for bit where the texture meets everything else -- C0's scene with its sphere matte and checkered beside the checkered
    ground, path depth 5, integrator 2, the table samplers, a wide box filter, three ranks."""
    from pbrt_amd import INTEGRATOR_PATH_MIS, loader
    from util import check_checker_sphere, checker_sphere_scene
    sd = checker_sphere_scene(200, 120)
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(max_depth=1, spp=(4, 4), seed=3)
    check_checker_sphere(pbrt_amd.film_to_rgb(film))
    assert_bit_equal(film, oracle.OracleScene(sd).render(max_depth=1, spp=(4, 4), seed=3)[0], "checkered sphere under the sky")
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "c0_check_sphere.pbrt")).read()
    text = text.replace("[400]", "[80]").replace('"integer pixelsamples" 128', '"integer pixelsamples" 8')
    assert 'Material "mirror"' in text
    text = text.replace('Material "mirror"', 'Texture "dots" "spectrum" "checkerboard" "float uscale" [10] "float vscale" [5] "rgb tex1" [.7 .2 .2] "rgb tex2" [.9 .9 .8]\n  Material "matte" "texture Kd" "dots"', 1)
    ls = loader.load_string(text)
    assert ls.scene.mat_tex[int(ls.scene.spheres[0, 4])] != 0 and not any("mean colour" in w for w in ls.warnings)
    o = oracle.OracleScene(ls.scene)
    kw = ls.render_kwargs()
    with gpu.Scene(ls.scene) as sc:
        for extra in (dict(), dict(integrator=INTEGRATOR_PATH_MIS), dict(sampler="sobol_nd"), dict(filter_width=(1.25, 1.5)), dict(sampler="stratified", integrator=INTEGRATOR_PATH_MIS, filter_width=(0.75, 2.0))):
            k2 = dict(kw, seed=4, **extra)
            assert_bit_equal(sc.render(**k2)[0], o.render(**k2)[0], f"C0 with a checkered sphere, {extra}")
        parts = sum(sc.render(rank=r, world_size=3, seed=4, **kw)[0] for r in range(3))
    assert_bit_equal(parts, o.render(seed=4, **kw)[0], "three ranks")


@pytest.mark.parametrize("builder", [None, "host"])
@pytest.mark.parametrize("name", ["mesh1k", "cornell", "mesh20k"])
def test_closest_hits_equal_a_float64_brute_force_on_the_gpu(gpu, name, builder):
    """pbrt_hip_intersect (the production walk over the quantised 4-wide tree, either builder) against every ray x every triangle in
    float64 numpy (util.brute_force_hits_f64; no oracle, no BVH): the same triangle and the same distance for every ray whose answer
    cannot depend on rounding."""
    from util import check_hits_against_brute_force
    sd = SMALL_SCENES[name]()
    o, d, tmax = random_rays(1500 if name == "mesh20k" else 3000, 11, inside=1.5)
    with gpu.Scene(sd, builder=builder) as sc:
        t, prim = sc.intersect(o, d, tmax)[:2]
    check_hits_against_brute_force(sd, o, d, tmax, t, prim)


@pytest.mark.parametrize("rung", range(4))
def test_sphere_hits_against_float64(gpu, oracle, rung):
    """tests/test_oracle_selfcheck.py's test of the same name through pbrt_hip_intersect (the production walk): the ladder of distance /
    radius, every robust ray's sphere and t against float64 under the error model of util.sphere_hits_f64 -- and every ray, robust or
    not, equal to the oracle bit for bit.  (The sphere test without a walk around it: tests/test_blocks_gpu.py, op SPHERE_HIT.)"""
    from util import SPHERE_LADDER, check_sphere_hits, sphere_ladder_rays, sphere_ladder_scene
    dist, radius = SPHERE_LADDER[rung]
    sd = sphere_ladder_scene(radius)
    o, d, tmax, kind = sphere_ladder_rays(dist, radius)
    with gpu.Scene(sd) as sc:
        t, prim = sc.intersect(o, d, tmax)[:2]
    rt, rp = oracle.OracleScene(sd).intersect(o, d, tmax)[:2]
    assert_bit_equal(prim, rp, "prim"); assert_bit_equal(t, rt, "t")
    print(dist, radius, check_sphere_hits(sd.spheres, o, d, tmax, kind, t, prim))


@pytest.mark.parametrize("max_depth", [2, 5])
def test_path_integrator_agrees_with_an_independent_estimator_on_the_gpu(gpu, max_depth):
    """The HIP path against tests/independent_mc.py (float64 numpy, own random numbers, no light sampling: the emitter is collected only
    by running into it; no oracle involved): the closed box with a mirror wall at 1024 samples per pixel, integrators 0 and 2, the
    stratified and the Halton sampler: every 8 x 8 block within 5 standard errors (+ 0.4 %) of the independent estimate, the image's
    sum within 0.6 %; one bounce fewer is seen (8-11 standard errors, 3-4 % of the sum)."""
    import independent_mc as im
    from pbrt_amd import INTEGRATOR_PATH_MIS
    mean, se = im.block_means(64, 64, 8, max_depth, 4_000_000)
    sd = im.furnished_box_scene(64, 64)
    with gpu.Scene(sd) as sc:
        for kw in (dict(), dict(integrator=INTEGRATOR_PATH_MIS), dict(sampler="halton"), dict(sampler="sobol_nd", integrator=INTEGRATOR_PATH_MIS)):
            film, _ = sc.render(max_depth=max_depth, spp=(32, 32), seed=2, **kw)
            z, rel = im.compare_with_blocks(pbrt_amd.film_to_rgb(film), mean, se, 8)
            assert z < 5.0 and abs(rel) < 6e-3, (kw, z, rel)
        film, _ = sc.render(max_depth=max_depth - 1, spp=(32, 32), seed=2)
        z, rel = im.compare_with_blocks(pbrt_amd.film_to_rgb(film), mean, se, 8)
        assert z > 6 and rel < -0.02, (z, rel)


def test_c1_at_full_size_equals_the_analytic_image_on_the_gpu(gpu):
    """BASELINE config C1 as written (1024 x 1024, 64 spp, direct lighting) against the image computed from first principles in float64
    numpy (util.c1_analytic_image; no oracle): camera model, sphere root, I / r^2, Kd / pi and the terminator, over 140 000 smooth pixels."""
    from util import check_c1_against_analytic
    rgb = _hip_rgb_direct(gpu, scenes.sphere_scene(1024, 1024))
    check_c1_against_analytic(rgb)
    rgb = _hip_rgb_direct(gpu, scenes.sphere_scene(640, 360))  # a wide frame: the fov spans the shorter axis
    check_c1_against_analytic(rgb)


def _hip_rgb_direct(gpu, sd):
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(8, 8), seed=0)
    return pbrt_amd.film_to_rgb(film)


@pytest.mark.parametrize("kind", ["distant", "infinite"])
@pytest.mark.parametrize("max_depth", [1, 5])
def test_lit_plane_closed_forms_on_the_gpu(gpu, kind, max_depth):
    from util import lit_plane_scene
    sd, want = lit_plane_scene(kind, res=64)
    rgb = _hip_rgb(gpu, sd, max_depth, (4, 4), 9)
    assert np.allclose(rgb, want, rtol=3e-6, atol=1e-7), (rgb.min((0, 1)), rgb.max((0, 1)), want)


# ---- accelerator built on the device: a different tree, the same answers ----

@pytest.mark.parametrize("builder", ["gpu", "gpu-plain"])
@pytest.mark.parametrize("name", ["mesh1k", "mesh20k", "cornell", "ties", "deep", "check_sphere", "spheres2k"])
def test_gpu_built_scene_matches_oracle(gpu, oracle, name, builder):
    """PBRT_HIP_SCENE_GPU_BUILD: binned SAH on the device, the tree optimised by parallel re-insertion ("gpu", the default) or
    left as built ("gpu-plain", PBRT_HIP_SCENE_PLAIN_TREE).  Hit records and film must equal the oracle's bit for
    bit (a hit does not depend on the tree), the canonical counters too, and the quantised tree must pass the
    same structural checks as the host-built one (every decoded child box encloses what is below it, every triangle reachable
    exactly once, stack bound honest) -- a move that lost or duplicated a subtree would fail them."""
    from test_host import _check_quads
    import sys
    sys.setrecursionlimit(100000)
    sd = SMALL_SCENES[name]()
    o, d, tmax = random_rays(100_000, 5)
    ref = oracle.OracleScene(sd)
    rt, rp, rb1, rb2, _ = ref.intersect(o, d, tmax)
    film_ref, rst = ref.render(max_depth=6, spp=(2, 2), seed=11)
    rcnt = ref.intersect(o, d, tmax)[4]
    with gpu.Scene(sd, builder=builder) as sc:
        bi = sc.build_info()
        assert bi["gpu_built"] and bi["build_ms"] > 0 and not bi["canonical_tree_ready"]
        if builder == "gpu-plain":
            assert bi["reinsert_passes"] == 0 and bi["reinsert_moves"] == 0
        elif len(sd.idx) >= 8:
            assert bi["reinsert_passes"] >= 1 and 0 < bi["reinsert_ms"] < bi["build_ms"]
        t, prim, b1, b2, _ = sc.intersect(o, d, tmax)
        occ = sc.occluded(o, d, tmax)
        film, st = sc.render(max_depth=6, spp=(2, 2), seed=11)
        quads, order = sc.export_quads()
        need = sc.info()["quad_stack_need"]
        # the counter flags count the CANONICAL walk: the oracle's tree is built on the host at first use
        film_c, stc = sc.render(max_depth=6, spp=(2, 2), seed=11, counters=True)
        cnt = sc.intersect(o, d, tmax, counters=True)[4]
        assert sc.build_info()["canonical_tree_ready"]
        film_after, _ = sc.render(max_depth=6, spp=(2, 2), seed=11)  # the production arrays are untouched by it
    assert_bit_equal(film_c, film_ref, "film of the counting pass")
    assert_bit_equal(film_after, film_ref, "film after the canonical tree was added")
    for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
        assert stc[k] == rst[k], f"{k}: {stc[k]} vs oracle {rst[k]}"
    assert tuple(cnt) == tuple(rcnt), f"ray-batch counters {cnt} vs oracle {rcnt}"
    assert_bit_equal(prim, rp, "prim")
    assert_bit_equal(t, rt, "t")
    assert_bit_equal(b1, rb1, "b1")
    assert_bit_equal(b2, rb2, "b2")
    assert np.array_equal(occ != 0, ref.occluded(o, d, tmax) != 0)
    assert_bit_equal(film, film_ref, "film of the device-built scene")
    from util import with_sphere_proxies
    Pp, Ip = with_sphere_proxies(sd)  # (a sphere is primitive n_tris + s, bounded through its proxy triangle: round 6)
    assert sorted(order.tolist()) == list(range(len(Ip)))
    _check_quads(quads, need, Pp, Ip, order)


def test_device_reinsertion_cuts_the_walks_work(gpu, oracle):
    """The device builder's re-insertion passes (the default) against its tree as built, on BASELINE C2's scene: the same film bit
    for bit, at least 3 % fewer node fetches per ray by the production walk's own counters (measured: 30.8 -> 28.8, and 40.2 -> 38.4
    on C3's million triangles) and no more triangle tests; the build stays far below a second and the optimised tree is
    deterministic (two builds: the same leaf order, and the same quad nodes up to the order the collapse's atomics numbered them in)."""
    sd = scenes.random_mesh_scene(100_000, 1024, 1024, crop=(0.30, 0.55, 0.35, 0.60))
    out = {}
    for builder in ("gpu-plain", "gpu"):
        with gpu.Scene(sd, builder=builder) as sc:
            film, _ = sc.render(max_depth=8, spp=(2, 2), seed=0)
            _, wk = sc.render(max_depth=8, spp=(2, 2), seed=0, counters="walk")
            out[builder] = (film, wk, sc.build_info(), sc.export_quads())
    assert_bit_equal(out["gpu"][0], out["gpu-plain"][0], "optimised vs plain device tree")
    a, b = out["gpu-plain"][1], out["gpu"][1]
    assert b["nodes_visited"] < 0.97 * a["nodes_visited"], (a["nodes_visited"], b["nodes_visited"])
    assert b["tris_tested"] <= 1.01 * a["tris_tested"], (a["tris_tested"], b["tris_tested"])
    bi = out["gpu"][2]
    assert bi["reinsert_passes"] >= 2 and bi["reinsert_moves"] > 1000 and bi["build_ms"] < 1000.0, bi
    with gpu.Scene(sd, builder="gpu") as sc:
        quads, order = sc.export_quads()
    assert np.array_equal(order, out["gpu"][3][1]), "leaf order differs between two device builds"
    from util import sorted_quad_rows as rows  # a node's origin, cells and child planes (words 0-11), sorted
    assert quads.shape == out["gpu"][3][0].shape and np.array_equal(rows(quads), rows(out["gpu"][3][0])), "quad nodes differ between two device builds"
    # the objective the passes lower, and its guard: the summed area of the interior nodes fell, by more than a tenth
    assert 0 < bi["reinsert_area_after"] < 0.9 * bi["reinsert_area_before"], bi


def test_device_refit_of_what_moved_equals_the_full_refit(gpu, monkeypatch):
    """after a pass the device refits only the chains above the nodes that moved (a pass moves about one node in
    seventy; ri_mark_kernel / ri_refit_dirty_kernel).  The tree that comes out must be the one a refit of EVERY box after every pass
    makes (PBRT_HIP_REINSERT_FULL_REFIT: the round-4 kernel, kept for this comparison), word for word -- the searches of the next
    pass read those boxes, so a single stale box would change moves -- on 100k triangles and on the degenerate `ties` scene."""
    from util import sorted_quad_rows as rows
    for make in (lambda: scenes.random_mesh_scene(100_000, 64, 64), SMALL_SCENES["ties"], SMALL_SCENES["mesh20k"]):
        sd = make()
        got = {}
        for full in (False, True):
            if full:
                monkeypatch.setenv("PBRT_HIP_REINSERT_FULL_REFIT", "1")
            else:
                monkeypatch.delenv("PBRT_HIP_REINSERT_FULL_REFIT", raising=False)
            with gpu.Scene(sd, builder="gpu") as sc:
                got[full] = (sc.export_quads(), sc.build_info())
        monkeypatch.delenv("PBRT_HIP_REINSERT_FULL_REFIT", raising=False)
        (qa, oa), ia = got[False]
        (qb, ob), ib = got[True]
        assert np.array_equal(oa, ob) and qa.shape == qb.shape and np.array_equal(rows(qa), rows(qb)), "sparse refit changed the tree"
        assert (ia["reinsert_passes"], ia["reinsert_moves"], ia["reinsert_area_after"]) == (ib["reinsert_passes"], ib["reinsert_moves"], ib["reinsert_area_after"])
        assert ia["reinsert_moves"] > 0


@functools.lru_cache(maxsize=None)
def _recorded_device_trees():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_trees.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("builder", ["gpu", "gpu-plain"])
@pytest.mark.parametrize("name", ["mesh1k", "mesh20k", "cornell", "ties", "deep", "check_sphere", "spheres2k"])
def test_device_built_trees_are_the_recorded_ones(gpu, name, builder):
    """The device builder makes THE tree that tests/golden/device_trees.json records (make_golden_device_trees.py), not just a valid
    one: quad count, stack need, re-insertion passes, moves and summed areas, the leaf order and the quad nodes' words 0-11 (rows
    sorted) are equal.  The scenes reach every branch of the builder's host code: the greedy collapse (mesh1k, cornell: fewer than
    1024 triangles) and the dynamic programme, several re-insertion passes (mesh20k), degenerate boxes (ties), many levels (deep),
    proxy triangles (spheres2k, check_sphere); "gpu-plain" skips the re-insertion."""
    from util import device_tree_record
    want = _recorded_device_trees()[f"{name}/{builder}"]
    with gpu.Scene(SMALL_SCENES[name](), builder=builder) as sc:
        got = device_tree_record(sc)
    assert got == want, {k: (got[k], want[k]) for k in want if got.get(k) != want[k]}


def test_device_build_of_coincident_boxes_is_bounded(gpu, oracle):
    """30 000 copies of one triangle among 3 000 random ones: no search of the re-insertion pass can prune among equal boxes, so
    its visit cap and budget are what bound the build (round 3's host pass was quadratic here); the hits stay the oracle's."""
    rng = np.random.default_rng(5)
    tri = np.array([[0.1, 0.1, 0.0], [0.5, 0.1, 0.1], [0.1, 0.5, 0.2]], np.float32)
    c = rng.uniform(-1, 1, (3000, 1, 3))
    P = np.concatenate([np.tile(tri, (30000, 1)), (c + rng.uniform(-0.1, 0.1, (3000, 3, 3))).reshape(-1, 3)]).astype(np.float32)
    sd = SMALL_SCENES["mesh1k"]()
    import dataclasses
    sd = dataclasses.replace(sd, P=P, idx=np.arange(len(P), dtype=np.uint32).reshape(-1, 3), mat_id=np.zeros(len(P) // 3, np.uint16)).normalized()
    o, d, tmax = random_rays(3000, 9)
    rt, rp, rb1, rb2, _ = oracle.OracleScene(sd).intersect(o, d, tmax)
    import time
    t0 = time.time()
    with gpu.Scene(sd, builder="gpu") as sc:
        wall = time.time() - t0
        bi = sc.build_info()
        t, prim, b1, b2, _ = sc.intersect(o, d, tmax)
    assert wall < 20.0 and bi["build_ms"] < 5000.0, (wall, bi)
    assert_bit_equal(prim, rp, "prim")
    assert_bit_equal(t, rt, "t")


def test_gpu_built_scene_equals_host_built_scene_c2(gpu):
    """BASELINE config C2's scene (100k triangles), both builders, same crop window at 64 spp: identical films."""
    sd = scenes.random_mesh_scene(100_000, 1024, 1024, crop=(0.40, 0.46, 0.50, 0.56))
    with gpu.Scene(sd, builder="host") as a, gpu.Scene(sd, builder="gpu") as b:
        fa, _ = a.render(max_depth=8, spp=(8, 8), seed=0)
        fb, _ = b.render(max_depth=8, spp=(8, 8), seed=0)
        assert b.build_info()["gpu_built"] and not a.build_info()["gpu_built"]
    assert_bit_equal(fa, fb, "host-built vs device-built")


# ---- randomised scenes: everything the path takes as input, drawn at random ----

from util import random_scene as _random_scene  # noqa: E402  (the soak's scene generator: also the CPU soaks' and the twin's, tests/util.py)


def test_optimized_tree_scene_matches_oracle(gpu, oracle):
    """PBRT_HIP_SCENE_OPTIMIZED_TREE (host build + re-insertion): the same film, hit records and occlusion bit for bit (the tie
    rule makes a hit independent of the tree), fewer node fetches than the default host tree, and the counter flags still count
    the oracle's canonical walk."""
    sd = SMALL_SCENES["mesh20k"]()
    ref, rst = oracle.OracleScene(sd).render(max_depth=5, spp=(2, 2), seed=3)
    o, d, tmax = random_rays(20000, 5, inside=2.5)
    rhit = oracle.OracleScene(sd).intersect(o, d, tmax)
    walk = {}
    for builder in ("host", "host-optimized"):
        with gpu.Scene(sd, builder=builder) as sc:
            film, st = sc.render(max_depth=5, spp=(2, 2), seed=3, counters=True)
            _, wk = sc.render(max_depth=5, spp=(2, 2), seed=3, counters="walk")
            hit = sc.intersect(o, d, tmax)
            occ = sc.occluded(o, d, tmax)
        assert_bit_equal(film, ref, f"{builder}: film")
        for a, b, what in zip(hit[:4], rhit[:4], ("t", "prim", "b1", "b2")):
            assert_bit_equal(a, b, f"{builder}: {what}")
        assert np.array_equal(occ != 0, oracle.OracleScene(sd).occluded(o, d, tmax) != 0)
        for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
            assert st[k] == rst[k], f"{builder} {k}: {st[k]} vs oracle {rst[k]}"
        walk[builder] = wk["nodes_visited"]
    assert walk["host-optimized"] < walk["host"], walk


_SOAK_FIRST = int(os.environ.get("PBRT_SOAK_FIRST", "0"))  # (tools/soak.sh N FIRST: seeds FIRST ... FIRST + N - 1, scenes no earlier soak drew)


@pytest.mark.parametrize("seed", range(_SOAK_FIRST, _SOAK_FIRST + int(os.environ.get("PBRT_SOAK_SEEDS", "48"))))
def test_random_scenes_match_oracle(gpu, oracle, monkeypatch, seed):
    """Triangle counts 0..300 (with duplicates and degenerate triangles), random materials (mirrors, emitters),
    0-3 lights of every kind, 0-2 spheres, random camera / resolution / crop / strata / depth / integrator /
    seed / rank split; odd seeds use the Sobol sampler, every fourth a tiny grid of persistent waves, every third
    builds the tree on the device.  Then the film paths of round 3 (random wide box filter, luminance clamp) and samplers 2 / 3, and
    round 5's variants: random checkerboard textures and integrator 2 (MIS) on the same scene."""
    sd, rng = _random_scene(seed)
    integ = INTEGRATOR_DIRECT if seed % 5 == 4 else INTEGRATOR_PATH
    depth, spp, rseed = int(rng.integers(0, 12)), (int(rng.integers(1, 7)), int(rng.integers(1, 6))), int(rng.integers(0, 1 << 20))
    world = int(rng.integers(1, 4))
    sampler = "sobol" if seed % 2 else "stratified"
    ref, rst = oracle.OracleScene(sd).render(integrator=integ, max_depth=depth, spp=spp, seed=rseed, sampler=sampler)
    if seed % 4 == 3:
        monkeypatch.setenv("PBRT_HIP_RENDER_WORKGROUPS", "3")
    with gpu.Scene(sd, builder="gpu" if seed % 3 == 2 else "host") as sc:
        acc = None
        for r in range(world):
            part, _ = sc.render(integrator=integ, max_depth=depth, spp=spp, seed=rseed, rank=r, world_size=world, sampler=sampler)
            acc = part if acc is None else acc + part
        _, st = sc.render(integrator=integ, max_depth=depth, spp=spp, seed=rseed, counters=True, sampler=sampler)
        o, d, tmax = random_rays(3000, seed, inside=2.5)
        hit = sc.intersect(o, d, tmax)
        occ = sc.occluded(o, d, tmax)
    rhit = oracle.OracleScene(sd).intersect(o, d, tmax)
    for a, b, what in zip(hit[:4], rhit[:4], ("t", "prim", "b1", "b2")):
        assert_bit_equal(a, b, f"random scene {seed}: {what}")
    assert np.array_equal(occ != 0, oracle.OracleScene(sd).occluded(o, d, tmax) != 0)
    assert_bit_equal(acc, ref, f"random scene {seed} ({len(sd.idx)} tris, {len(sd.spheres)} spheres, {len(sd.lights)} lights, {world} ranks)")
    if st is not None:
        for k in ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested"):
            assert st[k] == rst[k], f"{k}: {st[k]} vs oracle {rst[k]}"
    # round 3's film paths on the same random scene: a random box filter radius (fixed-point film; ranks add as integers),
    # a luminance clamp, and the Sobol' sampler with its own dimensions
    fw = (float(rng.uniform(0.3, 2.6)), float(rng.uniform(0.3, 2.6)))
    ml = float(rng.uniform(0.2, 3.0)) if seed % 2 else 0.0
    kw = dict(integrator=integ, max_depth=depth, spp=spp, seed=rseed, sampler=sampler, max_sample_luminance=ml)
    o = oracle.OracleScene(sd)
    with gpu.Scene(sd, builder="gpu" if seed % 3 == 1 else "host") as sc:
        parts = sum(sc.render_acc(fw, rank=r, world_size=world, **kw)[0] for r in range(world))
        nd, _ = sc.render(**dict(kw, sampler="sobol_nd"))
        hal, _ = sc.render(**dict(kw, sampler="halton"))
    assert np.array_equal(parts, o.render_acc(fw, **kw)[0]), f"random scene {seed}: accumulators, box filter {fw}, {world} ranks, clamp {ml}"
    assert_bit_equal(nd, o.render(**dict(kw, sampler="sobol_nd"))[0], f"random scene {seed}: sampler 2")
    assert_bit_equal(hal, o.render(**dict(kw, sampler="halton"))[0], f"random scene {seed}: sampler 3")
    # round 5's variants on the same random scene: random checkerboards as the Kd of some matte materials over random corner (u, v),
    # integrator 2 (MIS) on even seeds, any of the four samplers, the device-built tree on every other seed
    import dataclasses
    from pbrt_amd import INTEGRATOR_PATH_MIS
    n_tex = int(rng.integers(1, 4))
    tex = np.concatenate([np.zeros((n_tex, 1)), rng.uniform(0.05, 0.95, (n_tex, 6)), rng.uniform(-9, 9, (n_tex, 2)), rng.uniform(-2, 2, (n_tex, 2))], 1)
    mat_tex = np.where((sd.materials[:, 0] == 0) & (rng.random(len(sd.materials)) < 0.7), rng.integers(1, n_tex + 1, len(sd.materials)), 0).astype(np.uint32)
    tsd = dataclasses.replace(sd, textures=tex.astype(np.float32), mat_tex=mat_tex, tri_uv=rng.uniform(-1.5, 2.5, (len(sd.idx), 6)).astype(np.float32)).normalized()
    vkw = dict(integrator=INTEGRATOR_PATH_MIS if seed % 2 == 0 else INTEGRATOR_PATH, max_depth=depth, spp=spp, seed=rseed,
               sampler=("stratified", "sobol", "sobol_nd", "halton")[seed % 4])
    with gpu.Scene(tsd, builder="gpu" if seed % 2 else "host") as sc:
        var = sum(sc.render(rank=r, world_size=world, **vkw)[0] for r in range(world))
        wvar = sc.render(filter_width=fw, **vkw)[0] if seed % 3 == 0 else None  # ... and all of it under the random wide box filter
    assert_bit_equal(var, oracle.OracleScene(tsd).render(**vkw)[0], f"random scene {seed}: textures {mat_tex.tolist()}, {vkw}")
    if wvar is not None:
        assert_bit_equal(wvar, oracle.OracleScene(tsd).render(filter_width=fw, **vkw)[0], f"random scene {seed}: the variants under box filter {fw}")


@pytest.mark.timeout(900)
def test_bench_withholds_a_stale_profile(gpu, tmp_path):
    """a committed profile prices only the KERNEL it was taken on -- identified by a hash of its
    machine code (pbrt_amd/isa_id.py).  bench.py run against a copy of profiles/pmc_c2.json whose kernel id is not that of the
    loaded library's kernel must say so and withhold the figures that rest on it; with the right id it must not complain,
    whatever the library's source hash is (an edit elsewhere in csrc/ does not invalidate it)."""
    import json
    import subprocess
    import sys
    from pbrt_amd import isa_id
    from pbrt_amd._lib import LIB_PATH
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kernel = "void pbrt_hip::(anonymous namespace)::render_kernel<false, false, false, 30, 3, false, false>(pbrt_hip::DevScene, pbrt_hip::RenderParams)"
    good = isa_id.kernel_id(LIB_PATH, kernel)
    assert good, "the library has no such kernel"
    pmc = {"kernel": kernel, "kernel_isa_id": "0123456789abcdef", "build_id": "some-other-source-hash", "valu_issue_quadcycles_per_ray": 100.0,
           "valu_issue_busy_measured": 0.5, "traffic_bytes_raw": 1.0, "avg_ms": 1.0, "lane_utilisation": 0.5, "l2_hit_rate": 0.7}
    (tmp_path / "pmc_c2.json").write_text(json.dumps(pmc))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0", "--workload", "c2", "--spp", "1", "1", "--full", "--no-cpu-baseline",
           "--profiles", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert "0123456789abcdef" in line["roofline"]["stale_profile"] and good in line["roofline"]["stale_profile"]
    assert line["roofline"]["frac"] is None and line["roofline"]["traffic"] is None and "valu" not in line["roofline"]
    assert line["config"]["library_build_id"] == pbrt_amd.build_id()
    pmc["kernel_isa_id"] = good
    (tmp_path / "pmc_c2.json").write_text(json.dumps(pmc))
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    roof = line["roofline"]
    assert "stale_profile" not in roof and roof["profile_kernel"]["isa_id"] == good
    # ... and the line is recomputable from (profile, rays_per_launch, kernel_ms) by the formulas of bench.py's docstring
    rays_per_s = roof["rays_per_launch"] / (roof["kernel_ms"] * 1e-3)
    # (round 6: frac is the USEFUL share -- busy x lane utilisation --, frac_busy how often the issue port was occupied)
    assert abs(roof["achieved_busy"] - 100.0 * rays_per_s / 1e9) < 1e-6 * roof["achieved_busy"] and abs(roof["achieved"] - 0.5 * roof["achieved_busy"]) < 1e-9 * roof["achieved"]
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12 and abs(roof["frac_busy"] - roof["achieved_busy"] / roof["peak"]) < 1e-12
    assert roof["frac_useful"] == roof["frac"] and abs(roof["frac"] - roof["frac_busy"] * 0.5) < 1e-12
    assert roof["traffic"] is None  # (--spp overrides the workload's sample count and this profile does not say which one it was taken at)
    recs = (roof["hbm"]["kernel_fetches_per_ray"] + roof["hbm"]["kernel_tris_per_ray"]) * rays_per_s / 1e9
    assert abs(roof["l2_miss"]["requests_per_s_G"] - recs * 0.3) < 1e-6 * recs and roof["l2_miss"]["peak_G"] == 58.08
    assert roof["hbm"]["cache_resident"] is True and roof["hbm"]["hot_working_set_bytes"] < 20e6  # C2: 9 MB of quad nodes + triangle records
    # ... the per-ray counters belong to ONE tree (a builder edit leaves the render kernel's ISA alone): a profile that records
    # its tree's work per ray is withheld when the live walk does other work, and used when it does the same; the memory-side traffic is
    # FETCH_SIZE x the profile's measured calibration factor + WRITE_SIZE
    fetches, tris = roof["hbm"]["kernel_fetches_per_ray"], roof["hbm"]["kernel_tris_per_ray"]
    pmc.update({"tree": {"kernel_fetches_per_ray": fetches * 1.02, "kernel_tris_per_ray": tris, "spp": 1}, "FETCH_SIZE_KB_per_launch": 3.0,
                "WRITE_SIZE_KB_per_launch": 1.0, "traffic_bytes_raw": 4096.0, "fetch_size_calibration": {"factor": 2.0, "source": "test"}})
    (tmp_path / "pmc_c2.json").write_text(json.dumps(pmc))
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    roof = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["roofline"]
    assert "tree" in roof["stale_profile"] and roof["frac"] is None and roof["traffic"] is None and "valu" not in roof and "profile_kernel" not in roof
    pmc["tree"]["kernel_fetches_per_ray"] = fetches
    (tmp_path / "pmc_c2.json").write_text(json.dumps(pmc))
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    roof = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["roofline"]
    assert "stale_profile" not in roof and roof["frac"] > 0 and roof["traffic"] == (3.0 * 2.0 + 1.0) * 1024 and roof["traffic_bytes_raw"] == 4096.0


@pytest.mark.timeout(600)
def test_plain_bench_run_times_its_steps_and_dumps_the_last_film(gpu, tmp_path):
    """bench.py without --full: the headline alone (none of --full's passes, checks or baseline), --steps timed steps whose
    ms_per_step is what `value` rests on, and --dump-outputs writes the film the last timed step computed -- the film the same
    scene and arguments render in this process."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--workload", "c2", "--spp", "1", "1",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["metric"].startswith("Msamples/sec")
    assert line["steps"] == 3 and line["value"] > 0 and abs(line["ms_per_step"] - 1024 * 1024 / line["value"] / 1e3) < 1e-9 * line["ms_per_step"]
    assert "cpu_baseline" not in line and "film_check" not in line
    assert line["roofline"]["frac"] is None and line["roofline"]["clock"] is None and "hbm" not in line["roofline"]
    assert line["dumped_outputs"] == {"film.npy": [1024, 1024, 4]} and sorted(os.listdir(out_dir)) == ["film.npy"]
    film = np.load(out_dir / "film.npy")
    assert film.dtype == np.float32 and (film[..., 3] == 1).all()
    with pbrt_amd.Scene(scenes.random_mesh_scene(100_000, 1024, 1024), device=0, builder="gpu") as sc:
        want, _ = sc.render(integrator=INTEGRATOR_PATH, max_depth=8, spp=(1, 1), seed=0, sampler="stratified")
    assert_bit_equal(film, want, "bench.py --dump-outputs against the same render in this process")


@pytest.mark.timeout(900)
def test_bench_under_torchrun_uses_rccl(gpu):
    """bench.py as the driver launches it for N > 1 -- torch.distributed.run, one rank per GPU, RCCL ("nccl") process
    group with device_id, barrier, all_reduce of the times, gather of the slabs -- on min(2, device_count) ranks.  On a
    single-GPU box the one-rank group still runs every one of those calls, so the first multi-GPU run of the driver is
    not the first time they execute."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = min(2, gpu.device_count())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.pop("PBRT_DIST_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", "29533",
           os.path.join(root, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "1", "--workload", "c2", "--spp", "2", "2", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root, env=env, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == n and out["value"] > 0 and out["film_check"]["weight_ok"] and out["film_check"]["finite"]
    assert out["roofline"]["bound"] == "valu" and out["roofline"]["hbm"]["achieved_gbps"] > 0
    assert len(out["per_rank_kernel_ms"]["mean_per_rank"]) == n and "exchange_ms" in out  # (every rank's kernel time: RCCL all_gather)
    if gpu.device_count() >= 2:  # and all GPUs from ONE process through the library's own ncclGather
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--single-process", "--steps", "1", "--warmup", "1",
                            "--workload", "c2", "--spp", "2", "2", "--full", "--no-cpu-baseline"], capture_output=True, text=True, cwd=root, timeout=800)
        assert r.returncode == 0, r.stderr[-3000:]
        out2 = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out2["film_check"]["weight_ok"] and abs(out2["film_check"]["mean_Y"] - out["film_check"]["mean_Y"]) < 1e-12


@pytest.mark.timeout(300)
def test_multi_gpu_launch_failure_leaves_nobody_waiting(gpu, oracle, monkeypatch):
    """VERDICT r02 item 7b / ADVICE: a GPU whose launch fails must not leave the others in a collective for ever.  The
    in-library path launches every shard BEFORE the frame's one collective is enqueued, so a failure (injected here on the
    last rank) returns an error at once, drains the launches that did start, and the handle renders correctly afterwards;
    the caller's current device is untouched."""
    import ctypes as C
    sd = scenes.cornell_scene(200, 136)
    kw = dict(max_depth=3, spp=(2, 1), seed=2)
    n = min(2, gpu.device_count())
    hip = C.CDLL("libamdhip64.so")
    before = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(before)) == 0
    with gpu.MultiScene(sd, n) as ms:
        monkeypatch.setenv("PBRT_HIP_MULTI_FAIL_RANK", str(n - 1))
        with pytest.raises(RuntimeError) as e:
            ms.render(**kw)
        assert "injected launch failure" in str(e.value)
        monkeypatch.delenv("PBRT_HIP_MULTI_FAIL_RANK")
        film, _ = ms.render(**kw)
    after = C.c_int(-1)
    assert hip.hipGetDevice(C.byref(after)) == 0 and after.value == before.value
    assert_bit_equal(film, oracle.OracleScene(sd).render(**kw)[0], "frame after a failed one")
    # all visible GPUs asked for, but a 64x64 film has one super-tile: the library uses one GPU (no scene copies for idle ranks)
    with gpu.MultiScene(scenes.cornell_scene(64, 64), 0) as ms:
        assert ms.n_gpus == 1


@pytest.mark.timeout(1200)
def test_bench_eight_ranks_share_one_gpu_under_gloo(gpu):
    """The driver's 8-GPU command line -- torch.distributed.run --nproc-per-node 8 bench.py --gpus 8 -- end to end before
    an 8-GPU node ever sees it: eight ranks share this box's GPU(s) with PBRT_DIST_BACKEND=gloo
    (RCCL wants one GPU per rank), every rank renders its eighth of the super-tiles, barrier, max-over-ranks timing,
    gather on rank 0, one JSON line whose film is complete.  Then the same with a wide box filter: the exchange is the
    integer sum reduction instead of the gather."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PBRT_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    base = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1", "--master-port", "29541",
            os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--workload", "c2", "--spp", "2", "2", "--full", "--no-cpu-baseline"]
    r = subprocess.run(base, capture_output=True, text=True, cwd=root, env=env, timeout=1000)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 alone prints the line"
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["steps"] == 2 and out["scaling"] == "strong" and out["value"] > 0
    assert out["film_check"]["weight_ok"] and out["film_check"]["finite"]
    # (round 6) the line of an N-rank run carries EVERY rank's kernel time and sample count, and what a step costs beyond
    # its slowest kernel: an imbalance or a slow gather shows in the first real 8-GPU record
    pr = out["per_rank_kernel_ms"]
    assert len(pr["mean_per_rank"]) == len(pr["max_step_per_rank"]) == len(pr["samples_per_rank"]) == 8 and min(pr["mean_per_rank"]) > 0
    assert sum(pr["samples_per_rank"]) == 1024 * 1024 * 4 and pr["max"] == max(pr["mean_per_rank"]) and pr["imbalance"] >= 1.0
    assert abs(out["exchange_ms"] - (out["ms_per_step"] - pr["max"])) < 1e-9 and "unmeasured" in out["scaling_note"]
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0", "--workload", "c2", "--spp", "2", "2",
                          "--full", "--no-cpu-baseline", "--no-counters"], capture_output=True, text=True, cwd=root, timeout=600)
    assert one.returncode == 0, one.stderr[-3000:]
    ref = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    assert abs(ref["film_check"]["mean_Y"] - out["film_check"]["mean_Y"]) < 1e-12  # eight shares assemble the one-rank film
    wide = subprocess.run(base + ["--filter", "1.5", "1.5", "--no-counters"], capture_output=True, text=True, cwd=root, env=env, timeout=1000)
    assert wide.returncode == 0, wide.stderr[-3000:]
    w8 = json.loads([l for l in wide.stdout.splitlines() if l.startswith("{")][-1])
    w1 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "0", "--workload", "c2", "--spp", "2", "2",
                         "--full", "--no-cpu-baseline", "--no-counters", "--filter", "1.5", "1.5"], capture_output=True, text=True, cwd=root, timeout=600)
    assert w1.returncode == 0, w1.stderr[-3000:]
    w1 = json.loads([l for l in w1.stdout.splitlines() if l.startswith("{")][-1])
    assert w8["film_check"]["finite"] and abs(w8["film_check"]["mean_Y"] - w1["film_check"]["mean_Y"]) < 1e-12
    # 3 x 3 pixels x 4 spp (a film point x + jx that rounds up to x + 1 in fp32 reaches one pixel further: a few per thousand)
    assert w8["film_check"]["mean_weight"] == w1["film_check"]["mean_weight"] and abs(w8["film_check"]["mean_weight"] - 36.0) < 0.01


# ---- box filter radii other than 0.5 and Film "maxsampleluminance"  ----
WIDE_CASES = [
    ("mesh1k", INTEGRATOR_PATH, 6, (2, 2), 3, (1.5, 1.5), "stratified"),
    ("mesh1k", INTEGRATOR_PATH, 6, (3, 2), 4, (1.0, 2.0), "sobol"),
    ("cornell", INTEGRATOR_PATH, 8, (2, 2), 1, (0.3, 0.75), "stratified"),  # narrower than a pixel: some samples land nowhere
    ("cornell", INTEGRATOR_PATH, 8, (9, 8), 2, (2.5, 0.5), "stratified"),   # 72 spp: two chunks per pixel; default radius on one axis
    ("check_sphere", INTEGRATOR_PATH, 5, (2, 2), 9, (2.0, 2.0), "stratified"),  # the sphere kernel
    ("sphere", INTEGRATOR_DIRECT, 5, (4, 2), 0, (1.25, 3.0), "sobol"),
    ("ties", INTEGRATOR_PATH, 6, (2, 1), 5, (0.75, 0.75), "stratified"),
]


@pytest.mark.parametrize("name,integrator,depth,spp,seed,fw,sampler", WIDE_CASES)
def test_wide_box_filter_matches_oracle(gpu, oracle, name, integrator, depth, spp, seed, fw, sampler):
    """`PixelFilter "box" "float xwidth" r`: every sample inside the sample bounds (film.rs:166-175) adds to all pixels
    within the radius; the film is accumulated in 64-bit fixed point with integer atomics, so it is
    reproducible and must equal the oracle's bit for bit -- film, accumulators, and the sum over three ranks."""
    sd = SMALL_SCENES[name]()
    kw = dict(integrator=integrator, max_depth=depth, spp=spp, seed=seed, sampler=sampler)
    o = oracle.OracleScene(sd)
    ref, _ = o.render(filter_width=fw, **kw)
    ref_acc, _ = o.render_acc(fw, **kw)
    with gpu.Scene(sd) as sc:
        film, st = sc.render(filter_width=fw, **kw)
        again, _ = sc.render(filter_width=fw, **kw)
        acc, _ = sc.render_acc(fw, **kw)
        parts = [sc.render_acc(fw, rank=r, world_size=3, **kw)[0] for r in range(3)]
        default, _ = sc.render(**kw)  # the default path still works on the same handle afterwards
    assert_bit_equal(film, ref, f"{name} film, box filter {fw}")
    assert_bit_equal(again, ref, "second frame (atomics: still deterministic)")
    assert np.array_equal(acc, ref_acc), "accumulators"
    assert np.array_equal(parts[0] + parts[1] + parts[2], ref_acc), "accumulators of three ranks add up to one rank's"
    assert_bit_equal(gpu.film_from_acc(ref_acc), ref, "host conversion of the accumulators")
    assert_bit_equal(default, o.render(**kw)[0], "default filter after a wide one")
    # weights: a pixel collects the samples of (2 rx) x (2 ry) pixel areas (interior and border alike: the halo is sampled)
    w = film[..., 3]
    area = 4 * fw[0] * fw[1] * spp[0] * spp[1]
    assert abs(w.mean() - area) < 0.2 * area + 1


def test_wide_box_filter_crop_window_and_big_sums(gpu, oracle):
    """A crop window (sample bounds reach outside it, negative pixel coordinates included at the image corner), and
    radiance sums far beyond 2^24 fixed-point units: the int64 -> float conversion must round as the CPU's does."""
    sd = scenes.cornell_scene(96, 80, crop=(0.0, 0.4, 0.0, 0.55))
    kw = dict(max_depth=6, spp=(6, 6), seed=11, filter_width=(3.0, 1.5))
    ref, _ = oracle.OracleScene(sd).render(**kw)
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(**kw)
    assert_bit_equal(film, ref, "cropped film, box filter (3, 1.5)")
    assert film[..., 3].max() >= 36 * 6 * 3 * 0.9


def test_max_sample_luminance_matches_oracle(gpu, oracle):
    """Film "float maxsampleluminance" (film.rs:75,279; pbrt-v3 FilmTile::AddSample): samples brighter than the bound are
    scaled down to it -- on the default film path and on the fixed-point one."""
    sd = scenes.cornell_scene(64, 64)  # the camera sees the ceiling light: Le = (17, 12, 4)
    kw = dict(max_depth=5, spp=(3, 3), seed=4)
    o = oracle.OracleScene(sd)
    plain, _ = o.render(**kw)
    ref, _ = o.render(max_sample_luminance=1.5, **kw)
    refw, _ = o.render(max_sample_luminance=1.5, filter_width=(1.5, 1.5), **kw)
    assert not np.array_equal(plain, ref)  # the bound bites
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(max_sample_luminance=1.5, **kw)
        filmw, _ = sc.render(max_sample_luminance=1.5, filter_width=(1.5, 1.5), **kw)
        unbounded, _ = sc.render(**kw)
    assert_bit_equal(film, ref, "clamped film")
    assert_bit_equal(filmw, refw, "clamped film, wide filter")
    assert_bit_equal(unbounded, plain, "no bound")


def test_wide_box_filter_in_one_process_multi_gpu_and_scene_file(gpu, oracle):
    """The in-library multi-GPU path with a wide filter (accumulators summed -- ncclReduce for n > 1 -- then converted on
    GPU 0), and the same through a scene file: `PixelFilter "box" "float xwidth" 1.5` + Film "maxsampleluminance"."""
    import os
    from pbrt_amd import loader
    sd = scenes.cornell_scene(200, 136)
    kw = dict(max_depth=3, spp=(2, 2), seed=8, filter_width=(1.5, 1.5))
    ref, _ = oracle.OracleScene(sd).render(**kw)
    n = min(2, gpu.device_count())
    with gpu.MultiScene(sd, n) as ms:
        film, _ = ms.render(**kw)
    assert_bit_equal(film, ref, f"wide filter on {n} GPU(s) in one process")
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "c0_check_sphere.pbrt")).read()
    text = text.replace("[400]", "[64]").replace('"integer pixelsamples" 128', '"integer pixelsamples" 4')
    text = text.replace("Film ", 'PixelFilter "box" "float xwidth" 1.5 "float ywidth" 1.5\nFilm ', 1).replace('"string filename"', '"float maxsampleluminance" 0.75 "string filename"', 1)
    ls = loader.load_string(text)
    assert ls.filter_width == (1.5, 1.5) and ls.max_sample_luminance == 0.75
    ref, _ = oracle.OracleScene(ls.scene).render(seed=0, **ls.render_kwargs())
    with gpu.Scene(ls.scene) as sc:
        film, _ = sc.render(seed=0, **ls.render_kwargs())
    assert_bit_equal(film, ref, "C0 scene file with a wide box filter")


@pytest.mark.parametrize("name,integrator,depth,spp,seed", [
    ("mesh1k", INTEGRATOR_PATH, 8, (4, 4), 3), ("cornell", INTEGRATOR_PATH, 12, (9, 8), 1), ("check_sphere", INTEGRATOR_PATH, 5, (2, 2), 9),
    ("sphere", INTEGRATOR_DIRECT, 5, (4, 2), 0), ("deep", INTEGRATOR_PATH, 6, (2, 2), 6), ("mesh20k", INTEGRATOR_PATH, 8, (5, 3), 2)])
@pytest.mark.parametrize("sampler", ["sobol_nd", "halton"])
def test_sobol_nd_sampler_matches_oracle(gpu, oracle, name, integrator, depth, spp, seed, sampler):
    """Sampler "sobol" (sampler 2): every request of a sample takes its own pair of Sobol' dimensions from
    the generator matrices (rows of the reference's SOBOL_MATRICES32), later requests fall back to the padded scheme: integer
    arithmetic, so the film equals the oracle's bit for bit -- sphere and triangle kernels, LDS and overflow stacks, a
    non-power-of-two sample count, three ranks.  Sampler "halton" (sampler 3, 3.13: scrambled radical inverses in 128 prime
    bases; the kernel divides by reciprocals where the oracle divides) in the same instantiations of the kernel, likewise."""
    sd = SMALL_SCENES[name]()
    kw = dict(integrator=integrator, max_depth=depth, spp=spp, seed=seed, sampler=sampler)
    ref, _ = oracle.OracleScene(sd).render(**kw)
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(**kw)
        acc = sum(sc.render(rank=r, world_size=3, **kw)[0] for r in range(3))
        from pbrt_amd import _lib
        with pytest.raises(_lib.PbrtHipError) as e:
            sc.render(**dict(kw, counters=True))
        assert e.value.code == -1
        wide, _ = sc.render(**dict(kw, filter_width=(1.5, 1.25)))  # (the table samplers under a wide box filter: render_kernel_x)
        other, _ = sc.render(**dict(kw, sampler="sobol"))
    assert_bit_equal(film, ref, f"{name} film, sampler {sampler}")
    assert_bit_equal(wide, oracle.OracleScene(sd).render(**dict(kw, filter_width=(1.5, 1.25)))[0], f"{name}, sampler {sampler}, box filter 1.5 x 1.25")
    assert_bit_equal(acc, ref, "three ranks")
    assert not np.array_equal(other, film)


def test_table_samplers_on_a_long_path(gpu, oracle):
    """maxdepth 16 in a closed Cornell-style box (BASELINE C4's scene and depth): a path makes up to 61 requests, every one of which
    has its own dimensions in samplers 2 and 3 since round 5 (64 requests: 128 Sobol' dimensions / 128 prime bases) -- films equal
    to the oracle's, and maxdepth 40 runs past the tables into the padded requests."""
    sd = scenes.cornell_scene(40, 24)
    for sampler in ("sobol_nd", "halton"):
        for depth in (16, 40):
            kw = dict(max_depth=depth, spp=(8, 8), seed=11, sampler=sampler)
            ref, _ = oracle.OracleScene(sd).render(**kw)
            with gpu.Scene(sd) as sc:
                film, _ = sc.render(**kw)
            assert_bit_equal(film, ref, f"{sampler}, maxdepth {depth}")
