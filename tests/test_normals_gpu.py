"""Shading normals on the GPU.  What stood before the oracle learnt normals (tests/test_normals_plastic_parity_gpu.py
holds the films to it word for word), held to tests/normals_ref.py: the hook against float64 with first-order
bounds, closed forms (one normal for a whole plane, the clipped cosine lobe, the mirror), the leaf-order gather triangle by triangle, the
tessellated sphere against C1's analytic image, and the library against itself (runs, shards, render_multi, scene file = arrays)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import normals_ref as nr
import pbrt_amd
import util
from pbrt_amd import INTEGRATOR_DIRECT, INTEGRATOR_PATH, INTEGRATOR_PATH_MIS, MIRROR, _lib, api, loader, scenes
from util import assert_bit_equal, lit_plane_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = dict(rtol=3e-6, atol=1e-7)  # the bar test_lit_plane_closed_forms holds


def _rgb(film):
    return pbrt_amd.film_to_rgb(film).astype(np.float64)


def _without_normals(sd):
    return dataclasses.replace(sd, tri_n=np.zeros((0, 9), np.float32)).normalized()


# ---- 1. the hook against float64 ----

def test_hook_against_float64(gpu):
    """2^16 elements through the statements the render kernels include (pbrt_hip_shading_normal_eval_device).  On ROBUST elements -- |n|,
    |dot(ns, ng)| and |dot(ng, wo)| each beyond 16 x their own bound -- the flips are float64's and every component of nsf lies within its
    first-order bound; the fallback returns +-ng bit for bit.  Largest error / bound measured on an MI355X: 0.88 (recorded in DESIGN.md 3.18)."""
    x, kind = nr.hook_inputs()
    ref = nr.shading_normal_f64(x)
    assert ref["robust"].mean() >= 0.90
    out = api.shading_normal_eval(x)
    nsf, fell = out[:, :3].astype(np.float64), out[:, 3]
    assert set(np.unique(fell)) <= {0.0, 1.0}
    rb = ref["robust"]
    assert not fell[rb].any()
    err = np.abs(nsf - ref["nsf"])
    assert (ref["bound"][rb] > 0).all()
    ratio = err[rb] / ref["bound"][rb]
    wrong_side = (err[rb] > 0.5).any(1)  # a flip decided the other way shows as an error of the component's own size
    print(f"robust {rb.mean():.4f}; largest error / bound {ratio.max():.3f}; largest error {err[rb].max():.3g}; flips decided otherwise {int(wrong_side.sum())}")
    assert not wrong_side.any()
    assert (ratio <= 1.0).all(), float(ratio.max())
    # the fallback: where float64 says the interpolated normal is zero the kernel says so too (every term is exactly zero there), and nsf
    # is ng or -ng bit for bit -- by the sign of fp32's own dot(ng, wo) where that is beyond its bound
    fb = ref["fell_back"]
    assert fell[fb].all() and fb.sum() >= 1024
    ng = x[:, 9:12]
    sure = fb & (np.abs(ref["c_wo"]) > nr.ROBUST_FACTOR * ref["c_wo_err"])
    want = np.where(ref["flip_wo"][:, None], -ng, ng)
    assert sure.sum() >= 900
    assert_bit_equal(out[sure, :3], want[sure], "fallback")
    either = (util.bits(out[fb, :3]) == util.bits(ng[fb])).all(1) | (util.bits(out[fb, :3]) == util.bits(-ng[fb])).all(1)
    assert either.all()
    # elements that are not robust still return a unit vector on one of the two sides
    ok = ~fb
    assert np.allclose(np.linalg.norm(nsf[ok], axis=1), 1.0, atol=1e-5)
    assert api.shading_normal_eval(np.zeros((0, 17), np.float32)).shape == (0, 4)


# ---- 2. one normal for the whole plane ----

SETTINGS = [dict(integrator=i, max_depth=d, sampler=s) for i in (INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS) for d in (1, 5) for s in ("stratified", "halton")]
WL = np.array([0.6, 0.0, 0.8])  # lit_plane_scene("distant")'s light
PLANE_CASES = {
    "towards the light": (nr.tilted(30.0, 0.0), WL),
    "away from the light": (nr.tilted(30.0, 180.0), WL),
    "handed in negated": (-nr.tilted(30.0, 0.0), WL),
    "handed in seven times as long": (7.0 * nr.tilted(30.0, 180.0), WL),
    "light above the shading hemisphere, below the plane": (nr.tilted(40.0, 0.0), np.array([0.9, 0.0, -0.1]) / np.hypot(0.9, 0.1)),
    "light above the plane, below the shading hemisphere": (nr.tilted(40.0, 180.0), np.array([0.95, 0.0, 0.2]) / np.hypot(0.95, 0.2)),
}


@pytest.mark.parametrize("case", list(PLANE_CASES))
def test_one_normal_for_the_whole_plane(gpu, oracle, case):
    n_star, wl = PLANE_CASES[case]
    sd, _ = lit_plane_scene("distant", 16)
    sd.lights[0, 1:4] = wl
    nr.with_normal(sd, n_star)
    n_unit = sd.tri_n[0, :3].astype(np.float64)
    n_unit /= np.linalg.norm(n_unit)
    if n_unit[2] < 0:
        n_unit = -n_unit  # turned to the winding's side
    wl32 = sd.lights[0, 1:4].astype(np.float64)
    lit = wl32[2] > 0 and n_unit @ wl32 > 0
    want = nr.lambert_distant(sd.materials[0, 1:4], (3.0, 2.0, 1.0), n_unit, wl32) if lit else np.zeros(3)
    assert lit == ("hemisphere" not in case)
    o = oracle.OracleScene(sd)
    with gpu.Scene(sd) as sc:
        for kw in SETTINGS:
            film = sc.render(spp=(2, 2), seed=9, **kw)[0]
            assert_bit_equal(film, o.render(spp=(2, 2), seed=9, **kw)[0], f"{case} {kw}: against the oracle")  # (beside the closed form: word for word)
            rgb = _rgb(film)
            if lit:
                assert np.allclose(rgb, want, **BAR), (case, kw, rgb.min((0, 1)), rgb.max((0, 1)), want)
            else:
                assert (rgb == 0).all(), (case, kw, rgb.max())
    if case == "towards the light":  # the same normal, not the plane's: the image must differ from the flat one
        assert not np.allclose(want, lit_plane_scene("distant", 16)[1], rtol=1e-2)


@pytest.mark.parametrize("kind", ["distant", "infinite"])
def test_zero_normals_are_the_plain_scene(gpu, oracle, kind):
    """all corner normals zero = "none": the NRM kernels fall back to the geometric normal and the film is the oracle's, bit for bit"""
    sd, _ = lit_plane_scene(kind, 16)
    plain = _without_normals(sd)
    nr.with_normal(sd, (0.0, 0.0, 0.0))
    with gpu.Scene(sd) as sc:
        for kw in SETTINGS[::3]:
            film, _ = sc.render(spp=(2, 2), seed=5, **kw)
            ref, _ = oracle.OracleScene(plain).render(spp=(2, 2), seed=5, **kw)
            assert_bit_equal(film, ref, f"{kind} {kw}")


# ---- 3. the clipped cosine lobe ----

@pytest.mark.parametrize("theta", [20.0, 40.0, 70.0])
def test_clipped_cosine_lobe(gpu, theta):
    """A constant sky over a plane whose shading normal is tilted by theta: a cosine-sampled direction about the shading normal counts only
    above the GEOMETRIC plane, so every sample expects rho Le (1 + cos theta) / 2 (1.0 without the geometric-side rule: 47 standard errors
    off at 40 degrees)."""
    sd, full = lit_plane_scene("infinite", 16)  # full = rho Le
    nr.with_normal(sd, nr.tilted(theta, 75.0))
    p = nr.clipped_lobe_fraction(theta)
    with gpu.Scene(sd) as sc:
        # integrator 0: a sample is rho Le x Bernoulli(p) -- the one light sample --, and stratification only narrows the mean
        rgb = _rgb(sc.render(integrator=INTEGRATOR_PATH, max_depth=1, spp=(8, 8), seed=3)[0])
        n = 16 * 16 * 64
        m = rgb.mean((0, 1)) / full
        print(f"theta {theta}: integrator 0 mean / (rho Le) = {m}, expected {p:.5f}, 5 sigma {5 * np.sqrt(p * (1 - p) / n):.5f}")
        assert (np.abs(m - p) <= 5 * np.sqrt(p * (1 - p) / n) + 1e-6).all(), (theta, m, p)
        assert np.allclose(rgb / full, (rgb / full)[..., :1], rtol=1e-5)  # one draw for the three channels
        # integrator 2: the light sample and the bounce ray that finds the sky share the estimate, half each
        rgb = _rgb(sc.render(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(8, 8), seed=3)[0])
        px = rgb[..., 1].reshape(-1) / full[1]
        se = px.std(ddof=1) / np.sqrt(px.size)
        print(f"theta {theta}: integrator 2 mean / (rho Le) = {px.mean():.5f}, standard error {se:.5f}")
        assert abs(px.mean() - p) <= 5 * se + 1e-3 * p, (theta, px.mean(), p, se)


# ---- 4. every slot gets ITS normals ----

def _check_grid(sc, sd, wl, L, rho, qualify, tri):
    rgb = _rgb(sc.render(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(1, 1), seed=1)[0])
    n = sd.tri_n[:128, :3].astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    vals = (rho / np.pi * L)[None, :] * (n @ wl)[:, None]  # (128, 3)
    want = vals[tri[0]]
    good = np.isclose(rgb, want, **BAR).all(-1)
    assert good[qualify].all(), (int((~good[qualify]).sum()), rgb[qualify][~good[qualify]][:3], want[qualify][~good[qualify]][:3])
    some = np.isclose(rgb[:, :, None, :], vals[None, None], **BAR).all(-1).any(-1)
    assert some.all(), int((~some).sum())


@pytest.fixture(scope="module")
def grid():
    sd, wl, L, rho = nr.grid_plane_scene(64)
    o, d = nr.pixel_corner_rays(sd)
    tri = nr.grid_triangle_of(*nr.plane_points(o, d))
    qualify = (tri == tri[0]).all(0) & (tri[0] >= 0)
    assert qualify.mean() >= 0.5 and len(np.unique(tri[0][qualify])) >= 80
    return sd, wl, L, rho, qualify, tri


@pytest.mark.parametrize("builder", [None, "host", "gpu-plain"])
def test_every_slot_gets_its_normals(gpu, grid, builder):
    """128 triangles, 128 normals, the leaf order the builder's: a pixel whose four corner rays meet one triangle holds THAT triangle's
    value, every other pixel some triangle's"""
    sd, wl, L, rho, qualify, tri = grid
    with gpu.Scene(sd, builder=builder) as sc:
        _check_grid(sc, sd, wl, L, rho, qualify, tri)
        order = sc.export_quads()[1]
    assert not np.array_equal(order, np.arange(128))  # (the leaf order is not the triangle order: the gather has something to do)


def test_every_slot_gets_its_normals_under_a_deep_tree(gpu, grid):
    """the same with 400 triangles of a degenerate tree hidden below the plane (zero normals): the tree needs the overflow stack, so a
    STACK = 30 instantiation renders"""
    _, wl, L, rho, qualify, tri = grid
    sd = nr.grid_plane_scene(64, below=util.deep_tree_scene(k=400))[0]
    assert sd.idx.shape[0] == 528 and not sd.tri_n[128:].any()
    with gpu.Scene(sd, builder="host") as sc:
        rows, waves, beyond = C.c_uint32(), C.c_uint32(), C.c_uint32()
        assert _lib.lib().pbrt_hip_render_stack_plan(sc.info()["quad_stack_need"], C.byref(rows), C.byref(waves), C.byref(beyond)) == 0
        assert beyond.value > 0 and rows.value == 30, (sc.info()["quad_stack_need"], rows.value, beyond.value)  # the precondition: the overflow variant
        _check_grid(sc, sd, wl, L, rho, qualify, tri)


# ---- 5. a tessellated sphere converges like h^2, not h ----

def test_tessellated_sphere_converges_like_h_squared(gpu):
    """C1 with its sphere tessellated (5120 triangles, h = 0.07 rad) against C1's analytic image: flat, a facet's normal is off by O(h) and
    so is the cosine; smooth, the interpolated normal and the sag of the hit point are off by O(h^2).  Measured on an MI355X: mean relative
    error over the interior pixels 9.0e-3 flat, 1.2e-3 smooth."""
    img, interior, _ = util.c1_analytic_image(128, 128)
    assert interior.mean() > 0.02
    err = {}
    for smooth in (True, False):
        with gpu.Scene(scenes.icosphere_scene(4, smooth=smooth, xres=128, yres=128)) as sc:
            rgb = _rgb(sc.render(integrator=INTEGRATOR_DIRECT, max_depth=5, spp=(8, 8), seed=0)[0])
        err[smooth] = float(np.abs(rgb[..., 1][interior] / img[interior] - 1).mean())
    print(f"mean relative error over {int(interior.sum())} interior pixels: smooth {err[True]:.3g}, flat {err[False]:.3g}, ratio {err[True] / err[False]:.3g}")
    assert err[True] <= 0.25 * err[False], err


# ---- 6. the mirror ----

def test_mirror_reflects_about_the_shading_normal(gpu):
    """A mirror plane under a constant sky, its shading normal tilted by 40 degrees: a pixel is Kr Le where the reflection about n* leaves
    on the geometric front side and exactly 0 where it would go through the plane"""
    sd, _ = lit_plane_scene("infinite", 16)
    sd.materials = np.array([[MIRROR, 0.9, 0.9, 0.9, 0, 0, 0]], np.float32)
    n_star = nr.tilted(40.0, 30.0)
    nr.with_normal(sd, n_star)
    n32 = sd.tri_n[0, :3].astype(np.float64)
    n32 /= np.linalg.norm(n32)
    o, d = nr.pixel_corner_rays(sd)
    up = nr.reflect(-d, n32)[..., 2] > 0
    agree = (up == up[0]).all(0)
    assert agree.mean() >= 0.8 and up[0][agree].any() and (~up[0][agree]).any(), (agree.mean(), up[0][agree].mean())
    want = np.where(up[0][..., None], 0.9 * np.array([0.5, 0.25, 1.0]), 0.0)
    with gpu.Scene(sd) as sc:
        for kw in (dict(integrator=INTEGRATOR_PATH, max_depth=5), dict(integrator=INTEGRATOR_PATH_MIS, max_depth=1, sampler="halton")):
            rgb = _rgb(sc.render(spp=(2, 2), seed=2, **kw)[0])
            assert np.allclose(rgb[agree], want[agree], **BAR), kw
            assert (rgb[agree & ~up[0]] == 0).all()


# ---- 7. face normals handed in change nothing but rounding ----

@pytest.mark.parametrize("integrator", [INTEGRATOR_PATH, INTEGRATOR_PATH_MIS])
@pytest.mark.parametrize("name", ["cornell", "glass_sphere", "envmap"])
def test_face_normals_change_nothing_but_rounding(gpu, oracle, name, integrator):
    """every triangle carries its own float64 face normal rounded to fp32: the NRM kernels (their GLS and ENV sides too) render what the
    oracle renders of the scene without the record, to the fixed cases' bar for rounding-only differences"""
    plain = {"cornell": scenes.cornell_scene, "glass_sphere": scenes.glass_sphere_scene, "envmap": scenes.envmap_scene}[name](32, 32)
    sd = dataclasses.replace(plain, tri_n=nr.face_normals(plain)).normalized()
    kw = dict(integrator=integrator, max_depth=5, spp=(4, 4), seed=7)
    ref, _ = oracle.OracleScene(plain).render(**kw)
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(**kw)
    ps, share, weights = util.twin_agreement(ref, film)
    print(f"{name} integrator {integrator}: PSNR {ps:.1f} dB, {100 * share:.2f} % of the pixels within 1e-4")
    assert weights and share >= 0.99 and ps >= 90.0, (name, integrator, ps, share)


# ---- 8. plumbing ----

KW = dict(integrator=INTEGRATOR_PATH_MIS, max_depth=5, spp=(2, 2), seed=4, sampler="halton")


def test_runs_shards_and_render_multi_agree(gpu):
    sd = scenes.smooth_mesh_scene(160, 96)  # 3 x 2 super-tiles
    with gpu.Scene(sd) as sc:
        whole, _ = sc.render(**KW)
        again, _ = sc.render(**KW)
        assert_bit_equal(whole, again, "two runs")
        owner = np.zeros((96, 160), np.int64)
        for t in range(6):
            owner[(t // 3) * 64:(t // 3) * 64 + 64, (t % 3) * 64:(t % 3) * 64 + 64] = t % 3
        for rank in range(3):
            part, _ = sc.render(rank=rank, world_size=3, **KW)
            assert_bit_equal(part[owner == rank], whole[owner == rank], f"rank {rank}: its tiles")
            assert not part[owner != rank].any()
    assert whole[..., :3].max() > 0
    multi, _ = api.render_multi(sd, n_gpus=1, **KW)
    assert_bit_equal(multi, whole, "pbrt_hip_render_multi")
    with api.MultiScene(sd, n_gpus=1) as ms:
        assert_bit_equal(ms.render(**KW)[0], whole, "pbrt_hip_multi_render")
    # the normals matter to this image
    with gpu.Scene(_without_normals(sd)) as sc:
        flat, _ = sc.render(**KW)
    assert not np.array_equal(flat, whole)


@pytest.mark.parametrize("builder", [None, "host"])
def test_device_bytes_grow_by_48_per_leaf_slot(gpu, builder):
    sd = scenes.smooth_mesh_scene(16, 16)
    sd.spheres = np.array([[0, 2, 1, 0.5, 0]], np.float32)  # a sphere's proxy slot gets a (zero) record too
    sd.normalized()
    with gpu.Scene(sd, builder=builder) as a, gpu.Scene(_without_normals(sd), builder=builder) as b:
        assert a.info()["device_bytes"] - b.info()["device_bytes"] == 48 * (sd.idx.shape[0] + 1)
        film, _ = a.render(**KW)  # (and the scene with a sphere renders: the SPH instantiation)
        assert np.isfinite(film).all() and film[..., :3].max() > 0


def test_render_time_refusals(gpu):
    with gpu.Scene(scenes.smooth_mesh_scene(16, 16)) as sc:
        for kw, word in ((dict(filter_width=(1.0, 1.0)), "filter"), (dict(filter_width=(0.5, 2.0)), "filter"), (dict(counters=True), "counter"), (dict(counters="walk"), "counter")):
            with pytest.raises(_lib.PbrtHipError) as e:
                sc.render(spp=(1, 1), **kw)
            assert e.value.code == -4 and "normals" in str(e.value) and word in str(e.value), str(e.value)
        with pytest.raises(_lib.PbrtHipError) as e:
            sc.render_acc((1.0, 1.0), spp=(1, 1))
        assert e.value.code == -4 and "normals" in str(e.value)
        film, _ = sc.render(spp=(1, 1), filter_width=(0.5, 0.5))  # the default radius, said explicitly
        assert film[..., :3].max() > 0


def test_scene_file_renders_like_the_generator(gpu):
    ls = loader.load_file(os.path.join(ROOT, "scenes", "smooth_mesh.pbrt"))
    kw = dict(ls.render_kwargs(), spp=(2, 2), seed=1)
    with gpu.Scene(ls.scene) as a, gpu.Scene(scenes.smooth_mesh_scene()) as b:
        fa, _ = a.render(**kw)
        fb, _ = b.render(**kw)
    assert_bit_equal(fa, fb, "scene file against the generator")
    assert fa[..., :3].max() > 0
