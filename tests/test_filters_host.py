"""Weighted pixel filters without a GPU: the reference of tests/filters_ref.py against the oracle's wide box filter, the
library's filter table against float64, the weighted film conversion, the parser and the loader, and the kernels' notes."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import filters_ref as fr
import pbrt_amd
from pbrt_amd import _lib, api, isa_id, loader, scenes
from test_host import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = (0.125, 0.875, 0.15, 0.85)  # of 24 x 20: pixels [3, 21) x [3, 17), strictly inside on all four sides
SEED, DEPTH = 11, 3
KIND_PARAMS = {  # default and non-default parameters
    "triangle": [(0.0, 0.0)], "gaussian": [(2.0, 0.0), (0.75, 0.0)], "mitchell": [(1.0 / 3.0, 1.0 / 3.0), (0.6, 0.15)], "sinc": [(3.0, 0.0), (2.25, 0.0)]}


def small_scene():
    sd = scenes.cornell_scene(24, 20)
    sd = dataclasses.replace(sd, crop=CROP).normalized()
    cb = pbrt_amd.film_cropped_bounds(sd.xres, sd.yres, sd.crop)
    assert cb == (3, 3, 21, 17)
    return sd, cb


# ---- 1. the reference is sound, independently of the product ----
@pytest.mark.parametrize("sampler,spp", [("sobol", (2, 2)), ("stratified", (1, 1))])
@pytest.mark.parametrize("radii", [(1.5, 1.0), (2.5, 2.5)])
def test_reference_reproduces_the_oracles_wide_box(oracle, radii, sampler, spp):
    """The box footprint, the restated film points and OracleScene.pixel_samples give OracleScene.render_acc bit for bit: the yardstick of the
    GPU test of the weighted filters, which swaps the weight 1 for a table entry.  (The stratified sampler at one sample per pixel: a later
    sample's film point lies behind its predecessors' path draws -- filters_ref.py.)"""
    sd, cb = small_scene()
    o = oracle.OracleScene(sd)
    want, _ = o.render_acc(radii, max_depth=DEPTH, spp=spp, seed=SEED, sampler=sampler)
    got = fr.reference_acc(o, sd, cb, radii, spp, SEED, sampler, DEPTH)
    assert want[..., 3].sum() > 0 and np.array_equal(got, want)


def emitters_scene():
    """A scene for max_depth 0, where a path ends at its first vertex without a draw: four emissive quads of different colours at different
    depths in front of the camera, partly overlapping, under a constant sky -- every pixel's radiance is an emitter's Le or the sky's L, and
    it changes from pixel to pixel along the quads' edges.  24 x 20 with the crop window of small_scene()."""
    from pbrt_amd import LIGHT_INFINITE, MATTE, SceneData, look_at
    quads = [((-1.2, 2.0, -0.9), (0.1, 2.0, -0.7), (0.0, 2.0, 0.6), (-1.1, 2.0, 0.4), (3.0, 0.5, 0.25)),
             ((-0.3, 1.5, -0.2), (1.0, 1.5, -0.5), (1.1, 1.5, 0.8), (-0.2, 1.5, 0.9), (0.25, 2.0, 0.75)),
             ((0.4, 1.0, -1.0), (0.9, 1.0, -1.0), (0.9, 1.0, 0.1), (0.4, 1.0, 0.1), (0.5, 0.5, 6.0)),
             ((-0.9, 2.5, 0.2), (0.9, 2.5, 0.3), (0.8, 2.5, 1.1), (-0.8, 2.5, 1.0), (40000.0, 1.0, 0.125))]  # (a component beyond the 2^15 clamp)
    P, idx, mats = [], [], []
    for k, (a, b, c, d, le) in enumerate(quads):
        P += [a, b, c, d]
        idx += [[4 * k, 4 * k + 1, 4 * k + 2], [4 * k, 4 * k + 2, 4 * k + 3], [4 * k, 4 * k + 2, 4 * k + 1], [4 * k, 4 * k + 3, 4 * k + 2]]  # both windings: seen from either side
        mats.append([MATTE, 0, 0, 0, *le])
    sd = SceneData(P=np.array(P, np.float32), idx=np.array(idx, np.uint32), mat_id=np.repeat(np.arange(4, dtype=np.uint16), 4), materials=np.array(mats, np.float32),
                   lights=np.array([[LIGHT_INFINITE, 0, 0, 0, 0.25, 0.5, 0.75]], np.float32), cam_to_world=look_at((0, -3, 0), (0, 0, 0), (0, 0, 1))[1], fov=50.0,
                   xres=24, yres=20, crop=CROP).normalized()
    return sd, pbrt_amd.film_cropped_bounds(sd.xres, sd.yres, sd.crop)


@pytest.mark.parametrize("spp", [(2, 2), (8, 8), (3, 5)])
@pytest.mark.parametrize("radii", [(1.5, 1.0), (2.5, 2.5)])
def test_reference_reproduces_the_oracles_wide_box_stratified_many_samples(oracle, radii, spp):
    """The stratified sampler with several samples in a chunk -- strata beyond (0, 0), inv_nx != 1 -- and, at 64 samples, two chunks of a pixel:
    at max_depth 0 no path draws, so every sample's film point is restated (filters_ref.py), and the box footprint with the oracle's radiances
    gives OracleScene.render_acc bit for bit.  The yardstick of the GPU test's stratified cases at these sample counts."""
    sd, cb = emitters_scene()
    o = oracle.OracleScene(sd)
    want, _ = o.render_acc(radii, max_depth=0, spp=spp, seed=SEED, sampler="stratified")
    got = fr.reference_acc(o, sd, cb, radii, spp, SEED, "stratified", 0)
    assert want[..., 3].sum() > 0 and len(np.unique(want[..., :3].reshape(-1, 3), axis=0)) > 50 and np.array_equal(got, want)


# ---- 2. the table ----
def _ulp_distance(a, b):
    ia, ib = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7FFFFFFF), i) for i in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("kind", list(KIND_PARAMS))
def test_filter_table_against_float64(kind):
    """pbrt_hip_filter_table is the float64 filter rounded to float once: within 1 float ulp of the float64 reference rounded to float (the
    ulp: two libms may differ in a double's last bit)."""
    k = fr.KINDS[kind]
    for params in KIND_PARAMS[kind]:
        for radius in [(0.0, 0.0), (1.5, 3.0)]:
            rx, ry = fr.radii_of(k, radius)
            got = pbrt_amd.filter_table((kind,) + params, radius)
            want64 = fr.table64(k, params, rx, ry)
            assert got.shape == (16, 16) and got.dtype == np.float32 and np.isfinite(got).all()
            assert _ulp_distance(got, want64.astype(np.float32)).max() <= 1, (kind, params, radius)
            if kind == "triangle":  # closed form: entry (0, 0) = (rx - rx / 32) (ry - ry / 32)
                assert got[0, 0] == np.float32((rx - rx / 32.0) * (ry - ry / 32.0))
            if kind == "mitchell":
                assert (got < 0).any() and got[0, 0] > 0
            if kind == "gaussian":
                assert (got >= 0).all() and (np.diff(got, axis=1) < 0).all() and (np.diff(got, axis=0) < 0).all()
            if kind == "sinc":
                assert (got < 0).any() and got[0, 0] > 0.9
    assert fr.default_radius(k) == api.filter_default_radius(kind) == (4.0 if kind == "sinc" else 2.0)


def test_filter_table_refuses_bad_records():
    out = np.zeros(256, np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    for rec, rx in [(_lib.PixelFilter(type=3, kind=9), 2.0), (_lib.PixelFilter(type=0, kind=1), 2.0), (_lib.PixelFilter(type=3, kind=1), 0.0),
                    (_lib.PixelFilter(type=3, kind=1), float("nan"))]:
        assert _lib.lib().pbrt_hip_filter_table(C.byref(rec), rx, 2.0, fp) == -1
        assert b"filter" in _lib.lib().pbrt_hip_last_error()
    bad = _lib.PixelFilter(type=3, kind=2)
    bad.param[0] = 0.0
    assert _lib.lib().pbrt_hip_filter_table(C.byref(bad), 2.0, 2.0, fp) == -1 and b"alpha" in _lib.lib().pbrt_hip_last_error()


# ---- 3. the weighted film conversion ----
def test_film_from_acc_weighted_is_the_restatement():
    rng = np.random.default_rng(5)
    acc = rng.integers(-2 ** 62, 2 ** 62, (4096, 4), dtype=np.int64)
    acc[:1024] = rng.integers(-2 ** 30, 2 ** 30, (1024, 4))
    acc[1024:1100, 3] = 0          # zero weight sums
    acc[1100:1200] = 0
    acc[1200:1300, :3] *= -1
    got = pbrt_amd.film_from_acc(acc, weighted=True)
    assert np.array_equal(got.view(np.uint32), fr.film_from_acc_weighted(acc).view(np.uint32))
    assert np.array_equal(got[:, 3], acc[:, 3].astype(np.float32) * np.float32(2.0 ** -24))
    assert np.array_equal(pbrt_amd.film_from_acc(acc)[:, :3].view(np.uint32), got[:, :3].view(np.uint32))  # (the box's conversion differs in the weight alone)
    assert np.isfinite(pbrt_amd.film_to_rgb(got[1024:1200])).all()  # a zero weight sum divides nothing


# ---- 4. parser and loader ----
HEAD = 'LookAt 0 -3 0  0 0 0  0 0 1\nCamera "perspective" "float fov" 40\nSampler "02sequence" "integer pixelsamples" 4\n'
TAIL = ('Film "image" "integer xresolution" [16] "integer yresolution" [16]\nWorldBegin\nLightSource "infinite" "rgb L" [1 1 1]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-1 1 -1  1 1 -1  0 1 1]\nWorldEnd\n')


@pytest.mark.parametrize("text,want_filter,want_radii", [
    ('PixelFilter "triangle"', (1, 0.0, 0.0), (2.0, 2.0)),
    ('PixelFilter "triangle" "float xwidth" 1.5 "float ywidth" 3', (1, 0.0, 0.0), (1.5, 3.0)),
    ('PixelFilter "gaussian"', (2, 2.0, 0.0), (2.0, 2.0)),
    ('PixelFilter "gaussian" "float alpha" 0.75 "float xwidth" 3', (2, 0.75, 0.0), (3.0, 2.0)),
    ('PixelFilter "mitchell"', (3, float(np.float32(1 / 3)), float(np.float32(1 / 3))), (2.0, 2.0)),
    ('PixelFilter "mitchell" "float B" 0.5 "float C" 0.25 "float ywidth" 1', (3, 0.5, 0.25), (2.0, 1.0)),
    ('PixelFilter "sinc"', (4, 3.0, 0.0), (4.0, 4.0)),
    ('PixelFilter "sinc" "float tau" 2 "float xwidth" 2 "float ywidth" 2', (4, 2.0, 0.0), (2.0, 2.0)),
])
def test_parser_fills_the_filter_record(text, want_filter, want_radii):
    ls = loader.load_string(HEAD + text + "\n" + TAIL)
    assert ls.scene.pixel_filter == want_filter and ls.filter_width == want_radii
    assert not [w for w in ls.warnings if "PixelFilter" in w], ls.warnings
    assert ls.names["filter"] == text.split('"')[1] and ls.render_kwargs()["filter_width"] == want_radii


def test_parser_keeps_the_box_and_warns_of_unknown_names():
    box = loader.load_string(HEAD + 'PixelFilter "box" "float xwidth" 1.5 "float ywidth" 1.5\n' + TAIL)
    assert box.scene.pixel_filter is None and box.filter_width == (1.5, 1.5) and not [w for w in box.warnings if "PixelFilter" in w]
    none = loader.load_string(HEAD + TAIL)
    assert none.scene.pixel_filter is None and none.filter_width == (0.5, 0.5)
    unknown = loader.load_string(HEAD + 'PixelFilter "catmullrom" "float xwidth" 1.25\n' + TAIL)
    assert unknown.scene.pixel_filter is None and unknown.filter_width == (1.25, 0.5)
    assert [w for w in unknown.warnings if "PixelFilter" in w and "catmullrom" in w]
    # a later directive replaces an earlier one, the box included
    twice = loader.load_string(HEAD + 'PixelFilter "gaussian"\nPixelFilter "box"\n' + TAIL)
    assert twice.scene.pixel_filter is None and twice.filter_width == (0.5, 0.5)


def test_filtered_cornell_loads():
    ls = loader.load_file(os.path.join(ROOT, "scenes", "filtered_cornell.pbrt"))
    assert ls.scene.pixel_filter == (3, float(np.float32(1 / 3)), float(np.float32(1 / 3))) and ls.filter_width == (2.0, 2.0)
    assert ls.scene.idx.shape[0] > 10 and not [w for w in ls.warnings if "PixelFilter" in w]


def test_scene_data_carries_the_filter_slot():
    """fill_desc emits the record as one more slot of the texture table, behind the checkerboards and the map, before the normals' record"""
    sd = dataclasses.replace(scenes.smooth_mesh_scene(16, 16), pixel_filter=("gaussian", 1.5)).normalized()
    assert sd.pixel_filter == (2, 1.5, 0.0)
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd, _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    assert [desc.textures[i].type for i in range(desc.n_textures)] == [3, 2]
    rec = _lib.PixelFilter.from_buffer_copy(bytes(C.string_at(C.byref(desc.textures[0]), 64)))
    assert (rec.kind, rec.param[0], rec.param[1]) == (2, 1.5, 0.0)
    assert C.sizeof(_lib.PixelFilter) == C.sizeof(_lib.Texture) == 64
    del keep


# ---- 5. the kernels' notes ----
# VGPRs / spilled VGPRs of the WIDE instantiations of the commit before the weighted filters, from the same compiler: render_kernel's stay
# within 96 VGPRs without a spill; render_kernel_x's must not gain spills -- one of them spilled two registers then
PARENT_X_SPILLS = {"render_kernel_x<false,30,true,true,true,true,false>": 2}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm llvm tools")
def test_wide_kernels_keep_their_register_budget():
    """render_kernel's WIDE instantiations without spheres: <= 96 VGPRs (92 and 93; the parent: 94 and 95), none with a spill or scratch.
    render_kernel_x's sixty: no spill gained over the parent -- none spills now, the parent's one that spilled two registers included.  (The
    weighted add is the direct-to-film branch the box's finish already had, with a weight: a finish of its own beside the box's cost four
    MIS instantiations a spilled register each.)"""
    import subprocess
    notes = _kernel_notes()
    demangled = subprocess.run(["c++filt"], input="\n".join(n[0] for n in notes), capture_output=True, text=True, check=True).stdout.split("\n")
    seen = {"render_kernel": 0, "render_kernel_x": 0}
    for d, (_, vgpr, spill, scratch) in zip(demangled, notes):
        name = isa_id.normalise(d)
        m = re.match(r"render_kernel<(\w+),false,false,(\d+),(\d+),true,(\w+)>", name)
        if m:
            seen["render_kernel"] += 1
            assert spill == 0 and scratch == 0, f"{name}: {vgpr} VGPRs, {spill} spilled, {scratch} B scratch"
            if m.group(1) == "false":
                assert vgpr <= 96, f"{name}: {vgpr} VGPRs do not fit 5 waves per SIMD"
        m = re.match(r"render_kernel_x<(\w+),(\d+),(\w+),(\w+),(\w+),true,(\w+)>", name)
        if m:
            seen["render_kernel_x"] += 1
            assert spill <= PARENT_X_SPILLS.get(name, 0), f"{name}: {vgpr} VGPRs, {spill} spilled, {scratch} B scratch (the parent: {PARENT_X_SPILLS.get(name, 0)})"
    assert seen == {"render_kernel": 4, "render_kernel_x": 60}, seen


def test_library_still_holds_240_render_kernels_and_binds_the_new_entry_points():
    built = {isa_id.normalise(k) for k in isa_id.kernel_ids(_lib.LIB_PATH)}
    assert len({k for k in built if k.startswith("render_kernel")}) == 240
    assert any("film_from_acc_weighted_kernel" in k for k in built) and any("filter_index_kernel" in k for k in built)
    l = _lib.lib()
    for name in ("pbrt_hip_filter_table", "pbrt_hip_film_from_acc_weighted", "pbrt_hip_filter_footprint_eval_device"):
        assert name in _lib.SYMBOLS and hasattr(l, name)
    assert b"0.9" in l.pbrt_hip_version()
    assert callable(pbrt_amd.filter_table) and pbrt_amd.film_from_acc(np.zeros((1, 4), np.int64), weighted=True).shape == (1, 4)
