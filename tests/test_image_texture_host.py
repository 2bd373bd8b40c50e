"""Image textures for Kd without a GPU: the host run of csrc/image_lookup.hpp against the float64 restatement of
tests/image_ref.py, the identity with the checkerboard, every refusal of scene creation, the parser and the loader, and the register budgets
of the TEX instantiations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import _lib, api, isa_id, loader, scenes

import image_ref as ref
from image_ref import BILINEAR, BLACK, CLAMP, POINT, REPEAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAPS = (REPEAT, CLAMP, BLACK)


def _images():
    return [ref.random_image(w, h, 100 + k) for k, (w, h) in enumerate(ref.SIZES)]


def _host(img, wrap, filt, mapping, uv):
    return api.image_lookup_eval_host([(img, wrap, filt, mapping)], 0, uv)


# ---- the host hook against float64 ----

def test_point_lookup_on_dyadic_inputs_is_exact():
    """(u, v) on the 2^-10 grid of [-3, 3]^2, identity mapping: every step is exact in fp32, so the texel is the restatement's for every input"""
    uv = ref.dyadic_inputs()
    ident = (1.0, 1.0, 0.0, 0.0)
    for img in _images():
        for wrap in WRAPS:
            got = _host(img, wrap, POINT, ident, uv)
            want = ref.point(img, wrap, *ref.mapped64(uv, ident)).astype(np.float32)
            bad = (got != want).any(-1)
            assert not bad.any(), (img.shape, wrap, int(bad.sum()), uv[bad][:4], got[bad][:2], want[bad][:2])


def test_point_lookup_on_random_inputs():
    """random (u, v) and mappings: the restatement's texel wherever float64's s W and t H are not within 1e-5 max(1, |.|) of an integer; the
    excluded share stays under 1 % (the restatement alone says so)"""
    worst_excluded = 0.0
    for k, img in enumerate(_images()):
        H, W = img.shape[:2]
        for wrap in WRAPS:
            uv, mapping = ref.random_inputs(200_000, 7 * k + wrap)
            s, t = ref.mapped64(uv, mapping)
            excluded = ref.near_integer(s * W) | ref.near_integer(t * H)
            worst_excluded = max(worst_excluded, excluded.mean())
            assert excluded.mean() < 0.01, (img.shape, wrap, excluded.mean())
            got = _host(img, wrap, POINT, mapping, uv)
            want = ref.point(img, wrap, s, t).astype(np.float32)
            bad = (got != want).any(-1) & ~excluded
            assert not bad.any(), (img.shape, wrap, mapping, int(bad.sum()), uv[bad][:4])
    print(f"point, random inputs: largest excluded share {worst_excluded:.5f}")


def _bilinear_ratio(img, wrap, uv, mapping, exclude_border):
    """largest |host - float64| / bound over the inputs, the bound per input (8 + 4 |s W| + 4 |t H|) 2^-24 max texel; the float64 reference
    takes the fp32 (s, t) as exact.  Bilinear is continuous: nothing is excluded, but for black, where random inputs within 1e-5 of the image's
    border are (dyadic inputs are exact, the border's own included)"""
    H, W = img.shape[:2]
    s32, t32 = ref.mapped32(uv, mapping)
    s, t = s32.astype(np.float64), t32.astype(np.float64)
    keep = np.ones(len(uv), bool)
    if wrap == BLACK and exclude_border:  # the image's border: within 1e-5 of s W = 0 or W, t H = 0 or H
        keep = ~((np.abs(s * W) <= 1e-5) | (np.abs(s * W - W) <= 1e-5) | (np.abs(t * H) <= 1e-5) | (np.abs(t * H - H) <= 1e-5))
        assert (~keep).mean() < 0.01
    got = _host(img, wrap, BILINEAR, mapping, uv).astype(np.float64)
    want = ref.bilinear(img, wrap, s, t)
    bound = (8.0 + 4.0 * np.abs(s * W) + 4.0 * np.abs(t * H)) * 2.0 ** -24 * float(img.max())
    ratio = np.abs(got - want).max(-1) / bound
    return float(ratio[keep].max())


def test_bilinear_lookup_against_float64():
    worst = 0.0
    for k, img in enumerate(_images()):
        for wrap in WRAPS:
            for random, (uv, mapping) in enumerate(((ref.dyadic_inputs(rows=9), (1.0, 1.0, 0.0, 0.0)), ref.random_inputs(100_000, 1000 + 7 * k + wrap))):
                r = _bilinear_ratio(img, wrap, uv, mapping, exclude_border=bool(random))
                worst = max(worst, r)
                assert r <= 1.0, (img.shape, wrap, mapping, r)
    print(f"bilinear: largest measured error / bound {worst:.4f}")


def test_non_finite_inputs_have_defined_texels():
    """NaN, +-inf, +-1e30 in u, in v, in both: the texel 3.20 states (the restatement follows its text), finite, and for the point lookup the
    cases spelled out"""
    uv = ref.non_finite_inputs()
    ident = (1.0, 1.0, 0.0, 0.0)
    for img in _images():
        H, W = img.shape[:2]
        for wrap in WRAPS:
            s, t = (x.astype(np.float64) for x in ref.mapped32(uv, ident))
            got = _host(img, wrap, POINT, ident, uv)
            assert np.isfinite(got).all() and np.array_equal(got, ref.point(img, wrap, s, t).astype(np.float32)), (img.shape, wrap)
            gb = _host(img, wrap, BILINEAR, ident, uv)
            wb = ref.bilinear(img, wrap, s, t)
            assert np.isfinite(gb).all() and np.abs(gb - wb).max() <= 16 * 2.0 ** -24, (img.shape, wrap, np.abs(gb - wb).max())
        row = H - 1 - min(int(np.floor(np.float32(0.3) * H)), H - 1)  # v = 0.3: a texel row counted from the bottom
        for k, x in enumerate(ref.NON_FINITE):  # rows 0 .. 4 of the inputs: u = x, v = 0.3
            assert np.array_equal(_host(img, REPEAT, POINT, ident, uv)[k], img[row, 0]), x  # NaN, inf - inf, 1e30 - 1e30 = 0: column 0
            assert np.array_equal(_host(img, CLAMP, POINT, ident, uv)[k], img[row, W - 1 if x > 0 else 0]), x
            assert np.array_equal(_host(img, BLACK, POINT, ident, uv)[k], np.zeros(3, np.float32)), x


def test_two_records_share_one_pool():
    """the hook packs every record it is given into one pool: the second record's texels sit behind the first's"""
    a, b = ref.random_image(3, 5, 1), ref.random_image(17, 4, 2)
    uv, mapping = ref.random_inputs(5000, 3)
    recs = [(a, REPEAT, POINT, mapping), (b, CLAMP, BILINEAR, mapping)]
    assert np.array_equal(api.image_lookup_eval_host(recs, 0, uv), _host(a, REPEAT, POINT, mapping, uv))
    assert np.array_equal(api.image_lookup_eval_host(recs, 1, uv), _host(b, CLAMP, BILINEAR, mapping, uv))


# ---- a point-sampled 2 x 2 image is the checkerboard ----

def _checker_colour(tex, uv):
    """the checkerboard's colour as tests/util.py checker_plane_scene states it, in the kernel's fp32: tex1 where floor(s) + floor(t) is even"""
    t = np.asarray(tex, np.float32)
    s, tt = ref.mapped32(uv, t[7:11])
    cell = np.floor(s) + np.floor(tt)
    even = (cell - np.float32(2) * np.floor(np.float32(0.5) * cell)) == 0
    return np.where(even[:, None], t[1:4], t[4:7]).astype(np.float32)


def test_point_sampled_2x2_image_is_the_checkerboard():
    rng = np.random.default_rng(11)
    n_small = 0
    for batch in range(20):
        uv = rng.uniform(-4, 4, (50_000, 2)).astype(np.float32)
        tex = np.concatenate([[0], rng.uniform(0.05, 0.95, 6), rng.uniform(-9, 9, 2), rng.uniform(-2, 2, 2)]).astype(np.float32)
        if batch >= 16:  # s' = s / 2 in (-0.5, 0) for most inputs: a tiny negative s, whose s' - floor(s') rounds to 1
            tex[7:9] = rng.uniform(-1e-3, 1e-3, 2)
            tex[9:11] = rng.uniform(-1e-7, 1e-7, 2)
        img, mapping = ref.checker_as_image(tex)
        s, t = ref.mapped32(uv, mapping)
        n_small += int(((s > -0.5) & (s < 0)).sum() + ((t > -0.5) & (t < 0)).sum())
        got = _host(img, REPEAT, POINT, mapping, uv)
        want = _checker_colour(tex, uv)
        bad = (got != want).any(-1)
        assert not bad.any(), (batch, tex, int(bad.sum()), uv[bad][:4])
    assert n_small > 100_000  # the interval where the reduction rounds was visited


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


def _record(desc, slot=0):
    return _lib.ImageTexture.from_address(C.addressof(desc.textures.contents) + slot * C.sizeof(_lib.Texture))


def _plane(images=None, rows=None, **kw):
    from util import checker_plane_scene
    sd, _ = checker_plane_scene(8)
    sd.images = [ref.random_image(4, 3, 5)] if images is None else images
    sd.textures = np.array([api.image_texture_row(0, "clamp", "bilinear", (2.0, 3.0, 0.25, -0.5))] if rows is None else rows, np.float32)
    for k, v in kw.items():
        setattr(sd, k, v)
    return sd.normalized()


def test_validation():
    no_device = -2 if pbrt_amd.device_count() == 0 else 0
    desc, keep = _desc(_plane())
    r = _record(desc)
    assert desc.n_textures == 1 and (r.type, r.width, r.height, r.wrap, r.filter) == (4, 4, 3, 1, 1) and (r.su, r.sv, r.du, r.dv) == (2.0, 3.0, 0.25, -0.5)
    assert _create_desc(desc)[0] == no_device  # a valid description is stopped by the missing device alone, if it is missing

    def refused(mutate, status, sd=None):
        desc, keep = _desc(sd if sd is not None else _plane())
        mutate(desc)
        code, msg = _create_desc(desc)
        assert code == status and "image" in msg, (code, msg)
        return msg

    def setf(name, value, slot=0):
        return lambda desc: setattr(_record(desc, slot), name, value)

    refused(setf("width", 0), -1)
    refused(setf("height", 0), -1)
    refused(setf("rgb", C.POINTER(C.c_float)()), -1)
    refused(setf("wrap", 3), -1)
    refused(setf("filter", 2), -1)
    for name in ("su", "sv", "du", "dv"):
        for bad in (np.nan, np.inf):
            refused(setf(name, bad), -1)
    for bad in (np.nan, np.inf, -np.inf, -1e-3):
        im = ref.random_image(4, 3, 5)
        im[1, 2, 1] = bad
        assert "texel 6" in refused(lambda d: None, -1, _plane(images=[im]))
    # the caps, refused before a texel is read (the 12 texels behind rgb are all there is)
    refused(setf("width", 16385), -4)
    refused(setf("height", 16385), -4)
    refused(lambda d: (setf("width", 16384)(d), setf("height", 4097)(d)), -4)  # one image above 2^26 texels
    two = _plane(images=[ref.random_image(4, 3, 5)] * 2, rows=[api.image_texture_row(0), api.image_texture_row(1)])
    refused(lambda d: (setf("width", 8192)(d), setf("height", 4096)(d), setf("width", 8192, 1)(d), setf("height", 4097, 1)(d)), -4, two)  # together
    many = _plane(images=[ref.random_image(2, 2, 5)] * 65, rows=[api.image_texture_row(k) for k in range(65)])
    assert "64" in refused(lambda d: None, -4, many)
    assert _create_desc(_desc(_plane(images=[ref.random_image(2, 2, 5)] * 64, rows=[api.image_texture_row(k) for k in range(64)]))[0])[0] == no_device
    # tri_uv missing for a textured triangle, as for the checkerboard
    desc, keep = _desc(_plane())
    desc.tri_uv = C.POINTER(C.c_float)()
    code, msg = _create_desc(desc)
    assert code == -1 and "tri_uv" in msg
    # the hooks validate like the library
    with pytest.raises(_lib.PbrtHipError) as e:
        api.image_lookup_eval_host([(np.full((2, 2, 3), -1.0, np.float32), REPEAT, POINT, (1, 1, 0, 0))], 0, np.zeros((1, 2)))
    assert e.value.code == -1 and "image" in str(e.value)
    with pytest.raises(_lib.PbrtHipError) as e:
        api.image_lookup_eval_host([(ref.random_image(2, 2, 1), 7, POINT, (1, 1, 0, 0))], 0, np.zeros((1, 2)))
    assert e.value.code == -1 and "image" in str(e.value)
    assert b"0.10" in _lib.lib().pbrt_hip_version()


def test_image_slot_beside_every_other_record():
    """a type-4 slot beside a checkerboard, a map, a pixel filter and the normals' record: every slot keeps its meaning, and a kd_tex that
    names one of the other records stays PBRT_HIP_ERR_INVALID"""
    from pbrt_amd.api import LIGHT_ENVMAP
    no_device = -2 if pbrt_amd.device_count() == 0 else 0
    sd = _plane(rows=[[0, .1, .2, .3, .8, .7, .6, 7, 7, .25, -.5], api.image_texture_row(0, "black", "point", (1.5, 2.5, 0.0, 0.5))])
    sd.mat_tex = np.array([2], np.uint32)
    sd.lights = np.array([[LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32)
    sd.envmap = ref.random_image(8, 4, 9)
    sd.pixel_filter = ("gaussian",)
    sd.tri_n = np.tile(np.array([0, 0, 1], np.float32), (len(sd.idx), 3))
    desc, keep = _desc(sd)
    assert [desc.textures[k].type for k in range(desc.n_textures)] == [0, 4, 1, 3, 2]
    r = _record(desc, 1)
    assert (r.width, r.height, r.wrap, r.filter, r.su, r.dv) == (4, 3, 2, 0, 1.5, 0.5)
    assert desc.textures[0].su == 7.0 and desc.mats[0].kd_tex == 2
    assert _create_desc(desc)[0] == no_device
    for other in (3, 4, 5):  # the map, the filter, the normals
        desc, keep = _desc(sd)
        desc.mats[0].kd_tex = other
        assert _create_desc(desc)[0] == -1
    desc, keep = _desc(sd)
    desc.mats[0].kd_tex = 1  # the checkerboard beside the image
    assert _create_desc(desc)[0] == no_device


def test_image_record_is_one_texture_slot(tmp_path):
    import subprocess
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbrt_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",sizeof(pbrt_hip_image_texture),'
                   "sizeof(pbrt_hip_texture),offsetof(pbrt_hip_image_texture,rgb),offsetof(pbrt_hip_image_texture,su),offsetof(pbrt_hip_image_texture,filter));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = _lib.ImageTexture
    assert sizes == [64, 64, T.rgb.offset, T.su.offset, T.filter.offset] and C.sizeof(T) == 64


# ---- the parser and the loader ----

def _srgb_inverse(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def _scene_text(texture_line, material='Material "matte" "texture Kd" "wood"'):
    return ('Camera "perspective" "float fov" 40\nWorldBegin\n' + texture_line + "\n" + material + "\n"
            'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0] "float st" [0 0 1 0 1 1 0 1]\nWorldEnd\n')


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_parser_reads_image_maps(tmp_path):
    rng = np.random.default_rng(5)
    img = rng.uniform(0.0, 1.0, (5, 7, 3)).astype(np.float32)  # H = 5, W = 7
    os.makedirs(tmp_path / "tex")
    api.write_image(str(tmp_path / "tex" / "wood.pfm"), img)
    api.write_image(str(tmp_path / "tex" / "wood.png"), img)
    png = api.read_image(str(tmp_path / "tex" / "wood.png"))  # 8-bit: byte / 255
    assert png.shape == (5, 7, 3) and np.array_equal(api.read_image(str(tmp_path / "tex" / "wood.pfm")), img)
    base = str(tmp_path)

    def load(params, name="tex/wood.pfm", **kw):
        ls = loader.load_string(_scene_text(f'Texture "wood" "spectrum" "imagemap" "string filename" "{name}" {params}', **kw), base_dir=base)
        return ls, ls.scene

    # the defaults: repeat, bilinear, identity mapping, no gamma for a .pfm; a relative name resolves against the scene's directory
    ls, sd = load("")
    assert ls.warnings == [] and len(sd.images) == 1 and np.array_equal(sd.images[0], img)
    assert sd.textures.tolist() == [[4, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0]] and sd.mat_tex.tolist() == [1] and sd.tri_uv.shape == (2, 6)
    np.testing.assert_allclose(sd.materials[0, 1:4], img.astype(np.float64).mean((0, 1)), rtol=1e-6)  # k = the mean colour
    assert np.array_equal(load("", name=str(tmp_path / "tex" / "wood.pfm"))[1].images[0], img)  # an absolute name
    # wrap, filter, mapping, scale
    for wrap, code in (("repeat", 0), ("clamp", 1), ("black", 2)):
        for filt, fcode in (("bilinear", 1), ("point", 0)):
            ls, sd = load(f'"string wrap" "{wrap}" "string filter" "{filt}" "float uscale" 2 "float vscale" 3 "float udelta" 0.25 "float vdelta" -0.5')
            assert ls.warnings == [] and sd.textures.tolist() == [[4, 0, code, fcode, 0, 0, 0, 2, 3, 0.25, -0.5]]
    ls, sd = load('"float scale" 0.5')
    assert np.array_equal(sd.images[0], img * np.float32(0.5))
    # gamma: default on for .png, off for .pfm; pbrt-v3's InverseGammaCorrect against numpy's own, to 1 ulp
    ls, sd = load("", name="tex/wood.png")
    assert ls.warnings == [] and _ulps(sd.images[0], _srgb_inverse(png).astype(np.float32)).max() <= 1
    assert np.array_equal(load('"bool gamma" "false"', name="tex/wood.png")[1].images[0], png)
    assert _ulps(load('"bool gamma" "true"')[1].images[0], _srgb_inverse(img).astype(np.float32)).max() <= 1
    ls, sd = load('"bool gamma" "true" "float scale" 2', name="tex/wood.png")
    assert _ulps(sd.images[0], _srgb_inverse(png).astype(np.float32) * np.float32(2)).max() <= 2  # (1 ulp of the power, doubled exactly: <= 1; kept loose by one)
    # mip-map parameters: read, one warning
    ls, sd = load('"bool trilinear" "true" "float maxanisotropy" 8')
    assert len(ls.warnings) == 1 and "mip map" in ls.warnings[0] and len(sd.images) == 1
    # a parameter other than a matte Kd gets the mean colour
    ls, sd = load("", material='Material "mirror" "texture Kr" "wood"')
    np.testing.assert_allclose(sd.materials[0, 1:4], img.astype(np.float64).mean((0, 1)), rtol=1e-6)
    assert sd.mat_tex.tolist() == [0]
    # fallbacks: a warning that holds "imagemap", never an error
    ls, sd = load("", name="tex/missing.png")
    assert len(ls.warnings) == 1 and "imagemap" in ls.warnings[0] and len(sd.images) == 0 and sd.mat_tex.tolist() == [0]
    assert sd.materials[0, 1:4].tolist() == [0.5, 0.5, 0.5]
    ls, sd = load('"string mapping" "spherical"')
    assert len(ls.warnings) == 1 and "imagemap" in ls.warnings[0] and "mean" in ls.warnings[0] and len(sd.images) == 0
    np.testing.assert_allclose(sd.materials[0, 1:4], img.astype(np.float64).mean((0, 1)), rtol=1e-6)
    bad = img.copy()
    bad[2, 3, 1] = -1.0
    api.write_image(str(tmp_path / "tex" / "bad.pfm"), bad)
    ls, sd = load("", name="tex/bad.pfm")
    assert len(ls.warnings) == 1 and "imagemap" in ls.warnings[0] and sd.materials[0, 1:4].tolist() == [0.5, 0.5, 0.5]
    # two images and a checkerboard keep their slots
    text = ('WorldBegin\nTexture "a" "spectrum" "imagemap" "string filename" "tex/wood.pfm"\nTexture "c" "spectrum" "checkerboard" "string aamode" "none"\n'
            'Texture "b" "spectrum" "imagemap" "string filename" "tex/wood.png" "string filter" "point"\n'
            'Material "matte" "texture Kd" "b"\nShape "sphere"\nMaterial "matte" "texture Kd" "c"\nShape "sphere"\nMaterial "matte" "texture Kd" "a"\nShape "sphere"\nWorldEnd')
    ls = loader.load_string(text, base_dir=base)
    sd = ls.scene
    assert ls.warnings == [] and sd.textures[:, 0].tolist() == [4, 0, 4] and sd.textures[:, 1].tolist()[::2] == [0, 1] and sd.mat_tex.tolist() == [3, 2, 1]
    assert np.array_equal(sd.images[0], img) and sd.images[1].shape == (5, 7, 3)
    desc, keep = _desc(sd)  # ... and the loaded scene is one the library takes
    assert _create_desc(desc)[0] == (-2 if pbrt_amd.device_count() == 0 else 0)


def test_demo_scene_loads():
    ls = loader.load_file(os.path.join(ROOT, "scenes", "textured_cornell.pbrt"))
    assert ls.warnings == [] and len(ls.scene.images) >= 1 and (ls.scene.textures[:, 0] == 4).any() and ls.scene.mat_tex.max() > 0
    im = ls.scene.images[0]
    assert im.std() > 0.05  # a pattern, not a flat colour
    sd = scenes.image_plane_scene(16)
    assert len(sd.images) == 1 and sd.textures[0, 0] == 4
    assert _create_desc(_desc(sd)[0])[0] == (-2 if pbrt_amd.device_count() == 0 else 0)


# ---- register budgets ----

def test_tex_instantiations_hold_their_register_budget():
    """every TEX instantiation of the three families that have the switch spills nothing, uses no scratch and stays within the VGPRs of its
    row of the variant table (512 per SIMD lane, handed out in granules of 8): 96 at 5 waves, 128 at 4, 168 at 3"""
    import render_variant_table
    syms = sorted(isa_id.kernel_ids_by_symbol(_lib.LIB_PATH))
    names = [isa_id.normalise(d) for d in isa_id._demangle(syms)]
    seen = {"x": 0, "env": 0, "n": 0}
    budgets = set()
    for n, s in zip(names, syms):
        m = re.fullmatch(r"render_kernel_(x|env|n)<(.*)>", n)
        if not m:
            continue
        fam, a = m.group(1), [x == "true" for x in m.group(2).split(",")]
        # template switches: x <SPH, STACK, MIS, TEX, SND, WIDE, GLS>, env <SPH, STACK, MIS, TEX, SND>, n <SPH, STACK, MIS, TEX, SND, ENV>
        if not a[3]:
            continue
        switches = dict(spheres=a[0], textured=True)
        if fam == "x":
            switches["glass"] = a[6]
        waves = render_variant_table.waves_per_simd(fam, **switches)
        budget = (512 // waves) // 8 * 8
        budgets.add(budget)
        r = isa_id.kernel_resources(_lib.LIB_PATH, s)
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
        assert r["vgpr_count"] + (r["agpr_count"] or 0) <= budget, (n, r, budget)
        seen[fam] += 1
    assert seen == {"x": 64, "env": 16, "n": 32} and budgets == {96, 128, 168}, (seen, budgets)
