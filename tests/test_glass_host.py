"""The glass material without a GPU: the parser, the validation of pbrt_hip_scene_create, the GLS instantiations of the
code object, and the independent reference (tests/independent_mc_glass.py) against itself."""
import os
import re

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import GLASS, MATTE, _lib, isa_id, loader, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = """
LookAt 0 -4 1  0 0 0  0 0 1
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" [16] "integer yresolution" [16]
WorldBegin
LightSource "infinite" "rgb L" [1 1 1]
"""
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0]\n'


def _glass_rows(sd):
    """[(Kr, Kt, eta)] of the glass materials of a loaded scene"""
    assert len(sd.mat_eta) == (len(sd.materials) if (sd.materials[:, 0] == GLASS).any() else 0)
    return [(tuple(m[1:4]), tuple(m[4:7]), float(sd.mat_eta[i])) for i, m in enumerate(sd.materials) if int(m[0]) == GLASS]


def test_parser_reads_glass():
    f32 = lambda *v: tuple(np.float32(x) for x in v)
    ls = loader.load_string(HEAD + 'Material "glass" "float index" 1.33 "rgb Kr" [.9 .8 .7] "rgb Kt" [.6 .5 .4]\n' + QUAD + "WorldEnd\n")
    assert _glass_rows(ls.scene) == [(f32(.9, .8, .7), f32(.6, .5, .4), float(np.float32(1.33)))]
    assert ls.scene.mat_tex.tolist() == [0] and not ls.warnings, ls.warnings
    # the same through MakeNamedMaterial, with pbrt-v3's other name of the index
    ls = loader.load_string(HEAD + 'MakeNamedMaterial "g" "string type" "glass" "float eta" 1.33 "rgb Kr" [.9 .8 .7] "rgb Kt" [.6 .5 .4]\n'
                            'NamedMaterial "g"\n' + QUAD + "WorldEnd\n")
    assert _glass_rows(ls.scene) == [(f32(.9, .8, .7), f32(.6, .5, .4), float(np.float32(1.33)))]
    assert not [w for w in ls.warnings if "not supported" in w], ls.warnings
    # the defaults: Kr = Kt = 1, index 1.5; also on a sphere
    ls = loader.load_string(HEAD + 'Material "glass"\n' + QUAD + 'Shape "sphere" "float radius" 0.5\nWorldEnd\n')
    assert _glass_rows(ls.scene) == [(f32(1, 1, 1), f32(1, 1, 1), 1.5)] and int(ls.scene.spheres[0, 4]) == 0 and not ls.warnings
    # what smooth glass drops is said, by name
    for param, name in (('"float uroughness" 0.1', "uroughness"), ('"float vroughness" 0.2', "vroughness"), ('"texture bumpmap" "b"', "bumpmap"),
                        ('"bool remaproughness" "false"', "remaproughness")):
        ls = loader.load_string(HEAD + 'Texture "b" "float" "constant" "float value" 1\nMaterial "glass" ' + param + "\n" + QUAD + "WorldEnd\n")
        assert [w for w in ls.warnings if name in w and "glass" in w], (name, ls.warnings)
        assert not [w for w in ls.warnings if "not supported by this path" in w], ls.warnings
        assert len(_glass_rows(ls.scene)) == 1
    ls = loader.load_string(HEAD + 'Material "glass" "float uroughness" 0 "float vroughness" 0\n' + QUAD + "WorldEnd\n")
    assert not ls.warnings, ls.warnings
    # two glasses that differ only in eta stay two materials; equal ones merge
    ls = loader.load_string(HEAD + 'Material "glass" "float index" 1.5\n' + QUAD + 'Material "glass" "float index" 1.6\n' + QUAD +
                            'Material "glass" "float index" 1.5\n' + QUAD + "WorldEnd\n")
    assert [r[2] for r in _glass_rows(ls.scene)] == [1.5, float(np.float32(1.6))] and ls.scene.mat_id.tolist() == [0, 0, 1, 1, 0, 0]
    # glass under an area light: the shape emits, as black matte, and the parser says so
    ls = loader.load_string(HEAD + 'AreaLightSource "diffuse" "rgb L" [3 2 1]\nMaterial "glass"\n' + QUAD + "WorldEnd\n")
    assert ls.scene.materials.tolist() == [[MATTE, 0, 0, 0, 3, 2, 1]] and [w for w in ls.warnings if "glass" in w and "AreaLightSource" in w]
    # another unsupported material still falls back to matte with the warning
    ls = loader.load_string(HEAD + 'Material "metal"\n' + QUAD + "WorldEnd\n")
    assert [w for w in ls.warnings if "not supported" in w] and int(ls.scene.materials[0, 0]) == MATTE


def test_scene_file_equals_the_generator():
    """scenes/glass_sphere.pbrt loads to the arrays scenes.glass_sphere_scene builds (tests/test_glass_gpu.py compares their films)"""
    ls = loader.load_file(os.path.join(ROOT, "scenes", "glass_sphere.pbrt"))
    sd = scenes.glass_sphere_scene(256, 256)
    assert not ls.warnings, ls.warnings
    for f in ("P", "idx", "mat_id", "materials", "lights", "spheres", "cam_to_world", "mat_tex", "tri_uv", "textures"):
        a, b = getattr(ls.scene, f), getattr(sd, f)
        assert a.shape == b.shape and np.array_equal(a, b), f  # (by value: the parser's camera matrix has a +0 where look_at gives -0)
    glass = sd.materials[:, 0] == GLASS
    assert glass.sum() == 2 and np.array_equal(ls.scene.mat_eta[glass], sd.mat_eta[glass])
    assert (ls.scene.fov, ls.scene.xres, ls.scene.yres, ls.max_depth) == (40.0, 256, 256, 8)


def _create(sd):
    try:
        pbrt_amd.Scene(sd).close()
    except _lib.PbrtHipError as e:
        return e.code, str(e)
    return 0, ""


def test_glass_is_validated_before_any_device_work():
    def scene(row=None, eta=None, mtype=None):
        sd = scenes.glass_sphere_scene(8, 8)
        m = sd.materials.copy()
        if row is not None:
            m[5, row[0]] = row[1]
        if mtype is not None:
            m[5, 0] = mtype
        sd.materials = m
        if eta is not None:
            sd.mat_eta = sd.mat_eta.copy()
            sd.mat_eta[5] = eta
        return sd
    for kw in (dict(eta=np.nan), dict(eta=0.5), dict(eta=np.inf), dict(eta=16.5), dict(row=(4, -1.0)), dict(row=(1, np.inf)), dict(row=(5, np.nan)),
               dict(row=(2, -0.5))):
        code, msg = _create(scene(**kw))
        assert code == -1 and "glass" in msg, (kw, code, msg)
    code, msg = _create(scene(mtype=3))
    assert code == -1 and "unknown material type" in msg, (code, msg)
    # a valid glass scene (eta = 1 and 16, the ends, included) passes the validation: what stops it is the missing device, if it is missing
    for eta in (None, 1.0, 16.0):
        code, msg = _create(scene(eta=eta))
        assert code == (0 if pbrt_amd.device_count() > 0 else -2), (eta, code, msg)
    assert b"0.6" in _lib.lib().pbrt_hip_version()


def test_glass_instantiations_hold_their_register_budget():
    """render_kernel_x<..., GLS = true> exists for both stack variants, with and without spheres, spills nothing and uses no scratch, and
    fits the 3 waves per SIMD that DESIGN.md 3.16 states (512 VGPRs per SIMD lane on gfx950, handed out in granules of 8: 168 at 3 waves)."""
    syms = sorted(isa_id.kernel_ids_by_symbol(_lib.LIB_PATH))
    names = [isa_id.normalise(d) for d in isa_id._demangle(syms)]
    gls = [(n, s) for n, s in zip(names, syms) if re.fullmatch(r"render_kernel_x<(true|false),\d+,(true|false),(true|false),(true|false),(true|false),true>", n)]
    assert len(gls) == 64, len(gls)  # SPH x STACK x MIS x TEX x SND x WIDE
    import render_variant_table
    waves = render_variant_table.waves_per_simd("x", glass=True)  # (render_variant.hpp)
    budget = (512 // waves) // 8 * 8
    assert budget == 168
    for stack in ("0", "30"):
        assert [n for n, _ in gls if n.split(",")[1] == stack], stack
    for n, s in gls:
        r = isa_id.kernel_resources(_lib.LIB_PATH, s)
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
        assert r["vgpr_count"] + (r["agpr_count"] or 0) <= budget, (n, r, budget)
    # and no instantiation without glass changed its name: the scenes without glass run what they ran
    assert len([n for n in names if n.startswith("render_kernel_x<") and n.endswith(",false>")]) == 52


def test_reference_checks_itself():
    """tests/independent_mc_glass.py against closed forms and against itself (no product involved); fixes its path counts."""
    import independent_mc_glass as g
    for eta in (1.33, 1.5, 2.4):
        r0 = ((eta - 1) / (eta + 1)) ** 2
        assert abs(g.fr_dielectric(1.0, 1.0, eta) - r0) < 1e-12 and abs(g.fr_dielectric(1.0, eta, 1.0) - r0) < 1e-12
        cos_c = np.sqrt(1 - 1 / eta ** 2)  # the critical angle, from inside
        assert np.all(np.abs(g.fr_dielectric(np.linspace(0, cos_c - 1e-9, 50), eta, 1.0) - 1.0) < 1e-12)
        assert g.fr_dielectric(cos_c + 1e-3, eta, 1.0) < 1.0
        assert abs(g.fr_dielectric(0.0, 1.0, eta) - 1.0) < 1e-12  # grazing
    assert np.all(g.fr_dielectric(np.linspace(0.01, 1, 30), 1.0, 1.0) < 1e-24)  # index-matched
    # the furnace: the environment's radiance comes back, within 5 of the reference's own standard errors, in every block
    for kind in ("sphere", "cube"):
        for eta in (1.5, 2.4):
            mean, se, cnt = g.furnace_block_means(kind, eta)
            assert cnt.min() > 0.5 * g.FURNACE_PATHS / cnt.size and (se > 0).any()  # (the object is in the frame)
            z = np.abs(mean - g.ENV) / np.where(se > 0, se, 1.0)
            assert np.all(np.where(se > 0, z, np.abs(mean - g.ENV) / g.ENV / 1e-9) < 5.0), (kind, eta, float(z.max()))
    # two runs of the box with different seeds agree block by block within the bar the GPU test holds the library to
    m1, s1 = g.block_means(64, 64, 8, g.BOX_DEPTH, g.BOX_PATHS, seed=12345)
    m2, s2 = g.block_means(64, 64, 8, g.BOX_DEPTH, g.BOX_PATHS, seed=54321)
    z = np.abs(m1 - m2) / (np.sqrt(s1 ** 2 + s2 ** 2) + 0.004 * np.abs(m1))
    assert z.max() < 5.0 and abs(m1.sum() / m2.sum() - 1) < 6e-3, (float(z.max()), m1.sum() / m2.sum() - 1)
    assert (s1 / m1).max() < 0.05  # the blocks are resolved: the bar is a few per cent everywhere
    # the glass is what the comparison sees: the reference with eta 1.3 is told from the one with 1.5
    m3, s3 = g.block_means(64, 64, 8, g.BOX_DEPTH, g.BOX_PATHS, seed=12345, eta=1.3)
    assert (np.abs(m1 - m3) / (np.sqrt(s1 ** 2 + s3 ** 2) + 0.004 * np.abs(m1))).max() > 6.0
