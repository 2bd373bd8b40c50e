"""Shading normals without a GPU: the record's layout, the refusals of pbrt_hip_scene_create, the parser and the PLY
reader against float64 of the same transforms, the NRM instantiations of the code object, and tests/normals_ref.py against itself.
tests/test_normals_gpu.py holds the kernels to that reference."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

import normals_ref as nr
import pbrt_amd
from pbrt_amd import GLASS, _lib, api, isa_id, loader, scenes
from util import lit_plane_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the record ----

def test_normals_record_is_one_texture_slot(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbrt_hip.h"\n#include "pbrt_hip_debug.h"\n'
                   'int main(void){printf("%zu %zu %zu %u\\n",sizeof(pbrt_hip_normals),sizeof(pbrt_hip_texture),offsetof(pbrt_hip_normals,tri_n),'
                   "PBRT_HIP_TEXTURE_NORMALS);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sizes == [64, 64, 16, 2]
    assert C.sizeof(_lib.Normals) == 64 and _lib.Normals.tri_n.offset == 16 and C.sizeof(_lib.Texture) == 64
    version = _lib.lib().pbrt_hip_version()
    assert b"0.8" in version and b"0.6" in version
    assert "pbrt_hip_shading_normal_eval_device" in _lib.SYMBOLS and len(api.BLOCK_OPS) == 15  # a hook of its own, not a 16th block op


def test_scene_data_carries_normals():
    sd = scenes.sphere_scene(8, 8)
    assert sd.tri_n.shape == (0, 9)  # empty by default
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd, _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    assert desc.n_textures == 0 and not desc.textures
    del keep
    # behind the checkerboards and the map
    from util import checker_plane_scene
    sd, _ = checker_plane_scene(8)
    sd.lights = np.array([[api.LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32)
    sd.envmap = np.ones((2, 4, 3), np.float32)
    nr.with_normal(sd, (0, 0, 2))
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd, _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    assert desc.n_textures == 3 and [desc.textures[i].type for i in range(3)] == [0, 1, 2]
    rec = _normals_record(desc)
    assert rec.n_tris == 2 and list(rec.reserved) == [0, 0] and list(rec.pad) == [0] * 10
    assert np.array_equal(np.ctypeslib.as_array(rec.tri_n, shape=(18,)), sd.tri_n.reshape(-1))
    assert _create_desc(desc)[0] == (-2 if pbrt_amd.device_count() == 0 else 0)
    del keep


# ---- validation (pbrt_hip_scene_create, before any device work) ----

def _desc(sd):
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd.normalized(), _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    return desc, keep


def _create_desc(desc, create=None):
    h = C.c_void_p()
    code = (create or (lambda d, out: _lib.lib().pbrt_hip_scene_create(d, -1, out)))(C.byref(desc), C.byref(h))
    msg = _lib.lib().pbrt_hip_last_error().decode()
    if code == 0:
        _lib.lib().pbrt_hip_scene_destroy(h)
    return code, msg


def _normals_record(desc, slot=None):
    """the pbrt_hip_normals that sits in a slot (default: the last) of desc.textures, as a view that writes through"""
    slot = desc.n_textures - 1 if slot is None else slot
    return _lib.Normals.from_address(C.addressof(desc.textures.contents) + slot * C.sizeof(_lib.Texture))


def _small_scene():
    sd, _ = lit_plane_scene("distant", 8)
    return nr.with_normal(sd, nr.tilted(30.0))


def test_validation():
    no_device = -2 if pbrt_amd.device_count() == 0 else 0
    desc, keep = _desc(_small_scene())
    assert desc.n_textures == 1 and desc.textures[0].type == 2
    assert _create_desc(desc)[0] == no_device  # a valid description is stopped by the missing device alone, if it is missing

    def refused(mutate, status, sd=None, create=None):
        desc, keep = _desc(sd if sd is not None else _small_scene())
        more = mutate(desc)
        code, msg = _create_desc(desc, create)
        assert code == status and "normal" in msg, (code, msg)
        del more
        return msg

    def setf(name, value):
        return lambda desc: setattr(_normals_record(desc), name, value)

    refused(setf("n_tris", 1), -1)
    refused(setf("n_tris", 3), -1)
    refused(setf("tri_n", C.POINTER(C.c_float)()), -1)
    for bad in (np.nan, np.inf, -np.inf):
        sd = _small_scene()
        sd.tri_n[1, 4] = bad
        assert "triangle 1" in refused(lambda d: None, -1, sd)
    # every entry point that creates a scene refuses alike, whatever the builder
    for flags in (api.SCENE_GPU_BUILD, api.SCENE_HOST_BUILD, api.SCENE_OPTIMIZED_TREE, api.SCENE_GPU_BUILD | api.SCENE_PLAIN_TREE):
        refused(setf("n_tris", 7), -1, create=lambda d, out, flags=flags: _lib.lib().pbrt_hip_scene_create_ex(d, -1, flags, out))

    def two_records(desc):
        texs = (_lib.Texture * 2)()
        C.memmove(texs, desc.textures, C.sizeof(_lib.Texture))
        C.memmove(C.byref(texs, C.sizeof(_lib.Texture)), desc.textures, C.sizeof(_lib.Texture))
        desc.textures, desc.n_textures = texs, 2
        return texs

    assert "more than one" in refused(two_records, -4)
    # a matte kd_tex that names the record: it is no texture for Kd
    refused(lambda d: setattr(d.mats[0], "kd_tex", 1), -1)
    # zero normals are "none", not an error; a glass material's kd_tex (its eta) is not a texture number
    sd = _small_scene()
    sd.tri_n[:] = 0
    assert _create_desc(_desc(sd)[0])[0] == no_device
    sd = _small_scene()
    sd.materials[0, 0] = GLASS
    assert _create_desc(_desc(sd)[0])[0] == no_device


# ---- parser ----

HEAD = """
LookAt 0 -4 1  0 0 0  0 0 1
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" [16] "integer yresolution" [16]
WorldBegin
"""
P4 = np.array([(-1, -1, 0), (1, -1, 0.25), (1, 1, 0), (-1, 1, 0.5)], np.float64)
N4 = np.array([(0.25, 0, 1), (0, 0.5, 2), (-0.5, 0.25, 0.75), (0, 0, 3)], np.float64)
TRIS = [(0, 1, 2), (0, 2, 3)]


def _fmt(a):
    return " ".join(repr(float(x)) for x in np.asarray(a).reshape(-1))


def _mesh(indices=TRIS, normals=True, extra=""):
    return (f'Shape "trianglemesh" "integer indices" [{" ".join(str(i) for t in indices for i in t)}] "point P" [{_fmt(P4)}] '
            + (f'"normal N" [{_fmt(N4)}] ' if normals else "") + extra + "\n")


def _rodrigues(deg, axis):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _unit_rows(n):
    n = np.asarray(n, np.float64).reshape(-1, 3)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _want(M3, tris, normals=N4):
    """float64: the corner normals of `tris` through the inverse transpose of M3, unit length, (n_tris, 3, 3)"""
    n = np.asarray(normals) @ np.linalg.inv(M3)  # rows: (inv(M)^T n)^T = n^T inv(M)
    return _unit_rows(n[np.asarray(tris).reshape(-1)]).reshape(-1, 3, 3)


def _got(sd):
    return _unit_rows(sd.tri_n).reshape(-1, 3, 3)


M3 = _rodrigues(35.0, (1, 2, 3)) @ np.diag([2.0, 1.0, 0.5])
XFORM = 'Translate 0.5 -1 2 Rotate 35 1 2 3 Scale 2 1 0.5\n'


def test_parser_reads_trianglemesh_normals():
    ls = loader.load_string(HEAD + "AttributeBegin " + XFORM + _mesh() + "AttributeEnd\nWorldEnd\n")
    assert not ls.warnings, ls.warnings
    sd = ls.scene
    assert sd.tri_n.shape == (2, 9) and sd.tri_n.dtype == np.float32
    assert np.allclose(sd.P, P4 @ M3.T + np.array([0.5, -1, 2]), atol=1e-5)  # (the transform is the one this test means)
    assert np.array_equal(sd.idx, np.array(TRIS, np.uint32))
    err = np.abs(_got(sd) - _want(M3, TRIS)).max()
    assert err <= 1e-6, err
    # not normalised: the lengths are the transform's
    assert np.allclose(np.linalg.norm(sd.tri_n[:, :3], axis=1), np.linalg.norm((N4 @ np.linalg.inv(M3))[[0, 0]], axis=1), rtol=1e-6)
    # a wrong count: a warning, and the mesh renders flat (no normals anywhere in the file: no record)
    ls = loader.load_string(HEAD + _mesh(extra="").replace(_fmt(N4), _fmt(N4[:3])) + "WorldEnd\n")
    assert [w for w in ls.warnings if '"N"' in w and "flat" in w], ls.warnings
    assert ls.scene.tri_n.shape == (0, 9)
    # a CTM that swaps handedness turns the winding round and takes the corners' normals with it
    ls = loader.load_string(HEAD + "AttributeBegin Scale 1 -1 1\n" + _mesh() + "AttributeEnd\nWorldEnd\n")
    assert np.array_equal(ls.scene.idx, np.array([(0, 2, 1), (0, 3, 2)], np.uint32))
    assert np.abs(_got(ls.scene) - _want(np.diag([1.0, -1.0, 1.0]), [(0, 2, 1), (0, 3, 2)])).max() <= 1e-6
    # glass ignores its normals: one warning per file, zero rows
    two = 'Material "glass"\n' + _mesh() + _mesh() + 'Material "matte"\n' + _mesh()
    ls = loader.load_string(HEAD + two + "WorldEnd\n")
    assert len([w for w in ls.warnings if "glass" in w and "normals" in w]) == 1, ls.warnings
    assert ls.scene.tri_n.shape == (6, 9) and not ls.scene.tri_n[:4].any() and ls.scene.tri_n[4:].any(axis=1).all()


def _ply(path, fmt, faces, normals=True):
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else [])
    head = ["ply", {"ascii": "format ascii 1.0", "le": "format binary_little_endian 1.0", "be": "format binary_big_endian 1.0"}[fmt],
            f"element vertex {len(P4)}"] + [f"property float {p}" for p in props] + [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    rows = np.concatenate([P4, N4], 1) if normals else P4
    body = b""
    if fmt == "ascii":
        body = "".join(" ".join(repr(float(x)) for x in r) + "\n" for r in rows).encode()
        body += "".join(f"{len(f)} " + " ".join(str(i) for i in f) + "\n" for f in faces).encode()
    else:
        e = "<" if fmt == "le" else ">"
        for r in rows:
            body += struct.pack(e + f"{len(r)}f", *[float(x) for x in r])
        for f in faces:
            body += struct.pack(e + "B" + f"{len(f)}i", len(f), *f)
    path.write_bytes(("\n".join(head) + "\n").encode() + body)


ASK = '"bool shadingnormals" "true"'


def test_ply_normals_in_three_encodings(tmp_path):
    inline = loader.load_string(HEAD + "AttributeBegin " + XFORM + _mesh() + "AttributeEnd\nWorldEnd\n").scene
    for fmt in ("ascii", "le", "be"):
        _ply(tmp_path / f"m_{fmt}.ply", fmt, TRIS)
        ls = loader.load_string(HEAD + "AttributeBegin " + XFORM + f'Shape "plymesh" "string filename" "m_{fmt}.ply" {ASK}\nAttributeEnd\nWorldEnd\n', base_dir=str(tmp_path))
        assert not ls.warnings, ls.warnings
        assert np.array_equal(ls.scene.tri_n, inline.tri_n) and np.array_equal(ls.scene.P, inline.P) and np.array_equal(ls.scene.idx, inline.idx), fmt
    # a quad is split as the positions are: (0 1 2) and (3 0 2)
    _ply(tmp_path / "quad.ply", "le", [(0, 1, 2, 3)])
    ls = loader.load_string(HEAD + "AttributeBegin " + XFORM + f'Shape "plymesh" "string filename" "quad.ply" {ASK}\nAttributeEnd\nWorldEnd\n', base_dir=str(tmp_path))
    assert np.array_equal(ls.scene.idx, np.array([(0, 1, 2), (3, 0, 2)], np.uint32))
    assert np.abs(_got(ls.scene) - _want(M3, [(0, 1, 2), (3, 0, 2)])).max() <= 1e-6
    # a PLY file without nx ny nz: no normals, no record, asked or not
    _ply(tmp_path / "flat.ply", "ascii", TRIS, normals=False)
    ls = loader.load_string(HEAD + f'Shape "plymesh" "string filename" "flat.ply" {ASK}\nWorldEnd\n', base_dir=str(tmp_path))
    assert ls.scene.tri_n.shape == (0, 9) and not ls.warnings
    # the file's normals are used on request only (the oracle, which every scene file's film is held to, does not know them): without
    # "bool shadingnormals" a PLY file renders as it always did
    ls = loader.load_string(HEAD + 'Shape "plymesh" "string filename" "m_le.ply"\nWorldEnd\n', base_dir=str(tmp_path))
    assert ls.scene.tri_n.shape == (0, 9) and not ls.warnings
    ls = loader.load_string(HEAD + 'Shape "plymesh" "string filename" "m_le.ply" "bool shadingnormals" "false"\nWorldEnd\n', base_dir=str(tmp_path))
    assert ls.scene.tri_n.shape == (0, 9) and not ls.warnings


def test_instances_carry_their_normals():
    text = (HEAD + 'ObjectBegin "o"\nRotate 20 0 1 0\n' + _mesh() + "ObjectEnd\n"
            "AttributeBegin Translate 1 2 3 Rotate 50 1 0 0\nObjectInstance \"o\"\nAttributeEnd\n"
            "AttributeBegin Translate -3 0 0 Scale -1 1 2\nObjectInstance \"o\"\nAttributeEnd\nWorldEnd\n")
    ls = loader.load_string(text)
    assert not ls.warnings, ls.warnings
    sd = ls.scene
    assert sd.tri_n.shape == (4, 9)
    own = _rodrigues(20.0, (0, 1, 0))
    moved = _rodrigues(50.0, (1, 0, 0)) @ own
    mirrored = np.diag([-1.0, 1.0, 2.0]) @ own
    assert np.array_equal(sd.idx, np.array([(0, 1, 2), (0, 2, 3), (4, 6, 5), (4, 7, 6)], np.uint32))  # the mirroring instance turns the winding round
    assert np.abs(_got(sd)[:2] - _want(moved, TRIS)).max() <= 1e-6
    assert np.abs(_got(sd)[2:] - _want(mirrored, [(0, 2, 1), (0, 3, 2)])).max() <= 1e-6  # ... and permutes the corner normals with the corners
    # every corner's normal still belongs to its vertex: the geometric normal of the mirrored copy is the transformed one
    Pm = sd.P.astype(np.float64)[sd.idx[2:].astype(int)]
    ng = np.cross(Pm[:, 1] - Pm[:, 0], Pm[:, 2] - Pm[:, 0])
    P0 = sd.P.astype(np.float64)[sd.idx[:2].astype(int)]
    ng0 = np.cross(P0[:, 1] - P0[:, 0], P0[:, 2] - P0[:, 0])
    assert ((_got(sd)[2:, 0] * ng).sum(1) > 0).all() == ((_got(sd)[:2, 0] * ng0).sum(1) > 0).all()


def test_smooth_and_flat_meshes_share_a_file():
    ls = loader.load_string(HEAD + _mesh() + "Translate 0 0 1\n" + _mesh(normals=False) + 'Shape "sphere"\nWorldEnd\n')
    sd = ls.scene
    assert sd.tri_n.shape == (4, 9) and sd.tri_n[:2].any(axis=1).all() and not sd.tri_n[2:].any()
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd, _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    assert desc.n_textures == 1 and _normals_record(desc).n_tris == 4
    assert _create_desc(desc)[0] == (-2 if pbrt_amd.device_count() == 0 else 0)
    del keep


def _raw_desc(text):
    """(n_textures, the types of the slots, tri_uv is NULL) of the description pbrt_hip_loaded_get hands out"""
    l = _lib.lib()
    h = C.c_void_p()
    b = text.encode()
    assert l.pbrt_hip_load_string(b, len(b), None, C.byref(h)) == 0
    try:
        d, r = _lib.SceneDesc(), _lib.RenderDesc()
        assert l.pbrt_hip_loaded_get(h, C.byref(d), C.byref(r), None, 0) == 0
        return d.n_textures, [d.textures[i].type for i in range(d.n_textures)], not d.tri_uv
    finally:
        l.pbrt_hip_loaded_free(h)


def test_a_file_without_normals_keeps_its_description():
    text = HEAD + 'Texture "chk" "spectrum" "checkerboard"\nMaterial "matte" "texture Kd" "chk"\n' + _mesh(normals=False) + "WorldEnd\n"
    assert _raw_desc(text) == (1, [0], False)
    assert loader.load_string(text).scene.tri_n.shape == (0, 9)
    assert _raw_desc(HEAD + _mesh(normals=False) + "WorldEnd\n") == (0, [], True)
    # with normals the record is the last slot
    text = HEAD + 'Texture "chk" "spectrum" "checkerboard"\nMaterial "matte" "texture Kd" "chk"\n' + _mesh() + "WorldEnd\n"
    assert _raw_desc(text) == (2, [0, 2], False)
    ls = loader.load_string(text)
    assert ls.scene.tri_n.shape == (2, 9) and len(ls.scene.textures) == 1 and ls.scene.mat_tex.tolist() == [1]


def test_scene_file_equals_the_generator():
    """scenes/smooth_mesh.pbrt loads to the arrays scenes.smooth_mesh_scene builds (tests/test_normals_gpu.py compares their films)"""
    ls = loader.load_file(os.path.join(ROOT, "scenes", "smooth_mesh.pbrt"))
    assert not ls.warnings, ls.warnings
    sd = scenes.smooth_mesh_scene()
    for f in ("P", "idx", "mat_id", "materials", "lights", "spheres", "cam_to_world", "mat_tex", "textures", "tri_n"):
        assert np.array_equal(getattr(ls.scene, f), getattr(sd, f)), f
    assert (ls.scene.fov, ls.scene.xres, ls.scene.yres) == (sd.fov, sd.xres, sd.yres) and ls.max_depth == 5
    assert not sd.tri_n[:2].any() and sd.tri_n[2:].any(axis=1).all()  # the ground is flat, the octahedra are smooth
    P = sd.P.astype(np.float64)[sd.idx[2:].astype(int)]
    ng = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    assert ((ng * sd.tri_n[2:, :3]).sum(1) > 0).all()  # wound outwards


def test_icosphere_scene():
    for level in (0, 2):
        sd = scenes.icosphere_scene(level, xres=8, yres=8)
        flat = scenes.icosphere_scene(level, smooth=False, xres=8, yres=8)
        assert sd.idx.shape == (20 * 4 ** level, 3) and sd.tri_n.shape == (20 * 4 ** level, 9) and flat.tri_n.shape == (0, 9)
        assert np.array_equal(sd.P, flat.P) and np.array_equal(sd.idx, flat.idx)
        P = sd.P.astype(np.float64)[sd.idx.astype(int)]
        assert np.allclose(np.linalg.norm(P, axis=2), 1.0, atol=1e-6)  # on the sphere
        assert ((np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) * P.mean(1)).sum(1) > 0).all()  # wound outwards
        assert np.array_equal(sd.tri_n.reshape(-1, 3, 3), sd.P[sd.idx.astype(int)])  # p - c with c = 0
    c1 = scenes.sphere_scene(8, 8)
    assert np.array_equal(sd.cam_to_world, c1.cam_to_world) and np.array_equal(sd.lights, c1.lights) and np.array_equal(sd.materials, c1.materials)
    big = scenes.icosphere_scene(1, radius=2.0, centre=(1, 0, 0), xres=8, yres=8)
    assert np.allclose(np.linalg.norm(big.tri_n[:, :3], axis=1), 2.0, rtol=1e-6)  # deliberately not unit length


# ---- the code object ----

def test_nrm_instantiations_hold_their_register_budget():
    """render_kernel_n exists for both stack variants, with and without spheres, MIS, textures, the table samplers and an environment
    map -- 64 kernels in a translation unit of their own --, spills nothing, uses no scratch, and fits the budget render_variant.hpp states."""
    import render_variant_table
    waves = render_variant_table.waves_per_simd("n")
    budget = 512 // waves
    assert budget == 128 and budget % 8 == 0  # 512 VGPRs per SIMD lane on gfx950, handed out in granules of 8: what 4 waves per SIMD leave a wave
    syms = sorted(isa_id.kernel_ids_by_symbol(_lib.LIB_PATH))
    names = [isa_id.normalise(d) for d in isa_id._demangle(syms)]
    nrm = [(n, s) for n, s in zip(names, syms) if re.fullmatch(r"render_kernel_n<(true|false),\d+(,(true|false)){4}>", n)]
    assert len(nrm) == 64 and len(set(n for n, _ in nrm)) == 64, len(nrm)  # SPH x STACK x MIS x TEX x SND x ENV
    for stack in ("0", "30"):
        assert len([n for n, _ in nrm if n.split(",")[1] == stack]) == 32, stack
    counts = isa_id.kernel_definition_counts(_lib.LIB_PATH)
    used = []
    for n, s in nrm:
        r = isa_id.kernel_resources(_lib.LIB_PATH, s)
        assert counts[s] == 1, n
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
        assert r["vgpr_count"] + (r["agpr_count"] or 0) <= budget, (n, r, budget)
        used.append(r["vgpr_count"] + (r["agpr_count"] or 0))
    print(f"render_kernel_n: {min(used)} .. {max(used)} VGPRs + AGPRs, budget {budget}")
    assert [n for n in names if n.startswith("pack_nrm_kernel") or "pack_nrm_kernel" in n] or any("pack_nrm_kernel" in s for s in syms)
    assert any("shading_normal_eval_kernel" in s for s in syms)


# ---- tests/normals_ref.py against itself ----

def test_reference_checks_itself():
    # the hook's input set: float64 alone leaves >= 90 % of the elements robust, and every kind of case is there
    x, kind = nr.hook_inputs()
    assert x.shape == (1 << 16, 17) and x.dtype == np.float32 and np.isfinite(x).all()
    r = nr.shading_normal_f64(x)
    print(f"robust {r['robust'].mean():.4f}, fell back {r['fell_back'].mean():.4f}, flips {r['flip_ng'].mean():.3f} / {r['flip_wo'].mean():.3f}")
    assert r["robust"].mean() >= 0.90
    for k in range(len(nr.KINDS)):
        assert (kind == k).sum() >= 1000, nr.KINDS[k]
    assert r["fell_back"][kind == 2].all() and not r["fell_back"][kind <= 1].any()
    assert 0 < r["fell_back"][kind == 3].sum() < 64  # (one zero corner, hit exactly at that corner: nothing to interpolate)
    assert r["flip_ng"][kind == 1].mean() > 0.9 and r["flip_ng"][kind == 0].mean() < 0.1  # the far side is where the flip applies
    assert 0.4 < r["flip_wo"].mean() < 0.6  # wo on either side
    lens = np.linalg.norm(x[:, :9].reshape(-1, 3, 3).astype(np.float64), axis=2)
    assert lens[kind == 0].min() < 2e-3 and lens.max() > 500  # scaled by 1e-3 .. 1e3
    b1, b2 = x[:, 12].astype(np.float64), x[:, 13].astype(np.float64)
    assert ((b1 == 0) & (b2 == 0)).any() and ((b1 == 1) & (b2 == 0)).any() and ((b1 == 0) & (b2 == 1)).any() and ((b1 + b2 == 1) & (b1 > 0) & (b2 > 0)).any()
    assert np.allclose(np.linalg.norm(r["nsf"], axis=1), 1.0, atol=1e-6)
    assert (((r["nsf"] * x[:, 9:12]).sum(1) > 0) == (r["c_wo"] >= 0))[r["robust"]].all()  # nsf lies on wo's geometric side
    assert r["bound"][r["robust"]].max() < 0.1 and np.median(r["bound"][r["robust"]]) < 1e-6
    # closed forms: equal corner normals of any length give that direction; the fallback gives +-ng exactly
    one = np.zeros((2, 17), np.float32)
    one[:, 0:9] = np.tile([0.0, 3.0, 4.0], 3) * np.array([[1.0], [1e-3]])
    one[:, 9:12], one[:, 12:14], one[0, 14:17], one[1, 14:17] = (0, 0, 1), (0.25, 0.5), (0, 0, 1), (0, 0, -1)
    got = nr.shading_normal_f64(one)
    assert np.allclose(got["nsf"], [[0, 0.6, 0.8], [0, -0.6, -0.8]], atol=1e-15)
    zero = one.copy()
    zero[:, :9] = 0
    got = nr.shading_normal_f64(zero)
    assert got["fell_back"].all() and np.array_equal(got["nsf"], [[0, 0, 1], [0, 0, -1]])
    # the clipped cosine lobe: the closed form against a cosine sampler that knows nothing of it
    for theta in (20.0, 40.0, 70.0):
        p, n = nr.clipped_lobe_fraction(theta), 1 << 22
        assert abs(nr.clipped_lobe_sampled(theta, n) - p) <= 5 * np.sqrt(p * (1 - p) / n), theta
    assert abs(nr.clipped_lobe_fraction(40.0) - 0.88302) < 1e-5 and nr.clipped_lobe_fraction(0.0) == 1.0
    # the lit plane
    sd, want = lit_plane_scene("distant", 8)
    assert np.allclose(nr.lambert_distant(sd.materials[0, 1:4], (3, 2, 1), (0, 0, 1), sd.lights[0, 1:4].astype(np.float64)), want, rtol=1e-7)
    # the camera: the centre ray looks at the look-at point
    o, d = nr.camera_rays(sd, 4.0, 4.0)
    to = np.array([0.2, 0.3, 0.0]) - o
    assert np.allclose(o, (1.0, -2.0, 3.0)) and np.allclose(d, to / np.linalg.norm(to), atol=1e-6)
    x_, y_ = nr.plane_points(o, d)
    assert abs(x_ - 0.2) < 1e-5 and abs(y_ - 0.3) < 1e-5
    assert np.allclose(nr.reflect(np.array([0.0, 0.6, 0.8]), np.array([0.0, 0.0, 1.0])), [0, -0.6, 0.8])


def test_gather_scene_conditions():
    """the float64 classification of the gather test alone: enough pixels qualify, enough triangles are seen, and any two triangles'
    values differ by more than 100 x the bar they are compared at"""
    sd, wl, L, rho = nr.grid_plane_scene(64)
    assert sd.idx.shape == (128, 3) and sd.tri_n.shape == (128, 9)
    o, d = nr.pixel_corner_rays(sd)
    tri = nr.grid_triangle_of(*nr.plane_points(o, d))
    assert (tri >= 0).all()  # the grid covers what the camera sees
    q = (tri == tri[0]).all(0)
    print(f"{100 * q.mean():.1f} % of the pixels qualify, {len(np.unique(tri[0][q]))} triangles seen")
    assert q.mean() >= 0.5 and len(np.unique(tri[0][q])) >= 80
    n = sd.tri_n[:, :3].astype(np.float64)
    assert np.degrees(np.arccos(n[:, 2] / np.linalg.norm(n, axis=1))).max() <= 35.0
    vals = (rho / np.pi * L)[None, :] * (n @ wl)[:, None]
    for c in range(3):
        v = np.sort(vals[:, c])
        assert (np.diff(v) > 100 * (3e-6 * v[1:] + 1e-7)).all(), c
    # the triangle under a point: the library's own hit agrees (checked on the GPU); here, the cell arithmetic against the mesh
    P = sd.P.astype(np.float64)[sd.idx.astype(int)]
    cen = P.mean(1)
    assert np.array_equal(nr.grid_triangle_of(cen[:, 0], cen[:, 1]), np.arange(128))
