"""Projection and goniometric lights without a GPU: the parser, the validation of pbrt_hip_scene_create, and
pbrt_amd/csrc/light_map.hpp compiled for the host against the float64 reference of tests/light_map_ref.py."""
import os

import numpy as np

import pbrt_amd
from pbrt_amd import LIGHT_MAPPED, LIGHT_POINT, PLASTIC, _lib, api, loader, scenes

import image_ref
import light_map_host_build as hb
import light_map_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = """
LookAt 0 -4 1  0 0 0  0 0 1
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" [16] "integer yresolution" [16]
WorldBegin
"""
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0]\n'
f32 = np.float32


def _inv_tan(fov):
    return f32(1.0 / np.tan(float(f32(fov)) * (np.pi / 360.0)))


def _mapped(sd):
    """[(p, I, kind, image row of `textures`, the image, M, inv_tan, sx, sy)] of a loaded scene's mapped lights"""
    rows = [l for l in sd.lights if int(l[0]) == LIGHT_MAPPED]
    assert len(rows) == len(sd.light_maps)
    out = []
    for l, m in zip(rows, sd.light_maps):
        t = sd.textures[int(m[1]) - 1]
        assert int(t[0]) == api.TEXTURE_IMAGE
        out.append((l[1:4], l[4:7], int(m[0]), t, sd.images[int(t[1])], m[2:11].reshape(3, 3), m[11], m[12], m[13]))
    return out


def _create(sd):
    try:
        pbrt_amd.Scene(sd).close()
    except _lib.PbrtHipError as e:
        return e.code, str(e)
    return 0, ""


OK_OR_NO_DEVICE = lambda: 0 if pbrt_amd.device_count() > 0 else -2  # noqa: E731


# ---- the parser ----

def test_parser_reads_a_projection_light(tmp_path):
    img = np.random.default_rng(1).uniform(0.1, 0.9, (2, 4, 3)).astype(f32)
    api.write_image(str(tmp_path / "slide.pfm"), img)
    # the defaults, with a map: I = 1, fov 45, at the origin, the identity; the window from the image's aspect 2
    ls = loader.load_string(HEAD + 'LightSource "projection" "string mapname" "slide.pfm"\n' + QUAD + "WorldEnd\n", base_dir=str(tmp_path))
    assert not ls.warnings, ls.warnings  # (above all not "light type 'projection' unknown")
    (p, I, kind, t, image, M, inv_tan, sx, sy), = _mapped(ls.scene)
    assert p.tolist() == [0, 0, 0] and I.tolist() == [1, 1, 1] and kind == api.LIGHT_MAP_PROJECTION and np.array_equal(M, np.eye(3))
    assert inv_tan == _inv_tan(45) and (sx, sy) == (2, 1) and np.array_equal(image, img)
    assert (int(t[2]), int(t[3])) == (api.WRAP_CLAMP, api.TEXFILTER_BILINEAR)
    # every parameter: I x scale, fov; a tall image: the window is (1, 1 / aspect)
    api.write_image(str(tmp_path / "tall.pfm"), np.full((4, 2, 3), 0.5, f32))
    ls = loader.load_string(HEAD + 'Translate 1 2 3\nLightSource "projection" "rgb I" [1 2 3] "rgb scale" [2 2 .5] "float fov" 70 "string mapname" "tall.pfm"\n' + QUAD +
                            "WorldEnd\n", base_dir=str(tmp_path))
    (p, I, kind, t, image, M, inv_tan, sx, sy), = _mapped(ls.scene)
    assert not ls.warnings and p.tolist() == [1, 2, 3] and I.tolist() == [2, 4, 1.5] and inv_tan == _inv_tan(70) and (sx, sy) == (1, 2)
    # a PNG goes through the inverse gamma as Texture "imagemap" reads one: 0 and 1 are carried exactly
    api.write_image(str(tmp_path / "bw.png"), np.array([[[0, 0, 0], [1, 1, 1]]], f32))
    ls = loader.load_string(HEAD + 'LightSource "projection" "string mapname" "bw.png"\n' + QUAD + "WorldEnd\n", base_dir=str(tmp_path))
    assert _mapped(ls.scene)[0][4].tolist() == [[[0, 0, 0], [1, 1, 1]]]
    assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()


def test_parser_reads_a_goniometric_light(tmp_path):
    img = np.random.default_rng(2).uniform(0.1, 0.9, (4, 8, 3)).astype(f32)
    api.write_image(str(tmp_path / "gonio.pfm"), img)
    ls = loader.load_string(HEAD + 'LightSource "goniometric" "string mapname" "gonio.pfm"\n' + QUAD + "WorldEnd\n", base_dir=str(tmp_path))
    assert not ls.warnings, ls.warnings
    (p, I, kind, t, image, M, inv_tan, sx, sy), = _mapped(ls.scene)
    assert p.tolist() == [0, 0, 0] and I.tolist() == [1, 1, 1] and kind == api.LIGHT_MAP_GONIOMETRIC and np.array_equal(M, np.eye(3))
    assert (inv_tan, sx, sy) == (0, 0, 0) and np.array_equal(image, img) and (int(t[2]), int(t[3])) == (api.WRAP_REPEAT, api.TEXFILTER_BILINEAR)
    ls = loader.load_string(HEAD + 'Translate -1 0 2\nRotate 90 0 0 1\nLightSource "goniometric" "rgb I" [3 2 1] "rgb scale" [.5 .5 2] "string mapname" "gonio.pfm"\n' + QUAD +
                            "WorldEnd\n", base_dir=str(tmp_path))
    (p, I, kind, t, image, M, inv_tan, sx, sy), = _mapped(ls.scene)
    assert not ls.warnings and p.tolist() == [-1, 0, 2] and I.tolist() == [1.5, 1, 2]
    # world_to_light is the rotation inverted: the light's x axis is the world's y after Rotate 90 about z
    assert np.abs(M - np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]])).max() < 1e-6
    assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()


def test_parser_warns(tmp_path):
    api.write_image(str(tmp_path / "m.pfm"), np.full((2, 2, 3), 0.5, f32))

    def load(body):
        return loader.load_string(HEAD + body + "\n" + QUAD + "WorldEnd\n", base_dir=str(tmp_path))
    # no map, or an unreadable one: a projection projects plain I (a 1 x 1 image of ones), a goniometric light is a point light
    for params in ("", '"string mapname" "missing.pfm"'):
        ls = load('LightSource "projection" "rgb I" [2 2 2] ' + params)
        assert [w for w in ls.warnings if "projection" in w and "1 x 1" in w] and not [w for w in ls.warnings if "unknown" in w], ls.warnings
        (p, I, kind, t, image, M, inv_tan, sx, sy), = _mapped(ls.scene)
        assert image.tolist() == [[[1, 1, 1]]] and (sx, sy) == (1, 1) and I.tolist() == [2, 2, 2]
        assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()
        ls = load('Translate 0 0 2\nLightSource "goniometric" "rgb I" [2 2 2] ' + params)
        assert [w for w in ls.warnings if "goniometric" in w and "point light" in w] and not [w for w in ls.warnings if "unknown" in w], ls.warnings
        assert ls.scene.lights.tolist() == [[LIGHT_POINT, 0, 0, 2, 2, 2, 2]] and len(ls.scene.light_maps) == 0 and len(ls.scene.textures) == 0
    # fov outside (0, 180): the default, and said so
    for fov in (0, -10, 180, 200):
        ls = load('LightSource "projection" "float fov" %d "string mapname" "m.pfm"' % fov)
        assert [w for w in ls.warnings if "projection" in w and "fov" in w], (fov, ls.warnings)
        assert _mapped(ls.scene)[0][6] == _inv_tan(45)
    # a CTM that scales unevenly or shears: said, and the rotation part is used; a rotation is taken as it is
    for xf, warns in (("Scale 1 1 3", True), ("ConcatTransform [1 0 0 0  0.5 1 0 0  0 0 1 0  0 0 0 1]", True), ("Rotate 33 0 1 1", False), ("Translate 5 0 0", False)):
        for name in ("projection", "goniometric"):
            ls = load(xf + '\nLightSource "%s" "string mapname" "m.pfm"' % name)
            assert bool([w for w in ls.warnings if name in w and "shears" in w]) == warns, (xf, name, ls.warnings)
            M = _mapped(ls.scene)[0][5].astype(np.float64)
            assert np.abs(M @ M.T - np.eye(3)).max() < 1e-6
            assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()
    # the "unknown" warning keeps its wording for every other name
    ls = load('LightSource "laser"')
    assert ls.warnings == ["light_source: light type 'laser' unknown."] and len(ls.scene.lights) == 0


def test_slots_keep_their_numbers_and_loaded_files_are_taken(tmp_path):
    api.write_image(str(tmp_path / "m.pfm"), np.full((2, 2, 3), 0.5, f32))
    api.write_image(str(tmp_path / "sky.pfm"), np.full((2, 4, 3), 0.5, f32))
    # textures declared before and after the lights, and a spot light: the materials' numbers do not move, the cone keeps its place, the
    # lights' images come behind every texture
    tex = 'Texture "c%d" "spectrum" "checkerboard" "rgb tex1" [.1 .1 .1] "rgb tex2" [.9 .9 .9]\n'
    uvquad = QUAD.replace("\n", ' "float uv" [0 0 1 0 1 1 0 1]\n')
    text = (HEAD + tex % 1 + 'LightSource "projection" "string mapname" "m.pfm"\n' + tex % 2 + 'Material "matte" "texture Kd" "c1"\n' + uvquad +
            'LightSource "spot"\nLightSource "goniometric" "string mapname" "m.pfm"\n' + 'Material "matte" "texture Kd" "c2"\n' + uvquad + "WorldEnd\n")
    ls = loader.load_string(text, base_dir=str(tmp_path))
    sd = ls.scene
    assert not [w for w in ls.warnings if "checkerboard" not in w], ls.warnings
    assert sd.mat_tex.tolist() == [1, 2] and sd.textures[:, 0].tolist() == [0, 0, 4, 4] and sd.light_maps[:, 1].tolist() == [3, 4]
    assert sd.lights[:, 0].tolist() == [LIGHT_MAPPED, pbrt_amd.LIGHT_SPOT, LIGHT_MAPPED] and len(sd.spot_cones) == 1
    assert [m[2] for m in _mapped(sd)] == [api.LIGHT_MAP_PROJECTION, api.LIGHT_MAP_GONIOMETRIC]
    assert _create(sd)[0] == OK_OR_NO_DEVICE()
    # the same file without the mapped lights: every other number is where it was
    ls0 = loader.load_string(text.replace('LightSource "projection" "string mapname" "m.pfm"\n', "").replace('LightSource "goniometric" "string mapname" "m.pfm"\n', ""),
                             base_dir=str(tmp_path))
    assert ls0.scene.mat_tex.tolist() == [1, 2] and np.array_equal(ls0.scene.textures, sd.textures[:2]) and np.array_equal(ls0.scene.spot_cones, sd.spot_cones)
    # a mapped light + normals: the normals are dropped, and said so
    for name in ("projection", "goniometric"):
        ls = loader.load_string(HEAD + 'LightSource "%s" "string mapname" "m.pfm"\n' % name + QUAD.replace("\n", ' "normal N" [0 0 1 0 0 1 0 0 1 0 0 1]\n') + "WorldEnd\n",
                                base_dir=str(tmp_path))
        assert ls.scene.tri_n.shape[0] == 0 and [w for w in ls.warnings if name in w and "normals" in w] and len(_mapped(ls.scene)) == 1
        assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()
        # + an environment map: the mapped lights are dropped, and said so; the other lights stay
        ls = loader.load_string(HEAD + 'LightSource "%s" "string mapname" "m.pfm"\nLightSource "infinite" "string mapname" "sky.pfm"\nLightSource "point"\n' % name + QUAD +
                                "WorldEnd\n", base_dir=str(tmp_path))
        assert [w for w in ls.warnings if name in w and "environment map" in w], ls.warnings
        assert ls.scene.lights[:, 0].tolist() == [pbrt_amd.LIGHT_ENVMAP, LIGHT_POINT] and len(ls.scene.light_maps) == 0 and ls.scene.envmap.size
        assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()


def test_scene_file_equals_the_generator():
    """scenes/projector_cornell.pbrt loads to the arrays scenes.projector_scene builds"""
    ls = loader.load_file(os.path.join(ROOT, "scenes", "projector_cornell.pbrt"))
    sd = scenes.projector_scene(256, 256)
    assert not ls.warnings, ls.warnings
    for f in ("P", "idx", "mat_id", "materials", "lights", "spheres", "cam_to_world", "mat_tex", "tri_uv", "textures", "mat_eta", "spot_cones", "light_maps"):
        a, b = getattr(ls.scene, f), getattr(sd, f)
        assert a.shape == b.shape and np.array_equal(a, b), (f, a, b)
    assert len(ls.scene.images) == len(sd.images) == 2 and all(np.array_equal(a, b) for a, b in zip(ls.scene.images, sd.images))
    assert sd.lights[:, 0].tolist() == [LIGHT_MAPPED, LIGHT_MAPPED] and sd.light_maps[:, 0].tolist() == [0, 1] and (sd.materials[:, 0] == PLASTIC).sum() == 1
    assert not (sd.materials[:, 4:7] > 0).any() or (sd.materials[:, 0] == PLASTIC)[(sd.materials[:, 4:7] > 0).any(1)].all()  # no emitter
    assert (ls.scene.fov, ls.scene.xres, ls.scene.yres, ls.max_depth) == (40.0, 256, 256, 5)
    assert set(np.unique(scenes.procedural_slide())) == {0.0, 1.0} and scenes.procedural_gonio().min() >= 0.05


# ---- the validation of pbrt_hip_scene_create ----

def test_mapped_lights_are_validated_before_any_device_work():
    def scene(edit=None, n_maps=None, **kw):
        sd = scenes.projector_scene(8, 8)
        sd.light_maps = sd.light_maps.copy()
        if edit is not None:
            row, col, value = edit
            sd.light_maps[row, col] = value
        if n_maps is not None:
            sd.light_maps = sd.light_maps[:n_maps]
        for k, v in kw.items():
            setattr(sd, k, v)
        return sd
    bad = [dict(n_maps=0), dict(n_maps=1),  # a type-6 light that names no type-8 slot
           dict(edit=(0, 0, 2)), dict(edit=(1, 0, 7)),  # a kind other than 0 or 1
           dict(edit=(0, 1, 0)), dict(edit=(0, 1, 3)), dict(edit=(1, 1, 9)),  # an image that names no type-4 slot: none, the other record's slot, beyond the table
           dict(edit=(0, 2, np.nan)), dict(edit=(1, 6, np.inf)), dict(edit=(0, 2, -0.9)), dict(edit=(1, 3, 0.02)),  # world_to_light not finite / off orthonormal
           dict(edit=(0, 11, 0.0)), dict(edit=(0, 11, np.inf)), dict(edit=(0, 12, -1.0)), dict(edit=(0, 13, np.nan)), dict(edit=(0, 13, 0.0)),  # a projection's window
           dict(edit=(1, 11, 1.0)), dict(edit=(1, 12, 1.0)), dict(edit=(1, 13, -1.0))]  # a goniometric record's three must be 0
    for kw in bad:
        code, msg = _create(scene(**kw))
        assert code == -1 and "light map" in msg, (kw, code, msg)
    # a rotation within 1e-4 of orthonormal passes; just beyond does not
    for s, ok in ((1.00004, True), (0.99996, True), (1.0001, False), (0.9999, False)):
        sd = scene()
        sd.light_maps[0, 2:5] *= f32(s)
        code, msg = _create(sd)
        assert (code == OK_OR_NO_DEVICE()) if ok else (code == -1 and "light map" in msg), (s, code, msg)
    # a record that no light names is held to the same rules
    sd = scene()
    sd.light_maps = np.concatenate([sd.light_maps, sd.light_maps[:1]])
    assert _create(sd)[0] == OK_OR_NO_DEVICE()
    sd.light_maps[2, 0] = 5
    code, msg = _create(sd)
    assert code == -1 and "light map" in msg, (code, msg)
    # a matte kd_tex that names a record's slot (slots 1 and 2 are the images, 3 and 4 the records); the image's slot itself is a texture
    sd = scene(mat_tex=np.array([3, 0, 0, 0, 0], np.uint32), tri_uv=np.zeros((10, 6), np.float32))
    code, msg = _create(sd)
    assert code == -1 and "light map" in msg and "kd_tex" in msg, (code, msg)
    assert _create(scene(mat_tex=np.array([1, 0, 0, 0, 0], np.uint32), tri_uv=np.zeros((10, 6), np.float32)))[0] == OK_OR_NO_DEVICE()
    # beside an environment-map slot or a normals slot: a limit of the kernel families, said at creation
    env = dict(envmap=np.full((2, 4, 3), 0.5, f32))
    nrm = dict(tri_n=np.tile(np.array([0, 0, 1], f32), (10, 3)))
    base = scenes.projector_scene(8, 8).materials
    matte = np.where(base[:, :1] == PLASTIC, np.array([[0, .5, .5, .5, 0, 0, 0]], f32), base)
    for kw in (env, nrm):
        code, msg = _create(scene(**kw))  # (with the plastic sphere, plastic's own refusal of the pair comes first, in its own words)
        assert code == -4 and "plastic" in msg and "light map" not in msg, (list(kw), code, msg)
        code, msg = _create(scene(materials=matte, **kw))
        assert code == -4 and "light map" in msg, (list(kw), code, msg)
        sd = scene(materials=matte, **kw)  # (a spot light's refusal comes before a mapped light's)
        cone_light, cone = api.spot_light((0, 0, 0.5), (0, 0, -1))
        sd.lights, sd.spot_cones = np.concatenate([sd.lights, [cone_light]]).astype(f32), np.array([cone], f32)
        code, msg = _create(sd)
        assert code == -4 and "spot" in msg and "light map" not in msg, (list(kw), code, msg)
        sd = scene(materials=matte, **kw)  # (the same scene with point lights is fine)
        sd.lights = sd.lights.copy()
        sd.lights[:, 0] = LIGHT_POINT
        assert _create(sd)[0] == OK_OR_NO_DEVICE(), list(kw)
    assert _create(scene())[0] == OK_OR_NO_DEVICE()


def test_the_neighbouring_type_numbers_stay_unknown():
    for t in (4, 7):
        sd = scenes.projector_scene(8, 8)
        sd.lights = sd.lights.copy()
        sd.lights[0, 0] = t
        code, msg = _create(sd)
        assert code == -1 and "unknown light type" in msg and "light map" not in msg, (t, code, msg)
    for t in (5, 7, 9):
        sd = scenes.projector_scene(8, 8)
        sd.textures = np.concatenate([sd.textures, [[t, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0]]]).astype(f32)
        code, msg = _create(sd)
        assert code == -1 and "unknown texture type" in msg, (t, code, msg)
    # a fault that is refused before the light-type check still wins against a bad mapped light
    sd = scenes.projector_scene(8, 8)
    sd.light_maps = sd.light_maps[:0]
    sd.fov = 0.0
    code, msg = _create(sd)
    assert code == -1 and "fov" in msg, (code, msg)
    assert "pbrt_hip_light_map_eval_device" in _lib.SYMBOLS and api.LIGHT_MAPPED == 6 and _lib.SLOT_LIGHT_MAP == 8
    version = api.lib().pbrt_hip_version().decode()
    assert "0.12" in version and all(v in version for v in ("0.6", "0.7", "0.9", "0.10", "0.11"))


# ---- the header, compiled for the host, against the reference ----

# Measured on the first run over domain_cases() (2^16 inputs per kind; DESIGN.md 3.23's table): the largest ABSOLUTE errors of s, t and rgb
# and the largest RELATIVE error of scale.  scale is the point light's (cs / dist2) nL: a dot product of two unit vectors down to cs = 0.05
# and three roundings.  Projection: s and t are px / (2 sx) + 1/2 with px = (w.x / w.z) inv_tan; w carries a few ulps of 1 from the rotation
# of a normalised difference, and w.z goes down to cos(60 degrees + the window's 10 %) ~ 0.3 at fov 120, where the quotient's error is ~ 4
# times w's.  Goniometric: s = phi / 2 pi carries poly_atan_pos's 1.4e-7 and the quotient's error, divided by 2 pi; t = 1 - theta / pi carries
# poly_acos's 3e-7 plus w.y's error times 1 / sin(theta) <= 20 at the domain's caps, divided by pi.  rgb follows (s, t) with the smooth
# image's slope between neighbouring texels (up to ~ 6 per unit of t over its 8 rows) and adds the bilinear sum's own roundings.  The goniometric s is
# compared as an angle: a direction within rounding of the seam may be given as 0 or as 1.  Asserted at TWICE the measured value,
# as 3.21 and 3.22 do.
MEASURED = {
    hb.PROJECTION: dict(s=1.49e-7, t=2.69e-7, scale=1.56e-6, rgb=4.83e-7),
    hb.GONIOMETRIC: dict(s=1.50e-7, t=4.98e-7, scale=1.56e-6, rgb=2.86e-6),
}


def _reference(case, **kw):
    X = case.x.astype(np.float64)
    return ref.sample(X[:, 0:3], X[:, 3:6], X[:, 6:9], case.kind, case.M.astype(np.float64), float(f32(case.inv_tan)), float(f32(case.sx)), float(f32(case.sy)),
                      case.image.astype(np.float64), case.wrap, case.filt, X[:, 9], **kw)


def _near_an_edge(case, r):
    """inputs whose float64 px / py lies within 4 fp32 ulp of a window edge, or whose w.z lies within 4 ulp of the least depth: float32 may
    put them on the other side"""
    if case.kind != hb.PROJECTION:
        return np.zeros(len(case.x), bool)
    sx, sy = float(f32(case.sx)), float(f32(case.sy))
    u = lambda v: 4.0 * float(np.spacing(f32(v)))  # noqa: E731
    with np.errstate(all="ignore"):
        return ((np.abs(np.abs(r["px"]) - sx) <= u(sx)) | (np.abs(np.abs(r["py"]) - sy) <= u(sy)) | (np.abs(r["wz"] - ref.MIN_Z) <= u(ref.MIN_Z))) & r["geometric"]


def test_header_on_the_host_matches_float64(tmp_path):
    exe = hb.build(tmp_path)
    for kind in (hb.PROJECTION, hb.GONIOMETRIC):
        cases = hb.domain_cases(kind)
        assert sum(len(c.x) for c in cases) == 1 << 16
        got = dict(s=0.0, t=0.0, scale=0.0, rgb=0.0)
        n_near = n_ok = n_out = 0
        for c in cases:
            y = hb.run(exe, c, tmp_path).astype(np.float64)
            r = _reference(c)
            near = _near_an_edge(c, r)
            n_near += int(near.sum())
            far = ~near
            # (an input near an edge is compared on `ok` alone: it is a sample or it is none, and either side is the reference snapped to it)
            assert np.isin(y[near, 0], (0.0, 1.0)).all()
            assert np.array_equal(y[far, 0] != 0, r["ok"][far])  # every other input counts: a sample in both or in neither
            m = far & r["ok"]
            n_ok, n_out = n_ok + int(m.sum()), n_out + int((far & ~r["ok"]).sum())
            assert (y[far & ~r["ok"]] == 0).all()
            # the rest of the sample is the point light's: direction and distance to rounding
            assert np.abs(y[m, 1:4] - r["wi"][m]).max() < 3e-7 and (np.abs(y[m, 4] - r["tmax"][m]) / r["tmax"][m]).max() < 3e-7
            ds = np.abs(y[m, 6] - r["s"][m])
            if kind == hb.GONIOMETRIC:  # (s is an angle over 2 pi: a direction within rounding of the seam may be given as 0 or as 1, the same place)
                ds = np.minimum(ds, 1.0 - ds)
            got["s"] = max(got["s"], ds.max())
            got["t"] = max(got["t"], np.abs(y[m, 7] - r["t"][m]).max())
            got["scale"] = max(got["scale"], (np.abs(y[m, 5] - r["scale"][m]) / r["scale"][m]).max())
            got["rgb"] = max(got["rgb"], np.abs(y[m, 8:11] - r["rgb"][m]).max())
            # under the POINT filter rgb is the reference lookup at the header's own float32 (s, t), exactly (the texel choice is
            # image_lookup.hpp's business, tested in 3.20; 16 and 8 are powers of two, so the float64 index is the float32 one)
            yp = hb.run(exe, c.with_filter(hb.POINT), tmp_path)
            lit = yp[:, 0] != 0
            assert np.array_equal(lit, y[:, 0] != 0) and np.array_equal(yp[lit, :8], y[lit, :8].astype(f32))
            want = image_ref.point(c.image, c.wrap, yp[lit, 6].astype(np.float64), yp[lit, 7].astype(np.float64)).astype(f32)
            assert np.array_equal(yp[lit, 8:11], want)
        print(f"kind {kind}: inputs near an edge: {n_near} of {1 << 16}; samples {n_ok}, none {n_out}; measured:", {k: f"{v:.3e}" for k, v in got.items()})
        assert n_near <= (1 << 16) // 1000
        assert n_ok > (1 << 16) // 2 and (kind == hb.GONIOMETRIC or n_out > (1 << 16) // 8)  # (10 % outside on either axis: 1 - 1 / 1.21 of the projection's inputs)
        for k, v in got.items():
            assert v <= 2.0 * MEASURED[kind][k], (kind, k, v, MEASURED[kind][k])


def test_edge_inputs_on_the_host(tmp_path):
    exe = hb.build(tmp_path)
    cases = hb.edge_cases()
    seen = {}
    for c in cases:
        y = hb.run(exe, c, tmp_path)
        assert np.isfinite(y).all()
        name = hb.EDGE_KINDS[int(c.tag[0])]
        assert (c.tag == c.tag[0]).all()
        seen[name] = seen.get(name, 0) + len(y)
        ok = y[:, 0] == 1
        wi, w, d2, _ = hb.header_f32(c.x, c.M)
        with np.errstate(all="ignore"):
            front = (wi[:, 0] * c.x[:, 3] + wi[:, 1] * c.x[:, 4]) + wi[:, 2] * c.x[:, 5] > 0  # (cs in the header's own float32)
        if name in ("px_at_plus_sx", "px_at_minus_sx", "py_at_plus_sy"):
            # px exactly +-sx (py exactly sy): inside, and s (t) is exactly at the window's end
            assert front.all() and ok.all()
            col, want = (6, 1.0 if name == "px_at_plus_sx" else 0.0) if name.startswith("px") else (7, 1.0)
            assert (y[:, col] == want).all(), (name, y[:, col])
        elif name in ("px_one_ulp_beyond", "py_one_ulp_beyond", "wz_at_min", "po_is_p"):
            assert (y == 0).all(), name  # one ulp outside the window; w.z AT 1e-3 (the comparison is strict); no direction
        elif name == "wz_one_ulp_above":
            assert front.all() and ok.all() and (w[:, 2] == np.nextafter(hb.MIN_Z, f32(1))).all()
        elif name == "pole_plus":  # theta = 0, phi = 0 (w.x = w.z = 0): the top row's left end
            assert ok.all() and (y[:, 6] == 0).all() and (y[:, 7] == 1).all()
        elif name == "pole_minus":  # theta = pi: t = 1 - fl(pi) / pi within rounding of 0
            assert ok.all() and (y[:, 6] == 0).all() and (np.abs(y[:, 7]) <= 1.2e-7).all()
        elif name == "seam_zero":  # w.z = 0 exactly, w.x > 0: phi = 0
            assert ok.all() and (y[:, 6] == 0).all()
        elif name == "seam_below":  # w.z a hair below 0: phi a hair below 2 pi, s at most one rounding above 1
            assert ok.all() and (y[:, 6] > 0.999999).all() and (y[:, 6] <= f32(1) + f32(1.2e-7)).all()
        elif name == "black_texel":
            # the 2 x 2 image's top-left texel is black: no sample exactly where the header's own (s, t) lands there
            r = _reference(c)
            lit_geo = front & (d2 > 0)
            if c.kind == hb.PROJECTION:
                with np.errstate(all="ignore"):
                    px, py = (w[:, 0] / w[:, 2]) * f32(c.inv_tan), (w[:, 1] / w[:, 2]) * f32(c.inv_tan)
                    lit_geo &= (w[:, 2] > hb.MIN_Z) & (np.abs(px) <= f32(c.sx)) & (np.abs(py) <= f32(c.sy))
            assert (y[~lit_geo] == 0).all()
            agree = (r["ok"] == ok) | ~lit_geo
            assert agree.mean() > 0.995  # (a direction within rounding of the texel's border may fall on either side)
            assert ok.sum() > len(y) // 4 and (lit_geo & ~ok).sum() > len(y) // 16
            assert (y[ok, 8:11] != 0).any(1).all()
        elif name == "ones":
            # a texel of ones: rgb is 1 and scale equals the point light's (cs / dist2) nL bit for bit
            assert ok.sum() > len(y) // 2 and (y[ok, 8:11] == 1).all()
            assert np.array_equal(y[ok, 5].view(np.uint32), hb.point_scale_f32(c.x)[ok].astype(f32).view(np.uint32))
    assert set(seen) == set(hb.EDGE_KINDS) and sum(seen.values()) > 3000 and all(n >= 24 for n in seen.values()), seen
