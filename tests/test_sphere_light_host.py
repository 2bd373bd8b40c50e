"""Sphere lights without a GPU: the parser, the validation of pbrt_hip_scene_create, the device tables' rows, the float64
reference of tests/sphere_light_ref.py against the closed form, and pbrt_amd/csrc/sphere_light.hpp compiled for the host against that
reference."""
import dataclasses
import os

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import GLASS, LIGHT_SPHERE, MATTE, MIRROR, PLASTIC, SUBSTRATE, _lib, api, loader, scenes

import scene_tables_cases
import sphere_light_host_build as hb
import sphere_light_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = """
LookAt 0 -4 1  0 0 0  0 0 1
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" [16] "integer yresolution" [16]
WorldBegin
"""
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0]\n'
LAMP = 'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [3 2 1]\n%sTranslate 0 0 2\nShape "sphere" "float radius" 0.25\nAttributeEnd\n'
f32 = np.float32


def _create(sd):
    try:
        pbrt_amd.Scene(sd).close()
    except _lib.PbrtHipError as e:
        return e.code, str(e)
    return 0, ""


OK_OR_NO_DEVICE = lambda: 0 if pbrt_amd.device_count() > 0 else -2  # noqa: E731


# ---- the parser ----

def test_parser_makes_a_sphere_and_a_light_that_names_it():
    ls = loader.load_string(HEAD + QUAD + LAMP % "" + "WorldEnd\n")
    assert not ls.warnings, ls.warnings  # (above all not "sphere area lights emit but are not sampled")
    sd = ls.scene
    assert sd.spheres.tolist() == [[0, 0, 2, 0.25, 1]] and sd.lights.tolist() == [[LIGHT_SPHERE, 0, 0, 0, 3, 2, 1]]
    assert sd.materials[1].tolist() == [MATTE, 0.5, 0.5, 0.5, 3, 2, 1]
    assert _create(sd)[0] == OK_OR_NO_DEVICE()
    # L x scale is what the material gets and what the light says; a second lamp is the second light and names the second sphere
    ls = loader.load_string(HEAD + 'LightSource "point"\n' + LAMP % "" + QUAD + LAMP.replace("[3 2 1]", '[1 2 3] "rgb scale" [2 2 .5]') % "" + "WorldEnd\n")
    assert not ls.warnings and ls.scene.lights[:, 0].tolist() == [0, LIGHT_SPHERE, LIGHT_SPHERE]
    assert ls.scene.lights[1:, 1].tolist() == [0, 1] and ls.scene.lights[2, 4:7].tolist() == [2, 4, 1.5]
    assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()
    # an area light of no radiance lights nothing and makes no light
    ls = loader.load_string(HEAD + QUAD + LAMP.replace("[3 2 1]", "[0 0 0]") % "" + "WorldEnd\n")
    assert len(ls.scene.lights) == 0 and len(ls.scene.spheres) == 1 and _create(ls.scene)[0] == OK_OR_NO_DEVICE()


@pytest.mark.parametrize("material", ["glass", "plastic", "substrate"])
def test_parser_keeps_the_black_matte_emitter_of_a_material_that_reuses_le(material):
    ls = loader.load_string(HEAD + QUAD + LAMP % ('Material "%s"\n' % material) + "WorldEnd\n")
    assert [w for w in ls.warnings if material in w and "AreaLightSource" in w] and len(ls.warnings) == 1, ls.warnings
    assert ls.scene.materials[1].tolist() == [MATTE, 0, 0, 0, 3, 2, 1] and ls.scene.lights.tolist() == [[LIGHT_SPHERE, 0, 0, 0, 3, 2, 1]]
    assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()


def test_parser_keeps_the_other_warnings():
    ls = loader.load_string(HEAD + QUAD + LAMP.replace("[3 2 1]", '[3 2 1] "bool twosided" "true"') % "" + "WorldEnd\n")
    assert [w for w in ls.warnings if "twosided" in w] and len(ls.scene.lights) == 1
    ls = loader.load_string(HEAD + QUAD + 'ObjectBegin "a"\n' + LAMP % "" + 'ObjectEnd\nObjectInstance "a"\nWorldEnd\n')
    assert [w for w in ls.warnings if "Area lights not supported with object instancing" in w]
    assert len(ls.scene.lights) == 0 and len(ls.scene.spheres) == 1 and not ls.scene.materials[:, 4:7].any()


def test_parser_drops_the_lights_beside_a_map_and_the_normals_beside_the_lights(tmp_path):
    api.write_image(str(tmp_path / "sky.pfm"), np.full((2, 4, 3), 0.5, np.float32))
    ls = loader.load_string(HEAD + 'LightSource "infinite" "string mapname" "sky.pfm"\nLightSource "point"\n' + QUAD + LAMP % "" + "WorldEnd\n", base_dir=str(tmp_path))
    assert [w for w in ls.warnings if "sphere light" in w and "environment map" in w], ls.warnings
    assert ls.scene.lights[:, 0].tolist() == [pbrt_amd.LIGHT_ENVMAP, pbrt_amd.LIGHT_POINT] and ls.scene.envmap.size
    assert len(ls.scene.spheres) == 1 and ls.scene.materials[1, 4:7].tolist() == [3, 2, 1]  # the sphere still emits, unsampled
    assert _create(ls.scene)[0] == OK_OR_NO_DEVICE()
    ls = loader.load_string(HEAD + QUAD.replace("\n", ' "normal N" [0 0 1 0 0 1 0 0 1 0 0 1]\n') + LAMP % "" + "WorldEnd\n")
    assert ls.scene.tri_n.shape[0] == 0 and [w for w in ls.warnings if "sphere light" in w and "normals" in w], ls.warnings
    assert ls.scene.lights[:, 0].tolist() == [LIGHT_SPHERE] and _create(ls.scene)[0] == OK_OR_NO_DEVICE()
    # without a lamp the normals stay
    ls = loader.load_string(HEAD + QUAD.replace("\n", ' "normal N" [0 0 1 0 0 1 0 0 1 0 0 1]\n') + "WorldEnd\n")
    assert ls.scene.tri_n.shape[0] == 2 and not ls.warnings


def test_scene_file_equals_the_generator():
    """scenes/sphere_light_cornell.pbrt loads to the arrays scenes.sphere_light_scene builds"""
    ls = loader.load_file(os.path.join(ROOT, "scenes", "sphere_light_cornell.pbrt"))
    sd = scenes.sphere_light_scene(256, 256)
    assert not ls.warnings, ls.warnings
    for f in ("P", "idx", "mat_id", "materials", "lights", "spheres", "cam_to_world", "mat_tex", "tri_uv", "textures", "mat_eta", "spot_cones", "light_maps"):
        a, b = getattr(ls.scene, f), getattr(sd, f)
        assert a.shape == b.shape and np.array_equal(a, b), (f, a, b)
    assert sd.lights[:, 0].tolist() == [LIGHT_SPHERE, LIGHT_SPHERE] and sd.spheres[:2, 3].tolist() == [f32(0.15), f32(0.05)]
    assert (sd.materials[:, 0] == PLASTIC).sum() == 1 and (sd.materials[:, 0] == MIRROR).sum() == 1
    assert not (sd.materials[sd.mat_id][:, 4:7] > 0).any()  # no emissive triangle: the lamps are the only lights
    assert (ls.scene.fov, ls.scene.xres, ls.scene.yres, ls.max_depth) == (40.0, 256, 256, 5)
    assert _create(sd)[0] == OK_OR_NO_DEVICE()


# ---- the validation of pbrt_hip_scene_create ----

def _lamp_scene(**kw):
    sd = scenes.sphere_light_scene(8, 8)
    for k, v in kw.items():
        setattr(sd, k, v)
    return sd


def test_sphere_lights_are_validated_before_any_device_work():
    base = _lamp_scene()
    assert _create(base)[0] == OK_OR_NO_DEVICE()

    def lights(rows):
        return np.array(rows, np.float32)
    warm, cool = base.lights.tolist()
    mats = lambda k, row: np.concatenate([base.materials[:k], np.array([row], np.float32), base.materials[k + 1:]])  # noqa: E731
    bad = [dict(lights=lights([[LIGHT_SPHERE, 4, 0, 0, *warm[4:7]]])), dict(lights=lights([[LIGHT_SPHERE, -1, 0, 0, *warm[4:7]]])),  # a pad that names no sphere
           dict(lights=lights([warm, cool, warm])),  # two lights naming one sphere
           dict(lights=lights([warm, [LIGHT_SPHERE, 2, 0, 0, 0.3, 0.3, 0.3]])),  # the plastic sphere: its `le` is Ks
           dict(lights=lights([warm, [LIGHT_SPHERE, 3, 0, 0, 0, 0, 0]])),  # the mirror sphere: no positive le
           dict(lights=lights([[LIGHT_SPHERE, 0, 0, 0, 20, 16, 10.000001]])),  # c differs from le in the last bit
           dict(lights=lights([[LIGHT_SPHERE, 0, 0, 0, *cool[4:7]]])),  # another lamp's radiance
           dict(materials=mats(3, [GLASS, 1, 1, 1, 20, 16, 10])), dict(materials=mats(3, [SUBSTRATE, .5, .5, .5, 1, 1, 1])),
           dict(materials=mats(3, [MATTE, 0, 0, 0, 0, 0, 0])), dict(materials=mats(3, [MATTE, 0, 0, 0, -1, 0, -2]))]
    for kw in bad:
        sd = _lamp_scene(**kw)
        if "materials" in kw and kw["materials"][3, 0] in (GLASS, SUBSTRATE):
            sd.lights = lights([[LIGHT_SPHERE, 0, 0, 0, *kw["materials"][3, 4:7]]])  # (c = the record's le words: the material is what is wrong)
            sd.mat_eta = np.array([1.5, 1.5, 1.5, 0.5 if kw["materials"][3, 0] == SUBSTRATE else 1.5, 1.5, sd.mat_eta[5], 1.5], np.float32)
        code, msg = _create(sd)
        assert code == -1 and "sphere light" in msg, (kw, code, msg)
        # ... and the same scene without the light rows passes
        sd.lights = np.zeros((0, 7), np.float32)
        assert _create(sd)[0] == OK_OR_NO_DEVICE(), kw
    # a lamp's sphere is held to every sphere's rules before the light is looked at: a radius that is not positive never reaches the sampler
    for r in (0.0, -0.15, np.nan):
        sd = _lamp_scene()
        sd.spheres = sd.spheres.copy()
        sd.spheres[0, 3] = r
        code, msg = _create(sd)
        assert code == -1 and "radius positive" in msg, (r, code, msg)
    # a channel of le may be zero, or negative, while another is positive
    sd = _lamp_scene(materials=mats(3, [MATTE, 0, 0, 0, 0, 5, -1]), lights=lights([[LIGHT_SPHERE, 0, 0, 0, 0, 5, -1], cool]))
    assert _create(sd)[0] == OK_OR_NO_DEVICE()
    # beside an environment-map slot or a normals slot: a limit of the kernel families, said at creation
    env = dict(envmap=np.full((2, 4, 3), 0.5, np.float32))
    nrm = dict(tri_n=np.tile(np.array([0, 0, 1], np.float32), (10, 3)))
    for kw in (env, nrm):
        code, msg = _create(_lamp_scene(**kw))  # (with the plastic sphere, plastic's own refusal of the pair comes first)
        assert code == -4 and "plastic" in msg and "sphere light" not in msg, (list(kw), code, msg)
        matte = np.where(base.materials[:, :1] == PLASTIC, np.array([[MATTE, .5, .5, .5, 0, 0, 0]], np.float32), base.materials)
        code, msg = _create(_lamp_scene(materials=matte, **kw))
        assert code == -4 and "sphere light" in msg, (list(kw), code, msg)
        assert _create(_lamp_scene(materials=matte, lights=np.zeros((0, 7), np.float32), **kw))[0] == OK_OR_NO_DEVICE()
    # a spot light beside the lamp keeps its word, and wins
    sd = _lamp_scene(materials=matte, **env)
    row, cone = api.spot_light((0, 0, 0.5), (0, 0, -1))
    sd.lights, sd.spot_cones = np.array([row, *sd.lights.tolist()], np.float32), np.array([cone], np.float32)
    code, msg = _create(sd)
    assert code == -4 and "spot" in msg and "sphere light" not in msg


def test_unknown_types_stay_unknown_and_the_version_says_0_14():
    for t in (4, 7, 9):
        sd = _lamp_scene()
        sd.lights = np.array([[t, 0, 0, 0, 1, 1, 1]], np.float32)
        code, msg = _create(sd)
        assert code == -1 and "unknown light type" in msg, (t, code, msg)
    sd = _lamp_scene()
    sd.materials = sd.materials.copy()
    sd.materials[0, 0] = 5
    code, msg = _create(sd)
    assert code == -1 and "unknown material type" in msg
    version = _lib.lib().pbrt_hip_version().decode()
    assert "0.14" in version and all(v in version for v in ("0.6", "0.7", "0.8", "0.9", "0.10", "0.11", "0.12", "0.13"))
    assert "pbrt_hip_sphere_light_eval_device" in _lib.SYMBOLS and pbrt_amd.LIGHT_SPHERE == 8 == api.LIGHT_SPHERE


def test_device_tables_hold_the_light_and_mark_the_sphere():
    """scene_tables.hpp's rows, restated from DESIGN.md section 4: {8, centre} {r, 0 0 0} 0 {L, 0} 0 at the light's place in the description's
    order, and the listed sphere's row 1 {material id, 1, 0, 0}; an unlisted sphere's row and a scene without the light are what they were"""
    sd = _lamp_scene()
    sd.lights = np.array([[0, 1, 2, 3, 4, 5, 6], sd.lights[1].tolist(), [1, 0, 0, 1, 1, 1, 1]], np.float32)  # point, the COOL lamp, distant
    t = scene_tables_cases.tables(sd)
    rows = t["lights"].view(np.float32).reshape(-1, 5, 4)
    assert rows.shape[0] == 3 and t["lights"].reshape(-1, 5, 4)[:, 0, 0].tolist() == [0, 8, 1]
    c, r, L = sd.spheres[1, :3], sd.spheres[1, 3], sd.materials[4, 4:7]
    want = np.array([[0, *c], [r, 0, 0, 0], [0, 0, 0, 0], [*L, 0], [0, 0, 0, 0]], np.float32)
    want[0, 0] = np.array([8], np.uint32).view(np.float32)[0]
    assert np.array_equal(rows[1].view(np.uint32), want.view(np.uint32))
    sph = t["spheres"].reshape(-1, 2, 4)
    assert sph[:, 1, 0].tolist() == [3, 4, 5, 6] and sph[:, 1, 1].tolist() == [0, 1, 0, 0] and not sph[:, 1, 2:].any()
    plain = scene_tables_cases.tables(dataclasses.replace(sd, lights=sd.lights[[0, 2]]))
    assert not plain["spheres"].reshape(-1, 2, 4)[:, 1, 1:].any() and np.array_equal(plain["spheres"].reshape(-1, 2, 4)[:, 0], sph[:, 0])
    assert np.array_equal(plain["lights"].reshape(-1, 5, 4), t["lights"].reshape(-1, 5, 4)[[0, 2]])


# ---- the reference against the closed form ----

@pytest.mark.parametrize("ratio", [0.93, 0.33, 1e-2, 1e-4])
def test_reference_meets_the_closed_form(ratio):
    """A sphere wholly above the horizon of a matte point gives Lo = Kd L (r / d)^2 cos theta_c exactly; the reference's Monte Carlo mean over
    4 10^5 samples agrees within 5 of its own standard errors"""
    n = 400_000
    rng = np.random.default_rng(int(ratio * 1e6))
    kd, L, d = 0.7, 3.0, 1.7
    w = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    tilt = 0.8 * (np.pi / 2 - np.arcsin(ratio))  # the normal tilted away from the centre, the whole cone still above the horizon
    v2, _ = ref.frame(w[None])
    nf = np.cos(tilt) * w + np.sin(tilt) * v2[0]
    po = np.array([0.2, 0.1, -0.3])
    u = rng.random((n, 2))
    ok, wi, tmax, scale, pdf, cs = ref.sample(np.tile(po, (n, 1)), np.tile(nf, (n, 1)), po + w * d, np.full(n, ratio * d), u[:, 0], u[:, 1], 1.0)
    assert ok.all()
    est = (kd / np.pi) * L * scale
    want = float(ref.closed_form(kd, L, ratio * d, d, np.cos(tilt)))
    se = est.std(ddof=1) / np.sqrt(n)
    assert abs(est.mean() - want) <= 5 * se, (ratio, est.mean(), want, se)
    assert se < 0.01 * want  # (the check has teeth: a hundredth of the value)
    # the density integrates to one over the cone: every direction lies inside it and lands on the sphere at distance t
    assert np.allclose(np.linalg.norm(wi, axis=1), 1.0, atol=1e-12) and ((wi @ w) >= np.sqrt(1 - ratio ** 2) - 1e-12).all()
    # the variants the GPU controls use do NOT meet it
    # (the area density: 8 / 3 of the value as r / d -> 0; the float32 subtraction: exactly 0 from r / d = 2.4e-4 downwards)
    for wrong in ("area",) + (("omc_subtract",) if ratio <= 2e-4 else ()):
        _, _, _, scale_w, _, _ = ref.sample(np.tile(po, (n, 1)), np.tile(nf, (n, 1)), po + w * d, np.full(n, ratio * d), u[:, 0], u[:, 1], 1.0, wrong)
        est_w = (kd / np.pi) * L * scale_w
        assert abs(est_w.mean() - want) > 5 * est_w.std(ddof=1) / np.sqrt(n) and abs(est_w.mean() - want) > 0.1 * want, (wrong, ratio, est_w.mean(), want)


# ---- the header, compiled for the host, against the reference ----

@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sphere_light_host")
    return hb.build(tmp), tmp


# DESIGN.md 3.25's measured table: the largest error of the host compile over the 2^16 domain inputs; each is asserted at twice the figure
MEASURED = dict(scale=4.3e-7,   # |scale - ref| as a share of nL / pdf_omega, the value scale has at cs = 1
                pdf=6.4e-7,     # relative, the sample's and the hit side's
                tmax=2.5e-6,   # |tmax - ref| as a share of the distance to the centre
                angle=4.2e-7)   # radians between the directions


def test_header_meets_the_reference_on_the_domain(host):
    exe, tmp = host
    x = hb.domain_inputs()
    y = hb.run(exe, x, tmp).astype(np.float64)
    X = x.astype(np.float64)
    d = np.linalg.norm(X[:, 6:9] - X[:, 0:3], axis=1)
    w = (X[:, 6:9] - X[:, 0:3]) / d[:, None]
    # (the reference with the normal on the centre's direction: wi, tmax and pdf whatever the side of the real normal the direction falls on)
    _, wi, tmax, _, pdf, _ = ref.sample(X[:, 0:3], w, X[:, 6:9], X[:, 9], X[:, 10], X[:, 11], X[:, 12])
    cs = (wi * X[:, 3:6]).sum(1)
    knife = np.abs(cs) < 1e-6
    assert knife.mean() < 1e-3
    assert np.array_equal((y[:, 0] > 0)[~knife], (cs > 0)[~knife])
    m = (y[:, 0] > 0) & (cs > 0)
    assert m.mean() > 0.9
    scale = cs / pdf * X[:, 12]
    err = dict(scale=(np.abs(y[m, 5] - scale[m]) * pdf[m] / X[m, 12])[~knife[m]].max(),
               pdf=max((np.abs(y[m, 6] - pdf[m]) / pdf[m]).max(), (np.abs(y[:, 7] - ref.pdf_omega(X[:, 0:3], X[:, 6:9], X[:, 9])) / pdf).max()),
               tmax=(np.abs(y[m, 4] - tmax[m]) / d[m]).max(),
               angle=np.linalg.norm(np.cross(y[m, 1:4], wi[m]), axis=1).max())
    print(err)
    for k, v in err.items():
        assert v <= 2 * MEASURED[k], (k, v, MEASURED[k])
    assert np.abs(np.linalg.norm(y[m, 1:4], axis=1) - 1).max() < 1e-6
    assert not y[~(y[:, 0] > 0), 1:7].any()  # zeros behind ok = 0
    # 1 - cos theta_max keeps its digits down to r / d = 1e-4: scale / cs = 2 pi omc nL to 7 digits where the subtraction would give 0
    small = m & (X[:, 9] / d < 2.4e-4)
    assert small.sum() > 1000 and (y[small, 6] > 0).all() and np.isfinite(y[small, 5:7]).all()


def test_the_copied_disk_map_and_frame_equal_cosine_abouts(tmp_path):
    """sphere_light.hpp copies cosine_about's concentric map and tangent frame (a call would change every render kernel's machine code).  The
    copies are held to the original: the direction rebuilt from them equals cosine_about's bit for bit over 2^16 inputs and the pairs where
    the map branches -- the centre, the diagonals |ox| = |oy|, the square's edges"""
    exe = hb.build(tmp_path, hb.COPY_MAIN, "sphere_light_copy_check")
    r = np.random.default_rng(31)
    n = r.normal(size=(1 << 16, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:64] = np.repeat(np.concatenate([np.eye(3), -np.eye(3), [[0.6, 0.6, 0.52915026], [-0.6, 0.6, 0.52915026]]]), 8, 0)  # axes, and |x| = |y|
    u = r.uniform(0, 1, (1 << 16, 2))
    special = np.array([0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24])
    u[64:64 + 25] = np.stack(np.meshgrid(special, special), -1).reshape(-1, 2)
    u[100:1100, 1] = u[100:1100, 0]       # ox = oy
    u[1100:2100, 1] = 1.0 - u[1100:2100, 0]  # ox = -oy
    x = np.concatenate([n, u], 1).astype(np.float32)
    y = hb.run(exe, x, tmp_path, 5, 6)
    assert np.isfinite(y).all() and np.array_equal(y[:, 0:3].view(np.uint32), y[:, 3:6].view(np.uint32))
    assert np.abs(np.linalg.norm(y[:, 0:3].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_header_is_finite_and_zero_where_it_must_be_on_the_edges(host):
    exe, tmp = host
    x, kind = hb.edge_inputs()
    assert len(x) == 4096 and len(hb.all_inputs()) == 69632
    y = hb.run(exe, x, tmp)
    assert np.isfinite(y).all()
    k = lambda name: kind == hb.EDGE_KINDS.index(name)  # noqa: E731
    X = x.astype(np.float64)
    d2 = ((X[:, 6:9] - X[:, 0:3]) ** 2).sum(1)
    # a point inside the sphere or at its centre: no sample, and the hit side's density is 0 (the weight of a BSDF-sampled hit is then 1)
    for name in ("inside", "at_centre"):
        assert k(name).sum() > 500 and not y[k(name)].any(), name
    # a point ON the sphere is outside or not by the rounding of its float32 coordinates; either way the outputs are finite, zero where
    # not outside, and a sample that exists has a positive density and a tmax that does not pass the far side
    m = k("on_surface")
    out = (y[m, 7] > 0)
    assert not y[m][~out].any() and (y[m][y[m, 0] > 0, 6] > 0).all()
    assert (y[m, 4] <= 2.0 * x[m, 9] + 1e-3).all()
    # the corners of the unit square: samples like any other, unit directions, scale within its bound cs (1 / pdf) nL <= nL / pdf
    m = k("u_corners") & (y[:, 0] > 0)
    assert m.sum() > 500 and np.abs(np.linalg.norm(y[m, 1:4].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert (y[m, 5] <= x[m, 12] / y[m, 6] * (1 + 1e-6)).all() and (y[m, 5] > 0).all()
    # r / d = 1e-6: the solid angle is pi (r / d)^2 to 6 digits, not 0, and the shadow ray stops short of the sphere by the margin
    m = k("tiny") & (y[:, 0] > 0)
    assert m.sum() > 500
    assert np.allclose(1.0 / y[m, 6].astype(np.float64), np.pi * X[m, 9] ** 2 / d2[m], rtol=1e-5)
    # (2^-9 = 1.95e-3 of the distance for the rim's margin, 1e-4 for kShadowShrink)
    assert (y[m, 4] < (1 - 2.0e-3) * np.sqrt(d2[m])).all() and (y[m, 4] > (1 - 2.1e-3) * np.sqrt(d2[m])).all()


def test_shadow_ray_stops_short_of_the_lights_own_sphere(host):
    """The part DESIGN.md 3.25 derives: kernel_math.hpp's sphere_hit, restated here in its own float32 operations (c = oc . oc - r r and b =
    2 d . oc in float32, the quadratic in double), finds NO intersection of the shadow ray (po, wi, tmax) with the light's own sphere, on
    every input of the domain and with the rays aimed at the rim (s = 1), where the discriminant is of the size of its error; and tmax lies
    in front of the float64 intersection by no more than twice the margin plus kShadowShrink's share"""
    exe, tmp = host
    x = np.concatenate([hb.domain_inputs(), hb.domain_inputs(seed=4)])
    rim = x[1 << 16:]
    rim[::2, 10] = 0  # (a pair on the unit square's edge u = 0 maps onto the unit circle: s = 1 to rounding, the cone's rim)
    rim[1::2, 11] = 0
    y = hb.run(exe, x, tmp)
    m = y[:, 0] > 0
    assert m[1 << 16:].mean() > 0.7
    o, c, r, d, tmax = x[m, 0:3], x[m, 6:9], x[m, 9], y[m, 1:4], y[m, 4]
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]  # noqa: E731  (float32, kernel_math.hpp's order)
    oc = o - c
    qa, qb, qc = dot(d, d).astype(np.float64), (f32(2) * dot(d, oc)).astype(np.float64), (dot(oc, oc) - r * r).astype(np.float64)
    disc = qb * qb - 4.0 * qa * qc
    real = disc >= 0
    rd = np.sqrt(np.maximum(disc, 0.0))
    q = np.where(qb < 0, -0.5 * (qb - rd), -0.5 * (qb + rd))
    with np.errstate(all="ignore"):
        r0, r1 = (q / qa).astype(np.float32), (qc / q).astype(np.float32)
    t0, t1 = np.minimum(r0, r1), np.maximum(r0, r1)
    stopped = real & (((t0 > f32(1e-4)) & (t0 < tmax)) | ((t1 > f32(1e-4)) & (t1 < tmax)))
    assert real.mean() > 0.5 and not stopped.any(), (int(stopped.sum()), np.flatnonzero(stopped)[:5])
    # how much of the margin the float32 test used up at worst: the gap between tmax and ITS near root, as a share of the margin
    X, D = x[m].astype(np.float64), d.astype(np.float64)
    OC = X[:, 0:3] - X[:, 6:9]
    b = (OC * D).sum(1) / np.linalg.norm(D, axis=1)
    dc2 = (OC * OC).sum(1)
    dq = b * b - (dc2 - X[:, 9] ** 2)
    hits = dq > 0
    half = np.sqrt(np.maximum(dq, 0.0))
    dc = np.sqrt(dc2)
    with np.errstate(all="ignore"):
        margin = np.minimum(2.0 ** -9 * dc, 2.0 ** -18 * dc2 / half)
    gap = (-b - half) - tmax
    assert (gap[hits] <= 2.0 * margin[hits] + 1.5e-4 * dc[hits]).all()
    used = 1.0 - (np.where(t0 > f32(1e-4), t0, t1).astype(np.float64) - tmax)[real & hits] / margin[real & hits]
    print("share of the margin used at worst: %.3f" % used.max())
    assert used.max() < 1.0
