"""The substrate material without a GPU: the parser, the validation of pbrt_hip_scene_create, the float64 reference
(tests/substrate_ref.py) against itself, and pbrt_amd/csrc/substrate_bsdf.hpp compiled for the host against that reference."""
import os

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import MATTE, SUBSTRATE, _lib, api, loader, scenes

import substrate_host_build as hb
import substrate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = """
LookAt 0 -4 1  0 0 0  0 0 1
Camera "perspective" "float fov" 40
Film "image" "integer xresolution" [16] "integer yresolution" [16]
WorldBegin
LightSource "infinite" "rgb L" [1 1 1]
"""
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0 1 -1 0 1 1 0 -1 1 0]\n'
f32 = lambda *v: tuple(np.float32(x) for x in v)  # noqa: E731


def _rows(sd):
    """[(Kd, Ks, alpha)] of the substrate materials of a loaded scene"""
    assert len(sd.mat_eta) == (len(sd.materials) if (sd.materials[:, 0] == SUBSTRATE).any() else 0)
    return [(tuple(m[1:4]), tuple(m[4:7]), float(sd.mat_eta[i])) for i, m in enumerate(sd.materials) if int(m[0]) == SUBSTRATE]


def _alpha1(roughness, remap=True):
    """one roughness to its alpha: 3.21's polynomial on the float32 roughness in double, rounded to float32, clamped to [1e-3, 1]"""
    r = float(np.float32(roughness))
    a = np.float32(r)
    if remap:
        x = np.log(max(r, 1e-3))
        a = np.float32(1.62142 + 0.819955 * x + 0.1734 * x ** 2 + 0.0171201 * x ** 3 + 0.000640711 * x ** 4)
    return float(min(max(a, np.float32(1e-3)), np.float32(1.0)))


def _alpha(u, v=None, remap=True):
    """3.24: the geometric mean of the two alphas, in double, rounded to float32"""
    return float(np.float32(np.sqrt(_alpha1(u, remap) * _alpha1(u if v is None else v, remap))))


def _near(a, b):
    return abs(a - b) <= float(np.spacing(np.float32(b)))  # (one ulp: log in double on two hosts)


def test_parser_reads_substrate():
    # the defaults: Kd = Ks = 0.5, both roughnesses 0.1 remapped; no warning, and above all not "not supported"
    ls = loader.load_string(HEAD + 'Material "substrate"\n' + QUAD + 'Shape "sphere" "float radius" 0.5\nWorldEnd\n')
    (kd, ks, al), = _rows(ls.scene)
    assert (kd, ks) == (f32(.5, .5, .5), f32(.5, .5, .5)) and _near(al, _alpha(0.1)) and int(ls.scene.spheres[0, 4]) == 0 and not ls.warnings, ls.warnings
    assert ls.scene.mat_tex.tolist() == [0]
    assert al == float(api.substrate_material()[1]) and api.substrate_material()[0] == [SUBSTRATE, .5, .5, .5, .5, .5, .5]
    # a named material with every parameter
    ls = loader.load_string(HEAD + 'MakeNamedMaterial "s" "string type" "substrate" "rgb Kd" [.1 .2 .3] "rgb Ks" [.4 .5 .6] "float uroughness" 0.3 '
                            '"float vroughness" 0.3\nNamedMaterial "s"\n' + QUAD + "WorldEnd\n")
    (kd, ks, al), = _rows(ls.scene)
    assert (kd, ks) == (f32(.1, .2, .3), f32(.4, .5, .6)) and _near(al, _alpha(0.3)) and 0.8 < al < 0.9
    assert not ls.warnings, ls.warnings
    # remaproughness false: alpha is the roughness
    ls = loader.load_string(HEAD + 'Material "substrate" "float uroughness" 0.25 "float vroughness" 0.25 "bool remaproughness" "false"\n' + QUAD + "WorldEnd\n")
    assert _rows(ls.scene)[0][2] == 0.25 and not ls.warnings, ls.warnings


@pytest.mark.parametrize("u,v", [(0.05, 0.2), (0.2, 0.05), (0.01, 0.3), (0.1, 1.0)])
def test_parser_takes_the_geometric_mean_of_two_roughnesses(u, v):
    ls = loader.load_string(HEAD + 'Material "substrate" "float uroughness" %r "float vroughness" %r\n' % (u, v) + QUAD + "WorldEnd\n")
    got = _rows(ls.scene)[0][2]
    assert _near(got, _alpha(u, v)) and got == float(api.substrate_material(uroughness=u, vroughness=v)[1]), (got, _alpha(u, v))
    assert [w for w in ls.warnings if "substrate" in w and "vroughness" in w], ls.warnings
    clamped = [w for w in ls.warnings if "substrate" in w and "clamped" in w]
    assert bool(clamped) == (max(u, v) >= 0.5), ls.warnings  # (the polynomial leaves [0, 1] from roughness 0.4 on: 3.21)
    assert not [w for w in ls.warnings if "not supported by this path" in w]


def test_parser_warnings_and_merging():
    ls = loader.load_string(HEAD + 'Material "substrate" "float uroughness" 0.0001 "float vroughness" 0.0001 "bool remaproughness" "false"\n' + QUAD + "WorldEnd\n")
    assert _rows(ls.scene)[0][2] == float(np.float32(1e-3)) and [w for w in ls.warnings if "substrate" in w and "clamped" in w], ls.warnings
    # Ks above 1 is clamped to 1, and said so
    ls = loader.load_string(HEAD + 'Material "substrate" "rgb Ks" [0.5 1.5 1]\n' + QUAD + "WorldEnd\n")
    assert _rows(ls.scene)[0][1] == f32(0.5, 1, 1) and [w for w in ls.warnings if "substrate" in w and "Ks" in w and "clamped" in w], ls.warnings
    assert api.substrate_material(ks=(0.5, 1.5, 1))[0][4:7] == [0.5, 1.0, 1.0]
    # a texture on Kd / Ks collapses to its constant; a roughness texture and a bump map are named
    tex = 'Texture "c" "spectrum" "constant" "rgb value" [.2 .3 .4]\nTexture "b" "float" "constant" "float value" 1\n'
    ls = loader.load_string(HEAD + tex + 'Material "substrate" "texture Kd" "c" "texture Ks" "c"\n' + QUAD + "WorldEnd\n")
    assert not [w for w in ls.warnings if "not supported by this path" in w], ls.warnings
    assert _rows(ls.scene)[0][:2] == (f32(.2, .3, .4), f32(.2, .3, .4)) and ls.scene.mat_tex.tolist() == [0]
    for param, name in (('"texture uroughness" "b"', "uroughness"), ('"texture vroughness" "b"', "vroughness"), ('"texture bumpmap" "b"', "bumpmap")):
        ls = loader.load_string(HEAD + tex + 'Material "substrate" ' + param + "\n" + QUAD + "WorldEnd\n")
        assert [w for w in ls.warnings if name in w and "substrate" in w], (name, ls.warnings)
        assert not [w for w in ls.warnings if "not supported by this path" in w], ls.warnings
        assert _near(_rows(ls.scene)[0][2], _alpha(0.1))
    # equal materials merge; materials that differ only in alpha do not
    a, b = 'Material "substrate" "float uroughness" 0.1 "float vroughness" 0.1\n', 'Material "substrate" "float uroughness" 0.2 "float vroughness" 0.2\n'
    ls = loader.load_string(HEAD + a + QUAD + b + QUAD + a + QUAD + "WorldEnd\n")
    assert len(_rows(ls.scene)) == 2 and ls.scene.mat_id.tolist() == [0, 0, 1, 1, 0, 0]
    # a substrate material and a plastic one of the same words are two materials
    ls = loader.load_string(HEAD + 'Material "substrate" "rgb Kd" [.25 .25 .25] "rgb Ks" [.25 .25 .25]\n' + QUAD + 'Material "plastic"\n' + QUAD + "WorldEnd\n")
    assert ls.scene.materials[:, 0].tolist() == [SUBSTRATE, pbrt_amd.PLASTIC] and ls.scene.mat_id.tolist() == [0, 0, 1, 1]
    # substrate under an area light: the shape emits, as black matte, and the parser says so
    ls = loader.load_string(HEAD + 'AreaLightSource "diffuse" "rgb L" [3 2 1]\nMaterial "substrate"\n' + QUAD + "WorldEnd\n")
    assert ls.scene.materials.tolist() == [[MATTE, 0, 0, 0, 3, 2, 1]] and [w for w in ls.warnings if "substrate" in w and "AreaLightSource" in w]
    # a mesh's normals in a file with substrate are dropped, and said so: the scene stays one that scene creation takes
    ls = loader.load_string(HEAD + 'Material "substrate"\n' + QUAD.replace("\n", ' "normal N" [0 0 1 0 0 1 0 0 1 0 0 1]\n') + "WorldEnd\n")
    assert ls.scene.tri_n.shape[0] == 0 and [w for w in ls.warnings if "substrate" in w and "normals" in w], ls.warnings
    # metal and uber keep their fallback and its warning, word for word
    for name in ("metal", "uber"):
        ls = loader.load_string(HEAD + 'Material "%s"\n' % name + QUAD + "WorldEnd\n")
        assert 'Material "%s" is not supported by this path: using matte Kd 0.5' % name in ls.warnings and ls.scene.materials.tolist() == [[MATTE, .5, .5, .5, 0, 0, 0]]


def test_scene_file_equals_the_generator():
    """scenes/substrate_spheres.pbrt loads to the arrays scenes.substrate_scene builds"""
    ls = loader.load_file(os.path.join(ROOT, "scenes", "substrate_spheres.pbrt"))
    sd = scenes.substrate_scene(256, 256)
    # (roughness 0.4 remaps to 1.003: each of the orange sphere's two roughnesses is clamped to 1, and said so)
    assert ls.warnings and all("clamped" in w and "substrate" in w for w in ls.warnings), ls.warnings
    for f in ("P", "idx", "mat_id", "materials", "lights", "spheres", "cam_to_world", "mat_tex", "tri_uv", "textures", "mat_eta"):
        a, b = getattr(ls.scene, f), getattr(sd, f)
        assert a.shape == b.shape and np.array_equal(a, b), (f, a, b)
    assert (sd.materials[:, 0] == SUBSTRATE).sum() == 3 and len(sd.idx) <= 40 and len(sd.spheres) == 2
    assert (ls.scene.fov, ls.scene.xres, ls.scene.yres, ls.max_depth) == (40.0, 256, 256, 5)
    matte = scenes.substrate_scene(256, 256, substrate=False)
    assert (matte.materials[:, 0] == MATTE).all() and np.array_equal(matte.materials[:, 1:4], sd.materials[:, 1:4]) and len(matte.mat_eta) == 0


def _create(sd):
    try:
        pbrt_amd.Scene(sd).close()
    except _lib.PbrtHipError as e:
        return e.code, str(e)
    return 0, ""


def test_substrate_is_validated_before_any_device_work():
    def scene(row=None, alpha=None, **kw):
        sd = scenes.substrate_scene(8, 8)
        m = sd.materials.copy()
        if row is not None:
            m[5, row[0]] = row[1]
        sd.materials = m
        if alpha is not None:
            sd.mat_eta = sd.mat_eta.copy()
            sd.mat_eta[5] = alpha
        for k, v in kw.items():
            setattr(sd, k, v)
        return sd
    # alpha outside [1e-3, 1] or not finite; Kd negative or not finite; Ks negative, not finite or ABOVE ONE
    for kw in (dict(alpha=np.nan), dict(alpha=0.0), dict(alpha=2.0), dict(alpha=np.inf), dict(alpha=5e-4), dict(row=(4, -1.0)), dict(row=(6, np.nan)),
               dict(row=(1, np.inf)), dict(row=(2, -0.5)), dict(row=(3, np.nan)), dict(row=(5, 1.5)), dict(row=(4, np.inf)), dict(row=(6, np.float32(1.0) + np.float32(2.0 ** -23)))):
        code, msg = _create(scene(**kw))
        assert code == -1 and "substrate" in msg, (kw, code, msg)
    # type 5 is no material
    sd = scene()
    sd.materials[5, 0] = 5
    code, msg = _create(sd)
    assert code == -1 and "unknown material type" in msg and "substrate" not in msg, (code, msg)
    # substrate beside an environment-map slot or a normals slot: a limit of the kernel families, said at creation
    env = dict(envmap=np.full((2, 4, 3), 0.5, np.float32), lights=np.array([[pbrt_amd.LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32))
    nrm = dict(tri_n=np.tile(np.array([0, 0, 1], np.float32), (12, 3)))
    for kw in (env, nrm):
        code, msg = _create(scene(**kw))
        assert code == -4 and "substrate" in msg and "plastic" not in msg, (list(kw), code, msg)
        sd = scenes.substrate_scene(8, 8, substrate=False)  # (control: the same scene as matte is fine)
        for k, v in kw.items():
            setattr(sd, k, v)
        code, msg = _create(sd)
        assert code == (0 if pbrt_amd.device_count() > 0 else -2), (list(kw), code, msg)
        # plastic beside substrate: plastic's message, word for word
        sd = scene(**kw)
        sd.materials[6, 0] = pbrt_amd.PLASTIC
        code, msg = _create(sd)
        assert code == -4 and "a plastic material is not available in a scene with " in msg, (code, msg)
    # a valid substrate scene (alpha and Ks at both ends included) passes the validation: what stops it is the missing device, if it is missing
    for kw in (dict(), dict(alpha=np.float32(1e-3)), dict(alpha=np.float32(1.0)), dict(row=(4, 0.0)), dict(row=(4, 1.0)), dict(row=(1, 7.0))):
        code, msg = _create(scene(**kw))
        assert code == (0 if pbrt_amd.device_count() > 0 else -2), (kw, code, msg)
    version = _lib.lib().pbrt_hip_version().decode()
    assert "0.13" in version and all(v in version for v in ("0.6", "0.7", "0.8", "0.9", "0.10", "0.11", "0.12"))
    assert "pbrt_hip_substrate_eval_device" in _lib.SYMBOLS and pbrt_amd.SUBSTRATE == 4


# ---- the reference against itself, float64 ----

def _dirs_theta(n_theta, n_phi):
    """midpoints of a grid uniform in (theta, phi) over the hemisphere, and each one's solid angle: it resolves a lobe about the normal"""
    th = (np.arange(n_theta) + 0.5) * (np.pi / 2) / n_theta
    phi = (np.arange(n_phi) + 0.5) * 2 * np.pi / n_phi
    th, phi = (v.ravel() for v in np.meshgrid(th, phi, indexing="ij"))
    return np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)], 1), np.sin(th) * (np.pi / 2 / n_theta) * (2 * np.pi / n_phi)


def test_reference_is_reciprocal():
    x = hb.domain_inputs(4096, seed=5).astype(np.float64)
    for k in (0, 3, 6):  # (unit in float64: ih is wi . wh, and wo . wh equals it only for unit vectors)
        x[:, k:k + 3] /= np.linalg.norm(x[:, k:k + 3], axis=1, keepdims=True)
    f_ab, _ = ref.eval_f_pdf(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 11:14], x[:, 14:17], x[:, 17])
    f_ba, _ = ref.eval_f_pdf(x[:, 0:3], x[:, 6:9], x[:, 3:6], x[:, 11:14], x[:, 14:17], x[:, 17])
    assert (f_ab > 0).all() and np.abs(f_ab / f_ba - 1.0).max() < 1e-12


@pytest.mark.parametrize("alpha", [0.1, 0.5, 1.0])
def test_reference_density_integrates_to_one(alpha):
    """pdf_b over the hemisphere, by quadrature: one minus the mass of reflections that leave below the surface (the sampler drops those: at
    normal incidence 1/2 + 1/2 / (1 + alpha^2) in closed form, 3.21 -- the density is plastic's --, never more than one); together with the
    dropped mass, counted from the half vectors' own density D cos, it is one"""
    wh, dw = _dirs_theta(1 << 16, 1)
    assert abs((ref.ggx_d(wh[:, 2], alpha) * wh[:, 2] * dw).sum() - 1.0) < 1e-6
    wi, dw = _dirs_theta(1024, 1024)
    nf = np.tile([0.0, 0.0, 1.0], (len(wi), 1))
    wh, dwh = _dirs_theta(1024, 1024)
    for theta_o in (0.0, 60.0, 80.0):
        t = np.radians(theta_o)
        wo = np.tile([np.sin(t), 0.0, np.cos(t)], (len(wi), 1))
        _, pdf = ref.eval_f_pdf(nf, wo, wi, np.full(3, 0.5), np.full(3, 0.5), alpha)
        total = (pdf * dw).sum()
        # the half vectors whose reflection of wo is kept: wo . wh > 0 and the reflected direction above the surface
        oh = (wo * wh).sum(1)
        kept = (oh > 0) & ((-wo + wh * (2.0 * oh)[:, None])[:, 2] > 0)
        mass = (ref.ggx_d(wh[:, 2], alpha) * wh[:, 2] * dwh * kept).sum()
        print(f"alpha {alpha} theta_o {theta_o}: pdf_b integrates to {total:.6f}, 1/2 + 1/2 x the kept half vectors' mass {0.5 + 0.5 * mass:.6f}")
        assert total <= 1.0 + 1e-4 and abs(total - (0.5 + 0.5 * mass)) < 2e-3, (theta_o, total, mass)
        if theta_o == 0.0:
            assert abs(total - (0.5 + 0.5 / (1.0 + alpha * alpha))) < 1e-4, total


@pytest.mark.parametrize("alpha", [0.1, 0.5])
@pytest.mark.parametrize("theta_o", [0.0, 60.0, 80.0])
def test_reference_sampler_weight_averages_to_the_albedo(theta_o, alpha):
    """the Monte Carlo mean of the sampler's weight f cos / pdf_b over 2^20 draws equals albedo() -- quadrature of f cos -- within 5 standard errors"""
    n, kd, ks = 1 << 20, 0.6, 0.4
    r = np.random.default_rng(23)
    t = np.radians(theta_o)
    nf = np.tile([0.0, 0.0, 1.0], (n, 1))
    wo = np.tile([np.sin(t), 0.0, np.cos(t)], (n, 1))
    _, w, _, alive = ref.sample_f(nf, wo, r.uniform(0, 1, n), r.uniform(0, 1, n), np.full(3, kd), np.full(3, ks), alpha)
    mean, se = w[:, 0].mean(), w[:, 0].std(ddof=1) / np.sqrt(n)
    want = ref.albedo(t, alpha, kd, ks, n=1024)
    print(f"theta_o {theta_o} alpha {alpha}: mean weight {mean:.5f} +- {se:.1e}, albedo {want:.5f}; {100 * alive.mean():.1f} % of the samples live")
    assert 0.05 < want <= 1.0 and abs(mean - want) <= 5 * se + 1e-4 * want, (mean, want, se)  # (1e-4: the quadrature's own error at the lobe's peak)


# ---- the header, compiled for the host, against the reference ----

# Measured on the first run over domain_inputs() (2^16 inputs; cos_o, cos_i in [0.05, 1], alpha in [0.05, 1], Kd, Ks in [0, 1]): the largest
# relative error of f, of pdf_b and of f cos / pdf_b, and the largest angle between the two sampled directions (DESIGN.md 3.24's table says
# where each comes from).  Asserted at TWICE the measured value.
MEASURED = dict(f=5.230e-5, pdf=5.180e-5, weight=2.577e-3, angle=8.360e-5)


def _rel(a, b):
    assert ((b == 0) <= (a == 0)).all()  # (an exact zero of the reference is one of the header)
    with np.errstate(all="ignore"):
        return np.where(b != 0, np.abs(a - b) / np.abs(b), 0.0)


def test_header_on_the_host_matches_float64(tmp_path):
    exe = hb.build(tmp_path)
    x = hb.domain_inputs()
    assert len(x) == 1 << 16
    y = hb.run(exe, x, tmp_path).astype(np.float64)
    X = x.astype(np.float64)
    nf, wo, wi, kd, ks, al = X[:, 0:3], X[:, 3:6], X[:, 6:9], X[:, 11:14], X[:, 14:17], X[:, 17]
    f, pdf = ref.eval_f_pdf(nf, wo, wi, kd, ks, al)
    wis, w, _, alive = ref.sample_f(nf, wo, x[:, 9], x[:, 10], kd, ks, al)
    assert (pdf > 0).all() and alive.sum() > len(x) // 2
    alive_h = (y[:, 4:7] != 0).any(1)
    assert np.array_equal(alive_h, alive)  # every input counts: a sample dies in both or in neither
    angle = np.arctan2(np.linalg.norm(np.cross(y[alive, 4:7], wis[alive]), axis=1), (y[alive, 4:7] * wis[alive]).sum(1))  # (sound near 0, where acos is not)
    got = dict(f=_rel(y[:, 0:3], f).max(), pdf=_rel(y[:, 3], pdf).max(), weight=_rel(y[alive, 7:10], w[alive]).max(),
               angle=float(angle.max()))
    print("measured:", {k: f"{v:.3e}" for k, v in got.items()})
    assert (y[~alive, 4:10] == 0).all()
    for k, v in got.items():
        assert v <= 2.0 * MEASURED[k], (k, v, MEASURED[k])
    # the edge inputs are finite on the host, and zero where 3.24 says zero (the device must reproduce them bit for bit: tests/test_substrate_gpu.py)
    xe = hb.edge_inputs()
    ye = hb.run(exe, xe, tmp_path)
    assert np.isfinite(ye).all() and (ye[:, 0:4] >= 0).all() and (ye[:, 7:10] >= 0).all()
    Xe = xe.astype(np.float64)
    fe, pe = ref.eval_f_pdf(Xe[:, 0:3], Xe[:, 3:6], Xe[:, 6:9], Xe[:, 11:14], Xe[:, 14:17], Xe[:, 17])
    below = (xe[:, 6:9] * xe[:, 0:3]).sum(1, dtype=np.float32) < -1e-6  # (wi clearly under the surface, whatever the rounding of the dot product)
    assert below.sum() > 100 and (ye[below, 0:4] == 0).all() and (fe[below] == 0).all() and (pe[below] == 0).all()
