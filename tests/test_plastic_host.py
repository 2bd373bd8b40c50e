"""The plastic material without a GPU: the parser, the validation of pbrt_hip_scene_create, the float64 reference
(tests/plastic_ref.py) against itself, and pbrt_amd/csrc/plastic_bsdf.hpp compiled for the host against that reference."""
import os

import numpy as np
import pytest

import pbrt_amd
from pbrt_amd import MATTE, PLASTIC, _lib, api, loader, scenes

import plastic_host_build as hb
import plastic_ref as ref

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
    """[(Kd, Ks, alpha)] of the plastic materials of a loaded scene"""
    assert len(sd.mat_eta) == (len(sd.materials) if (sd.materials[:, 0] == PLASTIC).any() else 0)
    return [(tuple(m[1:4]), tuple(m[4:7]), float(sd.mat_eta[i])) for i, m in enumerate(sd.materials) if int(m[0]) == PLASTIC]


def _alpha(roughness):
    """the issue's polynomial on the float32 roughness in double, rounded to float32, clamped to [1e-3, 1]"""
    return float(min(max(np.float32(ref.roughness_to_alpha(float(np.float32(roughness)))), np.float32(1e-3)), np.float32(1.0)))


def test_parser_reads_plastic():
    # the defaults: Kd = Ks = 0.25, roughness 0.1 remapped; no warning, and above all not "not supported"
    ls = loader.load_string(HEAD + 'Material "plastic"\n' + QUAD + 'Shape "sphere" "float radius" 0.5\nWorldEnd\n')
    assert _rows(ls.scene) == [(f32(.25, .25, .25), f32(.25, .25, .25), _alpha(0.1))] and int(ls.scene.spheres[0, 4]) == 0 and not ls.warnings, ls.warnings
    assert ls.scene.mat_tex.tolist() == [0]
    # a named material with every parameter
    ls = loader.load_string(HEAD + 'MakeNamedMaterial "p" "string type" "plastic" "rgb Kd" [.1 .2 .3] "rgb Ks" [.4 .5 .6] "float roughness" 0.3\n'
                            'NamedMaterial "p"\n' + QUAD + "WorldEnd\n")
    assert _rows(ls.scene) == [(f32(.1, .2, .3), f32(.4, .5, .6), _alpha(0.3))] and 0.8 < _alpha(0.3) < 0.9
    assert not [w for w in ls.warnings if "not supported" in w], ls.warnings
    # remaproughness false: alpha is the roughness
    ls = loader.load_string(HEAD + 'Material "plastic" "float roughness" 0.3 "bool remaproughness" "false"\n' + QUAD + "WorldEnd\n")
    assert _rows(ls.scene)[0][2] == float(np.float32(0.3)) and not ls.warnings, ls.warnings


@pytest.mark.parametrize("roughness", [0.01, 0.1, 0.5, 1.0])
def test_parser_remaps_roughness_by_the_polynomial(roughness):
    ls = loader.load_string(HEAD + 'Material "plastic" "float roughness" %r\n' % roughness + QUAD + "WorldEnd\n")
    x = np.log(max(float(np.float32(roughness)), 1e-3))
    want = np.float32(1.62142 + 0.819955 * x + 0.1734 * x ** 2 + 0.0171201 * x ** 3 + 0.000640711 * x ** 4)
    want = min(max(want, np.float32(1e-3)), np.float32(1.0))
    got = _rows(ls.scene)[0][2]
    assert abs(got - float(want)) <= float(np.spacing(want)), (got, want)  # (one ulp: log in double on two hosts)
    assert got == float(api.roughness_to_alpha(roughness))
    clamped = [w for w in ls.warnings if "plastic" in w and "clamped" in w]
    assert bool(clamped) == (roughness >= 0.5), ls.warnings  # (the polynomial gives 1.13 at roughness 0.5 and 1.62 at 1: pbrt-v3's remap leaves [0, 1] there)


def test_parser_warnings_and_merging():
    ls = loader.load_string(HEAD + 'Material "plastic" "float roughness" 0.0001 "bool remaproughness" "false"\n' + QUAD + "WorldEnd\n")
    assert _rows(ls.scene)[0][2] == float(np.float32(1e-3)) and [w for w in ls.warnings if "plastic" in w and "clamped" in w], ls.warnings
    # a texture on Kd / Ks collapses to its constant (the Texture directive's own warning, if it has one, is all that is said); a roughness
    # texture and a bump map are named
    tex = 'Texture "c" "spectrum" "constant" "rgb value" [.2 .3 .4]\nTexture "b" "float" "constant" "float value" 1\n'
    ls = loader.load_string(HEAD + tex + 'Material "plastic" "texture Kd" "c" "texture Ks" "c"\n' + QUAD + "WorldEnd\n")
    assert not [w for w in ls.warnings if "not supported by this path" in w], ls.warnings
    assert len(_rows(ls.scene)) == 1 and ls.scene.mat_tex.tolist() == [0]
    for param, name in (('"texture roughness" "b"', "roughness"), ('"texture bumpmap" "b"', "bumpmap")):
        ls = loader.load_string(HEAD + tex + 'Material "plastic" ' + param + "\n" + QUAD + "WorldEnd\n")
        assert [w for w in ls.warnings if name in w and "plastic" in w], (name, ls.warnings)
        assert not [w for w in ls.warnings if "not supported by this path" in w], ls.warnings
        assert _rows(ls.scene)[0][2] == _alpha(0.1)
    # equal materials merge; materials that differ only in alpha do not
    ls = loader.load_string(HEAD + 'Material "plastic" "float roughness" 0.1\n' + QUAD + 'Material "plastic" "float roughness" 0.2\n' + QUAD +
                            'Material "plastic" "float roughness" 0.1\n' + QUAD + "WorldEnd\n")
    assert [r[2] for r in _rows(ls.scene)] == [_alpha(0.1), _alpha(0.2)] and ls.scene.mat_id.tolist() == [0, 0, 1, 1, 0, 0]
    # plastic under an area light: the shape emits, as black matte, and the parser says so
    ls = loader.load_string(HEAD + 'AreaLightSource "diffuse" "rgb L" [3 2 1]\nMaterial "plastic"\n' + QUAD + "WorldEnd\n")
    assert ls.scene.materials.tolist() == [[MATTE, 0, 0, 0, 3, 2, 1]] and [w for w in ls.warnings if "plastic" in w and "AreaLightSource" in w]
    # a mesh's normals in a file with plastic are dropped, and said so: the scene stays one that scene creation takes
    ls = loader.load_string(HEAD + 'Material "plastic"\n' + QUAD.replace("\n", ' "normal N" [0 0 1 0 0 1 0 0 1 0 0 1]\n') + "WorldEnd\n")
    assert ls.scene.tri_n.shape[0] == 0 and [w for w in ls.warnings if "plastic" in w and "normals" in w], ls.warnings
    # metal is still out
    ls = loader.load_string(HEAD + 'Material "metal"\n' + QUAD + "WorldEnd\n")
    assert [w for w in ls.warnings if "not supported" in w] and int(ls.scene.materials[0, 0]) == MATTE


def test_scene_file_equals_the_generator():
    """scenes/plastic_spheres.pbrt loads to the arrays scenes.plastic_scene builds"""
    ls = loader.load_file(os.path.join(ROOT, "scenes", "plastic_spheres.pbrt"))
    sd = scenes.plastic_scene(256, 256)
    # (roughness 0.4 remaps to 1.003: the one warning is its clamp to 1)
    assert len(ls.warnings) == 1 and "clamped" in ls.warnings[0] and not [w for w in ls.warnings if "not supported" in w], ls.warnings
    for f in ("P", "idx", "mat_id", "materials", "lights", "spheres", "cam_to_world", "mat_tex", "tri_uv", "textures", "mat_eta"):
        a, b = getattr(ls.scene, f), getattr(sd, f)
        assert a.shape == b.shape and np.array_equal(a, b), (f, a, b)
    assert (sd.materials[:, 0] == PLASTIC).sum() == 3 and len(sd.idx) <= 40 and len(sd.spheres) == 2
    assert (ls.scene.fov, ls.scene.xres, ls.scene.yres, ls.max_depth) == (40.0, 256, 256, 5)


def _create(sd):
    try:
        pbrt_amd.Scene(sd).close()
    except _lib.PbrtHipError as e:
        return e.code, str(e)
    return 0, ""


def test_plastic_is_validated_before_any_device_work():
    def scene(row=None, alpha=None, **kw):
        sd = scenes.plastic_scene(8, 8)
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
    for kw in (dict(alpha=np.nan), dict(alpha=0.0), dict(alpha=2.0), dict(alpha=np.inf), dict(alpha=5e-4), dict(row=(4, -1.0)), dict(row=(6, np.nan)),
               dict(row=(1, np.inf)), dict(row=(2, -0.5))):
        code, msg = _create(scene(**kw))
        assert code == -1 and "plastic" in msg, (kw, code, msg)
    # a type-3 record with nothing of plastic in it (no Ks, no alpha word) is what it was before there was plastic: an unknown type
    sd = scene(row=(4, 0.0), alpha=0.0)
    sd.materials[5, 4:7] = 0
    code, msg = _create(sd)
    assert code == -1 and "unknown material type" in msg and "plastic" not in msg, (code, msg)
    # plastic beside an environment-map slot or a normals slot: a limit of the kernel families, said at creation
    env = dict(envmap=np.full((2, 4, 3), 0.5, np.float32), lights=np.array([[pbrt_amd.LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]], np.float32))
    nrm = dict(tri_n=np.tile(np.array([0, 0, 1], np.float32), (12, 3)))
    for kw in (env, nrm):
        code, msg = _create(scene(**kw))
        assert code == -4 and "plastic" in msg, (list(kw), code, msg)
        sd = scene(**kw)  # (the same scene without plastic is fine)
        sd.materials[:, 0] = np.where(sd.materials[:, 0] == PLASTIC, MATTE, sd.materials[:, 0])
        sd.materials[:, 4:7] = np.where((scenes.plastic_scene(8, 8).materials[:, :1] == PLASTIC), 0, sd.materials[:, 4:7])
        code, msg = _create(sd)
        assert code == (0 if pbrt_amd.device_count() > 0 else -2), (list(kw), code, msg)
    # a valid plastic scene (alpha at both ends included) passes the validation: what stops it is the missing device, if it is missing
    for alpha in (None, 1e-3, 1.0):
        code, msg = _create(scene(alpha=None if alpha is None else np.float32(alpha)))
        assert code == (0 if pbrt_amd.device_count() > 0 else -2), (alpha, code, msg)
    assert b"0.11" in _lib.lib().pbrt_hip_version() and b"0.6" in _lib.lib().pbrt_hip_version()
    assert "pbrt_hip_plastic_eval_device" in _lib.SYMBOLS


# ---- the reference against itself, float64 ----

def _dirs(n_mu, n_phi):
    mu = (np.arange(n_mu) + 0.5) / n_mu
    phi = (np.arange(n_phi) + 0.5) * 2 * np.pi / n_phi
    mu, phi = (v.ravel() for v in np.meshgrid(mu, phi, indexing="ij"))
    st = np.sqrt(1.0 - mu * mu)
    return np.stack([st * np.cos(phi), st * np.sin(phi), mu], 1), 2 * np.pi / (n_mu * n_phi)


def _dirs_theta(n_theta, n_phi):
    """midpoints of a grid uniform in (theta, phi) over the hemisphere, and each one's solid angle: it resolves a lobe about the normal"""
    th = (np.arange(n_theta) + 0.5) * (np.pi / 2) / n_theta
    phi = (np.arange(n_phi) + 0.5) * 2 * np.pi / n_phi
    th, phi = (v.ravel() for v in np.meshgrid(th, phi, indexing="ij"))
    return np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)], 1), np.sin(th) * (np.pi / 2 / n_theta) * (2 * np.pi / n_phi)


def test_reference_is_reciprocal():
    x = hb.domain_inputs(4096, seed=5).astype(np.float64)
    for k in (0, 3, 6):  # (unit in float64: F takes wi . wh, and wo . wh equals it only for unit vectors)
        x[:, k:k + 3] /= np.linalg.norm(x[:, k:k + 3], axis=1, keepdims=True)
    f_ab, _ = ref.eval_f_pdf(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 11:14], x[:, 14:17], x[:, 17])
    f_ba, _ = ref.eval_f_pdf(x[:, 0:3], x[:, 6:9], x[:, 3:6], x[:, 11:14], x[:, 14:17], x[:, 17])
    assert (f_ab > 0).all() and np.abs(f_ab / f_ba - 1.0).max() < 1e-12


@pytest.mark.parametrize("alpha", [0.1, 0.5, 1.0])
def test_reference_density_and_energy(alpha):
    """D cos is a density over half vectors; pdf_b integrates to one minus the mass of reflections that leave below the surface (the sampler
    drops those: at normal incidence 1/2 + 1/2 / (1 + alpha^2) in closed form, never more than one); f cos integrates to at most one for Kd + Ks <= 1"""
    wh, dw = _dirs_theta(1 << 16, 1)
    assert abs((ref.ggx_d(wh[:, 2], alpha) * wh[:, 2] * dw).sum() - 1.0) < 1e-6
    wi, dw = _dirs_theta(1024, 1024)
    nf = np.tile([0.0, 0.0, 1.0], (len(wi), 1))
    for theta_o in (0.0, 60.0, 80.0):
        t = np.radians(theta_o)
        wo = np.tile([np.sin(t), 0.0, np.cos(t)], (len(wi), 1))
        for kd, ks in ((0.5, 0.5), (0.0, 1.0), (1.0, 0.0)):
            f, pdf = ref.eval_f_pdf(nf, wo, wi, np.full(3, kd), np.full(3, ks), alpha)
            total, energy = (pdf * dw).sum(), (f[:, 0] * wi[:, 2] * dw).sum()
            assert total <= 1.0 + 1e-4 and energy <= 1.0 + 1e-4, (theta_o, kd, ks, total, energy)
            if theta_o == 0.0:  # (half vectors beyond 45 degrees reflect below the surface: tan^2 > 1, a share alpha^2 / (1 + alpha^2) of the lobe)
                assert abs(total - (0.5 + 0.5 / (1.0 + alpha * alpha))) < 1e-4, total
            if ks == 0.0:
                assert abs(energy - kd) < 1e-4


def _chi2_quantile(dof, p_tail=1e-6):
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p_tail, dof))
    except ImportError:  # Wilson-Hilferty's cube-root normal approximation of the same quantile (z = the normal's at 1e-6)
        z = 4.753424
        return dof * (1.0 - 2.0 / (9.0 * dof) + z * np.sqrt(2.0 / (9.0 * dof))) ** 3


@pytest.mark.parametrize("theta_o,alpha", [(0.0, 0.3), (60.0, 0.3), (75.0, 0.6)])
def test_reference_sampler_matches_its_density(theta_o, alpha):
    """2^20 draws of the two-lobe sampler, binned over 16 x 32 (cos theta, phi) cells, against the integral of pdf_b over each cell (16 x 16
    midpoints): chi^2 over the cells with expectation >= 50 below the chi^2 distribution's quantile at a tail of 1e-6"""
    n, n_mu, n_phi, sub = 1 << 20, 16, 32, 16
    r = np.random.default_rng(17)
    t = np.radians(theta_o)
    nf = np.tile([0.0, 0.0, 1.0], (n, 1))
    wo = np.tile([np.sin(t), 0.0, np.cos(t)], (n, 1))
    wi, ok = ref.sample_wi(nf, wo, r.uniform(0, 1, n), r.uniform(0, 1, n), alpha)
    ok &= wi[:, 2] > 0
    wi = wi[ok] / np.linalg.norm(wi[ok], axis=1, keepdims=True)
    im = np.minimum((wi[:, 2] * n_mu).astype(np.int64), n_mu - 1)
    ip = np.minimum((np.mod(np.arctan2(wi[:, 1], wi[:, 0]), 2 * np.pi) / (2 * np.pi) * n_phi).astype(np.int64), n_phi - 1)
    got = np.bincount(im * n_phi + ip, minlength=n_mu * n_phi).astype(np.float64)
    d, dw = _dirs(n_mu * sub, n_phi * sub)
    _, pdf = ref.eval_f_pdf(np.tile([0.0, 0.0, 1.0], (len(d), 1)), np.tile(wo[0], (len(d), 1)), d, np.ones(3), np.ones(3), alpha)
    want = n * dw * pdf.reshape(n_mu, sub, n_phi, sub).sum((1, 3)).ravel()
    use = want >= 50
    chi2 = float((((got - want) ** 2 / np.maximum(want, 1e-300))[use]).sum())
    bound = _chi2_quantile(int(use.sum()))
    print(f"theta_o {theta_o} alpha {alpha}: chi^2 {chi2:.1f} over {int(use.sum())} cells, bound {bound:.1f}; {int(got[~use].sum())} draws in the other cells")
    assert use.sum() >= 100 and chi2 < bound
    # the negative control: the lobe chosen at 1/3 while the density says 1/2 is found out
    wi, ok = ref.sample_wi(nf, wo, r.uniform(0, 1, n), r.uniform(0, 1, n), alpha, lobe_pick=1.0 / 3.0)
    ok &= wi[:, 2] > 0
    wi = wi[ok] / np.linalg.norm(wi[ok], axis=1, keepdims=True)
    im = np.minimum((wi[:, 2] * n_mu).astype(np.int64), n_mu - 1)
    ip = np.minimum((np.mod(np.arctan2(wi[:, 1], wi[:, 0]), 2 * np.pi) / (2 * np.pi) * n_phi).astype(np.int64), n_phi - 1)
    bad = np.bincount(im * n_phi + ip, minlength=n_mu * n_phi).astype(np.float64)
    assert float((((bad - want) ** 2 / np.maximum(want, 1e-300))[use]).sum()) > 10 * bound


# ---- the header, compiled for the host, against the reference ----

# Measured on the first run over domain_inputs() (2^16 inputs; cos_o, cos_i in [0.05, 1], alpha in [0.05, 1], Kd, Ks in [0, 1]): the largest
# relative error of f, of pdf_b and of f cos / pdf_b, and the largest angle between the two sampled directions (DESIGN.md 3.21's table; where
# they come from: e = c^2 (alpha^2 - 1) + 1 cancels to alpha^2 at the lobe's peak, sin theta = sqrt(1 - cos^2 theta) cancels for a half
# vector close to the normal, and a sampled direction near the horizon has a cosine of a few ulps).  Asserted at TWICE the measured value.
MEASURED = dict(f=3.98e-5, pdf=5.19e-5, weight=2.58e-3, angle=8.37e-5)


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
    # the edge inputs are finite on the host (the device must reproduce them bit for bit: tests/test_plastic_gpu.py)
    ye = hb.run(exe, hb.edge_inputs(), tmp_path)
    assert np.isfinite(ye).all() and (ye[:, 0:4] >= 0).all() and (ye[:, 7:10] >= 0).all()
