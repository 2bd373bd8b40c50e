"""The sphere light of DESIGN.md 3.25 in float64 numpy, written from the section's text and sharing nothing with
pbrt_amd/csrc/sphere_light.hpp: the light sample, the hit side's density, and the path loop of tests/spot_ref.py restated for scenes of
matte, mirror and plastic materials over triangles and spheres under point, distant, constant-infinite, area, spot and SPHERE lights (the
plastic BSDF is tests/plastic_ref.py's, the spot light's sample tests/spot_ref.py's).  Glass and the mapped lights are not restated here.
The loop draws the SAME RANDOM NUMBERS as the library (3.1, 3.10, 3.12 - 3.14: the samplers are the twin's own classes, imported), so
sample s of pixel (x, y) is the same path up to rounding and films compare directly.

`wrong` exists for negative controls, which must FAIL the bars the right reference meets: "area" puts the density of sampling the
sphere's AREA uniformly, t^2 / (4 pi r^2 cos_l), in pdf_omega's place on the sample side; "hit_weight" leaves the MIS weight of a
BSDF-sampled hit on a listed sphere at 1; "omc_subtract" forms 1 - cos theta_max by a float32 subtraction."""
import numpy as np

from independent_twin import _EPS1, _Lds, _Pcg, _closest_prims, _cosine_about, _unit, psnr_db  # noqa: F401  (psnr_db: for the tests)
from plastic_ref import PLASTIC, eval_f_pdf, sample_f
from spot_ref import SPOT
from spot_ref import sample as spot_sample

SPHERE = 8
SELF_RIM, SELF_DELTA, SHRINK = 2.0 ** -9, 2.0 ** -18, 0.9999  # 3.25: the margin that keeps the shadow ray off the light's own sphere


def _dot(a, b):
    return (a * b).sum(-1)


def one_minus_cos_max(o, c, r, wrong=None):
    """-> (outside [n], wc [n, 3], dc2, cmax, omc): 3.25's s2 / (1 + cmax)"""
    o, c, r = np.asarray(o, np.float64), np.asarray(c, np.float64), np.asarray(r, np.float64)
    wc = c - o
    dc2 = _dot(wc, wc)
    outside = dc2 > r * r
    with np.errstate(all="ignore"):
        s2 = r * r / dc2
        cmax = np.sqrt(np.maximum(0.0, 1.0 - s2))
        omc = s2 / (1.0 + cmax)
        if wrong == "omc_subtract":
            omc = (np.float32(1.0) - cmax.astype(np.float32)).astype(np.float64)
    return outside, wc, dc2, cmax, omc


def pdf_omega(o, c, r):
    """the hit side: the density over solid angle with which the sphere is sampled from o; 0 where o is not outside"""
    outside, _, _, _, omc = one_minus_cos_max(o, c, r)
    with np.errstate(all="ignore"):
        return np.where(outside, 1.0 / (2.0 * np.pi * omc), 0.0)


def disk(u1, u2):
    """the concentric map of (u1, u2) in [0, 1)^2 onto the unit disk (Shirley and Chiu), as 3.8's cosine sampling has it"""
    ox, oy = 2.0 * np.asarray(u1, np.float64) - 1.0, 2.0 * np.asarray(u2, np.float64) - 1.0
    wide = np.abs(ox) > np.abs(oy)
    with np.errstate(all="ignore"):
        rad = np.where(wide, ox, oy)
        phi = np.where(wide, (np.pi / 4) * (oy / ox), np.pi / 2 - (np.pi / 4) * (ox / oy))
    zero = (ox == 0) & (oy == 0)
    return np.where(zero, 0.0, rad * np.cos(phi)), np.where(zero, 0.0, rad * np.sin(phi))


def frame(n):
    """3.8's tangent frame about the unit vectors n"""
    big_x = np.abs(n[..., 0]) > np.abs(n[..., 1])
    z = np.zeros_like(n[..., 0])
    with np.errstate(all="ignore"):
        a = np.stack([-n[..., 2], z, n[..., 0]], -1) / np.sqrt(n[..., 0] ** 2 + n[..., 2] ** 2)[..., None]
        b = np.stack([z, n[..., 2], -n[..., 1]], -1) / np.sqrt(n[..., 1] ** 2 + n[..., 2] ** 2)[..., None]
    v2 = np.where(big_x[..., None], a, b)
    return v2, np.cross(n, v2)


def sample(po, nf, c, r, u1, u2, nL, wrong=None):
    """-> (ok [n], wi [n, 3], tmax [n], scale [n], pdf [n], cs [n]) of the sphere light's sample at shading points po with normals nf;
    scale = cs (1 / pdf) nL.  The outputs behind ok = 0 are zero."""
    po, nf, c, r = (np.asarray(v, np.float64) for v in (po, nf, c, r))
    outside, wc, dc2, cmax, omc = one_minus_cos_max(po, c, r, wrong)
    with np.errstate(all="ignore"):
        dc = np.sqrt(dc2)
        w = wc / dc[..., None]
        dx, dy = disk(u1, u2)
        s = np.minimum(dx * dx + dy * dy, 1.0)
        ct = 1.0 - s * omc
        tang = np.sqrt(omc * (1.0 + ct))
        v2, v3 = frame(w)
        wi = v2 * (dx * tang)[..., None] + v3 * (dy * tang)[..., None] + w * ct[..., None]
        cs = _dot(wi, nf)
        half = r * np.sqrt(np.maximum(0.0, 1.0 - s * (1.0 + ct) / (1.0 + cmax)))
        t = dc * ct - half
        tmax = (t - np.minimum(SELF_RIM * dc, SELF_DELTA * dc2 / half)) * SHRINK
        pdf = 1.0 / (2.0 * np.pi * omc)
        if wrong == "area":
            nl = ((po + wi * t[..., None]) - c) / r[..., None]
            pdf = (t * t) / (4.0 * np.pi * r * r * -_dot(nl, wi))
        scale = cs / pdf * nL
    ok = outside & (cs > 0)
    z = np.zeros_like(dc2)
    return ok, np.where(ok[..., None], wi, 0.0), np.where(ok, tmax, z), np.where(ok, scale, z), np.where(ok, pdf, z), np.where(ok, cs, z)


def closed_form(kd, L, r, d, cos_c):
    """Lo of a matte point that sees the whole sphere above its horizon: Kd L (r / d)^2 cos theta_c (3.25)"""
    return np.asarray(kd, np.float64) * np.asarray(L, np.float64) * (r / d) ** 2 * cos_c


def render(sd, integrator=0, max_depth=5, spp=(1, 1), seed=0, sampler="stratified", filter_width=None, max_sample_luminance=0.0, sobol_matrices=None,
           wrong=None, samples=None):
    """-> film [h, w, 4] float64 {X, Y, Z, weight} of SceneData `sd` (matte / mirror / plastic under any light but the maps; see the module's text).  `samples`: a list that
    receives one [h, w, 3] array of sanitised radiance per sample (default filter only), for standard errors."""
    sd = sd.normalized()
    sampler = {0: "stratified", 1: "sobol", 2: "sobol_nd", 3: "halton"}.get(sampler, sampler)
    assert integrator in (0, 1, 2) and sampler in ("stratified", "sobol", "sobol_nd", "halton")
    assert tuple(sd.crop) == (0.0, 1.0, 0.0, 1.0) and not sd.envmap.size and not len(sd.textures)
    assert sampler != "sobol_nd" or sobol_matrices is not None
    rx, ry = (float(v) if float(v) != 0.0 else 0.5 for v in (filter_width or (0.5, 0.5)))
    wide = (rx, ry) != (0.5, 0.5)
    pad_x, pad_y = (int(np.ceil(rx - 0.5)), int(np.ceil(ry - 0.5))) if wide else (0, 0)
    mis = integrator == 2
    sph = sd.spheres.astype(np.float64)
    T = sd.idx.shape[0]
    W, H = int(sd.xres), int(sd.yres)
    nx, ny = spp
    n_spp = nx * ny
    K = 1
    while 2 * K <= 16 and 2 * K * 32 <= n_spp:
        K *= 2
    P = sd.P.astype(np.float64)[sd.idx.astype(np.int64)] if T else np.zeros((0, 3, 3))
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    e1, e2 = p1 - p0, p2 - p0
    mats = sd.materials.astype(np.float64)
    assert np.isin(mats[:, 0], (0, 1, PLASTIC)).all()
    mat_of = np.concatenate([sd.mat_id.astype(np.int64), sph[:, 4].astype(np.int64)])
    if len(mat_of) == 0:
        mat_of = np.zeros(1, np.int64)
    tri_area_all = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1) if T else np.zeros(0)
    is_matte, is_plastic = mats[:, 0] == 0, mats[:, 0] == PLASTIC
    # (3.21: a plastic row is (type, Kd, Ks) with alpha beside it; plastic does not emit)
    kcol, le = mats[:, 1:4], np.where(is_plastic[:, None], 0.0, mats[:, 4:7])
    k_spec = np.where(is_plastic[:, None], mats[:, 4:7], 0.0)
    alpha_of = np.where(is_plastic, sd.mat_eta.astype(np.float64) if len(sd.mat_eta) else 1.0, 1.0)
    L = [dict(type=int(row[0]), p=row[1:4], c=row[4:7]) for row in sd.lights.astype(np.float64)]
    assert all(l["type"] in (0, 1, 2, SPOT, SPHERE) for l in L)
    listed = np.zeros(max(len(sph), 1), bool)  # 3.25: the spheres that a sphere light names
    for l in L:
        if l["type"] == SPHERE:  # the row is (8, k, 0, 0, L): the light sits where sphere k does
            k = int(l["p"][0])
            assert not listed[k] and (le[int(sph[k, 4])] == l["c"]).all()
            listed[k] = True
            l.update(p=sph[k, :3], r=sph[k, 3])
    cones = iter(sd.spot_cones.astype(np.float64))  # (3.22: the k-th cone is the k-th spot light's)
    for l in L:
        if l["type"] == SPOT:
            cone = next(cones)
            l.update(axis=cone[0:3], cos_total=cone[3], cos_start=cone[4])
    le_inf = sum((l["c"] for l in L if l["type"] == 2), np.zeros(3))
    has_inf = any(l["type"] == 2 for l in L)
    for t in range(len(P)):
        if (le[mat_of[t]] > 0).any():
            cr = np.cross(e1[t], e2[t])
            L.append(dict(type=3, p=p0[t], p1=p1[t], p2=p2[t], c=le[mat_of[t]], n=cr / np.linalg.norm(cr), area=0.5 * np.linalg.norm(cr)))
    nL = len(L)
    nLf = np.float32(nL)
    ltype = np.array([l["type"] for l in L], np.int64) if nL else np.zeros(0, np.int64)
    lp = np.array([l["p"] for l in L]).reshape(-1, 3)
    lc = np.array([l["c"] for l in L]).reshape(-1, 3)
    lp1 = np.array([l.get("p1", np.zeros(3)) for l in L]).reshape(-1, 3)
    lp2 = np.array([l.get("p2", np.zeros(3)) for l in L]).reshape(-1, 3)
    ln = np.array([l.get("n", np.zeros(3)) for l in L]).reshape(-1, 3)
    larea = np.array([l.get("area", 0.0) for l in L])
    laxis = np.array([l.get("axis", np.zeros(3)) for l in L]).reshape(-1, 3)
    lcos = np.array([[l.get("cos_total", 0.0), l.get("cos_start", 0.0)] for l in L]).reshape(-1, 2)
    lrad = np.array([l.get("r", 1.0) for l in L])
    c2w = sd.cam_to_world.astype(np.float64)
    aspect = W / H
    x0, x1, y0, y1 = (-aspect, aspect, -1.0, 1.0) if aspect >= 1 else (-1.0, 1.0, -1.0 / aspect, 1.0 / aspect)
    th = float(np.float32(np.tan(float(sd.fov) * np.pi / 360.0)))
    ax, bx, ay, by = (x1 - x0) / W * th, x0 * th, -(y1 - y0) / H * th, y1 * th
    py, px = np.mgrid[-pad_y:H + pad_y, -pad_x:W + pad_x]
    px, py = px.ravel(), py.ravel()
    n_px = len(px)
    Wn, Hn = W + 2 * pad_x, H + 2 * pad_y
    film = np.zeros((n_px, 3))
    acc = np.zeros((H, W, 4), np.int64)
    for c in range(K):
        s_lo, s_hi = (c * n_spp) // K, ((c + 1) * n_spp) // K
        with np.errstate(over="ignore"):
            qpix = np.uint64(seed) * np.uint64(Wn) * np.uint64(Hn) + (py + pad_y).astype(np.uint64) * np.uint64(Wn) + (px + pad_x).astype(np.uint64)
            rng = _Pcg(qpix * np.uint64(K) + np.uint64(c)) if sampler == "stratified" else _Lds(sampler, qpix, n_spp, sobol_matrices)
        part = np.zeros((n_px, 3))
        everyone = np.ones(n_px, bool)
        for s in range(s_lo, s_hi):
            sx, sy = s % nx, s // nx
            rng.start_sample(s)
            u1, u2 = rng.get2(everyone)
            if sampler == "stratified":
                jx = np.minimum((np.float32(sx) + u1) * (np.float32(1) / np.float32(nx)), _EPS1)
                jy = np.minimum((np.float32(sy) + u2) * (np.float32(1) / np.float32(ny)), _EPS1)
            else:
                jx, jy = u1, u2
            fx = (px.astype(np.float32) + jx).astype(np.float64)
            fy = (py.astype(np.float32) + jy).astype(np.float64)
            dc = _unit(np.stack([fx * ax + bx, fy * ay + by, np.ones(n_px)], 1))
            d = dc @ c2w[:3, :3].T
            o = np.tile(c2w[:3, 3], (n_px, 1))
            Lsum, beta = np.zeros((n_px, 3)), np.ones((n_px, 3))
            alive = np.ones(n_px, bool)
            specular = np.zeros(n_px, bool)
            pb_prev = np.zeros(n_px)  # MIS: the density the ray in flight was drawn with
            bounces = 0
            while alive.any():
                a = np.flatnonzero(alive)
                t, tri, ub, vb = _closest_prims(o[a], d[a], np.full(len(a), np.inf), p0, e1, e2, sph)
                hit = tri >= 0
                on_tri = hit & (tri < T)
                wo = -d[a]
                m = mat_of[np.maximum(tri, 0)]
                ti = np.where(on_tri, tri, 0)
                ng = _unit(np.cross(e1[ti], e2[ti])) if T else np.zeros((len(a), 3))
                if len(sph):
                    si = np.clip(tri - T, 0, len(sph) - 1)
                    ph = (o[a] - sph[si, :3]) + d[a] * np.where(hit, t, 0.0)[:, None]
                    ng = np.where(on_tri[:, None], ng, ph / sph[si, 3:4])
                collect = (bounces == 0) | specular[a]
                front = _dot(ng, wo) > 0
                emits = hit & front & (le[m] > 0).any(1)
                Lsum[a] += np.where((emits & collect)[:, None], beta[a] * le[m], 0.0)
                if has_inf:
                    Lsum[a] += np.where((~hit & collect)[:, None], beta[a] * le_inf, 0.0)
                if mis:  # 3.14: the BSDF-sampled half of the previous vertex's estimate, weighted with the density that vertex kept
                    with np.errstate(all="ignore"):
                        cl = _dot(ng, wo)
                        pl = ((t * t) / (cl * tri_area_all[ti])) / nL if T else np.zeros(len(a))
                        wb = pb_prev[a] ** 2 / (pb_prev[a] ** 2 + pl ** 2)
                    Lsum[a] += np.where((emits & on_tri & ~collect)[:, None], beta[a] * le[m] * wb[:, None], 0.0)
                    if len(sph):  # 3.25: a listed sphere met from outside by a BSDF-sampled ray: pl = pdf_omega(origin) / nL
                        with np.errstate(all="ignore"):
                            pl_s = pdf_omega(o[a], sph[si, :3], sph[si, 3]) / nL
                            wb_s = pb_prev[a] ** 2 / (pb_prev[a] ** 2 + pl_s ** 2)
                        if wrong == "hit_weight":
                            wb_s = np.ones(len(a))
                        Lsum[a] += np.where((emits & ~on_tri & listed[si] & ~collect)[:, None], beta[a] * le[m] * wb_s[:, None], 0.0)
                    if has_inf:  # (the constant pair of weights, whatever the BSDF of the vertex the ray left: 3.14, 3.21)
                        Lsum[a] += np.where((~hit & ~collect)[:, None], beta[a] * le_inf * (nL * nL / (nL * nL + 1.0)), 0.0)
                alive[a[~hit]] = False
                if bounces >= max_depth:
                    alive[a] = False
                    break
                a, tri, ub, vb, m, ng, wo, on_tri, t = a[hit], tri[hit], ub[hit], vb[hit], m[hit], ng[hit], wo[hit], on_tri[hit], t[hit]
                if len(a) == 0:
                    break
                w = (1.0 - ub) - vb
                ti = np.where(on_tri, tri, 0)
                p = p0[ti] * w[:, None] + p1[ti] * ub[:, None] + p2[ti] * vb[:, None] if T else np.zeros((len(a), 3))
                if len(sph):
                    si = np.clip(tri - T, 0, len(sph) - 1)
                    p = np.where(on_tri[:, None], p, sph[si, :3] + ((o[a] - sph[si, :3]) + d[a] * t[:, None]))
                nf = np.where((_dot(ng, wo) < 0)[:, None], -ng, ng)
                po = p + nf * 1e-4
                matte, plastic = is_matte[m], is_plastic[m]
                scat = matte | plastic  # the vertices that draw a light sample and a bounce pair (3.21: plastic draws what matte draws)
                k, ks, al = kcol[m], k_spec[m], alpha_of[m]
                full = np.zeros(n_px, bool)
                lpend = np.zeros((len(a), 3))
                need_shadow = np.zeros(len(a), bool)
                sh_d, sh_t = np.zeros((len(a), 3)), np.full(len(a), np.inf)
                if nL > 0:
                    full[a[scat]] = True
                    xi = rng.get1(full)[a]
                    l1, l2 = (v[a] for v in rng.get2(full))
                    li = np.minimum((xi * nLf).astype(np.int64), nL - 1)
                    ty = ltype[li]
                    # every light as (wi, Lg = Li cos_i nL / pdf_l, pl = the density MIS compares; 0 for the delta lights)
                    dv = lp[li] - po
                    d2 = _dot(dv, dv)
                    with np.errstate(all="ignore"):
                        dist = np.sqrt(d2)
                        wi_p = dv / dist[:, None]
                        cs_p = _dot(wi_p, nf)
                        lg_p = lc[li] * ((cs_p / d2) * nL)[:, None]
                    ok_p = (ty == 0) & (d2 > 0) & (cs_p > 0)
                    # a spot light: the point light's sample times the cone's falloff (3.22); a delta light like it
                    ok_s, wi_sp, tmax_s, _, scale_s = spot_sample(po, nf, lp[li], laxis[li], lcos[li, 0], lcos[li, 1], float(nL))
                    ok_s &= ty == SPOT
                    lg_s = lc[li] * scale_s[:, None]
                    # a sphere light: uniform in the solid angle the sphere subtends, from the light's pair (3.25); an area light
                    ok_a, wi_a, tmax_a, scale_a, pdf_a, _ = sample(po, nf, lp[li], lrad[li], l1.astype(np.float64), l2.astype(np.float64), float(nL), wrong)
                    ok_a &= ty == SPHERE
                    lg_a = lc[li] * scale_a[:, None]
                    with np.errstate(all="ignore"):
                        pl_a = pdf_a / nL
                    cs_d = _dot(lp[li], nf)
                    ok_d = (ty == 1) & (cs_d > 0)
                    lg_d = lc[li] * (cs_d * nL)[:, None]
                    wi_i, z_i = _cosine_about(nf, l1.astype(np.float64), l2.astype(np.float64))
                    ok_i = (ty == 2) & (z_i != 0)
                    lg_i = lc[li] * np.pi * nL
                    su0 = np.sqrt(l1.astype(np.float64))
                    b0 = 1.0 - su0
                    b1 = l2.astype(np.float64) * su0
                    b2 = (1.0 - b0) - b1
                    pt = lp[li] * b0[:, None] + lp1[li] * b1[:, None] + lp2[li] * b2[:, None]
                    dv = pt - po
                    d2t = _dot(dv, dv)
                    with np.errstate(all="ignore"):
                        dist_t = np.sqrt(d2t)
                        wi_t = dv / dist_t[:, None]
                        cs_t = _dot(wi_t, nf)
                        cl_t = -_dot(wi_t, ln[li])
                        lg_t = lc[li] * ((((cs_t * cl_t) * larea[li]) / d2t) * nL)[:, None]
                        pl_t = (d2t / (cl_t * larea[li])) / nL
                    ok_t = (ty == 3) & (d2t > 0) & (cs_t > 0) & (cl_t > 0)
                    need_shadow = scat & (ok_p | ok_d | ok_i | ok_t | ok_s | ok_a)
                    with np.errstate(all="ignore"):
                        lg = np.where(ok_a[:, None], lg_a, np.where(ok_s[:, None], lg_s, np.where(ok_p[:, None], lg_p, np.where(ok_d[:, None], lg_d, np.where(ok_i[:, None], lg_i, lg_t)))))
                        sh_d = np.where(ok_a[:, None], wi_a, np.where(ok_s[:, None], wi_sp, np.where(ok_p[:, None], wi_p, np.where(ok_d[:, None], lp[li], np.where(ok_i[:, None], wi_i, wi_t)))))
                        sh_t = np.where(ok_a, tmax_a, np.where(ok_s, tmax_s, np.where(ok_p, dist * 0.9999, np.where(ok_t, dist_t * 0.9999, np.inf))))
                        cs = _dot(sh_d, nf)
                        # the BSDF for the light's direction and its density there: Kd / pi and cos / pi at a matte vertex
                        f_pl, pb_pl = eval_f_pdf(nf, wo, np.where(need_shadow[:, None], sh_d, nf), k, ks, al)
                        f_l = np.where(plastic[:, None], f_pl, k / np.pi)
                        pb_l = np.where(plastic, pb_pl, cs / np.pi)
                        ld = f_l * lg
                        if mis:  # the power heuristic for the area light; the constant pair for the constant infinite light
                            ld = np.where(ok_t[:, None], ld * (pl_t ** 2 / (pl_t ** 2 + pb_l ** 2))[:, None], ld)
                            ld = np.where(ok_a[:, None], ld * (pl_a ** 2 / (pl_a ** 2 + pb_l ** 2))[:, None], ld)
                            ld = np.where(ok_i[:, None], ld * (1.0 / (1.0 + nL * nL)), ld)
                    lpend = np.where(need_shadow[:, None], beta[a] * ld, 0.0)
                # --- the BSDF sample ---
                go = np.ones(len(a), bool)
                wi_next = -wo + nf * (2.0 * _dot(wo, nf))[:, None]
                new_beta = beta[a] * k  # (matte and mirror)
                if integrator == 1:
                    go &= ~scat  # direct lighting ends at the first vertex that is not specular
                else:
                    full[:] = False
                    full[a[scat]] = True
                    c1, c2 = (v[a] for v in rng.get2(full))
                    wi_c, z_c = _cosine_about(nf, c1.astype(np.float64), c2.astype(np.float64))
                    wi_next = np.where(matte[:, None], wi_c, wi_next)
                    go &= ~(matte & (z_c == 0))
                    pb_new = z_c / np.pi
                    if plastic.any():
                        wi_s, w_s, pdf_s, alive_s = sample_f(nf, wo, c1, c2, k, ks, al)
                        wi_next = np.where(plastic[:, None], wi_s, wi_next)
                        new_beta = np.where(plastic[:, None], beta[a] * w_s, new_beta)
                        go &= ~(plastic & ~alive_s)
                        pb_new = np.where(plastic, pdf_s, pb_new)
                    pb_prev[a] = pb_new
                new_beta = np.where(go[:, None], new_beta, beta[a])
                spec_next = ~scat
                go &= ~(new_beta == 0).all(1)
                if bounces > 3:  # Russian roulette (3.9)
                    full[:] = False
                    full[a[go]] = True
                    xr = rng.get1(full)[a]
                    q = np.maximum(0.05, 1.0 - new_beta.max(1))
                    die = go & (xr < q)
                    with np.errstate(all="ignore"):
                        new_beta = np.where((go & ~die)[:, None], new_beta / (1.0 - q)[:, None], new_beta)
                    go &= ~die
                if need_shadow.any():
                    sidx = np.flatnonzero(need_shadow)
                    _, blocker, _, _ = _closest_prims(po[sidx], sh_d[sidx], sh_t[sidx], p0, e1, e2, sph)
                    lit = np.zeros(len(a), bool)
                    lit[sidx] = blocker < 0
                    Lsum[a] += np.where(lit[:, None], lpend, 0.0)
                beta[a] = new_beta
                specular[a] = spec_next
                if not mis:
                    go &= ~((bounces + 1 >= max_depth) & ~spec_next)
                alive[a] = go
                o[a], d[a] = po, wi_next
                bounces += 1
            y = 0.212671 * Lsum[:, 0] + 0.715160 * Lsum[:, 1] + 0.072169 * Lsum[:, 2]
            bad = np.isnan(Lsum).any(1) | (y < -1e-5) | np.isinf(y)
            Ls = np.where(bad[:, None], 0.0, Lsum)
            if max_sample_luminance > 0:
                with np.errstate(all="ignore"):
                    Ls = np.where((y > max_sample_luminance)[:, None] & ~bad[:, None], Ls * (max_sample_luminance / y)[:, None], Ls)
            if samples is not None:
                assert not wide
                samples.append(Ls.reshape(H, W, 3).copy())
            if not wide:
                part += Ls
            else:  # 3.11: the fixed-point film of a box filter wider than 0.5
                q = (np.minimum(np.maximum(Ls, 0.0), 32768.0).astype(np.float32).astype(np.float64) * 16777216.0).astype(np.int64)
                f32 = np.float32
                dx, dy = fx.astype(f32) - f32(0.5), fy.astype(f32) - f32(0.5)
                bx0, bx1 = np.maximum(np.ceil(dx - f32(rx)).astype(np.int64), 0), np.minimum(np.floor(dx + f32(rx)).astype(np.int64), W - 1)
                by0, by1 = np.maximum(np.ceil(dy - f32(ry)).astype(np.int64), 0), np.minimum(np.floor(dy + f32(ry)).astype(np.int64), H - 1)
                for oy in range(2 * pad_y + 2):
                    for ox in range(2 * pad_x + 2):
                        xx, yy = bx0 + ox, by0 + oy
                        ok = (xx <= bx1) & (yy <= by1)
                        np.add.at(acc, (yy[ok], xx[ok]), np.concatenate([q[ok], np.ones((int(ok.sum()), 1), np.int64)], 1))
        film += part
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    if wide:
        return np.concatenate([(acc[..., :3].astype(np.float64) / 16777216.0) @ M.T, acc[..., 3:4].astype(np.float64)], -1)
    out = np.concatenate([film @ M.T, np.full((n_px, 1), float(n_spp))], 1)
    return out.reshape(H, W, 4)
