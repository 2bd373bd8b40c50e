"""The mapped lights of DESIGN.md 3.23 -- LightSource "projection" and "goniometric" -- in float64 numpy, written from the section's text
and sharing nothing with pbrt_amd/csrc/light_map.hpp: the direction's (s, t) of either kind, the light sample, and the path loop of
tests/spot_ref.py restated with MAPPED lights beside its point, distant, constant-infinite, area and spot lights (the image lookup is
tests/image_ref.py's, the spot light tests/spot_ref.py's, the plastic BSDF tests/plastic_ref.py's).  The loop draws the SAME RANDOM NUMBERS
as the library, so sample s of pixel (x, y) is the same path up to rounding and films compare directly.

`wrong` exists for negative controls: a reference with t flipped ("flip_t"), with the goniometric swap of y and z dropped ("no_swap"), with
inv_tan dropped ("no_inv_tan"), or with the image multiplied into a light other than the one that names it ("other_light": the light
AFTER it in the table, cyclically) must FAIL the bars the right one meets."""
import numpy as np

import image_ref
import spot_ref
from independent_twin import _EPS1, _Lds, _Pcg, _closest_prims, _cosine_about, _unit, psnr_db  # noqa: F401  (psnr_db: for the tests)
from plastic_ref import PLASTIC, eval_f_pdf, sample_f

SPOT, MAPPED = 5, 6
PROJECTION, GONIOMETRIC = 0, 1
MIN_Z = float(np.float32(1e-3))  # (the header's constant is the float32 nearest to 1e-3)


def _dot(a, b):
    return (a * b).sum(-1)


def direction_st(w, kind, inv_tan, sx, sy, wrong=None):
    """3.23: light-space directions w [n, 3] -> (inside [n], s [n], t [n], px [n], py [n]); px, py are the projection's screen coordinates
    (NaN for a goniometric map)"""
    w = np.asarray(w, np.float64)
    n = len(w)
    if kind == PROJECTION:
        it = 1.0 if wrong == "no_inv_tan" else float(inv_tan)
        with np.errstate(all="ignore"):
            px, py = (w[:, 0] / w[:, 2]) * it, (w[:, 1] / w[:, 2]) * it
            inside = (w[:, 2] > MIN_Z) & (px >= -sx) & (px <= sx) & (py >= -sy) & (py <= sy)
            s, t = (px + sx) / (2.0 * sx), (py + sy) / (2.0 * sy)
    else:
        pole, other = (w[:, 2], w[:, 1]) if wrong == "no_swap" else (w[:, 1], w[:, 2])
        theta = np.arccos(np.clip(pole, -1.0, 1.0))
        phi = np.arctan2(other, w[:, 0])
        phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
        inside = np.ones(n, bool)
        s, t = phi / (2.0 * np.pi), 1.0 - theta / np.pi
        px = py = np.full(n, np.nan)
    if wrong == "flip_t":
        t = 1.0 - t
    return inside, s, t, px, py


def lookup(image, wrap, filt, s, t):
    """the image (H, W, 3; row 0 = its top) at (s, t): tests/image_ref.py's float64 lookup"""
    return (image_ref.bilinear if filt == image_ref.BILINEAR else image_ref.point)(image, wrap, s, t)


def sample(po, nf, p, kind, M, inv_tan, sx, sy, image, wrap, filt, nL, wrong=None):
    """-> dict(ok, wi, tmax, scale, s, t, rgb, px, py, wz) of the mapped light's sample at shading points po [n, 3] with normals nf; M =
    world_to_light (3, 3); the outputs are zero behind ok = False but px, py, wz, which say how near an edge the input lies"""
    po, nf, p = (np.asarray(v, np.float64) for v in (po, nf, p))
    p = np.broadcast_to(p, po.shape)
    M = np.asarray(M, np.float64).reshape(3, 3)
    dv = p - po
    d2 = _dot(dv, dv)
    with np.errstate(all="ignore"):
        dist = np.sqrt(d2)
        wi = dv / dist[..., None]
        cs = _dot(wi, nf)
        w = (-wi) @ M.T
        inside, s, t, px, py = direction_st(w, kind, inv_tan, sx, sy, wrong)
        st_ok = np.isfinite(s) & np.isfinite(t)
        rgb = lookup(image, wrap, filt, np.where(st_ok, s, 0.0), np.where(st_ok, t, 0.0))
        scale = cs / d2 * nL
    ok = (d2 > 0) & (cs > 0) & inside & st_ok & (rgb != 0).any(-1)
    z = np.zeros_like(d2)
    o3 = ok[..., None]
    return dict(ok=ok, wi=np.where(o3, wi, 0.0), tmax=np.where(ok, dist * 0.9999, z), scale=np.where(ok, scale, z), s=np.where(ok, s, z), t=np.where(ok, t, z),
                rgb=np.where(o3, rgb, 0.0), px=px, py=py, wz=w[..., 2], geometric=(d2 > 0) & (cs > 0))


def render(sd, integrator=0, max_depth=5, spp=(1, 1), seed=0, sampler="stratified", filter_width=None, max_sample_luminance=0.0, sobol_matrices=None,
           wrong=None, samples=None):
    """-> film [h, w, 4] float64 {X, Y, Z, weight} of SceneData `sd` (matte / mirror / plastic under any light but the environment map; see the module's text).  `samples`: a list that
    receives one [h, w, 3] array of sanitised radiance per sample (default filter only), for standard errors."""
    sd = sd.normalized()
    sampler = {0: "stratified", 1: "sobol", 2: "sobol_nd", 3: "halton"}.get(sampler, sampler)
    assert integrator in (0, 1, 2) and sampler in ("stratified", "sobol", "sobol_nd", "halton")
    assert tuple(sd.crop) == (0.0, 1.0, 0.0, 1.0) and not sd.envmap.size and not sd.mat_tex.any()  # (the images serve the lights alone)
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
    assert all(l["type"] in (0, 1, 2, SPOT, MAPPED) for l in L)
    maps = iter(sd.light_maps.astype(np.float64))  # (3.23: the k-th record is the k-th mapped light's)
    mapped = []  # (the light's index, its record's dict)
    for i, l in enumerate(L):
        if l["type"] == MAPPED:
            m = next(maps)
            row = sd.textures[int(m[1]) - 1]
            assert int(row[0]) == 4
            mapped.append((i, dict(kind=int(m[0]), M=m[2:11].reshape(3, 3), inv_tan=m[11], sx=m[12], sy=m[13], image=sd.images[int(row[1])].astype(np.float64),
                                   wrap=int(row[2]), filt=int(row[3]))))
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
                    ok_s, wi_sp, tmax_s, _, scale_s = spot_ref.sample(po, nf, lp[li], laxis[li], lcos[li, 0], lcos[li, 1], float(nL))
                    ok_s &= ty == SPOT
                    lg_s = lc[li] * scale_s[:, None]
                    # a mapped light (3.23): the point light's sample times its image in the direction from the light; a delta light like it.
                    # (the control "other_light": image i, looked up from light i's position, multiplies the light BEHIND i in the table, and
                    # light i itself is the plain point light)
                    img = np.ones((len(a), 3))
                    ok_m = np.zeros(len(a), bool)
                    for i_l, m in mapped:
                        sel = li == ((i_l + 1) % nL if wrong == "other_light" else i_l)
                        if not sel.any():
                            continue
                        r = sample(po[sel], nf[sel], lp[i_l], m["kind"], m["M"], m["inv_tan"], m["sx"], m["sy"], m["image"], m["wrap"], m["filt"], float(nL), wrong)
                        ok_m[sel], img[sel] = r["ok"], r["rgb"]
                    if wrong == "other_light":
                        ok_m = (d2 > 0) & (cs_p > 0)
                    ok_p = ok_p | (ok_m & (ty == MAPPED))
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
                    need_shadow = scat & (ok_p | ok_d | ok_i | ok_t | ok_s)
                    with np.errstate(all="ignore"):
                        lg = np.where(ok_s[:, None], lg_s, np.where(ok_p[:, None], lg_p, np.where(ok_d[:, None], lg_d, np.where(ok_i[:, None], lg_i, lg_t))))
                        sh_d = np.where(ok_s[:, None], wi_sp, np.where(ok_p[:, None], wi_p, np.where(ok_d[:, None], lp[li], np.where(ok_i[:, None], wi_i, wi_t))))
                        sh_t = np.where(ok_s, tmax_s, np.where(ok_p, dist * 0.9999, np.where(ok_t, dist_t * 0.9999, np.inf)))
                        cs = _dot(sh_d, nf)
                        # the BSDF for the light's direction and its density there: Kd / pi and cos / pi at a matte vertex
                        f_pl, pb_pl = eval_f_pdf(nf, wo, np.where(need_shadow[:, None], sh_d, nf), k, ks, al)
                        f_l = np.where(plastic[:, None], f_pl, k / np.pi)
                        pb_l = np.where(plastic, pb_pl, cs / np.pi)
                        ld = (f_l * lg) * img
                        if mis:  # the power heuristic for the area light; the constant pair for the constant infinite light
                            ld = np.where(ok_t[:, None], ld * (pl_t ** 2 / (pl_t ** 2 + pb_l ** 2))[:, None], ld)
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
