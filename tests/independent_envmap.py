"""An independent float64 reference for scenes under an environment map: numpy only, nothing shared with the library
or the oracle.  Analytic intersections of a ground rectangle and spheres, a path tracer with COSINE SAMPLING ONLY -- it has NO light
sampling: a path collects the sky solely by escaping into it --, a nearest-texel lookup of the latitude-longitude map by numpy's own
arctan2 / arccos, its own random numbers (numpy's PCG64), and per-block means with their standard errors.

Because every contribution comes from an escaping ray, its noise grows with the map's dynamic range: it serves smooth skies (max / mean
<= 4).  The high-dynamic-range case belongs to the closed-form sun test of tests/test_envmap_gpu.py.

Depth convention (include/pbrt_hip.h max_depth, restated from the documentation, not from code): a path has at most `depth` surface
vertices that scatter; the ray leaving the last of them may still find the sky, and a surface it finds instead contributes nothing."""
import numpy as np

MATTE, MIRROR = 0, 1
GROUND_HALF = 50.0
GROUND_KD = np.array([0.5, 0.45, 0.4])
SPHERES = [  # centre, radius, kind, colour
    (np.array([-1.15, 0.0, 1.0]), 1.0, MATTE, np.array([0.7, 0.6, 0.3])),
    (np.array([1.15, 0.0, 1.0]), 1.0, MIRROR, np.array([0.9, 0.9, 0.9])),
]
EYE, LOOK, UP, FOV = np.array([0.0, -7.0, 2.6]), np.array([0.0, 0.0, 0.9]), np.array([0.0, 0.0, 1.0]), 40.0
DEPTH = 5
PATHS_PER_PIXEL = 1024


def smooth_sky(h=16, w=32):
    """a low-dynamic-range sky: a vertical gradient with a gentle variation in azimuth, every texel in [0.3, 1.6] (max / mean < 2)"""
    theta = (np.arange(h)[:, None] + 0.5) * np.pi / h
    phi = (np.arange(w)[None, :] + 0.5) * 2 * np.pi / w
    up = 0.5 + 0.5 * np.cos(theta)
    r = 0.45 + 0.55 * up + 0.25 * np.sin(phi) * np.sin(theta)
    g = 0.55 + 0.45 * up + 0.20 * np.cos(2 * phi) * np.sin(theta)
    b = 0.60 + 0.90 * up + 0.10 * np.cos(phi + 1.0) * np.sin(theta)
    sky = np.stack([r + 0 * phi, g + 0 * phi, b + 0 * phi], axis=-1)
    assert sky.min() > 0.25 and sky.max() / sky.mean() <= 4.0
    return sky


def lookup(sky, m, d):
    """nearest texel of direction d (n, 3) under world_to_light m: pbrt-v3 InfiniteAreaLight::Le's (u, v), point-sampled"""
    h, w = sky.shape[:2]
    wv = d @ np.asarray(m, np.float64).T
    phi = np.mod(np.arctan2(wv[:, 1], wv[:, 0]), 2 * np.pi)
    theta = np.arccos(np.clip(wv[:, 2], -1.0, 1.0))
    col = np.minimum((phi / (2 * np.pi) * w).astype(np.int64), w - 1)
    row = np.minimum((theta / np.pi * h).astype(np.int64), h - 1)
    return sky[row, col]


def camera_rays(res, px, py, jx, jy):
    fwd = (LOOK - EYE) / np.linalg.norm(LOOK - EYE)
    right = np.cross(UP / np.linalg.norm(UP), fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    t = np.tan(np.radians(FOV) / 2)
    x, y = px + jx, py + jy
    d = ((2 * x / res - 1) * t)[:, None] * right + ((1 - 2 * y / res) * t)[:, None] * up + fwd
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def intersect(o, d):
    """-> (t, normal, kind, colour) of the nearest hit; t = inf on a miss"""
    n = o.shape[0]
    t = np.full(n, np.inf)
    nrm = np.zeros((n, 3))
    kind = np.zeros(n, np.int64)
    col = np.zeros((n, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = -o[:, 2] / d[:, 2]
    p = o + tp[:, None] * d
    ok = (tp > 1e-6) & (np.abs(p[:, 0]) <= GROUND_HALF) & (np.abs(p[:, 1]) <= GROUND_HALF)
    t = np.where(ok, tp, t)
    nrm[ok] = (0.0, 0.0, 1.0)
    col[ok] = GROUND_KD
    for c, r, k, colour in SPHERES:
        oc = o - c
        b = (oc * d).sum(1)
        disc = b * b - ((oc * oc).sum(1) - r * r)
        sq = np.sqrt(np.maximum(disc, 0.0))
        t0, t1 = -b - sq, -b + sq
        ts = np.where(t0 > 1e-6, t0, t1)
        ok = (disc >= 0) & (ts > 1e-6) & (ts < t)
        t = np.where(ok, ts, t)
        nrm[ok] = ((o + ts[:, None] * d - c) / r)[ok]
        kind[ok] = k
        col[ok] = colour
    return t, nrm, kind, col


def cosine_direction(rng, nrm):
    n = nrm.shape[0]
    u1, u2 = rng.random(n), rng.random(n)
    r, a = np.sqrt(u1), 2 * np.pi * u2
    helper = np.where((np.abs(nrm[:, 0]) > 0.9)[:, None], np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]))
    t1 = np.cross(helper, nrm)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    return (r * np.cos(a))[:, None] * t1 + (r * np.sin(a))[:, None] * t2 + np.sqrt(np.maximum(0.0, 1 - u1))[:, None] * nrm


def radiance(rng, sky, m, o, d, depth=DEPTH, factor=(1.0, 1.0, 1.0)):
    n = o.shape[0]
    L = np.zeros((n, 3))
    beta = np.ones((n, 3))
    alive = np.ones(n, bool)
    for segment in range(depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, nrm, kind, col = intersect(o[idx], d[idx])
        miss = ~np.isfinite(t)
        L[idx[miss]] += beta[idx[miss]] * lookup(sky, m, d[idx[miss]]) * np.asarray(factor)
        alive[idx[miss]] = False
        hit = idx[~miss]
        if segment == depth:  # the last vertex does not scatter
            alive[hit] = False
            break
        th, nh, kh, ch = t[~miss], nrm[~miss], kind[~miss], col[~miss]
        p = o[hit] + th[:, None] * d[hit]
        nf = np.where(((nh * d[hit]).sum(1) > 0)[:, None], -nh, nh)
        mirror = kh == MIRROR
        refl = d[hit] - 2 * (d[hit] * nf).sum(1)[:, None] * nf
        diff = cosine_direction(rng, nf)
        nd = np.where(mirror[:, None], refl, diff)
        beta[hit] *= ch  # cosine sampling of a Lambertian: f cos / pdf = Kd; a mirror: Kr
        o[hit] = p + 1e-6 * nf
        d[hit] = nd / np.linalg.norm(nd, axis=1, keepdims=True)
    return L


def block_means(res, sky, m, block=8, paths=PATHS_PER_PIXEL, depth=DEPTH, seed=2024, factor=(1.0, 1.0, 1.0)):
    """-> (mean[res / block, res / block, 3], standard error of that mean) of the pixel radiance over blocks of block x block pixels"""
    rng = np.random.default_rng(seed)
    nb = res // block
    s1 = np.zeros((nb, nb, 3))
    s2 = np.zeros((nb, nb, 3))
    cnt = np.zeros((nb, nb))
    py, px = np.mgrid[0:res, 0:res]
    px, py = px.reshape(-1).astype(np.float64), py.reshape(-1).astype(np.float64)
    bi = (py.astype(np.int64) // block) * nb + px.astype(np.int64) // block
    for _ in range(paths // 16):
        pxx, pyy, bb = np.tile(px, 16), np.tile(py, 16), np.tile(bi, 16)
        d = camera_rays(res, pxx, pyy, rng.random(pxx.size), rng.random(pxx.size))
        o = np.broadcast_to(EYE, d.shape).copy()
        L = radiance(rng, sky, m, o, d, depth, factor)
        for c in range(3):
            s1[..., c] += np.bincount(bb, L[:, c], nb * nb).reshape(nb, nb)
            s2[..., c] += np.bincount(bb, L[:, c] ** 2, nb * nb).reshape(nb, nb)
        cnt += np.bincount(bb, minlength=nb * nb).reshape(nb, nb)
    mean = s1 / cnt[..., None]
    var = np.maximum(s2 / cnt[..., None] - mean ** 2, 0.0)
    return mean, np.sqrt(var / cnt[..., None])


def scene_data(res, sky, m, factor=(1.0, 1.0, 1.0)):
    """the same scene as arrays for the library (the only import of the package here: the container)"""
    from pbrt_amd import LIGHT_ENVMAP, SceneData, look_at
    g = GROUND_HALF
    P = np.array([(-g, -g, 0), (g, -g, 0), (g, g, 0), (-g, g, 0)], np.float32)
    mats = [[MATTE, *GROUND_KD, 0, 0, 0]] + [[k, *col, 0, 0, 0] for _, _, k, col in SPHERES]
    return SceneData(P=P, idx=np.array([(0, 1, 2), (0, 2, 3)], np.uint32), mat_id=np.zeros(2, np.uint16), materials=np.array(mats, np.float32),
                     spheres=np.array([[*c, r, i + 1] for i, (c, r, _, _) in enumerate(SPHERES)], np.float32),
                     lights=np.array([[LIGHT_ENVMAP, 0, 0, 0, *factor]], np.float32), envmap=sky.astype(np.float32), envmap_world_to_light=m,
                     cam_to_world=look_at(EYE, LOOK, UP)[1], fov=FOV, xres=res, yres=res).normalized()
