"""An independent Monte Carlo reference for the glass material, in float64 numpy: test infrastructure modelled on
tests/independent_mc.py -- analytic intersections (box planes, one sphere or one axis-aligned cube), its own random numbers, no light
sampling, nothing shared with the library or the oracle.

It does NOT use the library's strategy at a glass surface.  The library draws reflection with probability F (the Fresnel reflectance) and
weights by Kr, refraction with 1 - F and weights by Kt eta_i^2 / eta_t^2.  Here reflection and refraction are drawn with probability 1/2 each
and weighted by 2 F Kr and 2 (1 - F) Kt eta_i^2 / eta_t^2: an error in "divide by the probability" cannot cancel on both sides, and the
samples spread at least as widely as the library's (whose weight at Kr = Kt = 1 is exactly 1 or eta_i^2 / eta_t^2).

Two scenes:
  glass_box_scene   independent_mc's closed box (matte walls, the mirror wall) with the WHOLE ceiling emitting and a glass sphere (eta 1.5,
                    Kr = Kt = 1) in its middle: block_means / compare_with_blocks with the signature and meaning they have there.  (The
                    sphere, radius 0.45, sits 0.2 towards the camera and 0.2 down from the centre, so that it fills a third of the frame:
                    with radius 0.4 at the very centre the reference told eta 1.3 from 1.5 by 6 of its standard errors in one block only;
                    here it does by 8 to 12 in five -- measured between two reference runs, no product involved.)
  furnace_scene     a glass sphere or a glass triangle-mesh cube alone under a constant environment: whatever the path does, every sample's
                    expectation is the environment's radiance (energy conservation: F + (1 - F) = 1, and the eta^2 factors of the way in and
                    the way out cancel).  furnace_block_means gives the reference's own mean and standard error per block.
Russian roulette and the depth rule are the library's: a vertex reached after more than 3 scatterings survives with
probability 1 - max(0.05, 1 - max(beta)); a path has at most max_depth + 1 segments.

The path counts, fixed by tests/test_glass_host.py::test_reference_checks_itself (the reference against itself: no product involved):
  BOX_PATHS = 4 000 000 at 64 x 64, max_depth 8 (62 500 paths per 8 x 8 block; the library renders 64 x 64 samples per pixel, 262 144 per
  block, 4.2 times as many, so the reference's error dominates the comparison): 17 s on one core of the machine this was written on;
  FURNACE_PATHS = 2 000 000 at 32 x 32, max_depth 200: 2.5 s per object and index.
The whole self-check (three box runs, four furnaces) takes about 60 s there."""
import numpy as np

import independent_mc as im

LE_CEILING = np.array([2.0, 1.8, 1.5])
SPHERE_C, SPHERE_R = np.array([0.0, -0.2, -0.2]), 0.45
ETA = 1.5
BOX_PATHS, BOX_DEPTH = 4_000_000, 8
FURNACE_PATHS, FURNACE_DEPTH, FURNACE_RES = 2_000_000, 200, 32
ENV = np.array([1.0, 2.0, 3.0])
FURNACE_EYE, FURNACE_LOOK, FURNACE_UP, FURNACE_FOV = (0.9, -3.0, 0.7), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 26.0
FURNACE_SPHERE_R, FURNACE_CUBE_H = 0.5, 0.4


def fr_dielectric(cos_i, eta_i, eta_t):
    """Fresnel reflectance of a smooth dielectric for unpolarised light; cos_i >= 0 on the eta_i side.  Snell: sin_t = eta_i / eta_t sin_i;
    sin_t >= 1 is total internal reflection."""
    cos_i = np.clip(np.asarray(cos_i, np.float64), 0.0, 1.0)
    eta_i, eta_t = np.broadcast_to(np.asarray(eta_i, np.float64), cos_i.shape), np.broadcast_to(np.asarray(eta_t, np.float64), cos_i.shape)
    sin_t = eta_i / eta_t * np.sqrt(np.maximum(0.0, 1.0 - cos_i * cos_i))
    tir = sin_t >= 1.0
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    with np.errstate(divide="ignore", invalid="ignore"):
        r_par = (eta_t * cos_i - eta_i * cos_t) / (eta_t * cos_i + eta_i * cos_t)
        r_per = (eta_i * cos_i - eta_t * cos_t) / (eta_i * cos_i + eta_t * cos_t)
        f = 0.5 * (r_par * r_par + r_per * r_per)
    return np.where(tir, 1.0, f)


# ---- the scenes as arrays for the library ----

def _cube_mesh(h):
    """12 triangles of the cube [-h, h]^3, wound so that every normal points outwards"""
    c = [(-h, -h, -h), (h, -h, -h), (h, h, -h), (-h, h, -h), (-h, -h, h), (h, -h, h), (h, h, h), (-h, h, h)]
    faces = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]  # -z +z -y +y -x +x
    V, I = [], []
    for f in faces:
        b = len(V)
        V.extend(c[i] for i in f)
        I.extend([[b, b + 1, b + 2], [b, b + 2, b + 3]])
    return np.array(V, np.float32), np.array(I, np.uint32)


def glass_box_scene(xres, yres, eta=ETA):
    """furnished_box_scene with the whole ceiling emitting (no small emitter) and the glass sphere"""
    from pbrt_amd import GLASS, MATTE
    sd = im.furnished_box_scene(xres, yres)
    keep = sd.mat_id != 6  # the small emitter leaves
    sd.idx, sd.mat_id = sd.idx[keep], sd.mat_id[keep]
    mats = sd.materials.copy()
    mats[1] = [MATTE, 0, 0, 0, *LE_CEILING]  # the ceiling (its winding normal points down, into the box)
    mats[6] = [GLASS, 1, 1, 1, 1, 1, 1]
    sd.materials = mats
    sd.mat_eta = np.full(len(mats), eta, np.float32)
    sd.mat_tex = np.zeros(0, np.uint32)
    sd.spheres = np.array([[*SPHERE_C, SPHERE_R, 6]], np.float32)
    return sd.normalized()


def furnace_scene(kind, eta, xres=FURNACE_RES, yres=FURNACE_RES, env=ENV):
    """kind "sphere" / "cube": one glass object (Kr = Kt = 1) alone under a constant infinite light"""
    from pbrt_amd import GLASS, LIGHT_INFINITE, SceneData, look_at
    sd = SceneData(materials=np.array([[GLASS, 1, 1, 1, 1, 1, 1]], np.float32), mat_eta=np.array([eta], np.float32),
                   lights=np.array([[LIGHT_INFINITE, 0, 0, 0, *env]], np.float32),
                   cam_to_world=look_at(FURNACE_EYE, FURNACE_LOOK, FURNACE_UP)[1], fov=FURNACE_FOV, xres=xres, yres=yres)
    if kind == "sphere":
        sd.spheres = np.array([[0, 0, 0, FURNACE_SPHERE_R, 0]], np.float32)
    else:
        sd.P, sd.idx = _cube_mesh(FURNACE_CUBE_H)
        sd.mat_id = np.zeros(len(sd.idx), np.uint16)
    return sd.normalized()


# ---- the estimator ----

def _camera_rays(rng, n, xres, yres, eye, look, up, fov):
    eye, look, up = np.array(eye, np.float64), np.array(look, np.float64), np.array(up, np.float64)
    fwd = (look - eye) / np.linalg.norm(look - eye)
    right = np.cross(up / np.linalg.norm(up), fwd)
    right /= np.linalg.norm(right)
    new_up = np.cross(fwd, right)
    aspect = xres / yres
    wx, wy = (aspect, 1.0) if aspect >= 1 else (1.0, 1.0 / aspect)
    t = np.tan(np.radians(fov) / 2)
    fx, fy = rng.random(n) * xres, rng.random(n) * yres
    d = ((2 * fx / xres - 1) * wx * t)[:, None] * right + ((1 - 2 * fy / yres) * wy * t)[:, None] * new_up + fwd
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(eye, (n, 1)), d, fx.astype(np.int64), fy.astype(np.int64)


_T_MIN = 1e-7  # (origins sit on surfaces to ~1e-16: a root this close to 0 is the surface the ray leaves)


def _hit_sphere(o, d, c, r):
    """-> (t or inf, outward unit normal at the hit)"""
    oc = o - c
    b = (oc * d).sum(1)
    disc = b * b - ((oc * oc).sum(1) - r * r)
    sq = np.sqrt(np.maximum(disc, 0.0))
    t0, t1 = -b - sq, -b + sq
    t = np.where(t0 > _T_MIN, t0, np.where(t1 > _T_MIN, t1, np.inf))
    t = np.where(disc > 0, t, np.inf)
    tt = np.where(np.isfinite(t), t, 0.0)
    return t, (oc + tt[:, None] * d) / r


def _hit_cube(o, d, h):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        ta, tb = (-h - o) * inv, (h - o) * inv
    parallel = d == 0
    inside_slab = np.abs(o) <= h
    near = np.where(parallel, np.where(inside_slab, -np.inf, np.inf), np.minimum(ta, tb))
    far = np.where(parallel, np.where(inside_slab, np.inf, -np.inf), np.maximum(ta, tb))
    an, af = np.argmax(near, axis=1), np.argmin(far, axis=1)
    rows = np.arange(o.shape[0])
    tn, tf = near[rows, an], far[rows, af]
    hit = tn <= tf
    enter = hit & (tn > _T_MIN)
    leave = hit & ~enter & (tf > _T_MIN)
    t = np.where(enter, tn, np.where(leave, tf, np.inf))
    axis = np.where(enter, an, af)
    normal = np.zeros_like(o)
    sgn = np.sign(d[rows, axis])
    normal[rows, axis] = np.where(enter, -sgn, sgn)
    return t, normal


def _glass_vertex(rng, d, n_out, eta, beta):
    """The 1/2 - 1/2 strategy (module docstring), Kr = Kt = 1.  -> the new directions; `beta` is scaled in place."""
    cos_o = -(d * n_out).sum(1)
    entering = cos_o > 0
    eta_i, eta_t = np.where(entering, 1.0, eta), np.where(entering, eta, 1.0)
    nf = np.where(entering[:, None], n_out, -n_out)
    ci = np.abs(cos_o)
    f = fr_dielectric(ci, eta_i, eta_t)
    reflect = rng.random(d.shape[0]) < 0.5
    r = eta_i / eta_t
    ct = np.sqrt(np.maximum(0.0, 1.0 - r * r * np.maximum(0.0, 1.0 - ci * ci)))
    nd = np.where(reflect[:, None], d + 2.0 * ci[:, None] * nf, r[:, None] * d + (r * ci - ct)[:, None] * nf)
    beta *= np.where(reflect, 2.0 * f, 2.0 * (1.0 - f) * r * r)[:, None]
    nd /= np.linalg.norm(nd, axis=1, keepdims=True)
    return nd


def _run(rng, n, xres, yres, max_depth, camera, glass_hit, eta, box):
    """n paths -> (L[n, 3], px, py).  `box`: the closed box's walls and emitting ceiling around the glass; else the environment ENV."""
    o, d, px, py = _camera_rays(rng, n, xres, yres, *camera)
    beta = np.ones((n, 3))
    L = np.zeros((n, 3))
    alive = np.ones(n, bool)
    wall_kd = np.array([im.KD["left"], (0, 0, 0), im.KD["front"], im.KD["back"], im.KD["floor"], (0, 0, 0)])  # 2 * axis + (the + side)
    for segment in range(max_depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        oo, dd = o[idx], d[idx]
        t_g, n_g = glass_hit(oo, dd)
        if box:
            with np.errstate(divide="ignore", invalid="ignore"):
                t_axis = (np.where(dd > 0, 1.0, -1.0) - oo) / dd
                t_axis = np.where(dd == 0, np.inf, t_axis)
            axis = np.argmin(t_axis, axis=1)
            t_wall = t_axis[np.arange(idx.size), axis]
        else:
            t_wall = np.full(idx.size, np.inf)
        on_glass = t_g < t_wall
        if not box:
            miss = ~on_glass
            L[idx[miss]] += beta[idx[miss]] * ENV
            alive[idx[miss]] = False
        else:
            w = ~on_glass
            plus = dd[np.arange(idx.size), axis] > 0
            wall = 2 * axis + plus
            ceiling = w & (wall == 5)
            L[idx[ceiling]] += beta[idx[ceiling]] * LE_CEILING
            alive[idx[ceiling]] = False  # its Kd is 0
            w &= ~ceiling
            if segment < max_depth and w.any():
                wi = idx[w]
                p = oo[w] + t_wall[w, None] * dd[w]
                normal = np.zeros((wi.size, 3))
                normal[np.arange(wi.size), axis[w]] = np.where(plus[w], -1.0, 1.0)
                mirror = wall[w] == 1
                nd = np.empty((wi.size, 3))
                nd[mirror] = dd[w][mirror] - 2 * (dd[w][mirror] * normal[mirror]).sum(1, keepdims=True) * normal[mirror]
                nd[~mirror] = im._scatter_cosine(rng, normal[~mirror])
                beta[wi[mirror]] *= im.KR
                beta[wi[~mirror]] *= wall_kd[wall[w][~mirror]]
                o[wi], d[wi] = p, nd
        if segment >= max_depth:
            break
        g = on_glass
        gi = idx[g]
        if gi.size:
            o[gi] = oo[g] + t_g[g, None] * dd[g]
            bg = beta[gi]
            d[gi] = _glass_vertex(rng, dd[g], n_g[g], eta, bg)
            beta[gi] = bg
        # every vertex that scattered: dead at zero throughput; Russian roulette after more than 3 scatterings
        s = np.nonzero(alive)[0]
        mx = beta[s].max(1)
        alive[s[mx == 0]] = False
        if segment > 3:
            s, mx = s[mx > 0], mx[mx > 0]
            q = np.maximum(0.05, 1.0 - mx)
            dead = rng.random(s.size) < q
            alive[s[dead]] = False
            beta[s[~dead]] /= (1.0 - q[~dead])[:, None]
    return L, px, py


def _blocks(rng, xres, yres, block, n_paths, batch, run):
    bx_n, by_n = xres // block, yres // block
    s1, s2, cnt = np.zeros((by_n * bx_n, 3)), np.zeros((by_n * bx_n, 3)), np.zeros(by_n * bx_n)
    done = 0
    while done < n_paths:
        n = min(batch, n_paths - done)
        done += n
        L, px, py = run(rng, n)
        b = (py // block) * bx_n + (px // block)
        for c in range(3):
            s1[:, c] += np.bincount(b, L[:, c], by_n * bx_n)
            s2[:, c] += np.bincount(b, L[:, c] ** 2, by_n * bx_n)
        cnt += np.bincount(b, minlength=by_n * bx_n)
    mean = s1 / cnt[:, None]
    var = np.maximum(s2 / cnt[:, None] - mean ** 2, 0)
    return mean.reshape(by_n, bx_n, 3), np.sqrt(var / cnt[:, None]).reshape(by_n, bx_n, 3), cnt.reshape(by_n, bx_n)


_cache = {}


def block_means(xres, yres, block, max_depth, n_paths, seed=12345, batch=1 << 19, eta=ETA):
    """glass_box_scene -> (mean[by, bx, 3], standard error[by, bx, 3]) of the radiance over blocks of block x block pixels."""
    key = ("box", xres, yres, block, max_depth, n_paths, seed, eta)
    if key not in _cache:
        camera = (im.EYE, im.LOOK, im.UP, im.FOV)
        hit = lambda o, d: _hit_sphere(o, d, SPHERE_C, SPHERE_R)
        _cache[key] = _blocks(np.random.default_rng(seed), xres, yres, block, n_paths, batch,
                              lambda rng, n: _run(rng, n, xres, yres, max_depth, camera, hit, eta, True))[:2]
    return _cache[key]


def furnace_block_means(kind, eta, block=8, n_paths=FURNACE_PATHS, max_depth=FURNACE_DEPTH, res=FURNACE_RES, seed=777, batch=1 << 19):
    """furnace_scene -> (mean[by, bx, 3], standard error[by, bx, 3], paths[by, bx]) of the reference's own estimate"""
    key = ("furnace", kind, eta, block, n_paths, max_depth, res, seed)
    if key not in _cache:
        camera = (FURNACE_EYE, FURNACE_LOOK, FURNACE_UP, FURNACE_FOV)
        if kind == "sphere":
            hit = lambda o, d: _hit_sphere(o, d, np.zeros(3), FURNACE_SPHERE_R)
        else:
            hit = lambda o, d: _hit_cube(o, d, FURNACE_CUBE_H)
        _cache[key] = _blocks(np.random.default_rng(seed), res, res, block, n_paths, batch,
                              lambda rng, n: _run(rng, n, res, res, max_depth, camera, hit, eta, False))
    return _cache[key]


def compare_with_blocks(rgb, mean, se, block):
    """rgb[y, x, 3]: a render of glass_box_scene.  -> (largest |difference| in units of the estimate's standard error + 0.4 % of the
    value, the relative difference of the whole image's sum)."""
    return im.compare_with_blocks(rgb, mean, se, block)
