"""Float64 references of the shading normals for tests/test_normals_host.py and tests/test_normals_gpu.py.  Nothing below
shares a line with the library or the oracle (whose own restatement tests/test_oracle_normals_plastic_images.py holds to this): the normal's statement in float64 with its first-order error
bounds, closed forms of the lit plane, the clipped cosine lobe and the mirror, the camera of DESIGN.md 3.2 in float64, and the scenes the GPU
tests build.  Every bound is derived from the roundings the kernel states (fp32, fixed operation order, no contraction) -- none is taken
from the outputs under test.

THE NORMAL.  With u = 2^-24, gamma_k = k u / (1 - k u), and the inputs (float32 values) exact in float64:
  w  = fl(fl(1 - b1) - b2)                          |dw|    <= u (|1 - b1| + |w|)
  n  = fl(fl(fl(n0 w) + fl(n1 b1)) + fl(n2 b2))     |dn_k|  <= gamma_3 (|n0_k w| + |n1_k b1| + |n2_k b2|) + |n0_k| |dw|       =: E_k
  l2 = fl(fl(fl(nx nx) + fl(ny ny)) + fl(nz nz))    |dl2|   <= gamma_3 l2 + 2 sum_k |n_k| E_k
  s  = fl(sqrt(l2))                                 |ds|    <= |dl2| / (2 s) + u s                                             =: E_s
  ns = fl(n / s)                                    |dns_k| <= E_k / s + |n_k| E_s / s^2 + u |ns_k|                            =: B_k
  dot(ns, ng)                                       error   <= sum_k |ng_k| B_k + gamma_3 sum_k |ns_k ng_k|
  dot(ng, wo)                                       error   <= gamma_3 sum_k |ng_k wo_k|
(first-order terms; SECOND_ORDER covers the rest).  The flips are exact negations."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
GAMMA3 = 3 * U / (1 - 3 * U)
SECOND_ORDER = 1.0 + 2.0 ** -20
ROBUST_FACTOR = 16.0


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frame(axis):
    """two unit vectors orthogonal to the unit rows of `axis` and to each other"""
    a = np.where(np.abs(axis[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    s = _unit(np.cross(axis, a))
    return s, np.cross(axis, s)


def _cone(rng, axis, max_deg):
    """unit vectors within max_deg of the unit rows of `axis`, uniform in the angle"""
    th = np.radians(max_deg) * rng.random(len(axis))
    ph = 2 * np.pi * rng.random(len(axis))
    s, t = _frame(axis)
    return np.cos(th)[:, None] * axis + np.sin(th)[:, None] * (np.cos(ph)[:, None] * s + np.sin(ph)[:, None] * t)


def hook_inputs(n=1 << 16, seed=18):
    """-> (x (n, 17) float32 rows n0 n1 n2 ng b1 b2 wo, kind (n,) of KINDS).  Corner normals: unit vectors within 60 degrees of a common
    axis, scaled by 10^-3 .. 10^3 per corner; barycentrics uniform over the triangle, plus all corners and edge points; ng a unit vector
    within 80 degrees of the axis ("plain") or of its opposite ("far side": the flip applies); wo a uniform direction, so on either side.
    The edge cases: all-zero normals, one zero corner."""
    rng = np.random.default_rng(seed)
    axis = _unit(rng.normal(size=(n, 3)))
    nc = np.stack([_cone(rng, axis, 60.0) * 10.0 ** rng.uniform(-3, 3, (n, 1)) for _ in range(3)], 1)  # (n, 3 corners, 3)
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    b1, b2 = r1 * (1 - r2), r1 * r2  # uniform over the triangle; w = 1 - r1
    kind = np.zeros(n, np.int64)
    k = np.arange(n)
    # corners and edge points (the first 4096 elements)
    special = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.5, 0.0), (0.0, 0.5), (0.25, 0.75), (1.0 - 2.0 ** -24, 0.0)]
    for i, (p, q) in enumerate(special):
        m = (k < 4096) & (k % len(special) == i)
        b1[m], b2[m] = p, q
    edge = (k >= 4096) & (k < 8192)
    b2[edge & (k % 3 == 0)] = 0.0
    b1[edge & (k % 3 == 1)] = 0.0
    m = edge & (k % 3 == 2)
    b2[m] = 1.0 - b1[m]
    far = k % 4 == 1
    ng = _cone(rng, np.where(far[:, None], -axis, axis), 80.0)
    kind[far] = 1
    zero_all = (k % 64 == 7)
    nc[zero_all] = 0.0
    kind[zero_all] = 2
    one_zero = (k % 64 == 10)
    nc[one_zero, (k[one_zero] // 64) % 3] = 0.0
    kind[one_zero] = 3
    wo = _unit(rng.normal(size=(n, 3)))
    x = np.concatenate([nc.reshape(n, 9), _unit(ng.astype(F32).astype(np.float64)), b1[:, None], b2[:, None], wo], 1).astype(F32)
    return np.ascontiguousarray(x), kind


KINDS = ("plain", "far side", "all zero", "one zero corner")


def shading_normal_f64(x):
    """x (n, 17) float32 as given to the hook -> dict of float64 arrays: nsf (n, 3), bound (n, 3) on each of its components, fell_back,
    flip_ng (dot(ns, ng) < 0), flip_wo (dot(ng, wo) < 0), robust (|n|, |dot(ns, ng)|, |dot(ng, wo)| each beyond ROBUST_FACTOR x its bound)"""
    x = np.ascontiguousarray(x, F32).astype(np.float64)
    n0, n1, n2, ng, b1, b2, wo = x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12], x[:, 12:13], x[:, 13:14], x[:, 14:17]
    w = (1.0 - b1) - b2
    dw = U * (np.abs(1.0 - b1) + np.abs(w))
    n = n0 * w + n1 * b1 + n2 * b2
    E = GAMMA3 * (np.abs(n0 * w) + np.abs(n1 * b1) + np.abs(n2 * b2)) + np.abs(n0) * dw
    l2 = (n * n).sum(1, keepdims=True)
    fell_back = ~(l2[:, 0] > 0)
    with np.errstate(all="ignore"):
        dl2 = GAMMA3 * l2 + 2 * (np.abs(n) * E).sum(1, keepdims=True)
        s = np.sqrt(l2)
        Es = dl2 / (2 * s) + U * s
        ns = n / s
        B = (E / s + np.abs(n) * Es / (s * s) + U * np.abs(ns)) * SECOND_ORDER
        c_ng = (ns * ng).sum(1)
        c_ng_err = ((np.abs(ng) * B).sum(1) + GAMMA3 * np.abs(ns * ng).sum(1)) * SECOND_ORDER
    c_wo = (ng * wo).sum(1)
    c_wo_err = GAMMA3 * np.abs(ng * wo).sum(1) * SECOND_ORDER
    flip_ng, flip_wo = c_ng < 0, c_wo < 0
    ns = np.where(fell_back[:, None], ng, np.where(flip_ng[:, None], -ns, ns))
    nsf = np.where(flip_wo[:, None], -ns, ns)
    with np.errstate(invalid="ignore"):
        robust = ~fell_back & (s[:, 0] > ROBUST_FACTOR * Es[:, 0]) & (np.abs(c_ng) > ROBUST_FACTOR * c_ng_err) & (np.abs(c_wo) > ROBUST_FACTOR * c_wo_err)
    return dict(nsf=nsf, bound=np.where(fell_back[:, None], 0.0, B), fell_back=fell_back, flip_ng=flip_ng, flip_wo=flip_wo, robust=robust,
                c_wo=c_wo, c_wo_err=c_wo_err)


# ---- closed forms ----

def tilted(theta_deg, azimuth_deg=0.0):
    """the unit vector `theta` from +z towards the azimuth (0 = +x)"""
    t, a = np.radians(theta_deg), np.radians(azimuth_deg)
    return np.array([np.sin(t) * np.cos(a), np.sin(t) * np.sin(a), np.cos(t)])


def lambert_distant(rho, L, n, wl):
    """a matte surface of albedo rho and unit shading normal n under a distant light of radiance L from the unit direction wl"""
    return np.asarray(rho, np.float64) / np.pi * np.asarray(L, np.float64) * max(0.0, float(np.dot(n, wl)))


def clipped_lobe_fraction(theta_deg):
    """the share of a cosine lobe about a normal tilted by theta that lies above the geometric plane: (1 + cos theta) / 2"""
    return 0.5 * (1.0 + np.cos(np.radians(theta_deg)))


def clipped_lobe_sampled(theta_deg, n=1 << 22, seed=3):
    """the same share from a numpy cosine sampler (no closed form involved): directions drawn about the tilted normal, counted where z > 0"""
    rng = np.random.default_rng(seed)
    u1, u2 = rng.random(n), rng.random(n)
    r, ph = np.sqrt(u1), 2 * np.pi * u2
    loc = np.stack([r * np.cos(ph), r * np.sin(ph), np.sqrt(1 - u1)], 1)
    nz = tilted(theta_deg)
    s, t = _frame(nz[None])
    world = loc[:, :1] * s + loc[:, 1:2] * t + loc[:, 2:3] * nz
    return float((world[:, 2] > 0).mean())


def reflect(wo, n):
    return -wo + 2.0 * (wo * n).sum(-1, keepdims=True) * n


# ---- the camera of DESIGN.md 3.2, float64 ----

def camera_rays(sd, fx, fy):
    """origin (3,) and unit directions (..., 3) of the rays through the raster points (fx, fy) of SceneData sd: perspective camera, fov on
    the shorter axis, raster y down"""
    c2w = np.asarray(sd.cam_to_world, np.float64)
    aspect = sd.xres / sd.yres
    wx, wy = (aspect, 1.0) if aspect > 1 else (1.0, 1.0 / aspect)
    t = np.tan(np.radians(float(sd.fov)) / 2)
    cx = (2 * np.asarray(fx, np.float64) / sd.xres - 1) * wx * t
    cy = (1 - 2 * np.asarray(fy, np.float64) / sd.yres) * wy * t
    dc = np.stack(np.broadcast_arrays(cx, cy, np.ones_like(cx * cy)), -1)
    d = dc @ c2w[:3, :3].T
    return c2w[:3, 3].copy(), d / np.linalg.norm(d, axis=-1, keepdims=True)


def pixel_corner_rays(sd):
    """-> (o, d[4, yres, xres, 3]): the rays through the four corners of every pixel"""
    x, y = np.meshgrid(np.arange(sd.xres, dtype=np.float64), np.arange(sd.yres, dtype=np.float64))
    o, _ = camera_rays(sd, x, y)
    return o, np.stack([camera_rays(sd, x + dx, y + dy)[1] for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))])


def plane_points(o, d):
    """where rays from o with directions d meet z = 0 -> (x, y)"""
    t = -o[2] / d[..., 2]
    return o[0] + t * d[..., 0], o[1] + t * d[..., 1]


# ---- scenes ----

def with_normal(sd, n):
    """sd with every corner of every triangle carrying the normal n"""
    sd.tri_n = np.tile(np.asarray(n, np.float64), (sd.idx.shape[0], 3)).astype(F32)
    return sd.normalized()


def face_normals(sd):
    """float64 face normals (unit, of the winding) of every triangle, rounded to fp32, on all three corners -> (n_tris, 9)"""
    P = sd.P.astype(np.float64)[sd.idx.astype(np.int64)]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
    return np.tile(n, (1, 3)).astype(F32)


GRID_X, GRID_Y, GRID_N = (-2.6, 1.8), (-1.5, 3.5), 8


GRID_LIGHT = (8.0, 200.0)  # the distant light of the gather test: 8 degrees from the zenith


def grid_normals():
    """the 128 constant normals of the gather test.  Triangle k's value is proportional to n_k . wl, and any two must differ by far more than
    the bar they are compared at, so the COSINES are spaced evenly: n_k makes the angle acos(c_k) with the light, c_k = cos 27 + (cos 8 -
    cos 27) ((37 k) mod 128) / 127 -- 128 distinct values 7.8e-4 apart --, at the azimuth 47 k degrees about it: at most 8 + 27 = 35
    degrees from +z"""
    wl = tilted(*GRID_LIGHT)
    s, t = _frame(wl[None])
    out = []
    for k in range(2 * GRID_N * GRID_N):
        c = np.cos(np.radians(27.0)) + (np.cos(np.radians(8.0)) - np.cos(np.radians(27.0))) * ((37 * k) % 128) / 127.0
        psi = np.radians(47.0 * k)
        out.append(c * wl + np.sqrt(1 - c * c) * (np.cos(psi) * s[0] + np.sin(psi) * t[0]))
    return np.stack(out)


def grid_plane_scene(res=64, below=None):
    """lit_plane_scene's camera and material over a plane z = 0 cut into 8 x 8 cells x 2 triangles on GRID_X x GRID_Y, triangle k =
    2 (8 j + i) + h (h = 0: the cell's lower right half, 1: its upper left) carrying grid_normals()[k]; one distant light near the zenith.
    `below`: a SceneData whose triangles are added under the plane with zero normals.  -> (sd, wl, L, rho)"""
    import util
    from pbrt_amd.api import LIGHT_DISTANT
    sd, _ = util.lit_plane_scene("distant", res)
    xs, ys = np.linspace(*GRID_X, GRID_N + 1), np.linspace(*GRID_Y, GRID_N + 1)
    P = np.array([(x, y, 0.0) for y in ys for x in xs], np.float32)
    idx = []
    for j in range(GRID_N):
        for i in range(GRID_N):
            a, b, c, d = j * 9 + i, j * 9 + i + 1, (j + 1) * 9 + i + 1, (j + 1) * 9 + i
            idx += [(a, b, c), (a, c, d)]  # normal +z
    wl = tilted(*GRID_LIGHT)
    L = np.array([3.0, 2.0, 1.0])
    tri_n = np.repeat(grid_normals(), 3, axis=0).reshape(-1, 9)
    sd.P, sd.idx, sd.mat_id = P, np.array(idx, np.uint32), np.zeros(len(idx), np.uint16)
    if below is not None:
        Pb = below.P.astype(np.float32).copy()
        Pb[:, 2] -= 5.0  # under the plane: hidden from the camera and from the light
        sd.idx = np.concatenate([sd.idx, below.idx + np.uint32(len(P))])
        sd.P = np.concatenate([P, Pb])
        sd.mat_id = np.zeros(len(sd.idx), np.uint16)
        tri_n = np.concatenate([tri_n, np.zeros((len(below.idx), 9))])
    sd.tri_n = tri_n.astype(F32)
    sd.lights = np.array([[LIGHT_DISTANT, *wl.astype(F32), *L]], np.float32)
    return sd.normalized(), sd.lights[0, 1:4].astype(np.float64), L, sd.materials[0, 1:4].astype(np.float64)


def grid_triangle_of(x, y):
    """the triangle of grid_plane_scene under the plane point (x, y); -1 outside the grid"""
    u = (np.asarray(x) - GRID_X[0]) / (GRID_X[1] - GRID_X[0]) * GRID_N
    v = (np.asarray(y) - GRID_Y[0]) / (GRID_Y[1] - GRID_Y[0]) * GRID_N
    inside = (u >= 0) & (u < GRID_N) & (v >= 0) & (v < GRID_N)
    i, j = np.clip(np.floor(u), 0, GRID_N - 1).astype(int), np.clip(np.floor(v), 0, GRID_N - 1).astype(int)
    upper = (v - j) > (u - i)  # above the cell's diagonal a -> c: the triangle (a, c, d)
    return np.where(inside, 2 * (GRID_N * j + i) + upper.astype(int), -1)
