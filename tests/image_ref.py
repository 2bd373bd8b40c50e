"""DESIGN.md 3.20 restated in float64 numpy from its text (shares no code with pbrt_amd/csrc/image_lookup.hpp), and the inputs the host and
the GPU tests of the image textures share."""
import numpy as np

REPEAT, CLAMP, BLACK = 0, 1, 2
POINT, BILINEAR = 0, 1
WRAP_NAMES = {REPEAT: "repeat", CLAMP: "clamp", BLACK: "black"}
SIZES = ((1, 1), (2, 2), (3, 5), (8, 1), (1, 7), (17, 4))  # (W, H)


def random_image(w, h, seed):
    return np.random.default_rng(seed).uniform(0.05, 0.95, (h, w, 3)).astype(np.float32)


def mapped32(uv, mapping):
    """(s, t) as the kernel forms it: fp32, product then sum"""
    su, sv, du, dv = (np.float32(x) for x in mapping)
    uv = np.asarray(uv, np.float32)
    with np.errstate(all="ignore"):
        return (su * uv[:, 0] + du).astype(np.float32), (sv * uv[:, 1] + dv).astype(np.float32)


def mapped64(uv, mapping):
    su, sv, du, dv = (float(np.float32(x)) for x in mapping)
    uv = np.asarray(uv, np.float32).astype(np.float64)
    return su * uv[:, 0] + du, sv * uv[:, 1] + dv


def _clamp_index(xf, n):
    """fmaxf first (a NaN becomes 0), then fminf, then the cast"""
    return np.clip(np.where(np.isnan(xf), 0.0, xf), 0.0, n - 1.0).astype(np.int64)


def _inside(xf, n):
    return (xf >= 0.0) & (xf <= n - 1.0)


def point(img, wrap, s, t):
    """the texel of (s, t), float64 arithmetic: (n, 3) and the float indices before the clamp"""
    img = np.asarray(img, np.float64)
    H, W = img.shape[:2]
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        if wrap == REPEAT:
            xf, yf = np.floor((s - np.floor(s)) * W), np.floor((t - np.floor(t)) * H)
        else:
            xf, yf = np.floor(s * W), np.floor(t * H)
    c = img[H - 1 - _clamp_index(yf, H), _clamp_index(xf, W)]
    if wrap == BLACK:
        c = np.where((_inside(xf, W) & _inside(yf, H))[:, None], c, 0.0)
    return c


def bilinear(img, wrap, s, t):
    img = np.asarray(img, np.float64)
    H, W = img.shape[:2]
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        sx, sy = s * W - 0.5, t * H - 0.5
        x0, y0 = np.floor(sx), np.floor(sy)
        dx, dy = sx - x0, sy - y0
        dx, dy = np.clip(np.where(np.isnan(dx), 0.0, dx), 0.0, 1.0), np.clip(np.where(np.isnan(dy), 0.0, dy), 0.0, 1.0)
        acc = np.zeros(s.shape + (3,))
        for j in range(2):
            cy, wy = (y0 + j), (dy if j else 1.0 - dy)
            if wrap == REPEAT:
                cy = cy - H * np.floor(cy / H)
            if wrap == BLACK:
                wy = np.where(_inside(cy, H), wy, 0.0)
            for i in range(2):
                cx, wx = (x0 + i), (dx if i else 1.0 - dx)
                if wrap == REPEAT:
                    cx = cx - W * np.floor(cx / W)
                if wrap == BLACK:
                    wx = np.where(_inside(cx, W), wx, 0.0)
                acc = acc + img[H - 1 - _clamp_index(cy, H), _clamp_index(cx, W)] * (wx * wy)[:, None]
    return acc


def near_integer(x, eps=1e-5):
    """|x - nearest integer| <= eps max(1, |x|)"""
    return np.abs(x - np.round(x)) <= eps * np.maximum(1.0, np.abs(x))


def dyadic_inputs(seed=0, rows=17):
    """(u, v) on the 2^-10 grid of [-3, 3]^2: every grid value of u against `rows` grid values of v (the integers' neighbourhood among them),
    and the transpose"""
    rng = np.random.default_rng(seed)
    g = np.arange(-3 * 1024, 3 * 1024 + 1, dtype=np.float64) / 1024.0
    some = np.concatenate([[-3.0, -1.0, -1.0 / 1024, 0.0, 1.0 / 1024, 0.5, 1.0, 3.0], rng.choice(g, rows - 8, replace=False)])
    a = np.stack(np.meshgrid(g, some, indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([a, a[:, ::-1]]).astype(np.float32)


def random_inputs(n, seed):
    """random (u, v) in [-4, 4]^2 and a random mapping (su, sv, du, dv)"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-4, 4, (n, 2)).astype(np.float32)
    mapping = tuple(float(x) for x in np.concatenate([rng.uniform(-3, 3, 2), rng.uniform(-1, 1, 2)]).astype(np.float32))
    return uv, mapping


NON_FINITE = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)


def non_finite_inputs():
    """u or v or both among NaN, +-inf, +-1e30 (the other one ordinary), mapping the identity"""
    rows = [(x, 0.3) for x in NON_FINITE] + [(0.7, x) for x in NON_FINITE] + [(x, y) for x in NON_FINITE for y in NON_FINITE]
    return np.array(rows, np.float32)


def checker_as_image(tex_row):
    """a checkerboard row (0, tex1, tex2, su, sv, du, dv) of SceneData.textures as the 2 x 2 point-sampled repeat image that equals it
    (DESIGN.md 3.20): the image [[tex2, tex1], [tex1, tex2]] (rows top to bottom) and the mapping halved"""
    t = np.asarray(tex_row, np.float32)
    t1, t2 = t[1:4], t[4:7]
    img = np.array([[t2, t1], [t1, t2]], np.float32)
    return img, tuple(float(np.float32(x) * np.float32(0.5)) for x in t[7:11])


def with_checkers_as_images(sd):
    """a copy of the scene whose checkerboards are replaced, slot by slot, by their 2 x 2 images"""
    import dataclasses
    from pbrt_amd import api
    images, rows = [], []
    for t in sd.textures:
        assert int(t[0]) == 0
        img, mapping = checker_as_image(t)
        rows.append(api.image_texture_row(len(images), REPEAT, POINT, mapping))
        images.append(img)
    return dataclasses.replace(sd, textures=np.array(rows, np.float32).reshape(-1, 11), images=images).normalized()
