"""The weighted pixel filters of DESIGN.md 3.19, restated in numpy for the tests: the four filters in float64 and their 16 x 16 table, the
float32 footprint and table-index statements, the fixed-point add, the conversion to film pixels, and a sample's FILM POINT under the (0,2)
sampler (3.10: the first 2-D request of a sample) and under the stratified sampler (3.1).  Nothing here calls the product.

The stratified sampler's film point of a sample is two draws from its chunk's PCG32 stream, and a path draws from the same stream: the film
point of a chunk's FIRST sample is two draws from the fresh stream; that of a later sample lies behind the draws of the paths before it.  So
the stratified sampler is restated in two settings where the number of those draws is known without restating the path integrator: one
sample per pixel in any scene (every sample is its chunk's first), and ANY sample count in a render whose paths draw nothing -- max_depth 0:
a path ends at its first vertex with the emission it finds there, or in the sky -- where sample s of a chunk takes draws (2 s', 2 s' + 1) of
the chunk's stream, s' its place in the chunk (stratified_film_points_no_draws).  The (0,2) sampler's points depend on (pixel, sample) alone.
A sample's radiance comes from the oracle (OracleScene.pixel_samples), which is given the scene WITHOUT the filter."""
import numpy as np

from independent_twin import _Pcg

F32 = np.float32
TRIANGLE, GAUSSIAN, MITCHELL, SINC = 1, 2, 3, 4
KINDS = {"triangle": TRIANGLE, "gaussian": GAUSSIAN, "mitchell": MITCHELL, "sinc": SINC}
DEFAULT_PARAMS = {TRIANGLE: (0.0, 0.0), GAUSSIAN: (2.0, 0.0), MITCHELL: (1.0 / 3.0, 1.0 / 3.0), SINC: (3.0, 0.0)}
FIXED_ONE, FIXED_MAX = F32(16777216.0), F32(32768.0)
_EPS1 = F32(1.0) - F32(2.0 ** -23)


def default_radius(kind):
    return 4.0 if kind == SINC else 2.0


def radii_of(kind, width):
    """the radii a render's filter_width stands for: 0 = the kind's default"""
    return tuple(float(w) if float(w) != 0.0 else default_radius(kind) for w in width)


# ---- the filters in float64 (pbrt-v3's Evaluate) ----
def _gaussian(d, r, alpha):
    return np.maximum(0.0, np.exp(-alpha * d * d) - np.exp(-alpha * r * r))


def _mitchell(x, B, C):
    t = np.abs(2.0 * x)
    far = ((-B - 6.0 * C) * t * t * t + (6.0 * B + 30.0 * C) * t * t + (-12.0 * B - 48.0 * C) * t + (8.0 * B + 24.0 * C)) / 6.0
    near = ((12.0 - 9.0 * B - 6.0 * C) * t * t * t + (-18.0 + 12.0 * B + 6.0 * C) * t * t + (6.0 - 2.0 * B)) / 6.0
    return np.where(t > 1.0, far, near)


def _sinc(x):
    x = np.abs(x)
    with np.errstate(all="ignore"):
        return np.where(x < 1e-5, 1.0, np.sin(np.pi * x) / (np.pi * x))


def _windowed_sinc(x, r, tau):
    x = np.abs(x)
    return np.where(x > r, 0.0, _sinc(x) * _sinc(x / tau))


def evaluate(kind, params, x, y, rx, ry):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    p0, p1 = float(F32(params[0])), float(F32(params[1]))  # (the record holds floats)
    if kind == TRIANGLE:
        return np.maximum(0.0, rx - np.abs(x)) * np.maximum(0.0, ry - np.abs(y))
    if kind == GAUSSIAN:
        return _gaussian(x, rx, p0) * _gaussian(y, ry, p0)
    if kind == MITCHELL:
        return _mitchell(x / rx, p0, p1) * _mitchell(y / ry, p0, p1)
    if kind == SINC:
        return _windowed_sinc(x, rx, p0) * _windowed_sinc(y, ry, p0)
    raise ValueError(kind)


def table64(kind, params, rx, ry):
    """(16, 16) float64: [iy, ix] = the filter at ((ix + 0.5) rx / 16, (iy + 0.5) ry / 16); rx, ry as the floats the library is handed"""
    rx, ry = float(F32(rx)), float(F32(ry))
    i = np.arange(16) + 0.5
    return evaluate(kind, params, (i * rx / 16.0)[None, :], (i * ry / 16.0)[:, None], rx, ry)


def table(kind, params, rx, ry):
    return table64(kind, params, rx, ry).astype(F32)


# ---- where a sample lands: float32, the order of 3.11 / 3.19 ----
def sample_bounds(crop_bounds, rx, ry):
    """Film::get_sample_bounds (3.11): the sampled pixels x0, y0, x1, y1 (x1, y1 exclusive) and the halo's pads"""
    c = [F32(v) for v in crop_bounds]
    rx, ry = F32(rx), F32(ry)
    sb = (int(np.floor((c[0] + F32(0.5)) - rx)), int(np.floor((c[1] + F32(0.5)) - ry)), int(np.ceil((c[2] - F32(0.5)) + rx)), int(np.ceil((c[3] - F32(0.5)) + ry)))
    return sb, (max(0, int(np.ceil(rx - F32(0.5)))), max(0, int(np.ceil(ry - F32(0.5)))))


def footprint(fx, fy, rx, ry, crop_bounds):
    """(x0, y0, x1, y1) int64 arrays, x1 / y1 exclusive: d = p - 0.5, pixels [ceil(d - r), floor(d + r)] clipped to the window"""
    fx, fy, rx, ry = np.asarray(fx, F32), np.asarray(fy, F32), F32(rx), F32(ry)
    dx, dy = fx - F32(0.5), fy - F32(0.5)
    x0 = np.maximum(np.ceil(dx - rx).astype(np.int64), crop_bounds[0])
    x1 = np.minimum(np.floor(dx + rx).astype(np.int64) + 1, crop_bounds[2])
    y0 = np.maximum(np.ceil(dy - ry).astype(np.int64), crop_bounds[1])
    y1 = np.minimum(np.floor(dy + ry).astype(np.int64) + 1, crop_bounds[3])
    return x0, y0, x1, y1


def axis_index(p, d, inv_r):
    """min((int)floor(|((float)p - d) inv_r 16|), 15), every step a float32 operation"""
    v = np.abs(((np.asarray(p).astype(F32) - np.asarray(d, F32)) * F32(inv_r)) * F32(16.0))
    return np.minimum(np.floor(v).astype(np.int64), 15)


def table_index(fx, fy, px, py, rx, ry, crop_bounds):
    """iy * 16 + ix of pixel (px, py) for the sample at (fx, fy), -1 where the pixel is outside the clipped footprint"""
    fx, fy = np.asarray(fx, F32), np.asarray(fy, F32)
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    x0, y0, x1, y1 = footprint(fx, fy, rx, ry, crop_bounds)
    inv_rx, inv_ry = F32(1.0) / F32(rx), F32(1.0) / F32(ry)
    idx = axis_index(py, fy - F32(0.5), inv_ry) * 16 + axis_index(px, fx - F32(0.5), inv_rx)
    return np.where((px >= x0) & (px < x1) & (py >= y0) & (py < y1), idx, -1)


# ---- the fixed-point add ----
def _to_i64(v):
    """(int64) of float32 values: truncation toward zero"""
    return np.trunc(np.asarray(v, F32).astype(np.float64)).astype(np.int64)


def add_samples(acc, fx, fy, L, rx, ry, crop_bounds, tab=None):
    """FilmTile::AddSample of n samples into acc (h, w, 4) int64.  tab = None: the box of 3.11 -- weight 1, the fourth accumulator counts
    samples; else the (16, 16) float32 table of a weighted filter: q_c = (int64)((w Lc) 2^24), q_w = (int64)(w 2^24)."""
    fx, fy = np.asarray(fx, F32), np.asarray(fy, F32)
    Lc = np.minimum(np.maximum(np.asarray(L, F32), F32(0.0)), FIXED_MAX)
    x0, y0, x1, y1 = footprint(fx, fy, rx, ry, crop_bounds)
    inv_rx, inv_ry = F32(1.0) / F32(rx), F32(1.0) / F32(ry)
    flat = None if tab is None else np.asarray(tab, F32).reshape(256)
    nx, ny = int(max((x1 - x0).max(initial=0), 0)), int(max((y1 - y0).max(initial=0), 0))
    for oy in range(ny):
        for ox in range(nx):
            px, py = x0 + ox, y0 + oy
            ok = (px < x1) & (py < y1)
            if not ok.any():
                continue
            if flat is None:
                q = np.concatenate([_to_i64(Lc[ok] * FIXED_ONE), np.ones((int(ok.sum()), 1), np.int64)], 1)
            else:
                w = flat[axis_index(py[ok], fy[ok] - F32(0.5), inv_ry) * 16 + axis_index(px[ok], fx[ok] - F32(0.5), inv_rx)]
                q = np.concatenate([_to_i64((w[:, None] * Lc[ok]) * FIXED_ONE), _to_i64(w * FIXED_ONE)[:, None]], 1)
            np.add.at(acc, (py[ok] - crop_bounds[1], px[ok] - crop_bounds[0]), q)
    return acc


RGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], F32)


def film_from_acc_weighted(acc):
    """{XYZ of (float)acc_c 2^-24, (float)acc_w 2^-24}: all four scaled; the XYZ rows added left to right in float32 (spectrum.rs:139-145)"""
    a = np.asarray(acc, np.int64)
    inv = F32(1.0) / FIXED_ONE
    v = a.astype(F32) * inv
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    out = np.zeros(a.shape, F32)
    for k in range(3):
        out[..., k] = (RGB_TO_XYZ[k, 0] * r + RGB_TO_XYZ[k, 1] * g) + RGB_TO_XYZ[k, 2] * b
    out[..., 3] = v[..., 3]
    return out


# ---- film points ----
def _u32(v):
    return np.asarray(v).astype(np.uint64) & np.uint64(0xFFFFFFFF)


def _mix32(v):
    """lowbias32 on uint32 values held in uint64 arrays"""
    v = _u32(v)
    v ^= v >> np.uint64(16); v = _u32(v * np.uint64(0x7FEB352D))
    v ^= v >> np.uint64(15); v = _u32(v * np.uint64(0x846CA68B))
    v ^= v >> np.uint64(16)
    return v


def _bitrev32(v):
    v = _u32(v)
    out = np.zeros_like(v)
    for b in range(32):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return out


def pixel_sequence(x, y, xres, yres, pads, seed):
    """the number of sampled pixel (x, y) in the haloed image: seed W' H' + (y + pad_y) W' + (x + pad_x), modulo 2^64"""
    wn, hn = np.uint64(xres + 2 * pads[0]), np.uint64(yres + 2 * pads[1])
    with np.errstate(over="ignore"):
        return np.uint64(seed) * wn * hn + (np.asarray(y) + pads[1]).astype(np.uint64) * wn + (np.asarray(x) + pads[0]).astype(np.uint64)


def sobol02_film_points(x, y, xres, yres, pads, seed, n_spp):
    """3.10: (fx, fy) float32 arrays (n pixels, n_spp): request 0 of sample s is point s ^ (a & mask) of the first two Sobol' dimensions, XOR-
    scrambled, a = mix32(key), key = the pixel's"""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    q = pixel_sequence(x, y, xres, yres, pads, seed)
    key = _mix32(_u32(q) ^ _mix32(_u32((q >> np.uint64(32)) + np.uint64(0x9E3779B9))))
    a = _mix32(key)  # request j = 0: key + 0 * 0x9e3779b9
    log2 = 0
    while (1 << log2) < n_spp:
        log2 += 1
    fx, fy = np.zeros((len(x), n_spp), F32), np.zeros((len(x), n_spp), F32)
    for s in range(n_spp):
        i = np.uint64(s) ^ (a & np.uint64((1 << log2) - 1))
        px = _bitrev32(i)
        py = np.zeros_like(i)
        v = 0x80000000
        for b in range(32):  # the second dimension's generator matrix: columns v, v ^ v >> 1, ...
            py ^= np.where((i >> np.uint64(b)) & np.uint64(1), np.uint64(v), np.uint64(0))
            v ^= v >> 1
        px ^= _mix32(a ^ np.uint64(0x68E31DA4))
        py ^= _mix32(a ^ np.uint64(0xB5297A4D))
        u1 = np.minimum(px.astype(F32) * F32(2.3283064365386963e-10), _EPS1)
        u2 = np.minimum(py.astype(F32) * F32(2.3283064365386963e-10), _EPS1)
        fx[:, s] = x.astype(F32) + u1
        fy[:, s] = y.astype(F32) + u2
    return fx, fy


def stratified_first_film_points(x, y, xres, yres, pads, seed, spp):
    """3.1: the film point of the FIRST sample of chunk 0 of every pixel (sample 0, stratum (0, 0)): two draws from the fresh stream
    Rng::new(pixel sequence x K + 0).  With spp = (1, 1) that is every sample of the frame."""
    nx, ny = spp
    n = nx * ny
    k = 1
    while 2 * k <= 16 and 2 * k * 32 <= n:
        k *= 2
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    with np.errstate(over="ignore"):
        rng = _Pcg(pixel_sequence(x, y, xres, yres, pads, seed) * np.uint64(k))
    everyone = np.ones(len(x), bool)
    u1, u2 = rng.get2(everyone)
    jx = np.minimum((F32(0) + u1) * (F32(1) / F32(nx)), _EPS1)
    jy = np.minimum((F32(0) + u2) * (F32(1) / F32(ny)), _EPS1)
    return (x.astype(F32) + jx)[:, None], (y.astype(F32) + jy)[:, None]


def sample_chunks(n_spp):
    """K of 3.1: the largest power of two <= 16 that leaves a chunk at least 32 samples"""
    k = 1
    while 2 * k <= 16 and 2 * k * 32 <= n_spp:
        k *= 2
    return k


def stratified_film_points_no_draws(x, y, xres, yres, pads, seed, spp):
    """3.1 in a render whose paths draw nothing (max_depth 0): (fx, fy) float32 arrays (n pixels, n_spp).  Chunk c of a pixel holds the
    samples floor(c n / K) <= s < floor((c + 1) n / K) on the stream Rng::new(pixel sequence x K + c); sample s = stratum (s mod nx, s div nx)
    jittered by the stream's next two draws."""
    nx, ny = spp
    n = nx * ny
    k = sample_chunks(n)
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    q = pixel_sequence(x, y, xres, yres, pads, seed)
    everyone = np.ones(len(x), bool)
    fx, fy = np.zeros((len(x), n), F32), np.zeros((len(x), n), F32)
    inv_nx, inv_ny = F32(1) / F32(nx), F32(1) / F32(ny)
    for c in range(k):
        with np.errstate(over="ignore"):
            rng = _Pcg(q * np.uint64(k) + np.uint64(c))
        for s in range((c * n) // k, ((c + 1) * n) // k):
            u1, u2 = rng.get2(everyone)
            jx = np.minimum((F32(s % nx) + u1) * inv_nx, _EPS1)
            jy = np.minimum((F32(s // nx) + u2) * inv_ny, _EPS1)
            fx[:, s] = x.astype(F32) + jx
            fy[:, s] = y.astype(F32) + jy
    return fx, fy


def film_points(sampler, x, y, sd, pads, seed, spp, max_depth):
    if sampler in ("sobol", 1):
        return sobol02_film_points(x, y, sd.xres, sd.yres, pads, seed, spp[0] * spp[1])
    assert sampler in ("stratified", 0)
    if max_depth == 0:  # no path draws: every sample of a chunk is restated
        return stratified_film_points_no_draws(x, y, sd.xres, sd.yres, pads, seed, spp)
    assert tuple(spp) == (1, 1), "with path draws the stratified film point is restated for a chunk's first sample alone"
    return stratified_first_film_points(x, y, sd.xres, sd.yres, pads, seed, spp)


def reference_acc(oracle_scene, sd, crop_bounds, radii, spp, seed, sampler, max_depth, tab=None, cache=None):
    """The accumulators (h, w, 4) int64 of a render of `sd` -- the scene the oracle holds, without a filter record -- under the box (tab =
    None) or a weighted filter's table, radii `radii`: every sampled pixel's restated film points with the oracle's radiances.  cache: a
    dict that keeps the (film points, radiances) of (radii's pads, spp, seed, sampler, depth) across filters of equal pads."""
    sb, pads = sample_bounds(crop_bounds, *radii)
    key = (sb, pads, tuple(spp), seed, sampler, max_depth)
    if cache is None or key not in cache:
        ys, xs = np.mgrid[sb[1]:sb[3], sb[0]:sb[2]]
        xs, ys = xs.ravel(), ys.ravel()
        fx, fy = film_points(sampler, xs, ys, sd, pads, seed, spp, max_depth)
        # (the oracle numbers its streams by the pads of the radii it is handed: any radii of the same pads give the same samples)
        L = np.stack([oracle_scene.pixel_samples(int(px), int(py), max_depth=max_depth, spp=tuple(spp), seed=seed, sampler=sampler, filter_width=radii)
                      for px, py in zip(xs, ys)])
        got = (fx.reshape(-1), fy.reshape(-1), L.reshape(-1, 3))
        if cache is not None:
            cache[key] = got
    else:
        got = cache[key]
    h, w = crop_bounds[3] - crop_bounds[1], crop_bounds[2] - crop_bounds[0]
    return add_samples(np.zeros((h, w, 4), np.int64), got[0], got[1], got[2], radii[0], radii[1], crop_bounds, tab)
