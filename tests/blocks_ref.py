"""Input sets, float64 references and error bounds of the building-block tests (tests/test_blocks_host.py on the oracle's restatements,
tests/test_blocks_gpu.py on the device through pbrt_hip_blocks_eval_device).  The walk's node step and triangle test have theirs in
tests/walk_ref.py.

The references are numpy float64 written from the mathematics -- np.sin / np.cos / np.arctan / np.arccos, pbrt-v3's FrDielectric formula,
the concentric disk map, the sphere's (phi / 2 pi, 1 - theta / pi), the quadratic's roots (util.sphere_hits_f64) -- and share no line with
the oracle or the library.  The inputs are bit patterns, not random draws.

BOUNDS.  The polynomials' bounds (POLY_BOUND) are the largest error of the oracle against float64 over the input sets below, measured on
the CPU, plus half an ulp (a strided set can miss the peak of an error curve that wiggles by the rounding of one operation); they are
DESIGN.md 3.6's table.  The composite operations' bounds are derived from those by first-order propagation, evaluated in float64 per
element; nothing is taken from the outputs under test.  check(...) functions return the figures they assert on, so that a caller can
print them."""
import numpy as np

import walk_ref as wr

U = 2.0 ** -24                      # the unit roundoff of float32
F32 = np.float32
PI4 = float(F32(0.78539816339744830961))   # the float nearest pi / 4: the polynomials' domain end as the callers reach it
TWO_PI = float(F32(6.28318530717958647692))
K_ONE_MINUS_EPS = float(F32(1.0) - F32(2.0 ** -23))
K_RAY_TMIN = float(F32(1e-4))


# ---------------------------------------------------------------------------------------------------------------------------------
# bit patterns
# ---------------------------------------------------------------------------------------------------------------------------------
def _ord(x):
    """float32 -> its place in the order of all float32 (an int64: negative floats have negative places, +-0 share place 0)"""
    b = np.atleast_1d(np.asarray(x, F32)).view(np.uint32).astype(np.int64)
    return np.where(b < 0x80000000, b, -(b & 0x7fffffff))


def _from_ord(i):
    i = np.asarray(i, np.int64)
    return np.where(i >= 0, i, 0x80000000 | (-i)).astype(np.uint32).view(F32)


def strided(lo, hi, stride=64):
    """every stride-th float32 pattern of [lo, hi], both ends included"""
    a, b = int(_ord(lo)[0]), int(_ord(hi)[0])
    return _from_ord(np.append(np.arange(a, b, stride), b))


def around(x, k=4096):
    """all float32 patterns within +-k of x (through the denormals and across 0, -0 included)"""
    c = int(_ord(x)[0])
    v = _from_ord(np.arange(c - k, c + k + 1))
    return np.concatenate([v, F32([-0.0])]) if c - k <= 0 <= c + k else v


def _domain(parts, lo, hi):
    """the parts joined and cut to [lo, hi] (a pattern that two parts hold is simply evaluated twice)"""
    v = np.concatenate([np.asarray(p, F32).reshape(-1) for p in parts])
    return v[(v >= F32(lo)) & (v <= F32(hi))]


ATAN_T1, ATAN_T2 = F32(0.4142135623730950), F32(2.414213562373095)  # poly_atan_pos's range thresholds as float32 holds them


def poly_inputs(op):
    """SIN / COS: [-pi/4, pi/4]; ATAN_POS: [0, +inf]; ACOS: [-1, 1]; SINCOS: [0, 2 pi] -- every 64th pattern, and all patterns within 4096 of
    0 (both sides), of the domain's ends, of the branch thresholds and, for SINCOS, of every multiple of pi / 4"""
    if op in ("SIN", "COS"):
        return _domain([strided(-PI4, -0.0), strided(0.0, PI4), around(0.0), around(PI4), around(-PI4)], -PI4, PI4)
    if op == "ATAN_POS":
        x = _domain([strided(0.0, np.inf), around(0.0), around(np.inf), around(ATAN_T1), around(ATAN_T2), around(1.0)], 0.0, np.inf)
        return x[~np.signbit(x) | (x == 0)]
    if op == "ACOS":
        return _domain([strided(-1.0, -0.0), strided(0.0, 1.0), around(0.0), around(1.0), around(-1.0), around(0.5), around(-0.5)], -1.0, 1.0)
    if op == "SINCOS":
        x = _domain([strided(0.0, TWO_PI)] + [around(F32(k * np.pi / 4)) for k in range(9)], 0.0, TWO_PI)
        return x[~np.signbit(x)]
    raise KeyError(op)


def ulp32(x):
    """the spacing of float32 at |x| (x float64), 2^-149 at and below the denormals"""
    return np.spacing(np.abs(np.asarray(x, np.float64).astype(F32)))  # (float32 spacing; numpy widens it where it meets float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# The polynomials.  POLY_BOUND[op] = (kind, bound): kind "ulp" -- |got - ref| <= bound x ulp32(ref) --, or "abs" where the result crosses 0
# or the claim being replaced was absolute.  POLY_MEASURED is the oracle's largest error over poly_inputs (tests/test_blocks_host.py prints
# it and checks that it has not moved), the bound is that + 0.5 ulp (DESIGN.md 3.6's table):
#   poly_sin        0.754 ulp at x = 0.78520  -> 1.26         poly_cos   0.966 ulp at x = 0.73044 -> 1.47
#   poly_atan_pos   1.991 ulp at x = 0.43632 (1.39e-7 absolute, at results in [1, pi / 2))         -> 2.50
#   poly_acos       3.005e-7 at x = -0.50571 (1.26 ulp of a result near 2.1) + 0.5 ulp(pi) = 1.19e-7 -> 4.20e-7
#   sincos_0_2pi    7.72e-8 at x = 2.35674 + 0.5 ulp of a result below 1 = 2.98e-8                    -> 1.08e-7
# ---------------------------------------------------------------------------------------------------------------------------------
POLY_BOUND = {"SIN": ("ulp", 1.26), "COS": ("ulp", 1.47), "ATAN_POS": ("ulp", 2.50), "ACOS": ("abs", 4.20e-7), "SINCOS": ("abs", 1.08e-7)}
POLY_MEASURED = {"SIN": 0.754, "COS": 0.966, "ATAN_POS": 1.991, "ACOS": 3.005e-7, "SINCOS": 7.72e-8}


def poly_ref(op, x):
    x = np.asarray(x, np.float64)
    if op == "SINCOS":
        return np.stack([np.sin(x), np.cos(x)], 1)
    return {"SIN": np.sin, "COS": np.cos, "ATAN_POS": np.arctan, "ACOS": np.arccos}[op](x)[:, None]


def poly_error(op, x, got):
    """the largest error of `got` against float64 in the unit of POLY_BOUND[op], and the input it is at"""
    ref = poly_ref(op, x)
    err = np.abs(got - ref)
    if POLY_BOUND[op][0] == "ulp":
        err /= ulp32(ref)
    k = int(np.argmax(err)) // err.shape[1]
    return float(err[k].max()), float(x[k])


def check_poly(op, x, got):
    """-> (largest error, where): asserts the bound and the exact values at the ends"""
    assert np.isfinite(got).all(), op
    worst, at = poly_error(op, x, got)
    assert worst <= POLY_BOUND[op][1], (op, worst, at)  # DESIGN.md 3.6's table
    at_x = lambda v: got[x == F32(v), 0]
    if op == "ATAN_POS":
        assert (at_x(np.inf) == F32(np.pi / 2)).all() and (at_x(0.0) == 0).all() and len(at_x(np.inf))
    if op == "ACOS":
        assert (at_x(1.0) == 0).all() and (at_x(-1.0) == F32(np.pi)).all() and len(at_x(1.0)) and len(at_x(-1.0))
    if op == "SIN":
        assert (at_x(0.0) == 0).all()
    if op == "COS":
        assert (at_x(0.0) == 1).all()
    return worst, at


def _poly_abs(op, ref):
    """POLY_BOUND[op] as an absolute error at a result `ref` (float64)"""
    kind, b = POLY_BOUND[op]
    return b * ulp32(ref) if kind == "ulp" else np.full(np.shape(ref), b)


def share_below(bound, limit=1e-5):
    return float((np.asarray(bound) < limit).mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# SPHERE_UV
# ---------------------------------------------------------------------------------------------------------------------------------
def fibonacci_normals(n):
    """n unit vectors on a Fibonacci lattice (float64)"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)


def sphere_uv_inputs():
    tiny = [1e-45, 1e-38, 1e-30, 1e-7]
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    seam = [[nx, s * t, nz] for nx, nz in ((1.0, 0.0), (0.8, 0.6), (0.6, -0.8), (1e-3, 1.0)) for t in [0.0] + tiny for s in (1.0, -1.0)]
    poles = [[sx * 0.0, sy * 0.0, z] for sx in (1, -1) for sy in (1, -1) for z in (1.0, -1.0)] + [[t, t, z] for t in tiny for z in (1.0, -1.0)]
    nx0 = [[sx * 0.0, ny, nz] for sx in (1.0, -1.0) for ny, nz in ((1.0, 0.0), (-1.0, 0.0), (0.6, 0.8), (-0.6, -0.8), (1e-30, 1.0))]
    above = float(np.nextafter(F32(1), F32(2)))  # |nz| one ulp above 1: clamped
    clamp = [[1e-4, 1e-4, above], [1e-4, -1e-4, -above], [0.0, 0.0, above], [-1e-4, 0.0, -above]]
    return np.concatenate([fibonacci_normals(1 << 16), np.array(axes + seam + poles + nx0 + clamp, np.float64)]).astype(F32)


def check_sphere_uv(n, got):
    """n (N, 3) float32 as given to the op, got (N, 2).  u's bound: atan's / 2 pi (at the polynomial's own result, the quotient's rounding
    carried through atan's slope) + 2 ulp of u's range, ulp(1) = 2^-23 -- the reflections pi - phi and 2 pi - phi, float32's pi and 2 pi
    and the product with 1 / 2 pi; v's: acos' / pi + half an ulp of pi / pi for theta - pi + float32's pi against pi (2.8e-8) + half an ulp
    of v for the quotient.  -> (largest |du| / bound, largest |dv| / bound, shares of the bounds below 1e-5)"""
    x, y, z = (n[:, k].astype(np.float64) for k in range(3))
    u, v = got[:, 0].astype(np.float64), got[:, 1].astype(np.float64)
    assert (u >= 0).all() and (u <= 1).all() and (v >= 0).all() and (v <= 1).all()
    phi = np.arctan2(y, x)
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    phi = np.where((x == 0) & (y == 0), 0.0, phi)  # on the axis every phi is the same point: 0 by convention (arctan2(0, -0) is pi)
    u_ref = phi / (2 * np.pi)
    v_ref = 1.0 - np.arccos(np.clip(z, -1.0, 1.0)) / np.pi
    with np.errstate(all="ignore"):
        q = np.abs(y) / np.abs(x)
        first = np.where((x == 0) & (y == 0), 0.0, np.arctan(q))   # the first-quadrant angle the polynomial is asked for
        slope = np.where(np.isfinite(q), q / (1.0 + q * q), 0.0)   # d atan(q) x q: the quotient's relative rounding U in phi
    b_u = (_poly_abs("ATAN_POS", first) + U * slope) / (2 * np.pi) + 2 * 2.0 ** -23
    b_v = (POLY_BOUND["ACOS"][1] + 0.5 * ulp32(np.pi)) / np.pi + 2.8e-8 + 0.5 * ulp32(v_ref)
    du = np.abs(u - u_ref)
    du = np.minimum(du, 1.0 - du)  # modulo 1: the seam
    dv = np.abs(v - v_ref)
    assert (du <= b_u).all(), (float((du / b_u).max()), n[np.argmax(du / b_u)])
    assert (dv <= b_v).all(), (float((dv / b_v).max()), n[np.argmax(dv / b_v)])
    shares = share_below(b_u), share_below(b_v)
    assert min(shares) >= 0.99, shares
    return float((du / b_u).max()), float((dv / b_v).max()), shares


# ---------------------------------------------------------------------------------------------------------------------------------
# FRESNEL
# ---------------------------------------------------------------------------------------------------------------------------------
FRESNEL_R = [1 / 1.5, 1.5, 1 / 1.33, 1.33, 1.0, 1 / 2.4, 2.4]


def fresnel_inputs():
    """(ci, r) pairs: ci on 4097 grid values of [0, 1], 0 and 1 and the 64 patterns next to each; for r > 1 the critical angle +-64 patterns"""
    base = _domain([np.linspace(0.0, 1.0, 4097), around(0.0, 64), around(1.0, 64)], 0.0, 1.0)
    base = base[~np.signbit(base)]
    out = []
    for r in FRESNEL_R:
        r32 = F32(r)
        ci = base
        if r > 1:
            crit = F32(np.sqrt(1.0 - 1.0 / float(r32) ** 2))
            ci = _domain([base, around(crit, 64)], 0.0, 1.0)
        out.append(np.stack([ci, np.full(len(ci), r32, F32)], 1))
    return np.concatenate(out).astype(F32)


def fr_dielectric_f64(ci, r):
    """pbrt-v3 FrDielectric for cos theta_i = ci >= 0 with eta_i = r, eta_t = 1 -> (F, cos theta_t, sin^2 theta_t); total reflection: (1, 0, .)"""
    eta_i, eta_t = r, 1.0
    sin_i = np.sqrt(np.maximum(0.0, 1.0 - ci * ci))
    sin_t = eta_i / eta_t * sin_i
    tir = sin_t >= 1.0
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    with np.errstate(all="ignore"):
        r_parl = (eta_t * ci - eta_i * cos_t) / (eta_t * ci + eta_i * cos_t)
        r_perp = (eta_i * ci - eta_t * cos_t) / (eta_i * ci + eta_t * cos_t)
        F = 0.5 * (r_parl * r_parl + r_perp * r_perp)
    return np.where(tir, 1.0, F), np.where(tir, 0.0, cos_t), sin_t * sin_t


def check_fresnel(x, got):
    """x (N, 2) = (ci, r), got (N, 2) = (F, ct).  First-order propagation of float32's roundings through
    s2t = (r r)(1 - ci ci), ct = sqrt(1 - s2t), e = 1 / r, rpar = (e ci - ct) / (e ci + ct), rper = (ci - e ct) / (ci + e ct),
    F = (rpar^2 + rper^2) / 2:  x = 1 - s2t is off by d = r^2 (h(ci^2) + h(1 - ci^2)) + (1 - ci^2) h(r^2) + h(s2t) + h(x), h(v) = half an ulp of
    v, one rounding; ct lies in the root's image of [x - d, x + d], cut at 0 (at the critical angle ct -> 0 and total reflection may be
    decided either way), + U ct for the root's own rounding; F by its partial derivatives in
    e ci, ct and e ct (its condition numbers) times their errors, + 3 U per amplitude and 2 U for the squares' sum.
    -> (largest |dF| / bound, largest |dct| / bound, shares of the bounds below 1e-5)"""
    ci, r = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
    F, ct = got[:, 0].astype(np.float64), got[:, 1].astype(np.float64)
    F_ref, ct_ref, s2t = fr_dielectric_f64(ci, r)
    assert (F >= 0).all() and (F <= 1).all() and (ct >= 0).all() and (ct <= 1).all()
    s2i, xr = 1.0 - ci * ci, 1.0 - s2t
    half = lambda v: 0.5 * ulp32(v)  # one rounding of a result v
    d_x = r * r * (half(ci * ci) + half(s2i)) + s2i * half(r * r) + half(s2t) + half(xr)
    # total reflection, exactly: wherever the device says so it says F = 1, ct = 0, and it says so wherever float64 does beyond rounding
    assert (F[ct == 0] == 1.0).all()
    sure_tir = s2t >= 1.0 + d_x
    assert (ct[sure_tir] == 0).all() and (F[sure_tir] == 1.0).all()
    with np.errstate(all="ignore"):
        hi, lo = np.sqrt(np.maximum(xr + d_x, 0.0)), np.sqrt(np.maximum(xr - d_x, 0.0))  # the root's image of [xr - d_x, xr + d_x]
        b_ct = np.where(sure_tir, 0.0, np.maximum(hi - ct_ref, ct_ref - lo) + U * ct_ref)
        e = 1.0 / r
        A, B = e * ci, e * ct_ref
        d_A, d_B = 2.0 * U * A, e * b_ct + 2.0 * U * B
        rpar = np.where(A + ct_ref > 0, (A - ct_ref) / (A + ct_ref), 1.0)
        rper = np.where(ci + B > 0, (ci - B) / (ci + B), 1.0)
        d_rpar = np.where(A + ct_ref > 0, (2.0 * ct_ref * d_A + 2.0 * A * b_ct) / (A + ct_ref) ** 2, 0.0) + 3.0 * U * np.abs(rpar)
        d_rper = np.where(ci + B > 0, 2.0 * ci * d_B / (ci + B) ** 2, 0.0) + 3.0 * U * np.abs(rper)
        b_F = np.where(sure_tir, 0.0, np.abs(rpar) * d_rpar + np.abs(rper) * d_rper + 2.0 * U * F_ref)
    b_F = np.minimum(b_F, 1.0)
    dF, dct = np.abs(F - F_ref), np.abs(ct - ct_ref)
    assert (dF <= b_F).all(), (float(np.max(dF - b_F)), x[np.argmax(dF - b_F)])
    assert (dct <= b_ct).all(), (float(np.max(dct - b_ct)), x[np.argmax(dct - b_ct)])
    # normal incidence: ((1 - e) / (1 + e))^2
    at1 = ci == 1.0
    e1 = 1.0 / r[at1]
    assert at1.sum() >= len(FRESNEL_R) and (np.abs(F[at1] - ((1 - e1) / (1 + e1)) ** 2) <= b_F[at1] + 1e-17).all()
    # matched indices reflect nothing -- wherever FrDielectric's own formula is not total reflection (ci^2 below float64's resolution at 1
    # makes sin theta_t = 1 there too: 0 and the denormals next to it)
    matched = (r == 1.0) & (s2t < 1.0)
    assert matched.sum() >= 4096 and (F[matched] < 1e-12).all(), float(F[matched].max())
    shares = share_below(b_F), share_below(b_ct)
    assert min(shares) >= 0.99, shares
    with np.errstate(all="ignore"):
        return float(np.nanmax(np.where(b_F > 0, dF / b_F, 0.0))), float(np.nanmax(np.where(b_ct > 0, dct / b_ct, 0.0))), shares


# ---------------------------------------------------------------------------------------------------------------------------------
# COSINE_ABOUT
# ---------------------------------------------------------------------------------------------------------------------------------
def cosine_normals():
    """64 lattice normals, the six axes, normals with |n.x| == |n.y| (the frame's branch) and with n.z == 0 (float32, unit to rounding)"""
    s = np.sqrt(0.5)
    special = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
               [s, s, 0], [s, -s, 0], [-s, s, 0], [0.5, 0.5, s], [0.5, -0.5, -s], [-0.6, 0.6, np.sqrt(0.28)], [0.0, 0.0, 1.0],
               [0.6, 0.8, 0], [-0.8, 0.6, 0], [0.28, -0.96, 0], [np.cos(0.3), np.sin(0.3), 0]]
    n = np.concatenate([fibonacci_normals(64), np.array(special, np.float64)]).astype(F32)
    assert (np.abs(n[70:77, 0]) == np.abs(n[70:77, 1])).all()
    return n


def cosine_grid():
    """the 257 x 257 grid of (u1, u2): k / 256 with 1 replaced by the samplers' largest value; holds 0.5 exactly and both wedge diagonals"""
    g = (np.arange(257) / 256.0).astype(F32)
    g[-1] = F32(K_ONE_MINUS_EPS)
    u1, u2 = np.meshgrid(g, g, indexing="ij")
    return np.stack([u1.reshape(-1), u2.reshape(-1)], 1)


def cosine_inputs():
    n, g = cosine_normals(), cosine_grid()
    x = np.empty((len(n), len(g), 5), F32)
    x[:, :, :3] = n[:, None, :]
    x[:, :, 3:] = g[None, :, :]
    return x.reshape(-1, 5)


def check_cosine_about(x, got):
    """x (N, 5) = (n, u1, u2), got (N, 4) = (wi, z).  Roundings counted, each U = 2^-24 relative:
      z^2   (2 u - 1 is exact on the grid) the disk point is m (cos, sin) with m = max(|2 u1 - 1|, |2 u2 - 1|) and cos^2 + sin^2 = 1 whatever
            the angle's own error, so dx^2 + dy^2 = m^2 (1 + 2 e), e the polynomials' relative error (POLY_BOUND in ulps x 2 U); the two
            products, the two squares and the two subtractions add 6 U:  |z^2 - (1 - m^2)| <= m^2 (2 e + 4 U) + 2 U + 2 U z^2 (the root).
            The bound is asserted ON THE SQUARE: it is the same statement wherever z > 0 (|dz| = |d z^2| / (z + z_ref)) and stays finite on
            the disk's rim, which 1.55 % of the grid lies on (u = 0 or the largest sample): a bound on z itself is 5e-4 there.
      |wi|  v2 is unit to 2 U (root, quotient), v3 = n x v2 has n's length to 2 U more, wi's three products and two sums 3 U, z's root
            above 1.5 U: | |wi| - 1 | <= | |n| - 1 | + 8.5 U
      wi.n  v2.n and v3.n vanish up to 3 U and 4 U, the rest is z |n|^2: |wi.n - z| <= z | |n|^2 - 1 | + 10 U
    -> (the three largest error / bound, the share of the z bound below 1e-5)"""
    n, u1, u2 = x[:, :3].astype(np.float64), x[:, 3].astype(np.float64), x[:, 4].astype(np.float64)
    wi, z = got[:, :3].astype(np.float64), got[:, 3].astype(np.float64)
    assert np.isfinite(got).all() and (z >= 0).all()
    m = np.maximum(np.abs(2 * u1 - 1), np.abs(2 * u2 - 1))
    zz_ref = 1.0 - m * m                       # float64's 1 - r^2 of the concentric map, r = m
    e = max(POLY_BOUND["SIN"][1], POLY_BOUND["COS"][1]) * 2 * U
    b_zz = m * m * (2 * e + 4 * U) + 2 * U + 2 * U * zz_ref
    r_zz = np.abs(z * z - zz_ref) / b_zz
    assert (r_zz <= 1).all(), (float(r_zz.max()), x[np.argmax(r_zz)])
    nlen2 = (n * n).sum(1)
    b_len = np.abs(np.sqrt(nlen2) - 1.0) + 8.5 * U
    r_len = np.abs(np.sqrt((wi * wi).sum(1)) - 1.0) / b_len
    assert (r_len <= 1).all(), (float(r_len.max()), x[np.argmax(r_len)])
    b_dot = z * np.abs(nlen2 - 1.0) + 10 * U
    r_dot = np.abs((wi * n).sum(1) - z) / b_dot
    assert (r_dot <= 1).all(), (float(r_dot.max()), x[np.argmax(r_dot)])
    centre = (u1 == 0.5) & (u2 == 0.5)
    assert centre.sum() == len(cosine_normals()) and (wi[centre] == n[centre]).all() and (z[centre] == 1.0).all()
    share = min(share_below(b_zz), share_below(b_len), share_below(b_dot))
    assert share >= 0.99, share
    return float(r_zz.max()), float(r_len.max()), float(r_dot.max()), share


# ---------------------------------------------------------------------------------------------------------------------------------
# SPHERE_HIT through the hooks: the ladder of util.py, every ray against the rung's own sphere alone
# ---------------------------------------------------------------------------------------------------------------------------------
def sphere_hit_inputs():
    """-> (x (N, 11) = {centre, radius}, o, d, tmax; [(rung, slice, spheres, o, d, tmax, kind)])"""
    import util
    rows, parts, at = [], [], 0
    for dist, radius in util.SPHERE_LADDER:
        sph = util.sphere_ladder_scene(radius).spheres[:1]
        o, d, tmax, kind = util.sphere_ladder_rays(dist, radius)
        rows.append(np.concatenate([np.broadcast_to(sph[0, :4], (len(o), 4)), o, d, tmax[:, None]], 1).astype(F32))
        parts.append(((dist, radius), slice(at, at + len(o)), sph, o, d, tmax, kind))
        at += len(o)
    return np.concatenate(rows), parts


def check_sphere_hit(parts, got):
    """got (N, 2) = (hit, t) -> the measurements of util.check_sphere_hits per rung"""
    import util
    out = {}
    for rung, sl, sph, o, d, tmax, kind in parts:
        g = got[sl]
        assert np.isin(g[:, 0], (0.0, 1.0)).all() and (g[g[:, 0] == 0, 1] == 0).all()
        out[rung] = util.check_sphere_hits(sph, o, d, tmax, kind, g[:, 1], np.where(g[:, 0] > 0, 0, 0xffffffff).astype(np.uint32), walk=False)
    return out


def fresnel_above_one_inputs():
    """a cosine a hair (and more) above 1, what a caller that does not clamp |cos| hands in, for every r"""
    ci = F32([np.nextafter(F32(1), F32(2)), 1.0000005, 1.001, 1.5, 2.0])
    return np.stack(np.meshgrid(ci, F32(FRESNEL_R), indexing="ij"), -1).reshape(-1, 2)


def check_fresnel_above_one(x, got):
    """sin^2 theta_i is clamped at 0: the refracted cosine is 1 exactly and F stays a reflectance"""
    assert (got[:, 1] == 1.0).all(), got[got[:, 1] != 1.0]
    assert (got[:, 0] >= 0).all() and (got[:, 0] <= 1).all()


# inputs beyond the domains, for the comparison of device and oracle alone (NaN and inf results included): no float64 bound is asked of them
WILD = np.array([np.nan, np.inf, -np.inf, 2.0, -2.0, 1e30, -1e-30, 1.0000001, -1.0000001], F32)


def wild_inputs(op):
    """None where the operation's own arithmetic is undefined off its domain on the host (SINCOS casts to an unsigned integer)"""
    if op in ("SIN", "COS", "ATAN_POS", "ACOS"):
        return WILD[:, None]
    if op == "SPHERE_UV":
        return np.stack(np.meshgrid(WILD[:5], WILD[:5], WILD[[0, 1, 3, 8]], indexing="ij"), -1).reshape(-1, 3)
    if op == "FRESNEL":
        return np.stack(np.meshgrid(WILD, np.concatenate([WILD, F32([0.0])]), indexing="ij"), -1).reshape(-1, 2)
    return None


ALL_OPS = ("SIN", "COS", "ATAN_POS", "ACOS", "SINCOS", "SPHERE_UV", "FRESNEL", "COSINE_ABOUT", "SPHERE_HIT", "QUAD_STEP", "QUAD_STEP_PK", "TRI_HIT")


# ---------------------------------------------------------------------------------------------------------------------------------
# QUAD_STEP, QUAD_STEP_PK and TRI_HIT: the walk's node step and triangle test (tests/walk_ref.py).  TRI_HIT's set here is the flat triangles
# and the exact-arithmetic rays; its ladder of rungs has tests of its own (2^14 rays a rung: a size at a time)
# ---------------------------------------------------------------------------------------------------------------------------------
def tri_hit_inputs():
    flat, _ = wr.tri_flat_inputs()
    exact = wr.tri_exact_inputs()
    return np.concatenate([flat, exact]), len(flat)


def check_tri_hit_sets(x, n_flat, got):
    return {"flat": wr.check_tri_rays(x[:n_flat], got[:n_flat], flat=True), "exact": wr.check_tri_exact(x[n_flat:], got[n_flat:])}


def inputs(op):
    """-> (x, aux): the op's input set, and what its check needs beside it"""
    if op in POLY_BOUND:
        return poly_inputs(op)[:, None], None
    if op == "SPHERE_HIT":
        return sphere_hit_inputs()
    if op in ("QUAD_STEP", "QUAD_STEP_PK"):
        return wr.quad_step_inputs()
    if op == "TRI_HIT":
        return tri_hit_inputs()
    return {"SPHERE_UV": sphere_uv_inputs, "FRESNEL": fresnel_inputs, "COSINE_ABOUT": cosine_inputs}[op](), None


def check(op, x, aux, got):
    """the op's float64 checks on `got`; -> the figures they assert on"""
    if op in POLY_BOUND:
        return check_poly(op, x[:, 0], got)
    if op == "SPHERE_HIT":
        return check_sphere_hit(aux, got)
    if op in ("QUAD_STEP", "QUAD_STEP_PK"):
        return wr.check_quad_step(x, aux, got)
    if op == "TRI_HIT":
        return check_tri_hit_sets(x, aux, got)
    return {"SPHERE_UV": check_sphere_uv, "FRESNEL": check_fresnel, "COSINE_ABOUT": check_cosine_about}[op](x, got)
