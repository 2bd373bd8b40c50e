"""Input sets, float64 references and error bounds of the building-block tests (tests/test_blocks_host.py on the oracle's restatements,
tests/test_blocks_gpu.py on the device through pbrt_hip_blocks_eval_device).  The walk's node step and triangle test have theirs in
tests/walk_ref.py; the power heuristic's weights and the one-light direct estimate (sample_light) are below the composite operations.

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


# ---------------------------------------------------------------------------------------------------------------------------------
# MIS_W_LIGHT, MIS_W_BSDF: the power heuristic's two weights (kernel_math.hpp mis_weight_light / mis_weight_bsdf)
#
# BOUND.  w = fl(A / fl(A + B)) with A = fl(a a), B = fl(b b): four roundings.  A = a^2 (1 + d1), B = b^2 (1 + d2), the sum (1 + d3), the quotient
# (1 + d4), every |d| <= U:  w / w_true = (1 + d1)(1 + d4) / ((1 + d')(1 + d3)) with d' a weighted mean of d1 and d2, so
# |w / w_true - 1| <= (1 + U)^2 / (1 - U)^2 - 1 = 4 U / (1 - U)^2 <= 4 U (1 + 3 U).  That holds while no square overflows or underflows; a
# QUOTIENT that is itself a denormal is rounded to half a denormal step, 2^-150, which is added.
# ---------------------------------------------------------------------------------------------------------------------------------
MIS_W_BOUND = 4 * U * (1 + 3 * U)
DENORMAL_STEP = 2.0 ** -149
K_INV_PI = F32(0.31830988618379067154)
# cosine_about's z is sqrt(zz), zz = (1 - dx dx) - dy dy: where dx dx >= 1/2 the first difference is exact and a multiple of 2^-24, the float
# taken off it is either below half of it (zz >= 2^-25) or within a factor 2 (exact, a multiple of its own spacing >= 2^-48): a positive zz
# is >= 2^-48, z >= 2^-24, and the smallest density a bounce ray carries is pb = 2^-24 / pi = 1.9e-8.  2^-60 lies far below every render input.
MIS_PB = F32([2.0 ** -60, 2.0 ** -40, 2.0 ** -24 / np.pi, 1e-6, 2.0 ** -12 / np.pi, 1e-3, 0.01, 0.1, 0.25, K_INV_PI])
MIS_CORNER = F32([2.0 ** -76, 2.0 ** -100, 2.0 ** -149])  # squares that round to zero: the 0 / 0 corner


def mis_weight_inputs():
    """(pl, pb): pl = m 2^k for k = -70 ... +70 and four mantissas an octave (1, 1.25, 1.5, the last float below 2) against every pb of MIS_PB;
    then the 0 / 0 corner, both densities so small that both squares are zero -- NO RENDER INPUT REACHES IT: pb >= 2^-24 / pi (above)"""
    mant = np.array([1.0, 1.25, 1.5, 2.0 - 2.0 ** -23])
    pl = (mant[None, :] * (2.0 ** np.arange(-70, 71))[:, None]).reshape(-1).astype(F32)
    grid = np.stack(np.meshgrid(pl, MIS_PB, indexing="ij"), -1).reshape(-1, 2)
    corner = np.stack(np.meshgrid(MIS_CORNER, MIS_CORNER, indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([grid, corner]).astype(F32)


def _square_class(v):
    """of fl(v v) for float32 v (as float64, where v v is exact): (overflows to inf, is below the normal range, rounds to zero)"""
    sq = v * v
    return sq >= (2.0 - 2.0 ** -24) * 2.0 ** 127, sq < 2.0 ** -126, sq <= 2.0 ** -150


def check_mis_weight(op, x, got):
    """x (N, 2) = (pl, pb) finite and positive, got (N, 1).  -> figures: the largest error / bound where no square leaves the normal range, and
    how many elements each region holds"""
    pl, pb = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
    w = got[:, 0].astype(np.float64)
    assert np.isfinite(x).all() and (x > 0).all()
    nan = np.isnan(w)
    assert not nan.any(), (op, "NaN for finite positive densities", int(nan.sum()), x[nan][:4])
    assert (w >= 0).all() and (w <= 1).all(), op
    with np.errstate(all="ignore"):
        ref = 1.0 / (1.0 + (pb / pl) ** 2) if op == "MIS_W_LIGHT" else 1.0 / (1.0 + (pl / pb) ** 2)
    l_inf, l_sub, l_zero = _square_class(pl)
    b_inf, b_sub, b_zero = _square_class(pb)
    assert not b_inf.any()
    normal = ~(l_inf | l_sub | b_sub)
    ratio = np.abs(w - ref)[normal] / (MIS_W_BOUND * ref[normal] + 0.5 * DENORMAL_STEP)
    assert (ratio <= 1).all(), (op, float(ratio.max()), x[normal][np.argmax(ratio)])
    if op == "MIS_W_LIGHT":  # pl^2 overflows: the true weight is 1 - (pb / pl)^2, within 2^-128 of 1
        assert (np.abs(w[l_inf] - 1.0) <= MIS_W_BOUND).all(), (op, x[l_inf][:4], w[l_inf][:4])
    else:                    # ... and the bounce ray's is (pb / pl)^2 < 2^-128: zero, or a denormal step
        assert (w[l_inf] <= ref[l_inf] + DENORMAL_STEP).all(), (op, x[l_inf][:4], w[l_inf][:4])
    corner = l_zero & b_zero  # 0 / 0 as the expression stands (no render input: mis_weight_inputs): finite and a weight (asserted above on all)
    assert normal.sum() >= 2000 and l_inf.sum() >= 200 and corner.sum() == len(MIS_CORNER) ** 2
    return {"largest error / bound": float(ratio.max()), "normal": int(normal.sum()), "pl^2 overflows": int(l_inf.sum()),
            "a square underflows": int((l_sub | b_sub).sum()), "0 / 0 corner": int(corner.sum())}


# ---------------------------------------------------------------------------------------------------------------------------------
# LIGHT: one call of sample_light.  An element is the light's five records as the scene's table holds them, the
# shaded point po, its normal nf, Kd, (u1, u2), nL and the mis flag (include/pbrt_hip_debug.h).  The reference is the estimator of 3.8 / 3.14
# in float64 from the text; the RECORD -- area and unit normal of a triangle as the scene builder computed them in float32 -- is an input
# like the vertices: the reference takes it as it stands.
#
# ROUNDINGS, each U relative, in sample_light's statement order (the derivation of the constants of LIGHT_ROUNDINGS):
#   f = Kd (1 / pi)                 float32's 1 / pi against pi: U; the product: U                                            -> f_kd = 2
#   Ld = (f lc) scale               two products                                                                              -> 2 more
# point    dv = p0 - po             U of the RESULT (the operands are exact)
#          d2 = dv . dv             (1 + U)^2 from dv, the square U, two sums of positive terms 2 U                           -> d2 = 5
#          dist = sqrt(d2)          5 / 2 + U                                                                                 -> dist = 3.5
#          wi = dv / dist           U + 3.5 U + U, per component                                                              -> wi = 5.5
#          cs = wi . nf             (5.5 + 1) U per product, 2 U for the sums, of S = sum |wi_c nf_c|: |d cs| <= 8.5 U S       -> cs = 8.5
#          scale = (cs / d2) nL     d cs / cs + 5 U + 2 U;  Ld: 2 + 2 + 7 = 11 U + 8.5 U S / cs;  tmax = dist 0.9999f: 3.5 + 1
# distant  cs = wi . nf             wi is the record's: U per product + 2 U: 3 U S;  scale = cs nL: U;  Ld: 2 + 2 + 1 = 5 U + 3 U S / cs
# sky      Ld = (Kd lc) nL          2 U; with mis times 1 / (1 + nL nL): three roundings and the product                       -> 2 and 6
# triangle su0 = sqrt(u1) U; b0 = 1 - su0: |d b0| <= U (su0 + b0) = U; b1 = u2 su0: 2 U b1; b2 = (1 - b0) - b1: 2 U, then 5 U;
#          pl_c = (p0 b0 + p1 b1) + p2 b2: the products carry (1 + 1) U, (2 + 1) U, (5 + 1) U of M_c = max |vertex coordinate c|, the two
#          sums 2 U M_c:  |d pl_c| <= 13 U M_c =: E_c  (u1 = 0: b = (1, 0, 0) and every operation is exact, E = 0)             -> point = 13
#          dv = pl - po             |d dv_c| <= E_c + U |dv_c|
#          d2                       relative r2 = 5 U + 2 sum_c |dv_c| E_c / d2        -- the condition max |p| / dist
#          dist                     rd = r2 / (1 + sqrt(1 - r2)) + U
#          wi_c                     |d wi_c| <= (E_c + U |dv_c|) / dist + |wi_c| (rd / (1 - rd) + U)
#          cs, cl                   sum_c |nf_c| |d wi_c| + 3 U S                       -- the conditions 1 / cs, 1 / cl
#          scale = (((cs cl) A) / d2) nL       cs, cl, 1 / d2 and four roundings
#          pl = (d2 / (cl A)) / nL, pb = cs (1 / pi), w = mis_weight_light(pl, pb): the ratio pb / pl carries both, the weight moves by
#          (1 - w) of the square's error (w' / w = 1 / (1 + (1 - w) e)) + MIS_W_BOUND of its own; scale w: one more
# Relative errors are combined as products (1 + r1)(1 + r2) ... - 1, an error r of a DENOMINATOR as r / (1 - r): nothing is first-order only.
# Every bound is then widened by LIGHT_SLACK for the second-order terms of the roundings counted singly ((1 + U)^40 - 1 < 40 U (1 + 2^-18)),
# and Ld gets 8 denormal steps for products that are rounded as denormals.
# LIGHT_MEASURED: the largest error / bound of the oracle's values over light_inputs() on the CPU, as information: the tolerance is the bound.
# ---------------------------------------------------------------------------------------------------------------------------------
LIGHT_ROUNDINGS = {"f_kd": 2.0, "ld_products": 2.0, "d2": 5.0, "dist": 3.5, "wi": 5.5, "cs_point": 8.5, "cs_record": 3.0, "point": 13.0}
LIGHT_SLACK = 1.0 + 2.0 ** -12
LIGHT_MEASURED = {"Ld": 0.667, "wi": 0.277, "tmax": 0.499}
LIGHT_RUNG_COS = (1.0, 2.0 ** -5, 2.0 ** -12, 2.0 ** -20)
LIGHT_KINDS = ("point", "distant", "sky", "triangle")
K_SHADOW_SHRINK = float(F32(0.9999))


def _type_word(t):
    return np.array([t], np.uint32).view(F32)[0]


def _rows(rec, po, nf, kd, u1, u2, nl):
    """one element per row of the broadcast arguments, mis = 0"""
    n = max(len(np.atleast_2d(a)) for a in (rec, po, nf, kd))
    n = max(n, *(np.size(a) for a in (u1, u2, nl)))
    x = np.zeros((n, 33), F32)
    x[:, :20], x[:, 20:23], x[:, 23:26], x[:, 26:29] = rec, po, nf, kd
    x[:, 29], x[:, 30], x[:, 31] = u1, u2, nl
    return x


def _rung_normal(cs, sign=1.0):
    """a float32 normal whose cosine with +z is cs EXACTLY (its length is 1 to rounding; the estimator takes it as it is)"""
    return F32([np.sqrt(1.0 - cs * cs), 0.0, cs]) * F32(sign)


def _simple_record(t, p, c):
    rec = np.zeros(20, F32)
    rec[0], rec[1:4], rec[12:15] = _type_word(t), p, c
    return rec


def _triangle_record(p0, p1, p2, le):
    """the five records of an emissive triangle as the scene builder lays them out: area = |cross| / 2 and the unit normal in float32"""
    p0, p1, p2 = (np.asarray(p, F32) for p in (p0, p1, p2))
    a, b = p1 - p0, p2 - p0
    cr = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F32)
    ln = np.sqrt((cr[..., 0] * cr[..., 0] + cr[..., 1] * cr[..., 1]) + cr[..., 2] * cr[..., 2]).astype(F32)
    rec = np.zeros(p0.shape[:-1] + (20,), F32)
    rec[..., 0] = _type_word(3)
    rec[..., 1:4], rec[..., 4:7], rec[..., 7], rec[..., 8:11], rec[..., 12:15] = p0, p1, F32(0.5) * ln, p2, le
    rec[..., 16:19] = cr / ln[..., None]
    return rec


def light_inputs():
    """-> (x (2 N, 33), aux): N elements with mis = 0, then the same N with mis = 1.  aux: "kind" (index into LIGHT_KINDS) and "edge" (the rungs
    BUILT to sit on a decision's edge: excluded from the 2 % rule of check_light) per element.
    The ladders (cosines exact by construction: the direction to the light is +z, the normals are _rung_normal):
      point     distance D = 2^-10, 1, 2^10 -- the shaded point at the origin and 8 D away from it --, nL = 1, 3, 1000, cs = 1, 2^-5, 2^-12, 2^-20
                towards and away from the light; 8 x 8 lattice directions x normals per D; the shaded point ON the light
      distant   the same cosines, and a 16 x 16 lattice
      sky       the 81 normals of cosine_normals() x a 9 x 9 grid of (u1, u2) with 0, 1/2 and the samplers' largest value x nL (edge: the
                disk's rim, u1 or u2 at an end of its range)
      triangle  D as above x area 2^-40, 2^-20, 1, 2^20 x nL x cs x cl x (u1, u2) in {0, 2^-40, 2^-24, 1/4, 1/2, 1 - 2^-23} x {0, 0.3, 1/2, 1 - 2^-23}
                -- sqrt(u1) = 0 puts the sample on p0 --, the LIGHT at the origin (tiny vertices, max |p| / dist <= 1) and, where float32 still
                resolves the triangle there, the SHADED POINT at the origin (max |p| / dist = 1); seen from behind (p1, p2 swapped), from
                below the surface (nf negated), the shaded point ON p0 with u1 = 0 (edge: a cosine of 2^-20, of the order of the
                interpolated point's rounding seen from the shaded point, and a triangle 2^10 times as long as it is far away or longer,
                where that rounding, 13 U max |p| / dist, is of the order of the cosine 2^-12 and beyond)"""
    kd, kd0 = F32([0.7, 0.5, 0.3]), F32([0.0, 0.5, 1.0])
    lattice = fibonacci_normals(16).astype(F32)
    parts = []  # (kind, rows, edge)

    def add(kind, rows, edge=False):
        parts.append((kind, rows, np.full(len(rows), edge) if np.isscalar(edge) else edge))

    for D in (2.0 ** -10, 1.0, 2.0 ** 10):
        for off in (F32([0, 0, 0]), F32([8, -4, 2]) * F32(D)):
            p0 = off + F32([0, 0, D])
            for nl in (1.0, 3.0, 1000.0):
                for cs in LIGHT_RUNG_COS:
                    for sign in (1.0, -1.0):
                        add(0, _rows(_simple_record(0, p0, [6, 5, 4]), off, _rung_normal(cs, sign), kd, 0.5, 0.5, nl))
            pts = (off[None, :] + F32(D) * lattice[:8]).astype(F32)
            for n in lattice[8:]:
                rec = np.zeros((8, 20), F32)
                rec[:, 0], rec[:, 1:4], rec[:, 12:15] = _type_word(0), pts, [6, 5, 4]
                add(0, _rows(rec, off, n, kd0, 0.1, 0.9, 3.0))
            add(0, _rows(_simple_record(0, off, [6, 5, 4]), off, _rung_normal(1.0), kd, 0.5, 0.5, 3.0))  # the shaded point on the light
    for nl in (1.0, 3.0, 1000.0):
        for cs in LIGHT_RUNG_COS:
            for sign in (1.0, -1.0):
                add(1, _rows(_simple_record(1, [0, 0, 1], [1, 1.2, 1.5]), [0.3, -2, 5], _rung_normal(cs, sign), kd, 0.5, 0.5, nl))
    for w in lattice:
        rec = np.broadcast_to(_simple_record(1, w, [1, 1.2, 1.5]), (16, 20))
        add(1, _rows(rec, [0.3, -2, 5], lattice, kd0, 0.2, 0.7, 3.0))
    g = F32([0.0, 2.0 ** -6, 0.25, 0.4999, 0.5, 0.5001, 0.75, 0.96875, K_ONE_MINUS_EPS])
    u1, u2 = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    rim = np.isin(u1, g[[0, -1]]) | np.isin(u2, g[[0, -1]])
    for n in cosine_normals():
        for nl in (1.0, 3.0, 1000.0):
            add(2, _rows(_simple_record(2, [0, 0, 0], [0.2, 0.25, 0.3]), [1, 2, 3], n, kd, u1, u2, nl), rim)
    tu1, tu2 = (a.reshape(-1) for a in np.meshgrid(F32([0.0, 2.0 ** -40, 2.0 ** -24, 0.25, 0.5, K_ONE_MINUS_EPS]), F32([0.0, 0.3, 0.5, K_ONE_MINUS_EPS]), indexing="ij"))
    for D in (2.0 ** -10, 1.0, 2.0 ** 10):
        for e in (-40, -20, 0, 20):
            s1, s2 = 2.0 ** -((-(e + 1)) // 2), 2.0 ** ((e + 1) // 2)  # s1 s2 = 2 area, both powers of two
            for light_at_origin in (True, False):
                if not light_at_origin and s2 < D * 2.0 ** -10:
                    continue  # (float32 no longer resolves the triangle D away from the origin)
                p0 = F32([0, 0, 0]) if light_at_origin else F32([0, 0, D])
                po = F32([0, 0, -D]) if light_at_origin else F32([0, 0, 0])
                for cl in LIGHT_RUNG_COS:
                    p1 = p0 + F32([0, s1, 0])
                    p2 = p0 + F32(s2) * F32([cl, 0, np.sqrt(1.0 - cl * cl)])
                    rec, back = _triangle_record(p0, p1, p2, [20, 15, 10]), _triangle_record(p0, p2, p1, [20, 15, 10])
                    for cs in LIGHT_RUNG_COS:
                        edge = cs == 2.0 ** -20 or cl == 2.0 ** -20 or s1 >= 2.0 ** 10 * D
                        for nl in (1.0, 3.0, 1000.0):
                            add(3, _rows(rec, po, _rung_normal(cs), kd, tu1, tu2, nl), edge)
                        add(3, _rows(back, po, _rung_normal(cs), kd, tu1, tu2, 3.0), edge)           # seen from behind
                        add(3, _rows(rec, po, _rung_normal(cs, -1.0), kd0, tu1, tu2, 3.0), edge)     # the light below the surface
                    add(3, _rows(rec, p0, _rung_normal(1.0), kd, 0.0, tu2[:4], 3.0))                 # the shaded point on p0, the sample on p0
    x = np.concatenate([rows for _, rows, _ in parts])
    aux = {"kind": np.concatenate([np.full(len(rows), k) for k, rows, _ in parts]), "edge": np.concatenate([e for _, _, e in parts])}
    x1 = x.copy()
    x1[:, 32] = 1.0
    return np.concatenate([x, x1]), {k: np.concatenate([v, v]) for k, v in aux.items()}


def light_wild_inputs():
    """elements off the domain, for device against oracle alone: NaN, inf and zeros in the positions, u1 outside [0, 1), a zero area, nL = 0,
    a type word nobody defines (both sides take the triangle branch).  No sky: cosine_about has no wild set (wild_inputs)"""
    tri = _triangle_record([0, 0, 1], [0, 1, 1], [1, 0, 1.5], [20, 15, 10])
    rows = []
    for t in (0, 1, 3, 4, 7, 0x7fc00000):
        rec = tri.copy()
        rec[0] = _type_word(t)
        for v in (np.nan, np.inf, -np.inf, 0.0, 1e30, -2.0):
            for slot in (1, 7, 16, 20, 23, 29, 30, 31):
                r = _rows(rec, [0.1, 0.2, -1], [0, 0.6, 0.8], [0.7, 0.5, 0.3], 0.25, 0.5, 3.0)
                r[0, slot] = v
                rows.append(r)
    x = np.concatenate(rows)
    x1 = x.copy()
    x1[:, 32] = 1.0
    return np.concatenate([x, x1])


def _comb(*r):
    """relative errors combined as a product: (1 + r1)(1 + r2) ... - 1"""
    out = 1.0
    for v in r:
        out = out * (1.0 + v)
    return out - 1.0


def _denom(r):
    """what a relative error r of a denominator does to the quotient: r / (1 - r); inf from r = 1"""
    with np.errstate(all="ignore"):
        return np.where(r < 1.0, r / (1.0 - np.minimum(r, 0.999999)), np.inf)


def light_reference(x):
    """The float64 estimator and its error model per element -> dict of arrays: accept / reject (the decision where it is CERTAIN: every
    quantity it rests on further from zero than the float32 rounding of its own computation), Ld (N, 3), rel_ld (N), wi (N, 3), abs_wi (N, 3),
    tmax, rel_tmax, pl (the light-sampling density of a triangle's sample, NaN elsewhere), rel_pl"""
    R = LIGHT_ROUNDINGS
    x64 = x.astype(np.float64)
    t = np.ascontiguousarray(x[:, 0]).view(np.uint32)
    p0, p1, area, p2, lc, nrm = x64[:, 1:4], x64[:, 4:7], x64[:, 7], x64[:, 8:11], x64[:, 12:15], x64[:, 16:19]
    po, nf, kd, u1, u2, nl, mis = x64[:, 20:23], x64[:, 23:26], x64[:, 26:29], x64[:, 29], x64[:, 30], x64[:, 31], x64[:, 32] != 0
    N = len(x)
    out = {"accept": np.zeros(N, bool), "reject": np.zeros(N, bool), "Ld": np.zeros((N, 3)), "rel_ld": np.zeros(N), "wi": np.zeros((N, 3)),
           "abs_wi": np.zeros((N, 3)), "tmax": np.zeros(N), "rel_tmax": np.zeros(N), "pl": np.full(N, np.nan), "rel_pl": np.zeros(N)}
    f = kd / np.pi
    with np.errstate(all="ignore"):
        # ---- point ----
        dv = p0 - po
        d2 = (dv * dv).sum(1)
        dist = np.sqrt(d2)
        wi = dv / dist[:, None]
        cs = (wi * nf).sum(1)
        e_cs = R["cs_point"] * U * np.abs(wi * nf).sum(1) * LIGHT_SLACK
        k = t == 0
        acc, rej = (d2 > 0) & (cs > e_cs), (d2 == 0) | (cs < -e_cs)   # (dv is the rounding of an exact difference: zero only where it is zero)
        ld = f * lc * (cs / d2 * nl)[:, None]
        rel = _comb((R["f_kd"] + R["ld_products"] + R["d2"] + 2.0) * U, e_cs / cs)
        for name, val in (("accept", acc), ("reject", rej), ("Ld", ld), ("rel_ld", rel), ("wi", wi), ("abs_wi", R["wi"] * U * np.abs(wi)),
                          ("tmax", dist * K_SHADOW_SHRINK), ("rel_tmax", np.full(N, (R["dist"] + 1.0) * U))):
            out[name][k] = val[k]
        # ---- distant ----
        k = t == 1
        cs = (p0 * nf).sum(1)
        e_cs = R["cs_record"] * U * np.abs(p0 * nf).sum(1) * LIGHT_SLACK
        ld = f * lc * (cs * nl)[:, None]
        rel = _comb((R["f_kd"] + R["ld_products"] + 1.0) * U, e_cs / cs)
        for name, val in (("accept", cs > e_cs), ("reject", cs < -e_cs), ("Ld", ld), ("rel_ld", rel), ("wi", p0), ("tmax", np.full(N, np.inf))):
            out[name][k] = val[k]
        # ---- constant sky: cosine-sampled; accepted where the disk point lies inside the rim (check_cosine_about's bound on z^2) ----
        k = t == 2
        m = np.maximum(np.abs(2 * u1 - 1), np.abs(2 * u2 - 1))
        zz = 1.0 - m * m
        e = max(POLY_BOUND["SIN"][1], POLY_BOUND["COS"][1]) * 2 * U
        b_zz = m * m * (2 * e + 4 * U) + 2 * U + 2 * U * zz
        ld = kd * lc * np.where(mis, nl / (1.0 + nl * nl), nl)[:, None]
        for name, val in (("accept", zz > b_zz), ("reject", zz < -b_zz), ("Ld", ld), ("rel_ld", np.where(mis, 6.0, 2.0) * U), ("tmax", np.full(N, np.inf))):
            out[name][k] = val[k]
        out["zz"], out["b_zz"] = zz, b_zz
        # ---- emissive triangle: pbrt-v3 UniformSampleTriangle, one-sided ----
        k = t == 3
        su = np.sqrt(u1)
        pt = p0 * (1.0 - su)[:, None] + p1 * (u2 * su)[:, None] + p2 * (su * (1.0 - u2))[:, None]
        E = R["point"] * U * np.maximum(np.maximum(np.abs(p0), np.abs(p1)), np.abs(p2)) * (u1 != 0)[:, None]
        dv = pt - po
        d2 = (dv * dv).sum(1)
        dist = np.sqrt(d2)
        wi = dv / dist[:, None]
        r2 = R["d2"] * U + 2.0 * (np.abs(dv) * E).sum(1) / d2
        r2 = np.where(d2 > 0, r2, np.inf)
        rd = np.where(r2 < 1, r2 / (1.0 + np.sqrt(1.0 - np.minimum(r2, 1.0))), np.inf) + U
        e_wi = ((E + U * np.abs(dv)) / dist[:, None] + np.abs(wi) * (_denom(rd) + U)[:, None]) * LIGHT_SLACK
        cs, cl = (wi * nf).sum(1), -(wi * nrm).sum(1)
        e_cs = (np.abs(nf) * e_wi).sum(1) + 3.0 * U * np.abs(wi * nf).sum(1) * LIGHT_SLACK
        e_cl = (np.abs(nrm) * e_wi).sum(1) + 3.0 * U * np.abs(wi * nrm).sum(1) * LIGHT_SLACK
        e_cs, e_cl = (np.where(np.isfinite(v), v, np.inf) for v in (e_cs, e_cl))
        acc = (r2 < 1) & (d2 > 2.0 ** -100) & (cs > e_cs) & (cl > e_cl)
        rej = ((d2 == 0) & (E == 0).all(1)) | (cs < -e_cs) | (cl < -e_cl)
        rel_cs, rel_cl = e_cs / cs, e_cl / cl
        rel_scale = _comb(rel_cs, rel_cl, _denom(r2), 4.0 * U)
        pl = (d2 / (cl * area)) / nl
        pb = cs / np.pi
        rel_pl = _comb(r2, _denom(_comb(rel_cl, U)), 2.0 * U)
        rel_ratio = _comb(_comb(rel_cs, 2.0 * U), _denom(rel_pl))   # of pb / pl
        w = 1.0 / (1.0 + (pb / pl) ** 2)
        rel_w = _comb(_denom((1.0 - w) * _comb(rel_ratio, rel_ratio)), MIS_W_BOUND)
        ld = f * lc * ((((cs * cl) * area) / d2) * nl * np.where(mis, w, 1.0))[:, None]
        rel = _comb((R["f_kd"] + R["ld_products"]) * U, rel_scale, np.where(mis, _comb(rel_w, U), 0.0))
        for name, val in (("accept", acc), ("reject", rej), ("Ld", ld), ("rel_ld", rel), ("wi", wi), ("abs_wi", e_wi), ("tmax", dist * K_SHADOW_SHRINK),
                          ("rel_tmax", _comb(rd, U)), ("pl", pl), ("rel_pl", rel_pl)):
            out[name][k] = val[k]
    assert np.isin(t, (0, 1, 2, 3)).all()
    return out


def light_margin_shares(aux, ref):
    """per kind: the share of the elements outside the edge rungs whose decision float64 alone does not settle (of the reference and the
    inputs only: nothing of the outputs under test)"""
    open_ = ~(ref["accept"] | ref["reject"])
    return {name: float(open_[(aux["kind"] == k) & ~aux["edge"]].mean()) for k, name in enumerate(LIGHT_KINDS)}


def check_light(x, aux, got):
    """got (2 N, 8) = accepted, Ld, wi, tmax.  -> figures: per kind the elements, the accepted ones, the share in the margin outside the edge
    rungs; the largest error / bound of Ld, wi and tmax; the elements with pl >= 2^64 on which mis = 1 must give what mis = 0 gives"""
    n = len(x) // 2
    assert np.array_equal(x[:n, :32], x[n:, :32]) and (x[:n, 32] == 0).all() and (x[n:, 32] == 1).all() and np.isfinite(x).all()
    ref = light_reference(x)
    ok = got[:, 0] == 1.0
    g = got.astype(np.float64)
    assert np.isin(got[:, 0], (0.0, 1.0)).all() and (got[~ok] == 0).all()
    nan = np.isnan(got[:, 1:4]).any(1)
    assert not nan.any(), ("Ld is NaN for finite inputs", int(nan.sum()), x[nan][0])
    # the decision, wherever float64 settles it
    assert ok[ref["accept"]].all(), ("ruled out where float64 accepts", int((~ok & ref["accept"]).sum()), x[~ok & ref["accept"]][0])
    assert not ok[ref["reject"]].any(), ("accepted where float64 rules out", int((ok & ref["reject"]).sum()), x[ok & ref["reject"]][0])
    shares = light_margin_shares(aux, ref)
    assert max(shares.values()) <= 0.02, shares
    a = ok & ref["accept"]
    figures = {}
    for k, name in enumerate(LIGHT_KINDS):
        sel = aux["kind"] == k
        assert a[sel].sum() >= 200, name
        figures[name] = (int(sel.sum()), int(a[sel].sum()), shares[name])
    with np.errstate(all="ignore"):  # (the elements that are not asserted hold NaN and inf)
        b_ld = (ref["rel_ld"] * LIGHT_SLACK)[:, None] * np.abs(ref["Ld"]) + 8 * DENORMAL_STEP
        r_ld = (np.abs(g[:, 1:4] - ref["Ld"]) / b_ld)[a]
        r_t = (np.abs(g[:, 7] - ref["tmax"]) / (ref["rel_tmax"] * LIGHT_SLACK * ref["tmax"]))[a & np.isfinite(ref["tmax"])]
    assert (r_ld <= 1).all(), ("Ld", float(r_ld.max()), x[a][np.argmax(r_ld.max(1))], got[a][np.argmax(r_ld.max(1))])
    sky = aux["kind"] == 2
    b_wi = ref["abs_wi"] + DENORMAL_STEP
    r_wi = (np.abs(g[:, 4:7] - ref["wi"]) / b_wi)[a & ~sky]
    assert (r_wi <= 1).all(), ("wi", float(r_wi.max()), x[a & ~sky][np.argmax(r_wi.max(1))])
    # the sky's direction: unit to check_cosine_about's bound, and its cosine with the normal sqrt(1 - m^2) (that bound on wi . n - z and on z^2)
    s = a & sky
    nf, wi = x[s, 23:26].astype(np.float64), g[s, 4:7]
    nlen2, z_ref = (nf * nf).sum(1), np.sqrt(ref["zz"][s])
    r_len = np.abs(np.sqrt((wi * wi).sum(1)) - 1.0) / (np.abs(np.sqrt(nlen2) - 1.0) + 8.5 * U)
    r_dot = np.abs((wi * nf).sum(1) - z_ref * nlen2) / (10 * U + ref["b_zz"][s] / z_ref * nlen2 + 2 * U * z_ref)
    assert (r_len <= 1).all() and (r_dot <= 1).all(), ("sky wi", float(r_len.max()), float(r_dot.max()))
    fin = np.isfinite(ref["tmax"])
    assert (got[a & ~fin, 7] == np.inf).all()
    assert (r_t <= 1).all(), ("tmax", float(r_t.max()))
    # from pl = 2^64 upwards the weight is 1 to MIS_W_BOUND -- mis = 1 gives what mis = 0 gives
    big = ref["pl"][n:] * (1.0 - np.minimum(ref["rel_pl"][n:], 1.0)) >= 2.0 ** 64
    big &= a[:n] & a[n:]
    assert big.sum() >= 500, int(big.sum())
    d = np.abs(g[n:, 1:4] - g[:n, 1:4])[big] / (MIS_W_BOUND * np.abs(g[:n, 1:4])[big] + DENORMAL_STEP)
    assert (d <= 1).all(), ("mis = 1 against mis = 0 where pl >= 2^64", float(d.max()))
    figures.update({"Ld": float(r_ld.max()), "wi": float(max(r_wi.max(), r_len.max(), r_dot.max())), "tmax": float(r_t.max()), "pl >= 2^64": int(big.sum())})
    return figures


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
    if op in ("MIS_W_LIGHT", "MIS_W_BSDF"):
        w = np.concatenate([WILD, F32([0.0, -0.0, 1e-30, 0.25, 3e19, 1e-45])])
        return np.stack(np.meshgrid(w, w, indexing="ij"), -1).reshape(-1, 2)
    if op == "LIGHT":
        return light_wild_inputs()
    return None


ALL_OPS = ("SIN", "COS", "ATAN_POS", "ACOS", "SINCOS", "SPHERE_UV", "FRESNEL", "COSINE_ABOUT", "SPHERE_HIT", "QUAD_STEP", "QUAD_STEP_PK", "TRI_HIT",
           "MIS_W_LIGHT", "MIS_W_BSDF", "LIGHT")


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
    if op in ("MIS_W_LIGHT", "MIS_W_BSDF"):
        return mis_weight_inputs(), None
    if op == "LIGHT":
        return light_inputs()
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
    if op in ("MIS_W_LIGHT", "MIS_W_BSDF"):
        return check_mis_weight(op, x, got)
    if op == "LIGHT":
        return check_light(x, aux, got)
    return {"SPHERE_UV": check_sphere_uv, "FRESNEL": check_fresnel, "COSINE_ABOUT": check_cosine_about}[op](x, got)
