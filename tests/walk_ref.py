"""Input sets, float64 references and error bounds of the walk's two blocks (ops QUAD_STEP, QUAD_STEP_PK and TRI_HIT of the building-block
hooks; tests/blocks_ref.py dispatches here).  Nothing below shares a line with the oracle or the library: a quantised node is decoded from
its bytes, a plane origin + q * cell and a ray made of float32 values are exact in float64, and every bound is derived from the roundings
the kernel states -- none is taken from the outputs under test.

THE NODE STEP.  Per axis, with INV = 1 / d (the true quotient) or, for d == +-0, the stand-in +-inv_parallel:
  T = (P - o) INV  the true distance of the decoded plane P = origin + q cell,   G = (o - origin) INV.
The kernel computes inv = fl(1 / d) = INV (1 + e0), ci = cell inv (exact: cell is a power of two and the product a normal float),
g = fl(fl(o - origin) inv) = G (1 + e0)(1 + e1)(1 + e2), gn = fl(g + 6 u |g|) (the margin fma: between 5 u |g| and 7 u |g| beyond g),
t = fl(q ci - gn), every |e| <= u = 2^-24.  Hence for a NEAR plane
  gn >= G (1 + e0)                      (the margin's 5 u covers the 2 u of e1, e2)   =>   t <= T (1 + e0) + u |.|  <=  T + 2 u |T|
  gn <= G (1 + e0) + (2 + 7) u |G| (1 + 4 u)                                          =>   t >= T - QUAD_C u |G| - 2 u |T|,   QUAD_C = 9
(second-order terms: the factor 1 + 2^-20 below), and the mirror image for a FAR plane.  A denormal g or t is off by a denormal ulp
instead: TINY.  The hook returns tn = max(near t's, 1e-4) and the hit mask, so the plane bounds are asserted on tn and through hit."""
import functools
import itertools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
TMIN = float(F32(1e-4))
# THE PADS AS THEY ARE IN EFFECT (a finding of these tests).  The sources write kBoxPad = 0x1.000004p+0f and kOwnPad =
# 0x1.000001p+0f and call them 1 + 2^-19 and 1 + 2^-21; six hexadecimal digits are 24 bits, so the literals are 1 + 2^-22 (= 1 + 4 u) and
# 1 + 2^-24, and the second is no float32: it rounds to 1.  The node test pads by 4 u and the own-box rule by nothing, on both sides alike.
BOX_PAD = float.fromhex("0x1.000004p+0")
OWN_PAD = float(F32(float.fromhex("0x1.000001p+0")))
assert BOX_PAD == 1.0 + 2.0 ** -22 and OWN_PAD == 1.0
QUAD_C = 9.0
SECOND_ORDER = 1.0 + 2.0 ** -20
TINY = 2.0 ** -146          # eight denormal ulps: g, its margin and t each rounded where float32 has no relative precision left
F64_SLACK = 2.0 ** -50      # the float64 reference's own roundings (a quotient, a product, a difference), relative to the terms subtracted


def _f32(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(F32)


def nextafter32(x, steps):
    """float32 x moved by `steps` places in the order of all float32"""
    b = np.asarray(x, F32).view(np.uint32).astype(np.int64)
    i = np.where(b < 0x80000000, b, -(b & 0x7fffffff)) + steps
    return np.where(i >= 0, i, 0x80000000 | (-i)).astype(np.uint32).view(F32)


# ---------------------------------------------------------------------------------------------------------------------------------
# quantised nodes: 16 words -- origin xyz, cell x, qlo x y z, qhi x y z (a byte per child in each), cell y z, four child refs
# ---------------------------------------------------------------------------------------------------------------------------------
def quad_words(origin, cell, qlo, qhi):
    """origin, cell (M, 3) float32; qlo, qhi (M, 4, 3) integers 0 .. 255 -> (M, 16) uint32"""
    origin, cell = np.ascontiguousarray(origin, F32), np.ascontiguousarray(cell, F32)
    W = np.zeros((len(origin), 16), np.uint32)
    W[:, 0:3] = origin.view(np.uint32)
    W[:, 3], W[:, 10], W[:, 11] = (cell[:, a].copy().view(np.uint32) for a in range(3))
    for a in range(3):
        for k in range(4):
            W[:, 4 + a] |= (np.asarray(qlo)[:, k, a].astype(np.uint32) & 0xff) << np.uint32(8 * k)
            W[:, 7 + a] |= (np.asarray(qhi)[:, k, a].astype(np.uint32) & 0xff) << np.uint32(8 * k)
    W[:, 12:16] = 0x80000000
    return W


def quad_decode(W):
    """(M, 16) uint32 -> origin (M, 3) float32, cell (M, 3) float32, qlo, qhi (M, 4, 3) int64"""
    W = np.ascontiguousarray(W, np.uint32)
    origin = W[:, 0:3].copy().view(F32)
    cell = np.stack([W[:, 3], W[:, 10], W[:, 11]], 1).copy().view(F32)
    sh = (8 * np.arange(4))[None, :, None].astype(np.uint32)
    qlo = ((W[:, None, 4:7] >> sh) & 0xff).astype(np.int64)
    qhi = ((W[:, None, 7:10] >> sh) & 0xff).astype(np.int64)
    return origin, cell, qlo, qhi


def inv_parallel_for_box(lo, hi):
    """DESIGN.md 3.4's stand-in for 1 / 0 of a scene whose root box is [lo, hi] (float32 rows): 2^e, e = 123 - x clamped to [-100, 120],
    2 * extent = m 2^x with m in [0.5, 1), extent the box's largest side in float32 (0 or not finite: x = 0)"""
    with np.errstate(all="ignore"):
        ext = (np.asarray(hi, F32) - np.asarray(lo, F32)).max(axis=1).astype(np.float64)
    ok = np.isfinite(ext) & (ext > 0)
    x = np.where(ok, np.frexp(np.where(ok, 2.0 * ext, 1.0))[1], 0)
    return np.ldexp(1.0, np.clip(123 - x, -100, 120)).astype(F32)


QUAD_BYTES = (0, 1, 127, 254, 255)
QUAD_ORIGINS = (0.0, 1e-3, -1e-3, 1e6, -1e6)
QUAD_CELL_EXP = (-20, -9, -1, 0, 6, 20)


def synthetic_nodes(cell_exps=QUAD_CELL_EXP):
    """one node per (origin, cell, number of children): child boxes with bytes from QUAD_BYTES (flat ones, lo == hi, included), the unused
    slots inverted (qlo 255, qhi 0) -> (W (M, 16) uint32, root boxes (M, 6) float32: the node's own decoded box)"""
    rng = np.random.default_rng(5)
    pairs = np.array([(lo, hi) for lo in QUAD_BYTES for hi in QUAD_BYTES if lo <= hi])
    org, cel, qlo, qhi = [], [], [], []
    for i, (oi, ci, nch) in enumerate(itertools.product(range(len(QUAD_ORIGINS)), range(len(cell_exps)), (2, 3, 4))):
        org.append([QUAD_ORIGINS[(oi + a) % len(QUAD_ORIGINS)] for a in range(3)])
        e = cell_exps[ci]
        cel.append([2.0 ** e] * 3 if nch < 4 else [2.0 ** e, 2.0 ** (e + 1), 2.0 ** (e - 1)])
        p = pairs[rng.integers(0, len(pairs), (4, 3))]
        lo, hi = p[..., 0], p[..., 1]
        lo[nch:], hi[nch:] = 255, 0
        qlo.append(lo)
        qhi.append(hi)
    with np.errstate(over="ignore"):
        origin, cell = np.array(org, F32), np.array(cel, F32)
        boxes = np.concatenate([origin, origin + F32(255) * cell], 1).astype(F32)
    return quad_words(origin, cell, np.array(qlo), np.array(qhi)), boxes


def real_nodes(n_each=24):
    """nodes of the product's host builder on the small test scenes, evenly strided, with the boxes the bytes were quantised from
    -> (W, root boxes (M, 6), exact child boxes (M, 24))"""
    import util
    from pbrt_amd import api
    W, boxes, exact = [], [], []
    for name in ("mesh1k", "cornell"):
        sd = util.SMALL_SCENES[name]()
        t = api.quad_build_host_ex(sd.P, sd.idx)
        pick = np.unique(np.linspace(0, len(t["quads"]) - 1, n_each).astype(int))
        W.append(t["quads"][pick])
        exact.append(t["exact_boxes"][pick])
        boxes.append(np.broadcast_to(np.asarray(t["root_box"], F32), (len(pick), 6)))
    return np.concatenate(W), np.concatenate(boxes).astype(F32), np.concatenate(exact).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 statement of one step
# ---------------------------------------------------------------------------------------------------------------------------------
def quad_step_f64(x):
    """x (N, 24) float32 as given to the op -> dict of float64 arrays: per child and axis the true distances Tn, Tf of the near / far decoded
    planes (INV = 1 / d, or +-inv_parallel on an axis with d == +-0), G per axis, the error terms, `domain` (where bounds are asserted),
    `must_hit` / `may_hit` per child, the unused slots"""
    x = np.ascontiguousarray(x, F32)
    origin, cell, qlo, qhi = quad_decode(x.view(np.uint32)[:, :16])
    o, d = x[:, 16:19].astype(np.float64), x[:, 19:22].astype(np.float64)
    big, tfar = x[:, 22].astype(np.float64), x[:, 23].astype(np.float64)
    o64, c64 = origin.astype(np.float64), cell.astype(np.float64)
    zero = d == 0
    with np.errstate(all="ignore"):
        inv32 = (F32(1) / x[:, 19:22]).astype(np.float64)                    # what the kernel multiplies by, for the domain alone
        INV = np.where(zero, np.copysign(big[:, None], d), 1.0 / d)
        neg = np.signbit(d)[:, None, :]
        Plo, Phi = o64[:, None, :] + qlo * c64[:, None, :], o64[:, None, :] + qhi * c64[:, None, :]
        Pn, Pf = np.where(neg, Phi, Plo), np.where(neg, Plo, Phi)
        oo, ii = o[:, None, :], INV[:, None, :]
        Tn, Tf = (Pn - oo) * ii, (Pf - oo) * ii
        G = (o - o64) * INV
        slack = F64_SLACK * (np.abs(Pn) + np.abs(Pf) + np.abs(oo)) * np.abs(ii) + TINY
        e_g = QUAD_C * U * SECOND_ORDER * np.abs(G)[:, None, :]
        n_lo, n_up = Tn - e_g - 2 * U * SECOND_ORDER * np.abs(Tn) - slack, Tn + 2 * U * SECOND_ORDER * np.abs(Tn) + slack
        f_lo, f_up = Tf - 2 * U * SECOND_ORDER * np.abs(Tf) - slack, Tf + e_g + 2 * U * SECOND_ORDER * np.abs(Tf) + slack
        tn_star = np.maximum(Tn.max(2), TMIN)
        tn_lo, tn_up = np.maximum(n_lo.max(2), TMIN), np.maximum(n_up.max(2), TMIN)
        tf_up = np.minimum(f_up.min(2), tfar[:, None])
        # the exact rule: [1e-4, tfar] against the decoded box; an axis with d == 0 asks for the origin within the CLOSED slab, no more
        inside = (oo >= Plo) & (oo <= Phi)
        z = zero[:, None, :]
        tn_x = np.maximum(np.where(z, -np.inf, Tn).max(2), TMIN)
        tf_x = np.minimum(np.where(z, np.inf, Tf).min(2), tfar[:, None])
        closed = (tn_x <= tf_x) & (inside | ~z).all(2)
        # ... as far as a finite stand-in can tell: the step's ray on such an axis IS the ray with 1 / d = +-inv_parallel (the zero keeps its
        # sign), so a far plane that the origin lies ON, or within 1e-4 / inv_parallel of (about 1e-40 of the scene's extent: denormal
        # offsets), is nearer than 1e-4 -- as it is for every tiny d of that sign -- and what lies beyond it is behind the ray (DESIGN.md
        # 3.4).  must_hit is that rule; the closed-slab rays it leaves out are counted, and each must be of that kind
        must_hit = tn_star <= np.minimum(Tf.min(2), tfar[:, None])
        on_far = closed & ~must_hit
        near_far = (z & (np.abs(Pf - oo) * np.abs(ii) < TMIN)).any(2)
        may_hit = tn_lo <= tf_up * BOX_PAD * (1.0 + U)
        # the domain: finite inputs, a power-of-two cell, d and 1 / d normal (or d == 0), cell * inv normal, nothing overflows
        normal = lambda v: (np.abs(v) >= 2.0 ** -126) & (np.abs(v) < 2.0 ** 128)
        cbits = cell.view(np.uint32)
        pow2 = ((cbits & 0x807fffff) == 0) & (cbits >> 23 >= 1) & (cbits >> 23 <= 254)
        inv_k = np.where(zero, INV, inv32)
        domain = (np.isfinite(o).all(1) & np.isfinite(o64).all(1) & ~np.isnan(tfar) & pow2.all(1) & (zero | (normal(d) & normal(inv32))).all(1) &
                  normal(c64 * inv_k).all(1) & (np.abs(G) * (1 + 8 * U) < 2.0 ** 127).all(1) & (255.0 * c64 * np.abs(inv_k) < 2.0 ** 127).all(1) &
                  np.isfinite(big) & (big > 0) & (np.frexp(big)[0] == 0.5))
    unused = ((qlo == 255) & (qhi == 0)).all(2)
    size = (255.0 * c64).max(1)
    with np.errstate(all="ignore"):
        away = np.abs(o - (o64 + 127.5 * c64)).max(1) / size     # the origin's distance from the node's centre in node sizes
    return {"Tn": Tn, "Tf": Tf, "tn_star": tn_star, "tn_lo": tn_lo, "tn_up": tn_up, "must_hit": must_hit, "may_hit": may_hit, "domain": domain, "on_far": on_far, "near_far": near_far,
            "unused": unused, "away": away, "zero": zero, "Plo": Plo, "Phi": Phi, "tfar": tfar, "o": o, "d": d}


# ---------------------------------------------------------------------------------------------------------------------------------
# the rays
# ---------------------------------------------------------------------------------------------------------------------------------
_V = (np.array([0.6, 0.48, 0.64]), np.array([0.36, 0.8, 0.48]))
_SIGNS = np.array(list(itertools.product((1.0, -1.0), repeat=3)))


@functools.lru_cache(maxsize=1)
def quad_step_inputs():
    """-> (x (N, 24) float32, aux): about 2^18 (node, ray) pairs -- synthetic and real nodes x the ray families of the issue -- and a tail of
    inputs off the asserted domain (cell exponent bytes 1 and 254, denormal d, NaN and inf in o, d and tfar)"""
    Ws, Bs = synthetic_nodes()
    Wr, Br, Er = real_nodes()
    W, boxes = np.concatenate([Ws, Wr]), np.concatenate([Bs, Br])
    exact = np.concatenate([np.full((len(Ws), 24), np.nan, F32), Er])
    M = len(W)
    origin, cell, qlo, qhi = quad_decode(W)
    o64, c64 = origin.astype(np.float64), cell.astype(np.float64)
    Plo, Phi = o64[:, None, :] + qlo * c64[:, None, :], o64[:, None, :] + qhi * c64[:, None, :]
    size = (255.0 * c64).max(1)[:, None]
    big = inv_parallel_for_box(boxes[:, :3], boxes[:, 3:])
    rays = []  # (o (M, 3) float64 or float32, d (M, 3), tfar (M,))

    def add(o, d, tfar):
        rays.append((_f32(o), _f32(d), _f32(np.broadcast_to(tfar, (M,)))))

    unit = lambda v: v / np.sqrt((v * v).sum(1, keepdims=True))
    n = 0
    aimed_for_tfar = []
    # A: aimed at decoded corners, edge midpoints, face centres and centres, from 1 .. 10^6 node sizes away; exactly (d = target - o, the
    # target at t = 1 up to the subtraction's rounding) and a few ulps beside (a unit direction, one component moved by 1 or 4 places)
    for k in range(4):
        for sel in itertools.product((0, 1, 2), repeat=3):
            w = np.array(sel) / 2.0
            target = Plo[:, k] * (1 - w) + Phi[:, k] * w
            for dist in (1.0, 1e2, 1e4, 1e6):
                for vi in range(2):
                    n += 1
                    v = _V[vi] * _SIGNS[n % 8]
                    o = _f32(target + dist * size * v).astype(np.float64)
                    d = target - o
                    tf = np.inf if n % 2 else 1e30
                    if n % 4 < 2:
                        add(o, d, tf)
                        if sum(s == 1 for s in sel) == 0 and dist <= 1e2 and vi == 0:
                            aimed_for_tfar.append((o, _f32(d)))
                    else:
                        for step in ((1, -4), (-1, 4))[(n // 4) % 2]:
                            du = _f32(unit(d))
                            du[:, n % 3] = nextafter32(du[:, n % 3], step)
                            add(o, du, tf)
    # B: origins exactly on a plane of a child (the float32 nearest to it), elsewhere at the child's centre: a generic direction, and rays lying
    # in the face -- d_a = +0, -0 and a tiny normal number of either sign
    for k in range(4):
        centre = 0.5 * (Plo[:, k] + Phi[:, k])
        for a in range(3):
            for P in (Plo, Phi):
                o = centre.copy()
                o[:, a] = P[:, k, a]
                o = _f32(o).astype(np.float64)
                for da in (None, 0.0, -0.0, 1e-30, -1e-30):
                    n += 1
                    d = np.tile(_V[n % 2] * _SIGNS[n % 8], (M, 1))
                    if da is not None:
                        d[:, a] = da
                    add(o, d, np.inf)
    # C: one and two components exactly 0 (both signs): origins inside the child, and one place outside its slab on a parallel axis
    for k in range(4):
        centre = 0.5 * (Plo[:, k] + Phi[:, k])
        for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2)):
            for z in (0.0, -0.0):
                for where in (0, -1, 1):
                    n += 1
                    d = np.tile(_V[n % 2] * _SIGNS[n % 8], (M, 1))
                    d[:, list(axes)] = z
                    o = _f32(centre)
                    a = axes[0]
                    if where < 0:
                        o[:, a] = nextafter32(_f32(Plo[:, k, a]), -1)
                        o[:, a] = np.where(o[:, a].astype(np.float64) < Plo[:, k, a], o[:, a], nextafter32(o[:, a], -1))
                    if where > 0:
                        o[:, a] = nextafter32(_f32(Phi[:, k, a]), 1)
                        o[:, a] = np.where(o[:, a].astype(np.float64) > Phi[:, k, a], o[:, a], nextafter32(o[:, a], 1))
                    add(o, d, np.inf)
    # D: origins inside -- a child's centre, the node's centre
    for k in range(5):
        centre = 0.5 * (Plo[:, k] + Phi[:, k]) if k < 4 else o64 + 127.5 * c64
        for s in range(8):
            for vi in range(2):
                add(centre, np.tile(_V[vi] * _SIGNS[s], (M, 1)), np.inf if s % 2 else 1e30)

    def pack(node, o, d, tfar):
        x = np.zeros((len(node), 24), F32)
        x.view(np.uint32)[:, :16] = W[node]
        x[:, 16:19], x[:, 19:22], x[:, 22], x[:, 23] = o, d, big[node], tfar
        return x

    node = np.tile(np.arange(M), len(rays))
    x = pack(node, np.concatenate([r[0] for r in rays]), np.concatenate([r[1] for r in rays]), np.concatenate([r[2] for r in rays]))
    # E: tfar at the true entry distance of the aimed-at child and 1, 2 places either side, at 1e-4, one place below it, and at 0
    parts, nodes_e = [], []
    for j, (o, d) in enumerate(aimed_for_tfar):
        k = j // (len(aimed_for_tfar) // 4)
        tn = quad_step_f64(pack(np.arange(M), o, d, np.full(M, np.inf, F32)))["tn_star"][:, k]
        for step in (-2, -1, 0, 1, 2):
            parts.append(pack(np.arange(M), o, d, nextafter32(_f32(tn), step)))
        for tf in (F32(1e-4), nextafter32(F32(1e-4), -1)[()], F32(0.0)):
            parts.append(pack(np.arange(M), o, d, np.full(M, tf, F32)))
        nodes_e.append(np.tile(np.arange(M), 8))
    x = np.concatenate([x] + parts)
    node = np.concatenate([node] + nodes_e)
    # off the domain: nodes whose cell has exponent byte 1 or 254, a denormal component of d, NaN and inf in o, d and tfar
    Ww, Bw = synthetic_nodes(cell_exps=(-126, 127))
    wild = []
    sample = x[:: max(1, len(x) // 512)][:512].copy()
    for m in range(len(Ww)):
        s = sample[m::len(Ww)].copy()
        s.view(np.uint32)[:, :16] = Ww[m]
        wild.append(s)
    for col, vals in ((19, (1e-40, -1e-42, np.nan, np.inf, -np.inf)), (21, (1e-45, np.nan)), (16, (np.nan, np.inf, -np.inf)), (23, (np.nan, -np.inf, -1.0))):
        for v in vals:
            s = sample.copy()
            s[:, col] = F32(v)
            wild.append(s)
    wild = np.concatenate(wild)
    x = np.concatenate([x, wild])
    exact_x = np.concatenate([exact[node], np.full((len(wild), 24), np.nan, F32)])
    return x, {"exact": exact_x, "n_nodes": M}


def check_quad_step(x, aux, got, got_other=None):
    """got (N, 6) = tn of children 0 .. 3, the hit mask, the slot entered.  Asserts, on the domain of quad_step_f64: no false negative (the
    exact rule), tn within the plane bounds, no hit beyond the model, the slot entered, the unused slots; and that the other fma form gave
    the same bits.  -> the figures: sizes, the largest observed fractions of the bounds, counts"""
    if "ref" not in aux:   # (computed once: the two fma forms share the set)
        aux["ref"] = quad_step_f64(x)
    r = aux["ref"]
    dom = r["domain"]
    tn = got[:, :4].astype(np.float64)
    mask = got[:, 4].astype(np.int64)
    assert (got[:, 4] == mask).all() and (mask >= 0).all() and (mask < 16).all()
    hit = ((mask[:, None] >> np.arange(4)) & 1).astype(bool)
    D = dom[:, None]
    # no false negative: zero exceptions
    miss = D & r["must_hit"] & ~hit
    assert not miss.any(), (int(miss.sum()), x[np.argwhere(miss)[0][0]], np.argwhere(miss)[0])
    assert (~(D & r["on_far"]) | r["near_far"]).all()
    # the planes lie outside, and not further than the roundings and the margin put them
    with np.errstate(all="ignore"):
        assert (np.isfinite(tn) | ~D).all()
        low, high = D & (tn < r["tn_lo"]), D & (tn > r["tn_up"])
        assert not high.any(), ("a near plane inside the true one", int(high.sum()), x[np.argwhere(high)[0][0]], np.argwhere(high)[0])
        assert not low.any(), ("a near plane further out than the bound", int(low.sum()), x[np.argwhere(low)[0][0]], np.argwhere(low)[0])
        # (outward: where the bound says something -- on a parallel axis, or one with a tiny d, the margin is 9 u of |o - origin| times a
        # huge 1 / d, beyond any distance -- i.e. where it is below a thousandth of the distance)
        frac_out = np.where(D & (r["tn_lo"] > TMIN) & (r["tn_star"] - r["tn_lo"] < 1e-3 * r["tn_star"]), (r["tn_star"] - tn) / (r["tn_star"] - r["tn_lo"]), 0.0)
        frac_in = np.where(D & (r["tn_star"] > TMIN), (tn - r["tn_star"]) / (r["tn_up"] - r["tn_star"]), 0.0)
    # no false positive beyond the model
    beyond = D & hit & ~r["may_hit"]
    assert not beyond.any(), (int(beyond.sum()), x[np.argwhere(beyond)[0][0]], np.argwhere(beyond)[0])
    # the slot entered: the hit child of least tn, the lowest slot on a tie (everywhere: a function of the outputs alone)
    with np.errstate(all="ignore"):
        key = np.where(hit, np.minimum(tn, 1e300), np.inf)   # (a child hit at tn = inf, with tfar = inf, still comes before a missed one)
    slot = np.where(hit.any(1), np.argmin(key, 1), 4)
    ok = got[:, 5] == slot
    assert ok.all(), (int((~ok).sum()), got[~ok][0])
    # unused slots: never hit by a ray within 2 10^4 node sizes (pad and margins together are 4 u + 18 u of the distance: below one node size
    # -- what an inverted box is short of -- up to 7 10^5 node sizes); further out they may be, and the model above bounds that too
    un = D & r["unused"] & hit
    assert not (un & (r["away"][:, None] <= 2e4)).any(), x[np.argwhere(un)[0][0]]
    if got_other is not None:
        a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(got_other).view(np.uint32)
        assert ((a == b) | (np.isnan(got) & np.isnan(got_other))).all()
    ex = aux["exact"].astype(np.float64).reshape(-1, 4, 6)
    with np.errstate(all="ignore"):
        o, d = r["o"][:, None, :], r["d"][:, None, :]
        lo, hi = ex[..., :3], ex[..., 3:]
        a, b = (lo - o) / d, (hi - o) / d
        par = d == 0
        en = np.where(par, np.where((o >= lo) & (o <= hi), -np.inf, np.inf), np.minimum(a, b)).max(2)
        xf = np.where(par, np.inf, np.maximum(a, b)).min(2)
        meets = (lo <= hi).all(2) & (np.maximum(en, TMIN) <= np.minimum(xf, r["tfar"][:, None]))
    lost = D & meets & ~hit & ~r["near_far"]   # (but for the parallel axis' far plane at the origin: quad_step_f64)
    assert not lost.any(), ("a ray that meets a child's exact box is not let in", x[np.argwhere(lost)[0][0]])
    return {"pairs": len(x), "in the closed slab of a parallel axis, the origin within 1e-4 / inv_parallel of its far plane (hit / all)": (int((D & r["on_far"] & hit).sum()), int((D & r["on_far"]).sum())), "on the domain": int(dom.sum()), "must hit": int((D & r["must_hit"]).sum()), "hit": int((D & hit).sum()),
            "largest fraction of the outward bound": float(frac_out.max()), "largest fraction of the inward bound": float(frac_in.max()),
            "unused slots hit (all beyond 2e4 node sizes)": int(un.sum()), "rays that meet an exact child box": int((D & meets).sum())}


# ---------------------------------------------------------------------------------------------------------------------------------
# TRI_HIT: Moeller-Trumbore in float64 with a running first-order error bound per element
# ---------------------------------------------------------------------------------------------------------------------------------
def _gamma(n):
    return n * U / (1.0 - n * U)


def _cross(a, ea, b, eb):
    """a x b of float64 (N, 3) with the bound of its float32 evaluation: two rounded products and a rounded difference per component
    (gamma_2 of the terms' magnitudes) + the operands' own errors ea, eb carried through"""
    i, j = [1, 2, 0], [2, 0, 1]
    val = a[:, i] * b[:, j] - a[:, j] * b[:, i]
    err = (_gamma(2) * (np.abs(a[:, i] * b[:, j]) + np.abs(a[:, j] * b[:, i])) +
           ea[:, i] * np.abs(b[:, j]) + np.abs(a[:, i]) * eb[:, j] + ea[:, j] * np.abs(b[:, i]) + np.abs(a[:, j]) * eb[:, i])
    return val, err


def _dot(a, ea, b, eb):
    """a . b with gamma_3 of the summed magnitudes + the operands' errors carried through"""
    return (a * b).sum(1), _gamma(3) * np.abs(a * b).sum(1) + (ea * np.abs(b) + np.abs(a) * eb).sum(1)


def tri_hit_f64(x, flat=False):
    """x (N, 16) float32 = p0 p1 p2, o, d, tmax -> dict: valid, t, u, v of float64; the bounds on the float32 path's t, u, v; robust; ..."""
    x = np.ascontiguousarray(x, F32).astype(np.float64)
    p0, p1, p2, o, d, tmax = x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12], x[:, 12:15], x[:, 15]
    zero3 = np.zeros_like(d)
    with np.errstate(all="ignore"):
        e1, e2, tv = p1 - p0, p2 - p0, o - p0
        ee1, ee2, etv = U * np.abs(e1), U * np.abs(e2), U * np.abs(tv)
        pv, epv = _cross(d, zero3, e2, ee2)
        det, edet = _dot(e1, ee1, pv, epv)
        idet = 1.0 / det
        eidet = U * np.abs(idet) + edet * idet * idet
        su, esu = _dot(tv, etv, pv, epv)
        qv, eqv = _cross(tv, etv, e1, ee1)
        sv, esv = _dot(d, zero3, qv, eqv)
        st, est = _dot(e2, ee2, qv, eqv)
        quot = lambda s, es: (s * idet, U * np.abs(s * idet) + es * np.abs(idet) + np.abs(s) * eidet)
        (u, eu), (v, ev), (th, eth) = quot(su, esu), quot(sv, esv), quot(st, est)
        # the own box: slab distances of the three vertices with the true 1 / d, NaN-ignoring min / max (a 0 / 0 is skipped, as the kernel's)
        s = np.stack([(p - o) / d for p in (p0, p1, p2)])
        near, far = np.fmin(np.fmin(s[0], s[1]), s[2]), np.fmax(np.fmax(s[0], s[1]), s[2])
        entry = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], TMIN))
        exit_ = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        e_entry, e_exit = 4 * U * np.abs(entry), 4 * U * np.abs(exit_)   # (p - o) fl(1 / d): three roundings, 4 u generous
        t = np.fmax(th, entry)
        et = np.maximum(eth, e_entry) + U * np.abs(t)
        w, ew = 1.0 - u - v, eu + ev + U * np.abs(u + v)
        box_margin, e_box = exit_ * OWN_PAD - entry, e_entry + e_exit + U * np.abs(exit_)
        inside = (u >= 0) & (v >= 0) & (w >= 0)
        in_range = (th > TMIN) & (t < tmax)
        det_ok = ~(np.abs(det) < 1e-8)
        valid = inside & in_range & det_ok & (box_margin >= 0)
        K = 16.0
        sure_det = np.abs(np.abs(det) - 1e-8) > K * edet
        sure_uvw = (np.abs(u) > K * eu) & (np.abs(v) > K * ev) & (np.abs(w) > K * ew)
        sure_t = (np.abs(th - TMIN) > K * eth) & (np.abs(tmax - t) > K * et)
        sure_box = np.abs(box_margin) > K * e_box
        finite = np.isfinite(u) & np.isfinite(v) & np.isfinite(th) & np.isfinite(eu) & np.isfinite(ev) & np.isfinite(eth)
        # a miss decided by the det cut alone needs nothing else; otherwise every comparison has to be clear of its own bound
        robust = sure_det & (~det_ok | (finite & sure_uvw & sure_t & sure_box))
        # flat triangles: the box margin is 0 by construction (entry = exit), so "robustly inside" leaves it out
        robust_inside = sure_det & det_ok & finite & sure_uvw & inside & sure_t & in_range
        geometric = inside & in_range & (box_margin >= 0)   # what the cut takes away: hits but for |det| < 1e-8
    return {"valid": valid, "t": t, "u": u, "v": v, "et": et, "eu": eu, "ev": ev, "robust": robust, "robust_inside": robust_inside,
            "entry": entry, "exit": exit_, "det": det, "lost_to_cut": geometric & ~det_ok, "geometric": geometric}


TRI_ASPECTS, TRI_DISTS, TRI_SIZES, TRI_DLENS = (1.0, 1e2, 1e4), (1.0, 1e2, 1e4), (1e-3, 1.0, 1e3), (1e-3, 1.0, 1e3)
TRI_RAYS_PER_RUNG = 1 << 14
# The rungs (aspect, distance / size, size, |d|) that are ASSERTED: those on which the float64 reference alone finds at least half of the rays
# robust (checked in check_tri_hit, from float64 alone; the others are measured and printed).  The error of u, v grows with aspect x distance
# / size, and |det| = |d| size^2 cos / aspect falls under the 1e-8 cut for small triangles: see DESIGN.md 3.5's table.
def tri_rung_asserted(aspect, dist, size, dlen):
    """u and v are off by about 10 u x aspect x distance / size, and a sixteenth of the 1e-3 .. 1 that the aimed rays keep from the edges has
    to exceed that: aspect x distance / size <= 100; |det| = |d| size^2 cos / aspect with the cosine down to 0.02 has to stay clear of the
    1e-8 cut: |d| size^2 / aspect >= 1e-6; and the hit, at t = distance / |d|, clear of 1e-4: t >= 1e-3"""
    return aspect * dist <= 1e2 and dlen * size * size / aspect >= 1e-6 and dist * size / dlen >= 1e-3


def _frame(seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    b = np.cross(a, rng.normal(size=3))
    b /= np.linalg.norm(b)
    return a, b, np.cross(a, b)


def tri_rung_inputs(aspect, dist, size, dlen, n=TRI_RAYS_PER_RUNG, seed=0):
    """one triangle in general position -- longest edge `size`, height size / aspect -- and n rays of length |d| = dlen from dist x size away:
    5/8 aimed inside (barycentrics uniform), 1/8 within 1e-3 of an edge on either side, 1/8 outside, 1/8 inside with tmax at the hit +- places;
    incidence from head-on to grazing (the cosine to the normal from 1 down to 0.02)"""
    rng = np.random.default_rng(1000 + seed)
    ea, eb, en = _frame(seed)
    c = size * np.array([0.3, -0.2, 0.1])
    P = _f32(np.stack([c, c + size * ea, c + size * (0.5 * ea + eb / aspect)])).astype(np.float64)
    kind = np.arange(n) % 8
    r1, r2 = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    bu, bv = 1 - np.sqrt(r1), np.sqrt(r1) * r2
    edge = rng.uniform(-1e-3, 1e-3, n)
    bu = np.where(kind == 5, edge, bu)                                    # across the edge u = 0
    bu, bv = np.where(kind == 6, -0.2 - r1, bu), np.where(kind == 6, r2, bv)   # outside
    target = P[0] + bu[:, None] * (P[1] - P[0]) + bv[:, None] * (P[2] - P[0])
    cosn = np.where(kind == 4, 0.02 + 0.1 * rng.uniform(0, 1, n), 0.1 + 0.9 * rng.uniform(0, 1, n))   # kind 4 inside, grazing
    phi = 2 * np.pi * rng.uniform(0, 1, n)
    sinn = np.sqrt(1 - cosn * cosn)
    back = en * cosn[:, None] * np.where(rng.uniform(0, 1, n) < 0.5, 1.0, -1.0)[:, None] + (ea * np.cos(phi)[:, None] + eb * np.sin(phi)[:, None]) * sinn[:, None]
    o = _f32(target + dist * size * back)
    dv = target - o.astype(np.float64)
    dn = np.linalg.norm(dv, axis=1)
    d = _f32(dv / dn[:, None] * dlen)
    tmax = np.full(n, np.inf, F32)
    th = _f32(dn / dlen)
    tmax = np.where(kind == 7, nextafter32(th, np.array([-64, -2, 0, 2, 64, 4096])[(np.arange(n) // 8) % 6]), tmax)
    x = np.concatenate([np.broadcast_to(_f32(P).reshape(1, 9), (n, 9)), o, d, tmax[:, None]], 1).astype(F32)
    return x


def tri_flat_inputs(n=TRI_RAYS_PER_RUNG):
    """triangles FLAT in an axis plane -- a right triangle, and slivers of aspect 2e2 .. 2e4 rotated in the plane --, rays aimed inside them
    from a generic side, at their vertices and along their edges (util.adversarial_rays' kinds), and with tmax at the hit and +-1, 2 places
    -> (x, part): part[i] = the triangle's index"""
    rng = np.random.default_rng(77)
    tris = []
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for eps in (None, 1e-2, 1e-3, 1e-4):
            q = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)) if eps is None else ((0.0, 0.0), (2.0, 0.2), (2.0, 0.2 + eps * 2.0))
            T = np.zeros((3, 3))
            T[:, axis] = 0.5 * (axis + 1) + 0.125
            T[:, a], T[:, b] = [p[0] - 1.0 for p in q], [p[1] - 0.3 for p in q]
            tris.append(_f32(T).astype(np.float64))
    per = n // len(tris)
    xs, part = [], []
    for i, T in enumerate(tris):
        kind = np.arange(per) % 8
        r1, r2 = rng.uniform(0, 1, per), rng.uniform(0, 1, per)
        bu, bv = 1 - np.sqrt(r1), np.sqrt(r1) * r2
        bu, bv = np.where(kind == 5, (np.arange(per) // 8) % 2, bu), np.where(kind == 5, (np.arange(per) // 16) % 2 * (1 - (np.arange(per) // 8) % 2), bv)  # vertices
        bv = np.where(kind == 6, 0.0, bv)                                                                # points on the edge v = 0
        target = _f32(T[0] + bu[:, None] * (T[1] - T[0]) + bv[:, None] * (T[2] - T[0])).astype(np.float64)
        o = _f32(target + rng.uniform(-3, 3, (per, 3)))
        along = kind == 7                                                                                # along an edge's line, in the plane
        o = np.where(along[:, None], _f32(T[1] + (T[1] - T[0]) * r1[:, None]), o)
        target = np.where(along[:, None], T[0], target)
        dv = target - o.astype(np.float64)
        dn = np.linalg.norm(dv, axis=1)
        d = _f32(dv / dn[:, None])
        d = np.where((kind == 3)[:, None], _f32(dv), d)                                                  # unnormalised: the target at t = 1
        th = _f32(np.where(kind == 3, 1.0, dn))
        tmax = np.where(kind == 4, nextafter32(th, np.array([-2, -1, 0, 1, 2])[(np.arange(per) // 8) % 5]), F32(np.inf)).astype(F32)
        xs.append(np.concatenate([np.broadcast_to(_f32(T).reshape(1, 9), (per, 9)), o, d, tmax[:, None]], 1).astype(F32))
        part.append(np.full(per, i))
    return np.concatenate(xs), np.concatenate(part)


def tri_hit_inputs(size):
    """the 27 rungs of one size (aspect x distance / size x |d|), 2^14 rays each -> (x, [(rung, slice)])"""
    xs, parts, at = [], [], 0
    for k, (aspect, dist, dlen) in enumerate(itertools.product(TRI_ASPECTS, TRI_DISTS, TRI_DLENS)):
        x = tri_rung_inputs(aspect, dist, size, dlen, seed=k)
        xs.append(x)
        parts.append(((aspect, dist, size, dlen), slice(at, at + len(x))))
        at += len(x)
    return np.concatenate(xs), parts


def check_tri_rays(x, got, flat=False):
    """one set of rays against the float64 reference -> its measurements; asserts what holds on ALL rays, and (flat) the no-holes claim"""
    r = tri_hit_f64(x)
    ok = got[:, 0] == 1.0
    assert np.isin(got[:, 0], (0.0, 1.0)).all() and (got[~ok, 1:] == 0).all()
    t, u, v = (got[:, k].astype(np.float64) for k in (1, 2, 3))
    with np.errstate(all="ignore"):
        # on all rays: an accepted hit is not before its own box's entry, and its ray meets that box (4 u on either side for the three roundings
        # of a slab distance)
        assert (t[ok] >= r["entry"][ok] * (1 - 4 * U)).all()
        assert (r["entry"][ok] * (1 - 4 * U) <= r["exit"][ok] * OWN_PAD * (1 + 4 * U)).all()
        assert (t[ok] < x[ok, 15]).all() and (t[ok] >= TMIN).all() and (u[ok] >= 0).all() and (v[ok] >= 0).all()
        rb = r["robust"]
        same = ok == r["valid"]
        hits = rb & r["valid"] & ok
        ratio = lambda a, ref, e: float(np.max(np.abs(a[hits] - ref[hits]) / e[hits])) if hits.any() else 0.0
        m = {"robust": float(rb.mean()), "robust_equal": bool(same[rb].all()), "equal": float(same.mean()),
             "max_dt": float(np.max(np.abs(t[hits] - r["t"][hits]))) if hits.any() else 0.0,
             "max_duv": float(max(np.max(np.abs(u[hits] - r["u"][hits])), np.max(np.abs(v[hits] - r["v"][hits])))) if hits.any() else 0.0,
             "ratio_t": ratio(t, r["t"], r["et"]), "ratio_u": ratio(u, r["u"], r["eu"]), "ratio_v": ratio(v, r["v"], r["ev"]),
             "lost_to_cut": float(r["lost_to_cut"].sum() / max(1, r["geometric"].sum())), "hits": int(hits.sum())}
    if flat:
        ri = r["robust_inside"]
        assert ri.sum() > len(x) // 8 and ok[ri].all(), ("a hole in a flat triangle", x[ri & ~ok][:1])
        m["robustly inside"] = int(ri.sum())
    return m


def check_tri_hit(parts, x, got):
    """the rungs of tri_hit_inputs -> {rung: measurements}; an ASSERTED rung has at least half of its rays robust by float64 alone, equal
    hit-or-miss on every robust ray and |dt|, |du|, |dv| within their bounds on every robust hit"""
    out = {}
    for rung, sl in parts:
        m = check_tri_rays(x[sl], got[sl])
        m["asserted"] = tri_rung_asserted(*rung)
        if m["asserted"]:
            assert m["robust"] >= 0.5, (rung, m)   # (a condition on the reference alone)
            assert m["robust_equal"] and m["hits"] > 0, (rung, m)
            assert max(m["ratio_t"], m["ratio_u"], m["ratio_v"]) <= 1.0, (rung, m)
        out[rung] = m
    return out


def tri_exact_inputs():
    """Rays whose Moeller-Trumbore is EXACT in float32 (vertices on small integers, directions in eighths, det a power of two, the target
    at t = 3), aimed at a grid of barycentrics (-1/8 .. 9/8)^2: the vertices, points ON all three edges -- u = 0, v = 0 and u + v = 1, which
    count as hits --, inside and outside.  Only the own box's slab distances round (3 d fl(1 / d) comes out a place above 3 for d = 7/8, 7/16, 15/16): a ray through
    a vertex meets the triangle's box exactly at a corner, entry = exit in exact arithmetic, and the box test has to let it in (kOwnPad)."""
    tris = [np.array([[1, 2, -1], [5, 2, -1], [1, 6, -1]], np.float64)]         # flat in z
    tris.append(tris[0][:, [2, 0, 1]])                                         # the same flat in x
    dirs = [(a, b, c) for a in (0.875, -0.4375, 0.625, 0.0, -1.0) for b in (0.375, -0.875, -0.9375, 0.5) for c in (-1.0, -0.5, 1.0)]
    g = np.arange(-1, 10) / 8.0
    bu, bv = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    xs = []
    for i, T in enumerate(tris):
        target = T[0] + bu[:, None] * (T[1] - T[0]) + bv[:, None] * (T[2] - T[0])
        for dd in dirs:
            d = np.array(dd)[[0, 1, 2]] if i == 0 else np.array(dd)[[2, 0, 1]]
            o = target - 3.0 * d
            for tmax in (np.inf, 3.0, float(nextafter32(F32(3.0), 2))):
                xs.append(np.concatenate([np.broadcast_to(T.reshape(1, 9), (len(o), 9)), o, np.broadcast_to(d, o.shape), np.full((len(o), 1), tmax)], 1))
    x = np.concatenate(xs)
    assert (x.astype(F32).astype(np.float64) == x).all()
    return x.astype(F32)


def check_tri_exact(x, got):
    """u and v equal float64's exactly (the arithmetic is exact; the edges count) and t = 3 up to the own box's entry (4 u); no hit that float64
    does not have; and a hit of float64's is missed ONLY where the own box's float32 slab distances -- restated below in numpy float32 from
    DESIGN.md 3.5's formula -- put the entry a place beyond the exit: with a pad of 1 (OWN_PAD above) the rule rejects a ray through a corner or
    an edge of the box whenever a rounding goes the wrong way.  Those are counted (552 of the 10 320 hits at the time of writing); a pad
    of 1 + 2^-21, as DESIGN.md 3.5 meant it, would let every one of them in."""
    r = tri_hit_f64(x)
    ok = got[:, 0] == 1.0
    p, o, d = [x[:, 0:3], x[:, 3:6], x[:, 6:9]], x[:, 9:12], x[:, 12:15]
    with np.errstate(all="ignore"):
        inv = F32(1) / d
        s = np.stack([(q - o) * inv for q in p])
        near, far = np.fmin(np.fmin(s[0], s[1]), s[2]), np.fmax(np.fmax(s[0], s[1]), s[2])
        tn = np.fmax(np.fmax(near[:, 0], near[:, 1]), np.fmax(near[:, 2], F32(1e-4)))
        tf = np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2])
        grazed = tn > tf * F32(OWN_PAD)
    assert not (ok & ~r["valid"]).any(), x[ok & ~r["valid"]][0]
    lost = r["valid"] & ~ok
    assert not (lost & ~grazed).any(), (int((lost & ~grazed).sum()), x[lost & ~grazed][0])
    assert (tn[lost] <= tf[lost] * F32(1.0 + 2.0 ** -21)).all()   # (each within 8 u of its box: what the meant pad would have let in)
    assert (got[ok, 2] == r["u"][ok]).all() and (got[ok, 3] == r["v"][ok]).all()
    assert (np.abs(got[ok, 1] - 3.0) <= 12 * U).all() and (got[ok, 1] >= 3.0).all()
    on_edge = ok & ((r["u"] == 0) | (r["v"] == 0) | (r["u"] + r["v"] == 1))
    assert on_edge.sum() > 1000 and (ok & (r["u"] + r["v"] == 1)).sum() > 100
    return {"rays": len(x), "hits": int(ok.sum()), "on an edge or a vertex": int(on_edge.sum()), "lost at a corner or an edge of the own box": int(lost.sum())}
