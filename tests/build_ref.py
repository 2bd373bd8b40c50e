"""References for the device tree builder's stages (pbrt_amd/csrc/bvh_gpu.hip).  numpy only: nothing here imports
pbrt_amd, so nothing here can share a mistake with the code it is compared to except by misreading it -- and the float64 side checks
below are there to catch a shared misreading.

Stage 1 is restated in float32, statement by statement: the library is compiled without contraction and without fast math, so every float
statement of morton_kernel, sah_prepare_kernel, sah_bins_kernel and sah_split_kernel is one IEEE single operation, and numpy's float32
arithmetic gives the same bits.  The restatement is top-down over SETS of triangles: every partition of the builder is stable, so a
segment at the moment it is split is its set in (Morton key, triangle id) order, whatever the level-synchronous machinery around it.

The tail of stage 2 (child order, depth-first leaf numbering) is restated from reinsert_core.hpp's order_children and the ri_* kernels.

Stage 3's dynamic programme is restated in float64 from the recurrence in the header comment of quad_encode.hpp, without its functions.

Trees are exchanged in the builder's own form.  n leaves of one triangle each; interior nodes [0, n - 1), root 0; child[n - 1, 2] holds an
interior node or LEAF | leaf slot; parent_internal[n - 1] (the root's: NONE), parent_leaf[n]; boxes[2 n - 1, 6] = lo xyz, hi xyz, the leaf
of slot k as node (n - 1) + k; order[n] = leaf slot -> triangle.  The link form of re-insertion: par[2 n - 1], kid[n - 1, 2], boxes, nodes
numbered as in `boxes`."""
import numpy as np

F32 = np.float32
LEAF = 0x80000000
NONE = 0xFFFFFFFF
BUCKETS = 16
MEDIAN_LEVEL = 40  # kSahMedianLevel: from this level on a segment is halved as it stands
TRI_COST = 2.0     # quad::kDpTriCost

# The plane sweep's float32 cost against the same expression in float64 (plane_costs_f64).  With u = 2^-24, every operand positive:
#   dx, dy, dz = hi - lo                  one rounding each: two of them meet in a product            (1 + u)^2
#   dx * dy, dx * dz, dy * dz             one rounding                                                (1 + u)
#   (dx * dy + dx * dz) + dy * dz         two additions                                               (1 + u)^2
#   (float)c * area                       one rounding (c <= 2^24 is exact)                           (1 + u)
#   ... + (float)c_r * area_r             one addition                                                (1 + u)
# A sum of positive terms each within (1 + u)^7 of its exact value is within (1 + u)^7 of the exact sum: cost32 = cost64 (1 + e), |e| <
# 7.001 u < 2^-21 ("five roundings" of the operations after the two of the extents).  The plane k the float32 sweep chooses has cost32[k] <=
# cost32[j] for every j, so cost64[k] <= cost64[j] (1 + e) / (1 - e) < cost64[j] (1 + 2^-20): PLANE_MARGIN.  (float64's own rounding, 2^-53
# per operation, is five orders below the slack between 14.01 u and 16 u.)
PLANE_MARGIN = 2.0 ** -20

# The dynamic programme's float32 tables against the float64 recurrence (dp_tables_f64).  area_on_grid, with the cell size a power of two
# that both sides take from the same float32 statement (cell_size: it DEFINES the grid, it approximates nothing):
#   (hi - lo) + cell                      two roundings per axis, two axes meet in a product          (1 + u)^4
#   the three products, the two additions as above                                                    (1 + u)^3
# so an area is within (1 + u)^7; kDpTriCost = 2 and the triangle count 1 multiply exactly.  Every table entry is a minimum over sums of
# such areas, and a term passes through at most two more additions per interior node between it and the entry (`area + G` and `F(l) +
# F(r)`: dp_interior, dp_dist).  In a subtree of m nodes fewer than m / 2 are interior, so an entry is within (1 + u)^(7 + m) of the sum
# its choices give in exact arithmetic, and a minimum over candidates each within a factor is within that factor: |F32 - F64| <= ((1 +
# u)^(7 + m) - 1) F64 < DP_C m u F64 with DP_C = 10 for every m >= 1 (m = 1: 8.0001 u; m <= 2^22: (7 + m) u / (1 - (7 + m) u) < 1.4 m u).
# The tree the collapse EMITS by following the float32 choices costs, in float64, W with W32 = G32(root) by construction, so G64 <= W <=
# G64 (1 + e) / (1 - e) with e = (7 + m) u: twice the table bound, still below DP_C m u for m >= 3.
DP_C = 10.0


def dp_bound(m):
    """relative bound on a float32 table entry (and on the emitted tree's work) over a subtree of m nodes: m x DP_C x 2^-24"""
    return np.asarray(m, np.float64) * DP_C * 2.0 ** -24


# ---------------------------------------------------------------- stage 1 ----
def tri_boxes(P, idx):
    v = np.asarray(P, F32).reshape(-1, 3)[np.asarray(idx, np.int64).reshape(-1, 3)]
    return v.min(1), v.max(1)


def _spread10(v):
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def morton_keys(tlo, thi):
    """morton_kernel over the bounds centroid_bounds_kernel leaves: 10 bits per axis of the box centre within the centres' bounds"""
    c = F32(0.5) * tlo + F32(0.5) * thi
    mn, mx = c.min(0), c.max(0)
    ext = mx - mn
    u = np.where(ext > 0, (c - mn) / np.where(ext > 0, ext, F32(1)), F32(0)).astype(F32)
    u = np.minimum(np.maximum(u * F32(1024), F32(0)), F32(1023))
    q = u.astype(np.uint32)
    return ((_spread10(q[:, 0]) << 2) | (_spread10(q[:, 1]) << 1) | _spread10(q[:, 2])).astype(np.uint32)


def _area32(lo, hi):
    d = hi - lo
    return (d[..., 0] * d[..., 1] + d[..., 0] * d[..., 2]) + d[..., 1] * d[..., 2]


def build_stage1(P, idx):
    """-> dict(morton_keys, child, parent_internal, parent_leaf, boxes, order: what the builder holds after sah_build; splits: one record
    per interior node for the side checks; max_level).  Node ids as the header comment of bvh_gpu.hip numbers them: the root is 0, the
    segments of the next level get consecutive ids in segment order."""
    P = np.asarray(P, F32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    n = len(idx)
    assert n >= 2
    # (the builder reduces through order-preserving integers, where -0 < +0; a restatement with min / max would need the same order)
    assert not np.any(np.signbit(P) & (P == 0)), "inputs hold no negative zero"
    tlo, thi = tri_boxes(P, idx)
    cen = F32(0.5) * tlo + F32(0.5) * thi
    keys = morton_keys(tlo, thi)
    ids = np.argsort(keys, kind="stable")
    child = np.zeros((n - 1, 2), np.uint32)
    parent_internal = np.full(n - 1, NONE, np.uint32)
    parent_leaf = np.zeros(n, np.uint32)
    boxes = np.zeros((2 * n - 1, 6), F32)
    splits = []
    segs, next_node, level = [(0, n, 0)], 1, 0
    inf = F32(np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        while segs:
            nxt = []
            for st, en, node in segs:
                seg = ids[st:en]
                m = en - st
                c = cen[seg]
                mn = c.min(0)
                ext = c.max(0) - mn
                axis = 0 if (ext[0] > ext[1] and ext[0] > ext[2]) else (1 if ext[1] > ext[2] else 2)
                c0 = mn[axis]
                scale = F32(BUCKETS) / ext[axis] if ext[axis] > 0 else F32(0)
                v = (c[:, axis] - c0) * scale
                # (int) truncates; the clamp to 0 .. 15 takes an infinite product (a denormal extent) to 15 and 0 x inf to 0, as the
                # device's saturating conversion does
                b = np.where(v >= BUCKETS, BUCKETS - 1, np.where(v > 0, v, 0)).astype(np.int32)
                cnt = np.bincount(b, minlength=BUCKETS)
                blo = np.full((BUCKETS, 3), inf, F32)
                bhi = np.full((BUCKETS, 3), -inf, F32)
                np.minimum.at(blo, b, tlo[seg])
                np.maximum.at(bhi, b, thi[seg])
                boxes[node, :3], boxes[node, 3:] = blo.min(0), bhi.max(0)  # (empty buckets hold +-inf: the union of the others)
                # suffix sweep, then prefix sweep, over the 15 planes: plane k has buckets 0 .. k on its left
                slo, shi = np.minimum.accumulate(blo[::-1], 0)[::-1][1:], np.maximum.accumulate(bhi[::-1], 0)[::-1][1:]
                cnt_r = np.cumsum(cnt[::-1])[::-1][1:]
                area_r = np.where(cnt_r > 0, _area32(slo, shi), F32(0)).astype(F32)
                plo, phi = np.minimum.accumulate(blo, 0)[:-1], np.maximum.accumulate(bhi, 0)[:-1]
                cnt_l = np.cumsum(cnt)[:-1]
                valid = (cnt_l > 0) & (cnt_r > 0)  # a plane with an empty side splits nothing
                cost = cnt_l.astype(F32) * _area32(plo, phi) + cnt_r.astype(F32) * area_r
                cost = np.where(valid, cost, inf).astype(F32)
                best = int(np.argmin(cost)) if valid.any() and cost.min() < inf else -1  # the first strictly least cost
                halved = best < 0 or level >= MEDIAN_LEVEL
                if halved:
                    nl = m // 2
                else:
                    left = b <= best
                    nl = int(cnt_l[best])
                    ids[st:en] = np.concatenate([seg[left], seg[~left]])  # stable
                splits.append({"node": node, "level": level, "count": m, "cnt": cnt, "lo": blo, "hi": bhi, "cost": cost, "valid": valid,
                               "best": best, "halved": halved, "nl": nl})
                for k, (s0, s1) in enumerate(((st, st + nl), (st + nl, en))):
                    if s1 - s0 >= 2:
                        cid = next_node + len(nxt)
                        nxt.append((s0, s1, cid))
                        child[node, k] = cid
                        parent_internal[cid] = node
                    else:
                        child[node, k] = LEAF | s0
                        parent_leaf[s0] = node
            next_node += len(nxt)
            segs = nxt
            level += 1
    assert next_node == n - 1
    boxes[n - 1:, :3], boxes[n - 1:, 3:] = tlo[ids], thi[ids]
    return {"morton_keys": keys, "child": child, "parent_internal": parent_internal, "parent_leaf": parent_leaf, "boxes": boxes,
            "order": ids.astype(np.uint32), "splits": splits, "max_level": level - 1}


def plane_costs_f64(s):
    """-> (the 15 plane costs of a split record in float64 from its float32 bucket boxes, inf where a side is empty; whether the derivation
    of PLANE_MARGIN covers the node: every product of two extents is exactly 0 or at least 2^-126, so that no float32 product underflowed --
    true of every input whose coordinates lie within [2^-20, 2^20], where a non-zero extent is at least 2^-43)"""
    lo, hi, cnt = s["lo"].astype(np.float64), s["hi"].astype(np.float64), s["cnt"]
    with np.errstate(invalid="ignore"):
        dl = np.maximum.accumulate(hi, 0)[:-1] - np.minimum.accumulate(lo, 0)[:-1]
        dr = (np.maximum.accumulate(hi[::-1], 0)[::-1] - np.minimum.accumulate(lo[::-1], 0)[::-1])[1:]
    cl, cr = np.cumsum(cnt)[:-1], np.cumsum(cnt[::-1])[::-1][1:]
    ok = (cl > 0) & (cr > 0)
    prods = np.stack([d[ok][:, i] * d[ok][:, j] for d in (dl, dr) for i, j in ((0, 1), (0, 2), (1, 2))])
    cost = np.full(BUCKETS - 1, np.inf)
    area = lambda d: (d[:, 0] * d[:, 1] + d[:, 0] * d[:, 2]) + d[:, 1] * d[:, 2]
    cost[ok] = cl[ok] * area(dl[ok]) + cr[ok] * area(dr[ok])
    return cost, bool(np.all((prods == 0) | (prods >= 2.0 ** -126)))


def check_plane_choices(splits):
    """Float64 side check of the restatement itself, over the nodes split by a plane.  -> dict(split_nodes: those the derivation covers;
    underflowed: those it does not (plane_costs_f64), left out; over_margin: nodes whose chosen plane costs more than the least float64 cost
    x (1 + PLANE_MARGIN) -- none may; not_argmin: nodes whose chosen plane is not the float64 argmin; unexplained: those of them where no
    second cost lies within the margin of the least -- none may)"""
    out = {"split_nodes": 0, "underflowed": 0, "over_margin": [], "not_argmin": [], "unexplained": []}
    for s in splits:
        if s["halved"]:
            continue
        c64, covered = plane_costs_f64(s)
        assert np.array_equal(np.isfinite(c64), s["valid"])
        if not covered:
            out["underflowed"] += 1
            continue
        out["split_nodes"] += 1
        least, k = c64.min(), s["best"]
        if not c64[k] <= least * (1.0 + PLANE_MARGIN):
            out["over_margin"].append(s["node"])
        if k != int(np.argmin(c64)):
            out["not_argmin"].append(s["node"])
            if np.count_nonzero(c64 <= least * (1.0 + PLANE_MARGIN)) < 2:
                out["unexplained"].append(s["node"])
    return out


def check_lowest_index_among_equal(splits):
    """for inputs built to tie: the chosen plane has the least float32 cost and the lowest index among the planes of that cost"""
    bad = []
    for s in splits:
        if s["halved"]:
            continue
        k, cost = s["best"], s["cost"]
        if np.any(cost < cost[k]) or np.any(cost[:k] <= cost[k]):
            bad.append(s["node"])
    return bad


def check_binary_tree(t):
    """every triangle once, parents consistent, every interior box exactly the union of its children's boxes"""
    child, boxes = t["child"], t["boxes"]
    n = len(t["order"])
    assert np.array_equal(np.sort(t["order"]), np.arange(n)), "every triangle appears once"
    kid = unified_kids(child)
    assert np.array_equal(np.sort(kid.ravel()), np.arange(1, 2 * n - 1)), "every node but the root is one node's child"
    assert t["parent_internal"][0] == NONE
    par = np.concatenate([t["parent_internal"], t["parent_leaf"]])
    for k in range(2):
        assert np.array_equal(par[kid[:, k]], np.arange(n - 1)), "parents point back"
    a, b = boxes[kid[:, 0]], boxes[kid[:, 1]]
    assert np.array_equal(boxes[:n - 1, :3], np.minimum(a[:, :3], b[:, :3])) and np.array_equal(boxes[:n - 1, 3:], np.maximum(a[:, 3:], b[:, 3:])), \
        "a box is the union of its children's"
    pre = preorder(kid)
    assert len(pre) == 2 * n - 1, "the root reaches every node"


# ---------------------------------------------------------------- shared tree helpers ----
def unified_kids(child):
    """child words -> node ids in the numbering of `boxes` (leaf of slot k = n - 1 + k)"""
    child = np.asarray(child, np.int64)
    n_int = len(child)
    return np.where(child & LEAF, n_int + (child & 0x7FFFFFFF), child)


def preorder(kid):
    """nodes in depth-first order, first child first (iterative: trees here are up to a few hundred levels deep)"""
    n_int = len(kid)
    out, st = [], [0]
    while st:
        v = st.pop()
        out.append(v)
        if v < n_int:
            st.append(int(kid[v, 1]))
            st.append(int(kid[v, 0]))
    return out


# ---------------------------------------------------------------- tail of stage 2 ----
def order_children(kid, bx):
    """reins::order_children on every interior node of the link form: child 0 = the child whose box centre is lower along the axis that
    separates the two centres most (the first axis of equal separations; equal centres stay as they are)"""
    kid = np.asarray(kid, np.int64).copy()
    bx = np.asarray(bx, F32)
    a, b = bx[kid[:, 0]], bx[kid[:, 1]]
    sa, sb = a[:, :3] + a[:, 3:], b[:, :3] + b[:, 3:]  # (twice the centres, in float32 as the kernel adds them)
    ax = np.argmax(np.abs(sa - sb), 1)  # `ad > sep` from sep = -1: the first of the largest
    rows = np.arange(len(kid))
    swap = sa[rows, ax] > sb[rows, ax]
    kid[swap] = kid[swap][:, ::-1]
    return kid


def reinsert_tail(par, kid, bx, order):
    """The link form after the passes -> the builder's arrays as `reinsert` hands them on: order_children, the leaves renumbered
    depth-first, boxes and leaf order carried along."""
    bx = np.asarray(bx, F32)
    n_int = len(kid)
    n = n_int + 1
    assert len(par) == 2 * n - 1 and par[0] == NONE and np.array_equal(np.asarray(par)[np.asarray(kid, np.int64).ravel()], np.repeat(np.arange(n_int), 2))
    kid = order_children(kid, bx)
    rows = np.arange(n_int)
    newslot = np.zeros(n, np.int64)
    leaves = [v - n_int for v in preorder(kid) if v >= n_int]
    newslot[leaves] = np.arange(n)
    is_leaf = kid >= n_int
    child = np.where(is_leaf, LEAF | newslot[np.where(is_leaf, kid - n_int, 0)], kid).astype(np.uint32)
    parent_internal = np.full(n_int, NONE, np.uint32)
    parent_leaf = np.zeros(n, np.uint32)
    for k in range(2):
        i, l = rows[~is_leaf[:, k]], rows[is_leaf[:, k]]
        parent_internal[kid[i, k]] = i
        parent_leaf[newslot[kid[l, k] - n_int]] = l
    boxes = bx.copy()
    boxes[n_int + newslot] = bx[n_int:]
    order_out = np.zeros(n, np.uint32)
    order_out[newslot] = order
    return {"child": child, "parent_internal": parent_internal, "parent_leaf": parent_leaf, "boxes": boxes, "order": order_out}


# ---------------------------------------------------------------- stage 3 ----
def cell_size(ext32):
    """The cell of a quad node's 8-bit grid along an axis of float32 extent `ext32`: the smallest power of two with 255 cells covering it,
    2^-126 at least.  This DEFINES the grid (the quantiser uses the same statement), so it is taken in float32 as the builder takes it:
    frexp of the float32 quotient extent / 255."""
    ext32 = np.asarray(ext32, F32)
    _, e = np.frexp((ext32 / F32(255)).astype(F32))
    e = np.where(ext32 > 0, np.maximum(e, -126), -126)
    return np.ldexp(1.0, e)


def area_on_grid_f64(box, qbox):
    """the (half) surface area of `box` as the grid of a quad node with box `qbox` holds it, about one cell wider per axis: float64 from
    the float32 boxes ([..., 6])"""
    box, qbox = np.asarray(box, F32), np.asarray(qbox, F32)
    dd = (box[..., 3:].astype(np.float64) - box[..., :3].astype(np.float64)) + cell_size(qbox[..., 3:] - qbox[..., :3])
    return (dd[..., 0] * dd[..., 1] + dd[..., 0] * dd[..., 2]) + dd[..., 1] * dd[..., 2]


def _ancestors(kid):
    """anc[d - 1][v] = the ancestor of node v at distance d, the root at most (the root's own ancestor is the root)"""
    n_int = len(kid)
    par = np.zeros(2 * n_int + 1, np.int64)
    for k in range(2):
        par[kid[:, k]] = np.arange(n_int)
    a1 = par
    a2 = par[a1]
    return [a1, a2, par[a2]]


def dp_tables_f64(child, boxes):
    """The recurrence of quad_encode.hpp's header comment over a binary tree of one-triangle leaves, in float64.  With R the ancestor at
    binary distance d = 1 .. 3 of node v (the root at most) and Aq(v, R) = area_on_grid_f64:
      F(v, k, d) = min( Aq(v, R) x 2 for a leaf, Aq(v, R) + G(v) for an interior node;
                        for an interior node with k >= 2 and d < 3: min over k1 + k2 = k of F(l, k1, d + 1) + F(r, k2, d + 1) )
      G(v)       = min over k1 + k2 = 4 of F(l, k1, 1) + F(r, k2, 1)
    -> dict(F[2 n - 1, 4, 3], G[n - 1], nodes[2 n - 1] = nodes in the subtree of v)"""
    kid = unified_kids(child)
    n_int = len(kid)
    nn = 2 * n_int + 1
    boxes = np.asarray(boxes, F32)
    anc = _ancestors(kid)
    Aq = np.stack([area_on_grid_f64(boxes, boxes[anc[d]]) for d in range(3)], 1)  # [nn, 3]
    F = np.zeros((nn, 4, 3))
    F[n_int:] = (TRI_COST * Aq[n_int:])[:, None, :]
    G = np.zeros(n_int)
    nodes = np.ones(nn, np.int64)
    for v in reversed(preorder(kid)):
        if v >= n_int:
            continue
        l, r = int(kid[v, 0]), int(kid[v, 1])
        nodes[v] = 1 + nodes[l] + nodes[r]
        Fl, Fr = F[l], F[r]
        G[v] = min(Fl[k1 - 1, 0] + Fr[3 - k1, 0] for k1 in (1, 2, 3))
        for d in (1, 2, 3):
            one = Aq[v, d - 1] + G[v]
            F[v, :, d - 1] = one
            if d < 3:
                for k in (2, 3, 4):
                    F[v, k - 1, d - 1] = min(one, min(Fl[k1 - 1, d] + Fr[k - k1 - 1, d] for k1 in range(1, k)))
    return {"F": F, "G": G, "nodes": nodes}


def quad_tree_work_f64(quads, child, boxes):
    """The expected work, as the recurrence counts it, of a GIVEN quad tree over the binary tree it was collapsed from: per quad node R (a
    binary interior node), the sum over its children c of Aq(c, R) x 2 for a triangle and Aq(c, R) + work(c) for a quad node.  Which
    binary node a quad node is: the root is node 0; a child is found by its leaf set (a leaf child names its slot; a binary node's leaves
    are consecutive slots in the trees the builder makes, asserted here).  Every child must lie 1 .. 3 binary levels below its quad node
    and the children's leaves must be the node's leaves.  -> (work of the root, quad nodes reached)"""
    quads = np.asarray(quads, np.uint32).reshape(-1, 16)
    kid = unified_kids(child)
    n_int = len(kid)
    boxes = np.asarray(boxes, F32)
    anc1 = _ancestors(kid)[0]
    first = np.zeros(2 * n_int + 1, np.int64)
    count = np.ones(2 * n_int + 1, np.int64)
    first[n_int:] = np.arange(n_int + 1)
    for v in reversed(preorder(kid)):
        if v < n_int:
            l, r = kid[v]
            first[v], count[v] = min(first[l], first[r]), count[l] + count[r]
            assert max(first[l] + count[l], first[r] + count[r]) - first[v] == count[v], "a node's leaves are consecutive slots"
    node_of_range = {(int(first[v]), int(count[v])): v for v in range(2 * n_int + 1)}
    refs = quads[:, 12:16].astype(np.int64)
    # the quad tree top-down (which quads exist), then its leaf ranges bottom-up
    order, st = [], [0]
    while st:
        q = st.pop()
        order.append(q)
        st.extend(int(r) // 64 for r in refs[q] if not r & LEAF)
    assert len(set(order)) == len(order), "a quad node has one parent"
    qfirst, qcount = {}, {}
    for q in reversed(order):
        los, cnt = [], 0
        for r in refs[q]:
            if r & LEAF:
                if (r >> 24) & 0x7F:
                    assert (r >> 24) & 0x7F == 1
                    los.append(int(r & 0xFFFFFF))
                    cnt += 1
            else:
                los.append(qfirst[int(r) // 64])
                cnt += qcount[int(r) // 64]
        qfirst[q], qcount[q] = min(los), cnt
    node_of_quad = {0: 0}
    for q in order:
        b = node_of_quad[q]
        assert (qfirst[q], qcount[q]) == (int(first[b]), int(count[b])), "a quad node's children hold its binary node's leaves"
        for r in refs[q]:
            if not r & LEAF:
                c = int(r) // 64
                node_of_quad[c] = node_of_range[(qfirst[c], qcount[c])]
    work = {}
    for q in reversed(order):
        b = node_of_quad[q]
        w = 0.0
        for r in refs[q]:
            if r & LEAF:
                if not (r >> 24) & 0x7F:
                    continue
                v, below = n_int + int(r & 0xFFFFFF), None
            else:
                v, below = node_of_quad[int(r) // 64], work[int(r) // 64]
            up, steps = v, 0
            while up != b and steps < 3:
                up, steps = int(anc1[up]), steps + 1
            assert up == b and steps >= 1, "a child lies one to three binary levels below its quad node"
            a = float(area_on_grid_f64(boxes[v], boxes[b]))
            w += TRI_COST * a if below is None else a + below
        work[q] = w
    return work[0], len(order)
