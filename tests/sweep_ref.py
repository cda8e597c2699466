"""The sphere-sweep query (include/rtbvh.h rtbvh_sweep_*) restated in numpy float32.

A helper of the sweep tests, not a test.  Written from the header: a scene triangle is what its leaf record holds
(nearest_ref.leaf_data: a, e1 = fl(p1 - p0), e2 = fl(p2 - p0) and the leaf box), every operation is one float32
rounding in the header's order -- dots `(a*b + c*d) + e*f`, no fused multiply-add (numpy rounds every product),
np.fmin / np.fmax where the header says fminf / fmaxf, `/` and np.sqrt the IEEE results.  A sweep's answer is the
brute force over ALL triangles: x is a member iff (B) its leaf box grown by r passes the all-hits box rule
(ray_walk_ref._box and `!(mn > t_max)`) and (T) the start overlap (nearest_ref.tri_dist2) or one of the seven
candidates yields a t; the result is the member with the smallest (tk bits, triangle id), tk = fmax(t, mn) + 0.
No tree -- except walk(), the plain-Python pruned walk of the lemma over the oracle's tree.
"""
import numpy as np

from tests import nearest_ref as nr
from tests import ray_walk_ref as rw

NONE = np.uint32(0xFFFFFFFF)
INF = np.float32(np.inf)
SWEEP_HIT_DTYPE = np.dtype([("t", "<f4"), ("point", "<f4", (3,)), ("tri", "<u4"), ("feature", "<u4"),
                            ("reserved", "<u4", (2,))])
F0, F1 = np.float32(0), np.float32(1)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return tuple(a[k] - b[k] for k in range(3))


def _add(a, b):
    return tuple(a[k] + b[k] for k in range(3))


def _mul(a, s):
    return tuple(a[k] * s for k in range(3))


def _cols(x):
    return tuple(np.ascontiguousarray(x[..., k]) for k in range(3))


def walked(c, d, r, t_max):
    """The sweeps that are walked at all: finite c and d, d not all zero, 0 <= r < inf, t_max >= 0."""
    with np.errstate(all="ignore"):
        return (np.isfinite(c).all(1) & np.isfinite(d).all(1) & (d != 0).any(1) & (r >= 0) & (r < INF) & (t_max >= 0))


def face(c, d, r, a, e1, e2):
    """The face candidate of (K,) pairs (tuples of three (K,) float32 columns): (counts, t, point)."""
    n = _cross(e1, e2)
    nn = _dot(n, n)
    ok = nn > 0
    s = _dot(n, _sub(c, a))
    neg = s < 0
    n = tuple(np.where(neg, -n[k], n[k]) for k in range(3))
    s = np.where(neg, -s, s)
    ln = np.sqrt(nn)
    h = s - r * ln
    dn = _dot(n, d)
    ok &= (dn < 0) & (h >= 0)
    t = h / (-dn)
    p = _sub(_add(c, _mul(d, t)), _mul(n, r / ln))
    ap = _sub(p, a)
    d1, d2 = _dot(e1, ap), _dot(e2, ap)
    e11, e12, e22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
    den = e11 * e22 - e12 * e12
    u = (e22 * d1 - e12 * d2) / den
    v = (e11 * d2 - e12 * d1) / den
    ok &= (u >= 0) & (v >= 0) & (u + v <= 1)
    return ok, t, p


def edge(c, d, dd, r, A, E):
    m = _sub(c, A)
    ee, md, nd, mm, mdd = _dot(E, E), _dot(m, E), _dot(d, E), _dot(m, m), _dot(m, d)
    a_ = ee * dd - nd * nd
    k = mm - r * r
    c_ = ee * k - md * md
    b_ = ee * mdd - nd * md
    ok = (a_ > 0) & (c_ > 0) & (b_ < 0)
    disc = b_ * b_ - a_ * c_
    ok &= disc >= 0
    t = c_ / (np.sqrt(disc) - b_)
    s_ = md + t * nd
    ok &= (0 <= s_) & (s_ <= ee)
    return ok, t, _add(A, _mul(E, s_ / ee))


def vertex(c, d, dd, r, V):
    m = _sub(c, V)
    b = _dot(m, d)
    cc = _dot(m, m) - r * r
    ok = (cc > 0) & (b < 0)
    disc = b * b - dd * cc
    ok &= disc >= 0
    return ok, cc / (np.sqrt(disc) - b), V


def pair_tests(leaves, tri, c, d, r, t_max):
    """Sweep k against triangle tri[k], `leaves` = nearest_ref.leaf_data(tris): (member, t, point (K, 3), feature,
    mn).  Where there is no t: t = -1, point = 0, feature = 0."""
    a, e1, e2, lo, hi = (x[tri] for x in leaves)
    K = len(tri)
    with np.errstate(all="ignore"):
        r = (r + F0).astype(np.float32)
        t_max = (t_max + F0).astype(np.float32)
        inv = (F1 / d).astype(np.float32)
        box, mn = rw._box(lo - r[:, None], hi + r[:, None], c, inv)
        box &= ~(mn > t_max)
        dist2, _, _, q = nr.tri_dist2(c, a, e1, e2, lo, hi)
        start = dist2 <= r * r
        cc, dc, ac, e1c, e2c = _cols(c), _cols(d), _cols(a), _cols(e1), _cols(e2)
        dd = _dot(dc, dc)
        v1, v2 = _add(ac, e1c), _add(ac, e2c)
        cands = [face(cc, dc, r, ac, e1c, e2c),
                 edge(cc, dc, dd, r, ac, e1c), edge(cc, dc, dd, r, ac, e2c), edge(cc, dc, dd, r, v1, _sub(e2c, e1c)),
                 vertex(cc, dc, dd, r, ac), vertex(cc, dc, dd, r, v1), vertex(cc, dc, dd, r, v2)]
        feature = np.zeros(K, np.uint32)
        t = np.zeros(K, np.float32)
        pt = np.zeros((K, 3), np.float32)
        for k, (ok, tc, pc) in enumerate(cands):
            take = ok & (0 <= tc) & (tc <= t_max) & ((feature == 0) | (tc < t))   # the first smallest
            feature[take] = 2 + k
            t[take] = tc[take]
            pt[take] = np.stack(np.broadcast_arrays(*pc), -1)[take]
        feature[start], t[start], pt[start] = 1, 0, q[start]
        pt = np.fmax(lo, np.fmin(hi, pt))
        ok = box & (feature != 0) & walked(c, d, r, t_max)
        none = feature == 0
        t[none], pt[none] = -1, 0
    return ok, t.astype(np.float32), pt.astype(np.float32), feature, mn.astype(np.float32)


def key_t(t, mn):
    """tk of each member: fmax drops a NaN, as fmaxf does; + 0 makes +0 of a -0."""
    with np.errstate(all="ignore"):
        return (np.fmax(t, mn) + F0).astype(np.float32)


def keys(t, mn, tri):
    """The uint64 keys tk bits << 32 | tri: tk >= +0, so the bits order as the floats."""
    return rw.bits(key_t(t, mn)).astype(np.uint64) << np.uint64(32) | np.asarray(tri).astype(np.uint64)


def misses(n):
    out = np.zeros(n, SWEEP_HIT_DTYPE)
    out["t"], out["tri"] = -1, NONE
    return out


def members(tris, origins, directions, radius, t_max=INF, chunk=1 << 20):
    """Every member of every sweep, over ALL triangles, in (sweep, triangle id) order: a dict of flat arrays i (the
    sweep), tri, t, point, feature, mn, and n and T.  ((B) is evaluated for every pair, (T) for the pairs that
    pass it: a pair that fails (B) is no member whatever (T) says.)"""
    c = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    n, T = len(c), len(tris)
    r = np.broadcast_to(np.asarray(radius, np.float32), (n,)).copy()
    tm = np.broadcast_to(np.asarray(t_max, np.float32), (n,)).copy()
    leaves = nr.leaf_data(tris)
    lo, hi = leaves[3], leaves[4]
    parts = []
    step = max(1, chunk // max(T, 1))
    with np.errstate(all="ignore"):
        rr, tt = (r + F0).astype(np.float32), (tm + F0).astype(np.float32)
        inv = (F1 / d).astype(np.float32)
    for s in range(0, n, step):
        m = len(c[s:s + step])
        k = np.repeat(np.arange(s, s + m), T)
        tri = np.tile(np.arange(T), m)
        with np.errstate(all="ignore"):
            box, mn = rw._box(lo[tri] - rr[k, None], hi[tri] + rr[k, None], c[k], inv[k])
            box &= ~(mn > tt[k])
        k, tri = k[box], tri[box]
        ok, t, pt, f, mn = pair_tests(leaves, tri, c[k], d[k], r[k], tm[k])
        parts.append((k[ok], tri[ok], t[ok], pt[ok], f[ok], mn[ok]))
    cat = [np.concatenate(x) for x in zip(*parts)] if parts else [np.zeros(0, np.int64)] * 2 + [
        np.zeros(0, np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), np.zeros(0, np.float32)]
    return dict(zip(("i", "tri", "t", "point", "feature", "mn"), cat), n=n, T=T)


def records(mem, sel):
    """The member records mem[sel] as SWEEP_HIT_DTYPE."""
    out = misses(len(mem["i"][sel]))
    out["t"], out["point"], out["tri"], out["feature"] = (mem["t"][sel], mem["point"][sel], mem["tri"][sel],
                                                          mem["feature"][sel])
    return out


def find(mem, i, tri):
    """The positions in members()' lists of the pairs (i[k], tri[k]), -1 where the pair is no member."""
    flat = mem["i"].astype(np.int64) * max(mem["T"], 1) + mem["tri"]
    want = np.asarray(i, np.int64) * max(mem["T"], 1) + np.asarray(tri, np.int64)
    at = np.searchsorted(flat, want)
    at[at >= len(flat)] = 0
    return np.where(flat[at] == want, at, -1) if len(flat) else np.full(len(want), -1)


def select(mem):
    """The answer from members(): the member with the smallest (tk bits, id) of each sweep, or the miss record."""
    out = misses(mem["n"])
    key = keys(mem["t"], mem["mn"], mem["tri"])
    order = np.lexsort((key, mem["i"]))
    i = mem["i"][order]
    first = np.ones(len(i), bool)
    first[1:] = i[1:] != i[:-1]
    out[i[first]] = records(mem, order[first])
    return out


def brute(tris, origins, directions, radius, t_max=INF):
    return select(members(tris, origins, directions, radius, t_max))


def hit_words(hits):
    """(m, 8) uint32: the record's eight words (bit-exact comparisons)."""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 8)


def node_tests(nodes, c, d, r, relaxed=True):
    """(base, mn) of every node of the oracle's tree for one sweep: the first two slab conditions and the slab entry
    of the node's box grown by r.  The leaves [0, n) by (B) as written; the internal nodes, with `relaxed`, without
    the axes whose 1 / d is infinite (a NaN inv drops the axis out of mn and mx; with none left the node is
    entered), as the header's walk."""
    N = len(nodes)
    n = (N + 1) // 2
    rep = lambda x: np.repeat(np.asarray(x, np.float32)[None], N, 0)   # noqa: E731
    with np.errstate(all="ignore"):
        inv = (F1 / rep(d)).astype(np.float32)
        if relaxed:
            inv[n:] = np.where(np.isinf(inv[n:]), np.float32(np.nan), inv[n:])
        base, mn = rw._box(nodes["bb_min"] - np.float32(r), nodes["bb_max"] + np.float32(r), rep(c), inv)
        if relaxed and np.isnan(inv[n:]).all():   # no axis left (|d| below 2^-128 on all three): every child is entered
            base[n:], mn[n:] = True, -INF
        return base, mn


def walk(nodes, base, mn, ok, tk, tri, tmax, prune=True):
    """The walk of rtbvh_sweep_* for one sweep, in plain Python, over the oracle's tree (leaves [0, n), node n the
    root): base[x] says whether node x's box, grown by r, passes the first two slab conditions, mn[x] is its slab
    entry (node_tests: a leaf's own box by (B), an internal node's without the axes of an infinite 1 / d); ok[j] whether leaf j's triangle has a t within t_max, tk[j] its key's float, tri[j] its id (float32
    values as Python floats compare as the floats do).  The best (tk, id, leaf) starts at (tmax, NONE); a child's
    box, and a leaf's own at the leaf, is entered iff base and not mn > the best tk; the nearer child first, left on
    a tie.  prune = False keeps the bound at tmax.  Returns the best (or None) and the leaves visited."""
    n = (len(nodes) + 1) // 2
    best, leaves = (tmax, int(NONE), -1), 0
    cl, cr = nodes["child_l"], nodes["child_r"]

    def enter(x):
        return base[x] and not mn[x] > (best[0] if prune else tmax)

    stack = [n if n > 1 else 0]
    while stack:
        x = stack.pop()
        if x < n:   # a leaf
            leaves += 1
            if enter(x) and ok[x]:
                cand = (tk[x], tri[x], x)
                if cand[:2] < best[:2]:
                    best = cand
            continue
        l, r = int(cl[x]), int(cr[x])
        lh, rh = enter(l), enter(r)
        if lh and rh:
            stack.extend((l, r) if mn[r] < mn[l] else (r, l))   # the nearer one on top
        elif lh or rh:
            stack.append(l if lh else r)
    return (best if best[2] >= 0 else None), leaves
