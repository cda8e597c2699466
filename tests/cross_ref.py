"""The triangle query (include/rtbvh.h rtbvh_cross_*) restated in numpy.

A helper of the triangle-query tests, not a test.  A query triangle q is reduced to what a leaf record would hold of
it -- tests/nearest_ref.leaf_data of the query triangles: a, e1 = v1 - v0, e2 = v2 - v0 and the box of its vertices --
and scene triangle x is a member of q iff (B) the closed-interval test of the two boxes holds
(tests/overlap_ref.boxes_meet) and (X) one of the six segment-triangle tests does (tests/collide_ref.segments and
segment_crosses, unchanged).  The list of a query is the brute force over ALL scene triangles ordered by
`rank[triangle]`, the triangle's position in the build's sort order.  No tree.  A query with a non-finite vertex
component has an empty list.

`dtype=np.float64` evaluates (X) in double precision (the sanity check of test_cross_cpu.py).
"""
import numpy as np

from tests import collide_ref as cr
from tests import nearest_ref as nr
from tests import overlap_ref as ovr

NONE = np.uint32(0xFFFFFFFF)


def valid_queries(queries):
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 9)
    return np.isfinite(q).all(-1)


def crosses(k, j, qleaf, leaf):
    """(X) for the pairs (query k[i], scene triangle j[i]); qleaf, leaf: (a, e1, e2) in the dtype to evaluate in."""
    qa, qe1, qe2 = qleaf
    a, e1, e2 = leaf
    out = np.zeros(len(k), bool)
    for P, D in cr.segments(qa[k], qe1[k], qe2[k]):
        out |= cr.segment_crosses(P, D, a[j], e1[j], e2[j])
    for P, D in cr.segments(a[j], e1[j], e2[j]):
        out |= cr.segment_crosses(P, D, qa[k], qe1[k], qe2[k])
    return out


def member_pairs(tris, queries, dtype=np.float32, order=None, stages=None, chunk=1 << 22):
    """(k, j): the (query, scene triangle) member pairs, row-major -- by query, then by the triangle's place in
    `order` (default: id order); j indexes `order`.  `stages`, a list, receives the pair counts after (B) and (X)."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3, 3)
    walk = valid_queries(q)
    qs = np.where(walk[:, None, None], q, np.float32(0))       # (the unwalked ones: any finite stand-in)
    qlo, qhi = nr.leaf_data(qs)[3:]
    lo, hi = nr.leaf_data(tris)[3:]
    leaf = list(nr.leaf_data(tris, dtype)[:3])
    if order is not None:
        lo, hi = lo[order], hi[order]
        leaf = [x[order] for x in leaf]
    qleaf = nr.leaf_data(qs, dtype)[:3]
    T, n = len(lo), len(q)
    ks, js = [], []
    step = max(1, chunk // max(T, 1))
    for s in range(0, n, step):
        ok = ovr.boxes_meet(qlo[s:s + step, None], qhi[s:s + step, None], lo[None], hi[None]) & walk[s:s + step, None]
        k, j = np.nonzero(ok)
        ks.append(k + s)
        js.append(j)
    k, j = (np.concatenate(ks), np.concatenate(js)) if ks else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    nb = len(k)
    if nb:
        keep = crosses(k, j, qleaf, leaf)
        k, j = k[keep], j[keep]
    if stages is not None:
        stages[:] = [nb, len(k)]
    return k, j


def brute_cross(tris, queries, rank, stages=None):
    """(offsets uint64 (n + 1,), ids uint32): every member of every query, each list ascending by rank[triangle]."""
    n = len(np.ascontiguousarray(queries, np.float32).reshape(-1, 9))
    order = np.argsort(np.asarray(rank, np.int64), kind="stable")     # the triangles in sort order
    k, j = member_pairs(tris, queries, order=order, stages=stages)
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(np.bincount(k, minlength=n).astype(np.uint64), out=offsets[1:])
    return offsets, order[j].astype(np.uint32)


def first_of(offsets, ids):
    """rtbvh_cross_first's answer from the lists: each list's head, or 0xFFFFFFFF."""
    off = np.asarray(offsets).astype(np.int64)
    out = np.full(len(off) - 1, NONE, np.uint32)
    has = off[1:] > off[:-1]
    out[has] = ids[off[:-1][has]]
    return out


def without_neighbours(offsets, ids, indices):
    """The lists of a scene's own triangles as queries (query k = scene triangle k) with the entries that share a
    vertex index with their query removed, x = k among them: (offsets, ids)."""
    off = np.asarray(offsets).astype(np.int64)
    n = len(off) - 1
    owner = np.repeat(np.arange(n), np.diff(off))
    keep = ~cr.neighbours(indices, owner, ids.astype(np.int64))
    out = np.zeros(n + 1, np.uint64)
    np.cumsum(np.bincount(owner[keep], minlength=n).astype(np.uint64), out=out[1:])
    return out, ids[keep]


def shape_of(offsets):
    """[members, empty lists, lists of >= 2, longest list] of CSR offsets."""
    cnt = np.diff(np.asarray(offsets).astype(np.int64))
    return [int(cnt.sum()), int((cnt == 0).sum()), int((cnt >= 2).sum()), int(cnt.max())]


# [members, empty lists, lists of >= 2, longest list] of random_queries against the golden scenes under the identity
# camera, from this reference alone
IDENTITY_COUNTS = {"Rect": [131, 402, 20, 3], "Test": [159, 441, 30, 21], "Image_Test": [446, 402, 77, 15]}


def random_queries(tris, n=512, seed=7):
    """The tests' random query triangles, (n, 3, 3) float32: centres uniform in the mesh's box, vertices within
    `scale` times the box's extent about them; scale is 0.5 for every fourth query and 0.08 for the others."""
    lo, hi = nr.root_box(tris)
    ext = hi - lo
    rng = np.random.default_rng(seed)
    centre = lo + rng.random((n, 1, 3)) * ext
    scale = np.where(np.arange(n) % 4 == 0, 0.5, 0.08)[:, None, None]
    return (centre + (rng.random((n, 3, 3)) - 0.5) * ext * scale).astype(np.float32)


# ---------------------------------------------------------------- the exact-touching scene of the tests
def touching_case():
    """(vertices, indices, queries, members): collide_ref.crossing_quads' flat quad in z = 0 (two triangles, the
    diagonal along y = x) and two queries.  The first has a vertex exactly at (0.5, -0.25, 0), an interior point of
    the triangle below the diagonal (triangle 0), and the other two above it: it is a member of exactly that
    triangle.  The second is the first lifted by 2^-20: a member of nothing.  All coordinates are exact in fp32 and
    the plane is z = 0, so U, V, N and det of the deciding test are exact."""
    v, idx = cr.crossing_quads()
    v, idx = v[:4], idx[:6]
    q = np.array([[0.5, -0.25, 0.0], [0.75, -0.25, 0.5], [0.5, 0.0, 0.5]], np.float32)
    lifted = q.copy()
    lifted[:, 2] += np.float32(2.0 ** -20)
    return v, idx, np.stack([q, lifted]), [[0], []]


# ---------------------------------------------------------------- the deep tree's and the special queries
def fan_queries(n=12):
    """Query triangles cut across the window of collide_ref.thick_fan(): each stands on the fan's diagonal, spans
    the window's z and crosses the v0-v1 edge of nearly every fan triangle, so its walk passes the box test of both
    children level after level (test_cross_cpu.py: stack entries past 16, subtrees lost at a limit of 8)."""
    from tests import deep_scenes as ds
    P, R = ds.P, ds.R
    qs = []
    for i in range(n):
        f = 0.1 + 0.8 * i / (n - 1)                 # where along the diagonal
        cx, cy = P[0] + R * (f - 0.5), P[1] + R * (f - 0.5)
        w = R * (0.2 + 0.05 * i)
        qs.append([(cx - w, cy + w, -0.2 + 0.01 * i), (cx + w, cy - w, -0.2 + 0.02 * i), (cx, cy, 0.45 - 0.02 * i)])
    return np.array(qs, np.float32)


def special_queries(tris):
    """(queries, names): a NaN and an infinite vertex component (no walk), a point triangle (all e = 0: det = 0 in
    every test), two needles (v2 = v0: their own plane has det = 0, their edge still crosses triangles), one
    triangle across the whole mesh box in a slightly tilted plane y = const, and a plain one."""
    lo, hi = nr.root_box(tris)
    c, ext = (lo + hi) / 2, hi - lo
    plain = random_queries(tris, 4)[0]
    nan, inf = plain.copy(), plain.copy()
    nan[1, 2] = np.nan
    inf[2, 0] = -np.inf
    point = np.repeat(tris[5, :1], 3, 0)
    needle = np.array([lo, hi, lo], np.float32)
    m = tris[7].mean(0)
    short = np.array([m - ext * 0.1, m + ext * 0.1, m - ext * 0.1], np.float32)
    y = lo[1] + 0.4 * ext[1]
    span = np.array([[lo[0], y + 0.02 * ext[1], lo[2]], [hi[0], y - 0.02 * ext[1], lo[2]], [c[0], y, hi[2]]], np.float32)
    names = ["NaN", "infinite", "point", "needle", "short needle", "spanning", "plain"]
    return np.stack([nan, inf, point, needle, short, span, plain]).astype(np.float32), names
