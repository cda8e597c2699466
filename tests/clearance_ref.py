"""The clearance query (include/rtbvh.h rtbvh_clearance_*) restated in numpy.

A helper of the clearance tests, not a test.  A query triangle q is reduced to what a leaf record would hold of it
(tests/nearest_ref.leaf_data: a, e1, e2 and the box of its vertices), as a scene triangle x is.  The distance of the
pair is the first smallest of the header's fifteen candidates -- six vertex-triangle ones through
tests/nearest_ref.tri_dist2, unchanged, and nine segment-segment ones over tests/collide_ref.segments -- each a pair
of points clamped into the two boxes, and +0 where the triangle query's (B) and (X) hold
(tests/overlap_ref.boxes_meet, tests/collide_ref.segment_crosses).  Operation order is the kernels': left-to-right
dots `(a*b + c*d) + e*f`, every product rounded (numpy never fuses), np.fmin / np.fmax where the header says fminf /
fmaxf.  The answer of a query is the brute force over ALL scene triangles, keyed (dist2, triangle id): no tree.

`dtype=np.float64` evaluates the same formulas in double precision (the sanity bound of test_clearance_cpu.py).
"""
import numpy as np

from tests import collide_ref as cr
from tests import nearest_ref as nr
from tests import overlap_ref as ovr

NONE = 0xFFFFFFFF


def _c(x):
    return x[..., 0], x[..., 1], x[..., 2]


def _v(c):
    return np.stack(np.broadcast_arrays(*c), -1)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _clamp01(x):
    # fminf(fmaxf(x, 0), 1): a NaN becomes 0
    return np.fmin(np.fmax(x, x.dtype.type(0)), x.dtype.type(1))


def _clamp(lo, hi, p):
    return tuple(np.fmax(lo[k], np.fmin(hi[k], p[k])) for k in range(3))


def leaf(tris, dtype=np.float32):
    """(a, e1, e2, lo, hi), each (..., 3), of (..., 3, 3) float32 triangles: nearest_ref.leaf_data for any leading
    shape."""
    t = np.asarray(tris, np.float32)
    lo = np.fmin(np.fmin(t[..., 0, :], t[..., 1, :]), t[..., 2, :])
    hi = np.fmax(np.fmax(t[..., 0, :], t[..., 1, :]), t[..., 2, :])
    t = t.astype(dtype)
    return t[..., 0, :], t[..., 1, :] - t[..., 0, :], t[..., 2, :] - t[..., 0, :], lo.astype(dtype), hi.astype(dtype)


def segment_pair(P1, D1, P2, D2):
    """The header's closest points of two segments, on component tuples: (cq, cx) before the box clamps."""
    f = P1[0].dtype.type
    r = tuple(P1[k] - P2[k] for k in range(3))
    A, E, F, C, B = _dot(D1, D1), _dot(D2, D2), _dot(D2, r), _dot(D1, r), _dot(D1, D2)
    den = A * E - B * B
    s = np.where(den > 0, _clamp01((B * F - C * E) / den), f(0))
    t = (B * s + F) / E
    s = np.where(t < 0, _clamp01(-C / A), np.where(t > 1, _clamp01((B - C) / A), s))
    t = _clamp01(t)
    return tuple(P1[k] + D1[k] * s for k in range(3)), tuple(P2[k] + D2[k] * t for k in range(3))


def vertices(a, e1, e2):
    """V0, V1, V2 of a record."""
    return [a, a + e1, a + e2]


def candidates(ql, xl):
    """The fifteen (d, cq, cx) of broadcastable leaf data (a, e1, e2, lo, hi), in the header's order; cq, cx are
    component tuples."""
    qa, qe1, qe2, qlo, qhi = ql
    a, e1, e2, lo, hi = xl
    cqlo, cqhi, clo, chi = _c(qlo), _c(qhi), _c(lo), _c(hi)
    raw = []
    with np.errstate(all="ignore"):
        for V in vertices(qa, qe1, qe2):
            raw.append((_c(V), _c(nr.tri_dist2(V, a, e1, e2, lo, hi)[3])))
        for V in vertices(a, e1, e2):
            raw.append((_c(nr.tri_dist2(V, qa, qe1, qe2, qlo, qhi)[3]), _c(V)))
        for P1, D1 in cr.segments(qa, qe1, qe2):
            for P2, D2 in cr.segments(a, e1, e2):
                raw.append(segment_pair(_c(P1), _c(D1), _c(P2), _c(D2)))
        out = []
        for cq, cx in raw:
            cq, cx = _clamp(cqlo, cqhi, cq), _clamp(clo, chi, cx)
            e = tuple(cq[k] - cx[k] for k in range(3))
            out.append((_dot(e, e), cq, cx))
    return out


def feature_dist2(ql, xl):
    """(dist2, cq, cx, which) of the first candidate with the smallest d (strict <; a NaN never wins): the pair's
    distance without the override."""
    best = bq = bx = which = None
    for i, (d, cq, cx) in enumerate(candidates(ql, xl)):
        if best is None:
            best, bq, bx, which = d, _v(cq), _v(cx), np.zeros(d.shape, np.int8)
            continue
        with np.errstate(all="ignore"):
            take = (d < best) | np.isnan(best)
        best = np.where(take, d, best)
        bq, bx = np.where(take[..., None], _v(cq), bq), np.where(take[..., None], _v(cx), bx)
        which = np.where(take, np.int8(i), which)
    return best, bq, bx, which


def crossing(ql, xl):
    """The triangle query's (B) and (X) of broadcastable leaf data: the pairs whose dist2 is +0 by the override."""
    shape = np.broadcast_shapes(*(x.shape for x in ql + xl))
    ql, xl = [np.broadcast_to(x, shape) for x in ql], [np.broadcast_to(x, shape) for x in xl]
    out = ovr.boxes_meet(ql[3], ql[4], xl[3], xl[4])
    idx = np.nonzero(out)
    if len(idx[0]):
        q3, x3 = [x[idx] for x in ql[:3]], [x[idx] for x in xl[:3]]
        hit = np.zeros(len(idx[0]), bool)
        with np.errstate(all="ignore"):
            for P, D in cr.segments(*q3):
                hit |= cr.segment_crosses(P, D, *x3)
            for P, D in cr.segments(*x3):
                hit |= cr.segment_crosses(P, D, *q3)
        out = out.copy()
        out[idx] = hit
    return out


def pair_dist2(q, x, dtype=np.float32, override=True):
    """(dist2, point_q, point_x) of the pairs of broadcastable (..., 3, 3) float32 triangles q (query) and x (scene),
    in `dtype`."""
    ql, xl = leaf(q, dtype), leaf(x, dtype)
    d, cq, cx, _ = feature_dist2(ql, xl)
    if override:
        d = np.where(crossing(ql, xl), dtype(0), d)
    return d, cq, cx


def bb(q, lo, hi):
    """The header's box-box distance of the boxes of (..., 3, 3) query triangles and broadcastable boxes [lo, hi]."""
    qlo, qhi = leaf(q)[3:]
    with np.errstate(all="ignore"):
        d = np.fmax(np.fmax(lo - qhi, qlo - hi), np.float32(0))
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def valid_queries(queries):
    return np.isfinite(np.ascontiguousarray(queries, np.float32).reshape(-1, 9)).all(-1)


def matrix(tris, queries, dtype=np.float32, override=True, chunk=1 << 18):
    """dist2 of every (query, scene triangle) pair, (n, T) in `dtype`; queries that are not walked get finite
    stand-ins."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3, 3)
    q = np.where(valid_queries(q)[:, None, None], q, np.float32(0))
    n, T = len(q), len(tris)
    out = np.empty((n, T), dtype)
    step = max(1, chunk // max(T, 1))
    for s in range(0, n, step):
        out[s:s + step] = pair_dist2(q[s:s + step, None], tris[None], dtype, override)[0]
    return out


def no_result(n):
    return {"found": np.zeros(n, bool), "point_q": np.zeros((n, 3), np.float32), "dist2": np.full(n, -1, np.float32),
            "point_x": np.zeros((n, 3), np.float32), "tri": np.full(n, NONE, np.uint32), "ties": np.zeros(n, np.int64)}


def brute(tris, queries, max_dist2=np.inf, dist=None):
    """The answer of every query over all triangles: a dict of per-query arrays found, dist2, tri, point_q, point_x
    (no result: dist2 = -1, both points 0, tri = 0xFFFFFFFF) and ties (the triangles that share the minimum).
    `dist`: matrix(tris, queries), when the caller has it."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3, 3)
    n = len(q)
    out = no_result(n)
    with np.errstate(all="ignore"):
        bound = np.float32(max_dist2) + np.float32(0)
        walk = valid_queries(q) & bool(bound >= 0)
        d = matrix(tris, q) if dist is None else dist
        ok = (d <= bound) & walk[:, None]                                   # (a NaN dist2 never wins)
    dk = np.where(ok, d, np.float32(np.inf))
    cand = ok & (dk == dk.min(1)[:, None])
    found = cand.any(1)
    tri = np.argmax(cand, 1)                                                # the smallest id at the minimum
    qs = np.where(found[:, None, None], q, np.float32(0))
    dw, cq, cx = pair_dist2(qs, tris[tri])                                  # the winner's fields, again
    assert np.array_equal(dw[found], d[np.arange(n), tri][found])
    out["found"] = found
    out["ties"] = cand.sum(1)
    out["dist2"] = np.where(found, dw, np.float32(-1)).astype(np.float32)
    out["point_q"] = np.where(found[:, None], cq, np.float32(0)).astype(np.float32)
    out["point_x"] = np.where(found[:, None], cx, np.float32(0)).astype(np.float32)
    out["tri"] = np.where(found, tri, NONE).astype(np.uint32)
    return out


def records(b):
    """brute()'s answer as a CLEARANCE_DTYPE array."""
    import raytracebvh_amd as rt
    out = np.zeros(len(b["found"]), rt.CLEARANCE_DTYPE)
    out["point_q"], out["dist2"], out["point_x"], out["tri"] = b["point_q"], b["dist2"], b["point_x"], b["tri"]
    return out
