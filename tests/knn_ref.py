"""The k-nearest query (include/rtbvh.h rtbvh_knn_*) restated in numpy float32.

A helper of the k-nearest tests, not a test.  It builds on tests/nearest_ref.py: a triangle's dist2 is tri_dist2's,
the members of a point are the triangles with dist2 <= max_dist2, and the answer is the first k of them in
(dist2, triangle id) order -- a stable sort by dist2 over triangles in id order ties by ascending id.  No tree.
"""
import numpy as np

from tests import nearest_ref as nr

NONE = nr.NONE


def dist2_matrix(tris, points, chunk=1 << 18):
    """(n, T) float32: every point's dist2 to every triangle, and the (n,) mask of the points that are walked at all
    (finite coordinates)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    a, e1, e2, lo, hi = nr.leaf_data(tris)
    T = len(a)
    d = np.empty((len(p), T), np.float32)
    step = max(1, chunk // max(T, 1))
    for s in range(0, len(p), step):
        d[s:s + step] = nr.tri_dist2(p[s:s + step, None, :], a[None], e1[None], e2[None], lo[None], hi[None])[0]
    return d, np.isfinite(p).all(1)


def select_k(d, finite, k, max_dist2=np.inf):
    """The answer from dist2_matrix's (d, finite): (n, k) uint32 tri and float32 dist2, ascending in (dist2, tri),
    the slots past the number found holding (0xFFFFFFFF, -1)."""
    n, T = d.shape
    with np.errstate(all="ignore"):
        bound = np.broadcast_to(np.asarray(max_dist2, np.float32), (n,)) + np.float32(0)
        ok = (d <= bound[:, None]) & ((bound >= 0) & finite)[:, None]      # (a NaN dist2 is never a member)
    rows = np.arange(n)[:, None]
    order = np.argsort(np.where(ok, d, np.float32(np.inf)), axis=1, kind="stable")
    # (a member at dist2 = +inf, under max_dist2 = +inf, goes before every non-member, whatever their ids)
    if (ok & np.isinf(d)).any():
        order = order[rows, np.argsort(~ok[rows, order], axis=1, kind="stable")]
    order = order[:, :k]
    found = ok[rows, order]
    assert (found[:, :-1] >= found[:, 1:]).all()   # the members come first (no member at +inf behind a non-member)
    tri = np.full((n, k), NONE, np.uint32)
    dist2 = np.full((n, k), -1, np.float32)
    m = order.shape[1]
    tri[:, :m] = np.where(found, order, NONE).astype(np.uint32)
    dist2[:, :m] = np.where(found, d[rows, order], np.float32(-1))
    return tri, dist2


def brute_k(tris, points, k, max_dist2=np.inf):
    """(tri, dist2), each (n, k), of every point over all triangles."""
    d, finite = dist2_matrix(tris, points)
    return select_k(d, finite, k, max_dist2)


def as_pairs(tri, dist2):
    """The answer as the (n, k) PAIR_DTYPE array Context.knn returns."""
    from raytracebvh_amd import PAIR_DTYPE
    out = np.zeros(tri.shape, PAIR_DTYPE)
    out["tri"], out["dist2"] = tri, dist2
    return out
