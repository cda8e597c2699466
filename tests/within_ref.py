"""The radius query (include/rtbvh.h rtbvh_within_*) restated in numpy float32.

A helper of the radius-query tests, not a test.  A triangle's dist2 is tests/nearest_ref.tri_dist2, the closest-point
section's; the list of a point is the brute force over ALL triangles -- `dist2 <= bound`, false for a NaN -- ordered
by `rank[triangle]`, the triangle's position in the build's sort order.  No tree.
"""
import numpy as np

from tests import nearest_ref as nr

PAIR_DTYPE = np.dtype([("tri", "<u4"), ("dist2", "<f4")])


def rank_of(tri_ids):
    """rank[triangle] from the sort order (the tri_ids of read_sorted, or the oracle's leaves' index // 3)."""
    ids = np.asarray(tri_ids, np.int64)
    rank = np.empty(len(ids), np.int64)
    rank[ids] = np.arange(len(ids))
    return rank


def brute_within(tris, points, max_dist2, rank, chunk=1 << 20):
    """(offsets uint64 (n + 1,), pairs PAIR_DTYPE): every (triangle, dist2) with dist2 <= max_dist2 of every point,
    each point's list ascending by rank[triangle].  No list for a point without a walk: !(max_dist2 >= 0) or a
    non-finite coordinate."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    bound = np.broadcast_to(np.asarray(max_dist2, np.float32), (n,)).copy()
    order = np.argsort(np.asarray(rank, np.int64), kind="stable")     # the triangles in sort order
    a, e1, e2, lo, hi = (x[order] for x in nr.leaf_data(tris))
    T = len(a)
    with np.errstate(all="ignore"):
        bound = bound + np.float32(0)
        walk = (bound >= 0) & np.isfinite(p).all(1)
    counts = np.zeros(n, np.uint64)
    parts = []
    step = max(1, chunk // max(T, 1))
    for s in range(0, n, step):
        pp = p[s:s + step]
        d = nr.tri_dist2(pp[:, None, :], a[None], e1[None], e2[None], lo[None], hi[None])[0]
        with np.errstate(all="ignore"):
            ok = (d <= bound[s:s + step, None]) & walk[s:s + step, None]
        counts[s:s + len(pp)] = ok.sum(1)
        k, j = np.nonzero(ok)                                          # row-major: by point, then by rank
        part = np.zeros(len(k), PAIR_DTYPE)
        part["tri"] = order[j]
        part["dist2"] = d[k, j]
        parts.append(part)
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, np.concatenate(parts) if parts else np.zeros(0, PAIR_DTYPE)


def pair_bits(pairs):
    """(m, 2) uint32: the ids and the bits of dist2 (bit-exact comparisons)."""
    return np.ascontiguousarray(pairs).view(np.uint32).reshape(-1, 2)
