"""The box-overlap query (include/rtbvh.h rtbvh_overlap_*) restated in numpy.

A helper of the box-query tests, not a test.  Membership is the header's, on what a leaf record holds
(tests/nearest_ref.leaf_data): (B) the closed-interval test of the query box against the leaf box, comparisons only,
and (T) the ten separating axes of triangle against box with the header's operation order -- every product rounded
(numpy never fuses), left-to-right sums, np.fmin / np.fmax where the header says fminf / fmaxf, NaN comparisons
false.  The list of a box is the brute force over ALL triangles ordered by `rank[triangle]`, the triangle's position
in the build's sort order.  No tree.

`dtype=np.float64` evaluates the same formulas in double precision (the sanity check of test_overlap_cpu.py).
"""
import numpy as np

from tests import nearest_ref as nr


def valid_boxes(qlo, qhi):
    """The boxes that are walked: finite bounds and qlo <= qhi on every axis."""
    with np.errstate(all="ignore"):
        return np.isfinite(qlo).all(-1) & np.isfinite(qhi).all(-1) & (qlo <= qhi).all(-1)


def boxes_meet(qlo, qhi, lo, hi):
    """(B) for broadcastable (..., 3) arrays."""
    with np.errstate(all="ignore"):
        return ((qlo <= hi) & (lo <= qhi)).all(-1)


def triangle_meets(qlo, qhi, a, e1, e2, dtype=np.float32):
    """(T) for broadcastable (..., 3) arrays: True where none of the ten axes separates, evaluated in `dtype`."""
    qlo, qhi, a, e1, e2 = (np.asarray(x).astype(dtype) for x in (qlo, qhi, a, e1, e2))
    half = dtype(0.5)
    with np.errstate(all="ignore"):
        c = (qlo + qhi) * half
        h = (qhi - qlo) * half
        v0 = a - c
        v1 = v0 + e1
        v2 = v0 + e2
        hx, hy, hz = h[..., 0], h[..., 1], h[..., 2]
        e1x, e1y, e1z = e1[..., 0], e1[..., 1], e1[..., 2]
        e2x, e2y, e2z = e2[..., 0], e2[..., 1], e2[..., 2]
        nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
        d = (nx * v0[..., 0] + ny * v0[..., 1]) + nz * v0[..., 2]
        r = (hx * np.abs(nx) + hy * np.abs(ny)) + hz * np.abs(nz)
        sep = (d > r) | (d < -r)
        for f in (e1, e2 - e1, e2):
            fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
            for axis in range(3):
                if axis == 0:
                    p = [v[..., 2] * fy - v[..., 1] * fz for v in (v0, v1, v2)]
                    rr = hy * np.abs(fz) + hz * np.abs(fy)
                elif axis == 1:
                    p = [v[..., 0] * fz - v[..., 2] * fx for v in (v0, v1, v2)]
                    rr = hx * np.abs(fz) + hz * np.abs(fx)
                else:
                    p = [v[..., 1] * fx - v[..., 0] * fy for v in (v0, v1, v2)]
                    rr = hx * np.abs(fy) + hy * np.abs(fx)
                sep = sep | (np.fmin(np.fmin(p[0], p[1]), p[2]) > rr) | (np.fmax(np.fmax(p[0], p[1]), p[2]) < -rr)
    return ~sep


def box_pairs(tris, qlo, qhi, order=None, chunk=1 << 22):
    """(k, j): the (box, triangle) pairs that pass (B) among the walked boxes, row-major -- by box, then by the
    triangle's place in `order` (default: id order); j indexes `order`."""
    qlo = np.ascontiguousarray(qlo, np.float32).reshape(-1, 3)
    qhi = np.ascontiguousarray(qhi, np.float32).reshape(-1, 3)
    lo, hi = nr.leaf_data(tris)[3:]
    if order is not None:
        lo, hi = lo[order], hi[order]
    T, n = len(lo), len(qlo)
    walk = valid_boxes(qlo, qhi)
    ks, js = [], []
    step = max(1, chunk // max(T, 1))
    for s in range(0, n, step):
        ok = boxes_meet(qlo[s:s + step, None], qhi[s:s + step, None], lo[None], hi[None]) & walk[s:s + step, None]
        k, j = np.nonzero(ok)
        ks.append(k + s)
        js.append(j)
    return (np.concatenate(ks), np.concatenate(js)) if ks else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def brute_overlap(tris, qlo, qhi, rank, triangle=False):
    """(offsets uint64 (n + 1,), ids uint32): every member triangle of every box, each box's list ascending by
    rank[triangle].  No list for a box without a walk: a non-finite bound, or !(qlo <= qhi) on an axis."""
    qlo = np.ascontiguousarray(qlo, np.float32).reshape(-1, 3)
    qhi = np.ascontiguousarray(qhi, np.float32).reshape(-1, 3)
    n = len(qlo)
    order = np.argsort(np.asarray(rank, np.int64), kind="stable")     # the triangles in sort order
    k, j = box_pairs(tris, qlo, qhi, order)
    if triangle and len(k):
        a, e1, e2 = (x[order] for x in nr.leaf_data(tris)[:3])
        keep = triangle_meets(qlo[k], qhi[k], a[j], e1[j], e2[j])
        k, j = k[keep], j[keep]
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(np.bincount(k, minlength=n).astype(np.uint64), out=offsets[1:])
    return offsets, order[j].astype(np.uint32)


def sample_boxes(tris, seed, n_random=512, n_each=64):
    """The tests' boxes, (qlo, qhi): the centres are nearest_ref.sample_points' points, the half-extents uniform in
    [0.002, 0.082] x the root diagonal per axis.  Class k = index % 4: 0 and 3 fat boxes, 1 a point box
    (qlo == qhi), 2 flat in x."""
    c = nr.sample_points(tris, seed, n_random, n_each)[0]
    lo, hi = nr.root_box(tris)
    diag = np.float32(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    rng = np.random.default_rng(seed + 1000)
    h = ((0.002 + 0.08 * rng.random((len(c), 3))) * diag).astype(np.float32)
    cls = np.arange(len(c)) % 4
    h[cls == 1] = 0
    h[cls == 2, 0] = 0
    return (c - h).astype(np.float32), (c + h).astype(np.float32)
