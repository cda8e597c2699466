"""The closest-point query (include/rtbvh.h rtbvh_nearest_*) restated in numpy float32.

A helper of the closest-point tests, not a test.  It evaluates the header's formulas for (point, triangle)
pairs from what a leaf record holds -- a = p0, e1 = fl(p1 - p0), e2 = fl(p2 - p0) and the leaf box, the
componentwise min / max of the three vertices -- with the operation order of the kernels: left-to-right dots
`(a*b + c*d) + e*f`, no fused multiply-add (numpy rounds every product), np.fmin / np.fmax where the header says
fminf / fmaxf.  The answer of a point is the brute force over ALL triangles, keyed (dist2, triangle id): no tree.

`dtype=np.float64` evaluates the same formulas in double precision (the sanity bound of test_nearest_cpu.py).
"""
import numpy as np

NONE = 0xFFFFFFFF


def leaf_data(tris, dtype=np.float32):
    """(a, e1, e2, lo, hi), each (T, 3), of (T, 3, 3) float32 triangles (ray_walk_ref.clip_triangles)."""
    t = np.ascontiguousarray(tris, np.float32)
    lo = np.fmin(np.fmin(t[:, 0], t[:, 1]), t[:, 2])
    hi = np.fmax(np.fmax(t[:, 0], t[:, 1]), t[:, 2])
    t = t.astype(dtype)
    return t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], lo.astype(dtype), hi.astype(dtype)


def _split(x):
    return x[..., 0], x[..., 1], x[..., 2]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def tri_dist2(p, a, e1, e2, lo, hi):
    """The header's formulas for broadcastable (..., 3) arrays: (dist2, u, v, q), in the arrays' dtype.  (Computed
    by component, so that every large intermediate is a contiguous array.)"""
    f = p.dtype.type
    p, a, e1, e2, lo, hi = (_split(x) for x in (p, a, e1, e2, lo, hi))
    with np.errstate(all="ignore"):
        ap = tuple(p[k] - a[k] for k in range(3))
        d1, d2 = _dot(e1, ap), _dot(e2, ap)
        e11, e12, e22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        d3, d4, d5, d6 = d1 - e11, d2 - e12, d1 - e12, d2 - e22
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        den = f(1) / ((va + vb) + vc)
        u, v = vb * den, vc * den                                    # otherwise: the face
        w = d43 / (d43 + d56)
        r = (va <= 0) & (d43 >= 0) & (d56 >= 0)                      # later regions first: earlier ones overwrite
        u, v = np.where(r, f(1) - w, u), np.where(r, w, v)
        r = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        u, v = np.where(r, f(0), u), np.where(r, d2 / (d2 - d6), v)
        r = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        u, v = np.where(r, d1 / (d1 - d3), u), np.where(r, f(0), v)
        r = (d6 >= 0) & (d5 <= d6)
        u, v = np.where(r, f(0), u), np.where(r, f(1), v)
        r = (d3 >= 0) & (d4 <= d3)
        u, v = np.where(r, f(1), u), np.where(r, f(0), v)
        r = (d1 <= 0) & (d2 <= 0)
        u, v = np.where(r, f(0), u), np.where(r, f(0), v)
        u = np.where(np.isnan(u), f(0), u)
        v = np.where(np.isnan(v), f(0), v)
        q = tuple(np.fmax(lo[k], np.fmin(hi[k], (a[k] + e1[k] * u) + e2[k] * v)) for k in range(3))
        e = tuple(p[k] - q[k] for k in range(3))
        return _dot(e, e), u, v, np.stack(np.broadcast_arrays(*q), -1)


def box_dist2(p, lo, hi):
    """The header's point-box distance for broadcastable (..., 3) arrays."""
    with np.errstate(all="ignore"):
        d = np.fmax(np.fmax(lo - p, p - hi), p.dtype.type(0))
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def no_result(n):
    return {"found": np.zeros(n, bool), "point": np.zeros((n, 3), np.float32), "dist2": np.full(n, -1, np.float32),
            "u": np.zeros(n, np.float32), "v": np.zeros(n, np.float32), "tri": np.full(n, NONE, np.uint32),
            "ties": np.zeros(n, np.int64)}


def brute(tris, points, max_dist2=np.inf, chunk=1 << 18):
    """The answer of every point over all triangles: a dict of per-point arrays found, point, dist2, u, v, tri (no
    result: dist2 = -1, point = u = v = 0, tri = 0xFFFFFFFF) and ties (the triangles that share the minimum)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    bound = np.broadcast_to(np.asarray(max_dist2, np.float32), (n,)).copy()
    a, e1, e2, lo, hi = leaf_data(tris)
    T = len(a)
    out = no_result(n)
    with np.errstate(all="ignore"):
        bound = bound + np.float32(0)
        walk = (bound >= 0) & np.isfinite(p).all(1)
    step = max(1, chunk // max(T, 1))
    for s in range(0, n, step):
        pp = p[s:s + step]
        d = tri_dist2(pp[:, None, :], a[None], e1[None], e2[None], lo[None], hi[None])[0]
        with np.errstate(all="ignore"):
            ok = (d <= bound[s:s + step, None]) & walk[s:s + step, None]      # (a NaN dist2 never wins)
        dk = np.where(ok, d, np.float32(np.inf))
        cand = ok & (dk == dk.min(1)[:, None])
        found = cand.any(1)
        tri = np.argmax(cand, 1)                                               # the smallest id at the minimum
        dw, u, v, q = tri_dist2(pp, a[tri], e1[tri], e2[tri], lo[tri], hi[tri])   # the winner's fields, again
        assert np.array_equal(dw[found], d[np.arange(len(pp)), tri][found])
        sl = slice(s, s + len(pp))
        out["found"][sl] = found
        out["ties"][sl] = cand.sum(1)
        out["dist2"][sl] = np.where(found, dw, np.float32(-1))
        out["u"][sl] = np.where(found, u, np.float32(0))
        out["v"][sl] = np.where(found, v, np.float32(0))
        out["point"][sl] = np.where(found[:, None], q, np.float32(0))
        out["tri"][sl] = np.where(found, tri, NONE).astype(np.uint32)
    return out


def root_box(tris):
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    return t.min(0), t.max(0)


def sample_points(tris, seed=5, n_random=512, n_each=64, scale=1.5):
    """The tests' points: n_random uniform in `scale` times the root box, then n_each mesh vertices, centroids and
    edge midpoints.  Returns (points, first index of the vertices)."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(tris)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * scale
    pts = [(c + (rng.random((n_random, 3)) * 2 - 1) * h).astype(np.float32)]
    T = len(tris)
    pick = rng.integers(0, T, n_each)
    pts.append(tris[pick, rng.integers(0, 3, n_each)])
    pick = rng.integers(0, T, n_each)
    pts.append(((tris[pick, 0] + tris[pick, 1] + tris[pick, 2]) / np.float32(3)).astype(np.float32))
    pick = rng.integers(0, T, n_each)
    k = rng.integers(0, 3, n_each)
    pts.append(((tris[pick, k] + tris[pick, (k + 1) % 3]) * np.float32(.5)).astype(np.float32))
    return np.concatenate(pts).astype(np.float32), n_random


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
