"""The signed-distance query (include/rtbvh.h rtbvh_signed_*) restated in numpy float32.

A helper of the signed-distance tests, not a test.  The crossing count of ray j from a point is the brute force
over ALL triangles of the header's two conditions, evaluated on what a leaf record holds (nearest_ref.leaf_data):
(B) the leaf box passes the any-hit box rule (ray_walk_ref._box) with t_max = +inf, and (X) the division-free
triangle test, in the operation order of ray_walk_ref.tri_test.  The nearest fields are nearest_ref.brute's.  No tree.
"""
import numpy as np

from tests import nearest_ref as nr
from tests import ray_walk_ref as rw

NONE = 0xFFFFFFFF
DTYPE = np.dtype([("point", "<f4", (3,)), ("dist2", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"),
                  ("flags", "<u4")])
# the three rays' directions: exact in fp32, no zero component
D = np.array([[0.75, 0.5, 0.4375], [-0.5, 0.75, -0.4375], [0.4375, -0.5, -0.75]], np.float32)
INV = (np.float32(1) / D).astype(np.float32)
INF = np.float32(np.inf)


def box_pass(lo, hi, p, j):
    """(B) for (M, 3) boxes and (M, 3) origins: 0 <= mx && mn <= mx && !(mn > t_max), t_max = +inf."""
    ok, mn = rw._box(lo, hi, p, np.broadcast_to(INV[j], p.shape))
    with np.errstate(all="ignore"):
        return ok & ~(mn > INF)


def x_test(p, p0, e1, e2, j):
    """(X) for (M, 3) arrays: rayTriangleCollision's products in its order, no division, no epsilon."""
    d = np.broadcast_to(D[j], p.shape)
    with np.errstate(all="ignore"):
        tmp = rw._cross(d, e2)
        det = rw._dot(e1, tmp)
        rt = p - p0
        U = rw._dot(rt, tmp)
        tmp = rw._cross(rt, e1)
        V = rw._dot(d, tmp)
        N = rw._dot(e2, tmp)
        neg = det < 0
        det, U, V, N = (np.where(neg, -x, x) for x in (det, U, V, N))
        return (det > 0) & (U >= 0) & (V >= 0) & (U + V <= det) & (N > 0)


def crossing_matrix(tris, points, j, with_box=True):
    """bool (n, T): triangle x is crossed by ray j of point i -- (B) and (X), or (X) alone."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    a, e1, e2, lo, hi = nr.leaf_data(tris)
    n, T = len(p), len(a)
    pp = np.repeat(p, T, axis=0)
    i = np.tile(np.arange(T), n)
    out = x_test(pp, a[i], e1[i], e2[i], j)
    if with_box:
        out &= box_pass(lo[i], hi[i], pp, j)
    return out.reshape(n, T)


def box_pass_grid(lo, hi, p, j):
    """box_pass for every pair of (T, 3) boxes and (m, 3) origins, bool (m, T): the same operations by component,
    without materialising the pairs (test_signed_cpu.py compares the two)."""
    with np.errstate(all="ignore"):
        mn = mx = None
        for k in range(3):
            t0 = (lo[None, :, k] - p[:, None, k]) * INV[j, k]
            t1 = (hi[None, :, k] - p[:, None, k]) * INV[j, k]
            a, b = np.fmin(t0, t1), np.fmax(t0, t1)
            mn = a if k == 0 else np.fmax(mn, a)
            mx = b if k == 0 else np.fmin(mx, b)
        return (0 <= mx) & (mn <= mx) & ~(mn > INF)


def crossings(tris, points, j, chunk=1 << 22):
    """c_j of every point, int64 (n,): the triangles with (B) and (X), over all triangles.  ((X) is evaluated
    where (B) holds: the conjunction is the same.)  A non-finite coordinate fails (B) for every triangle."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    a, e1, e2, lo, hi = nr.leaf_data(tris)
    n, T = len(p), len(a)
    out = np.zeros(n, np.int64)
    step = max(1, chunk // max(T, 1))
    for s in range(0, n, step):
        pp = p[s:s + step]
        pi, ti = np.nonzero(box_pass_grid(lo, hi, pp, j))
        if len(pi):
            hit = x_test(pp[pi], a[ti], e1[ti], e2[ti], j)
            out[s:s + len(pp)] = np.bincount(pi[hit], minlength=len(pp))
    return out


def pack_flags(c, vote3):
    """flags of (n, 3) counts (a ray not cast: 0): inside, the parities, the bytes saturated at 255."""
    c = np.asarray(c, np.int64)
    odd = c & 1
    inside = (odd.sum(1) >= 2) if vote3 else (odd[:, 0] == 1)
    f = inside.astype(np.int64) | odd[:, 0] << 1 | odd[:, 1] << 2 | odd[:, 2] << 3
    sat = np.minimum(c, 255)
    return (f | sat[:, 0] << 8 | sat[:, 1] << 16 | sat[:, 2] << 24).astype(np.uint32)


def assemble(near, c, finite, vote3):
    """A DTYPE array of nearest_ref's per-point dict, (n, 3) crossing counts and the points' finiteness; the counts
    of rays 1 and 2 are dropped without vote3."""
    out = np.zeros(len(finite), DTYPE)
    for f in ("point", "dist2", "u", "v", "tri"):
        out[f] = near[f]
    c = np.asarray(c, np.int64) if vote3 else np.where(np.arange(3) == 0, c, 0)
    out["flags"] = np.where(finite, pack_flags(c, vote3), 0)
    return out


def brute(tris, points, max_dist2=np.inf, vote3=False, inside_only=False):
    """The record of every point, a DTYPE array: nearest_ref.brute's fields (inside_only: no result) and flags."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(p)
    near = nr.no_result(n) if inside_only else nr.brute(tris, p, max_dist2)
    c = np.zeros((n, 3), np.int64)
    finite = np.isfinite(p).all(1)
    for j in range(3 if vote3 else 1):
        c[finite, j] = crossings(tris, p[finite], j)
    return assemble(near, c, finite, vote3)


# ---------------------------------------------------------------- the analytic case: an icosphere
def icosphere(subdiv):
    """The 12-vertex icosahedron subdivided `subdiv` times onto the unit sphere: (V, 3) float32 vertices and
    (20 * 4^subdiv, 3) faces, outward-facing, a closed surface."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v).astype(np.float32), np.array(f, np.int64)


def inradius(verts, faces):
    """The smallest distance from the origin to a face's plane (float64): the ball of that radius is inside."""
    t = verts.astype(np.float64)[faces]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return float(np.abs((nrm * t[:, 0]).sum(1)).min())


def analytic_case(subdiv=3, n=20_000, seed=1):
    """(tris, points, keep, inside): the icosphere's (T, 3, 3) triangles, n points uniform in [-1.3, 1.3]^3, the
    points away from the surface (not 0.999 r_in <= |p| <= 1.001) and, for those, whether |p| < r_in."""
    verts, faces = icosphere(subdiv)
    tris = np.ascontiguousarray(verts[faces])
    r_in = inradius(verts, faces)
    rng = np.random.default_rng(seed)
    pts = ((rng.random((n, 3)) * 2 - 1) * 1.3).astype(np.float32)
    r = np.sqrt((pts.astype(np.float64) ** 2).sum(1))
    keep = ~((0.999 * r_in <= r) & (r <= 1.001))
    return tris, pts, keep, r < r_in


# ---------------------------------------------------------------- the saturation case: a stack of one triangle
def stack_case(j, copies=300):
    """(tris, points, counts): `copies` copies of one large triangle across ray j, copy k displaced by k/2 * D_j
    (exact in fp32), and points on the ray's line whose ray j crosses exactly counts[i] of them."""
    d = D[j].astype(np.float64)
    u = np.cross(d, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(d, u)
    v /= np.linalg.norm(v)
    base = np.array([16 * u, -8 * u + 14 * v, -8 * u - 14 * v]).astype(np.float32)   # the origin is well inside
    k = np.arange(1, copies + 1, dtype=np.float32)[:, None, None]
    tris = (base[None] + k * (np.float32(0.5) * D[j])[None, None, :]).astype(np.float32)
    s = np.array([0.5, 1.5, copies - 254.5, copies - 253.5, copies + 0.5], np.float32)
    pts = (s[:, None] * (np.float32(0.5) * D[j])[None]).astype(np.float32)
    counts = np.array([copies, copies - 1, 255, 254, 0], np.int64)
    return np.ascontiguousarray(tris), pts, counts
