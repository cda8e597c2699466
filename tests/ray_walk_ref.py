"""findCollision (RayTraceTraversal.hlsl:106-193) restated in numpy float32, vectorised over rays.

A helper of the ray-query tests, not a test.  It walks the exported BVH (NODE_DTYPE nodes: leaves
[0, n), internal node k at n + k, the root at n) for caller-given rays in the space the BVH was
built in (vertex positions times WVP, .xyz), with the operation order of oracle/rtbvh_oracle.cpp:
left-to-right dots `(a*b + c*d) + e*f`, min / max that drop NaN (np.fmin / np.fmax), no fused
multiply-add (numpy rounds every product), the matrix product of xform_point.

t_max (include/rtbvh.h rtbvh_ray) enters in two places only: a triangle's t is accepted iff the
reference accepts it and t <= t_max; a box passes iff the reference's first two conditions hold and
(hit ? mn <= dist : !(mn > t_max)).  With t_max = +inf this is the reference.

Any-hit: the same box test without the `hit` branch, the walk ends at the first accepted triangle.
"""
import numpy as np

EPS = np.float32(0.01)
STACK = 66   # oracle/rtbvh_oracle.cpp find_collision
NONE = 0xFFFFFFFF


def clip_triangles(vertices, indices, wvp):
    """(T, 3, 3) float32: each triangle's vertices times WVP (.xyz), as xform_point orders the sum."""
    p = np.ascontiguousarray(vertices, np.float32).reshape(-1, 8)[:, :3]
    m = np.ascontiguousarray(wvp, np.float32).reshape(16)
    c = np.empty((len(p), 3), np.float32)
    for a in range(3):
        c[:, a] = ((p[:, 0] * m[a] + p[:, 1] * m[4 + a]) + p[:, 2] * m[8 + a]) + m[12 + a]
    return c[np.asarray(indices, np.int64).reshape(-1, 3)]


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def tri_test(tris, tri, o, d):
    """rayTriangleCollision of ray k against triangle tri[k]: (t, u, v), t = -1 for no hit (u, v
    are then whatever the arithmetic gave up to the rejecting test, 0 where not computed)."""
    with np.errstate(all="ignore"):
        p = tris[tri]
        p0 = p[:, 0]
        e1, e2 = p[:, 1] - p0, p[:, 2] - p0
        tmp = _cross(d, e2)
        dx = _dot(e1, tmp)
        ok = ~(np.abs(dx) < EPS)
        idx = np.float32(1) / dx
        rt = o - p0
        u = _dot(rt, tmp) * idx
        ok &= ~((u < 0) | (np.float32(1) < u))
        tmp = _cross(rt, e1)
        v = _dot(d, tmp) * idx
        ok &= ~((v < 0) | (np.float32(1) < u + v))
        t = _dot(e2, tmp) * idx
        ok &= EPS < t
    return np.where(ok, t, np.float32(-1)).astype(np.float32), u.astype(np.float32), v.astype(np.float32)


def _box(bmin, bmax, o, inv):
    with np.errstate(all="ignore"):
        t0 = (bmin - o) * inv
        t1 = (bmax - o) * inv
        lo, hi = np.fmin(t0, t1), np.fmax(t0, t1)
        mn = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
        mx = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
        return (0 <= mx) & (mn <= mx), mn


def walk(nodes, tris, origins, directions, t_max=None, any_hit=False, order="reference"):
    """Walks every ray; returns a dict of per-ray arrays: hit (bool), t, u, v (float32; a miss has
    t = -1, u = v = 0), tri (uint32; a miss 0xFFFFFFFF), internal and leaf (visit counts, int64), max_stack (the
    ray's largest stack index, int64: find_collision's max_depth, 0 for a ray that never pushed).

    order="nearest" (closest hits only) restates the binary nearest-first walk of trace.hip (WalkRule<true>,
    walk_node): where both children pass, the right one first if its slab entry is the smaller (the left one is
    pushed), and a triangle at the best distance replaces the best hit if its sorted leaf index is smaller."""
    nearest = order == "nearest"
    assert order in ("reference", "nearest") and not (nearest and any_hit)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    R = len(o)
    tm = np.full(R, np.inf, np.float32) if t_max is None else np.broadcast_to(
        np.asarray(t_max, np.float32), (R,)).copy()
    with np.errstate(all="ignore"):
        inv = (np.float32(1) / d).astype(np.float32)
    n = (len(nodes) + 1) // 2
    cl = nodes["child_l"].astype(np.int64)
    cr = nodes["child_r"].astype(np.int64)
    is_leaf = (nodes["child_l"] == NONE) & (nodes["child_r"] == NONE)
    bmin, bmax = nodes["bb_min"], nodes["bb_max"]
    leaf_tri = (nodes["index"] // 3).astype(np.int64)

    hit = np.zeros(R, bool)
    best = np.zeros(R, np.float32)
    btri = np.zeros(R, np.int64)
    bleaf = np.zeros(R, np.int64)
    node = np.full(R, n if n > 1 else 0, np.int64)
    stack = np.full((R, STACK), -1, np.int64)
    sp = np.zeros(R, np.int64)
    n_int = np.zeros(R, np.int64)
    n_leaf = np.zeros(R, np.int64)
    max_sp = np.zeros(R, np.int64)
    act = np.arange(R)
    while len(act):
        nd = node[act]
        lf = is_leaf[nd]
        # leaves
        a = act[lf]
        if len(a):
            n_leaf[a] += 1
            tr = leaf_tri[nd[lf]]
            t, _, _ = tri_test(tris, tr, o[a], d[a])
            acc = (t != -1) & (t <= tm[a])
            if not any_hit:
                better = ~hit[a] | (t < best[a])
                if nearest:
                    better |= (t == best[a]) & (nd[lf] < bleaf[a])
                acc &= better
            w = a[acc]
            best[w] = t[acc]
            btri[w] = tr[acc]
            bleaf[w] = nd[lf][acc]
            hit[w] = True
            node[a] = stack[a, sp[a]]
            sp[a] -= 1
            if any_hit:
                sp[w] = -1   # the walk ends at the first accepted triangle
        # internal nodes
        b = act[~lf]
        if len(b):
            n_int[b] += 1
            nb = nd[~lf]
            L, Rr = cl[nb], cr[nb]
            lb, lmn = _box(bmin[L], bmax[L], o[b], inv[b])
            rb, rmn = _box(bmin[Rr], bmax[Rr], o[b], inv[b])
            with np.errstate(all="ignore"):
                if any_hit:
                    lh = lb & ~(lmn > tm[b])
                    rh = rb & ~(rmn > tm[b])
                else:
                    h = hit[b]
                    lh = lb & np.where(h, lmn <= best[b], ~(lmn > tm[b]))
                    rh = rb & np.where(h, rmn <= best[b], ~(rmn > tm[b]))
            none = ~lh & ~rh
            both = lh & rh
            full = both & (sp[b] + 1 >= STACK)
            pop = b[none | full]
            node[pop] = stack[pop, sp[pop]]
            sp[pop] -= 1
            psh = b[both & ~full]
            sp[psh] += 1
            with np.errstate(all="ignore"):
                swap = both & (rmn < lmn) if nearest else np.zeros(len(b), bool)
            stack[psh, sp[psh]] = np.where(swap, L, Rr)[both & ~full]
            max_sp[psh] = np.maximum(max_sp[psh], sp[psh])
            go = (lh | rh) & ~full
            node[b[go]] = np.where(swap, Rr, np.where(lh, L, Rr))[go]
        act = act[sp[act] != -1]

    out_t = np.where(hit, best, np.float32(-1)).astype(np.float32)
    u = np.zeros(R, np.float32)
    v = np.zeros(R, np.float32)
    w = np.nonzero(hit)[0]
    if len(w):
        _, uu, vv = tri_test(tris, btri[w], o[w], d[w])
        u[w], v[w] = uu, vv
    return {"hit": hit, "t": out_t, "u": u, "v": v,
            "tri": np.where(hit, btri, NONE).astype(np.uint32), "internal": n_int, "leaf": n_leaf,
            "max_stack": max_sp}


def bits(x):
    """float32 array as its uint32 bit patterns (bit-exact comparisons, NaN included)."""
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
