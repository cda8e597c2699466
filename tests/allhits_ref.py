"""The all-hits ray query (include/rtbvh.h rtbvh_allhits_*) restated in numpy float32.

A helper of the all-hits tests, not a test.  A ray's list is the brute force over ALL triangles: triangle x is a
member iff (B) its own leaf box passes the any-hit box rule with the ray's t_max (ray_walk_ref._box and
`!(mn > t_max)`) and (T) ray_walk_ref.tri_test accepts it with t <= t_max; its hit is the test's own (t, u, v) and
the triangle's id.  The list is ordered by `rank[triangle]`, the triangle's position in the build's sort order, or
(by_t) by the key t bits << 32 | tri.  No tree.  Also here: the tests' rays, and the stack scene of the ordering
pass's long lists.
"""
import numpy as np

import raytracebvh_amd as rt
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests.within_ref import rank_of   # noqa: F401  (the tests take it from here)

HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4")])
INF = np.float32(np.inf)


def walked(o, d, t_max):
    """The rays that are walked at all: finite origin and direction, a direction not all zero, t_max > 0."""
    with np.errstate(all="ignore"):
        return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1) & (t_max > 0)


def pair_tests(tris, tri, o, d, t_max, with_mn=False):
    """(member, t, u, v) of ray k against triangle tri[k]: conditions (B) and (T) of the header; with_mn: the
    leaf box's slab entry mn as well."""
    _, _, _, lo, hi = nr.leaf_data(tris)
    with np.errstate(all="ignore"):
        inv = (np.float32(1) / d).astype(np.float32)
        box, mn = rw._box(lo[tri], hi[tri], o, inv)
        box &= ~(mn > t_max)
        t, u, v = rw.tri_test(tris, tri, o, d)
        ok = box & (t != -1) & (t <= t_max) & walked(o, d, t_max)
    return (ok, t, u, v, mn) if with_mn else (ok, t, u, v)


def brute_allhits(tris, origins, directions, t_max, rank, by_t=False, with_mn=False, chunk=1 << 20):
    """(offsets uint64 (n + 1,), hits HIT_DTYPE): every member's hit of every ray, each ray's list ascending by
    rank[triangle], or with by_t by (t, tri).  with_mn: each hit's leaf-box slab entry as a third array (for cut)."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    n, T = len(o), len(tris)
    tm = np.broadcast_to(np.asarray(t_max, np.float32), (n,)).copy()
    order = np.argsort(np.asarray(rank, np.int64), kind="stable")     # the triangles in sort order
    counts = np.zeros(n, np.uint64)
    parts, mns = [], []
    step = max(1, chunk // max(T, 1))
    for s in range(0, n, step):
        m = len(o[s:s + step])
        k = np.repeat(np.arange(s, s + m), T)
        tri = np.tile(order, m)
        ok, t, u, v, mn = pair_tests(tris, tri, o[k], d[k], tm[k], with_mn=True)
        counts[s:s + m] = ok.reshape(m, T).sum(1)
        part = np.zeros(int(ok.sum()), HIT_DTYPE)                     # row-major: by ray, then by rank
        part["t"], part["u"], part["v"], part["tri"] = t[ok], u[ok], v[ok], tri[ok]
        parts.append(part)
        mns.append(mn[ok])
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(counts, out=offsets[1:])
    hits = np.concatenate(parts) if parts else np.zeros(0, HIT_DTYPE)
    if with_mn:
        return offsets, hits, np.concatenate(mns) if mns else np.zeros(0, np.float32)
    return offsets, order_by_t(offsets, hits) if by_t else hits


def cut(offsets, hits, mn, t_max):
    """The lists for a smaller t_max from those for t_max = +inf (brute_allhits with_mn): t_max enters the
    definition in `t <= t_max` and `!(mn > t_max)` only, and in the no-walk rule !(t_max > 0)."""
    cnt = np.diff(offsets.astype(np.int64))
    tm = np.repeat(np.asarray(t_max, np.float32), cnt)
    with np.errstate(all="ignore"):
        keep = (hits["t"] <= tm) & ~(mn > tm) & (tm > 0)
    ray = np.repeat(np.arange(len(cnt)), cnt)
    off = np.zeros(len(offsets), np.uint64)
    np.cumsum(np.bincount(ray[keep], minlength=len(cnt)).astype(np.uint64), out=off[1:])
    return off, hits[keep]


def hit_keys(hits):
    """The (t, tri) order's uint64 keys, t bits << 32 | tri: t > 0, so the bits order as the floats."""
    return rw.bits(hits["t"]).astype(np.uint64) << np.uint64(32) | hits["tri"].astype(np.uint64)


def order_by_t(offsets, hits):
    """Each ray's segment of hits ascending by hit_keys (the segments stay where they are)."""
    ray = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))
    return hits[np.lexsort((hit_keys(hits), ray))]


def hit_words(hits):
    """(m, 4) uint32: the bits of t, u, v and the ids (bit-exact comparisons)."""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 4)


def segments(offsets, hits):
    off = offsets.astype(np.int64)
    return [hits[off[k]:off[k + 1]] for k in range(len(off) - 1)]


# ---------------------------------------------------------------- the tests' rays
def sample_rays(tris, n_random, n_axis, n_through, n_plane=0, seed=7):
    """(o, d): n_random rays with origins uniform in the root box and unit normal directions, the 16 edge rays of
    tests/test_query_gpu.py, n_axis axis-parallel rays that start exactly on mesh vertices, n_through rays shot
    from outside the root box at points inside it (not unit) and n_plane rays that start level with a mesh vertex
    on one axis and have no component along it (1 / d is infinite there)."""
    from tests.test_query_gpu import edge_rays
    rng = np.random.default_rng(seed)
    lo, hi = nr.root_box(tris)
    lo, hi = lo.astype(np.float32), hi.astype(np.float32)
    c, ext = ((lo + hi) / 2).astype(np.float32), (hi - lo).astype(np.float32)
    verts = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    ro = (lo + rng.random((n_random, 3), dtype=np.float32) * ext).astype(np.float32)
    rd = rng.standard_normal((n_random, 3)).astype(np.float32)
    rd /= np.sqrt((rd * rd).sum(1, keepdims=True))
    box = np.zeros(3, dtype=[("bb_min", "<f4", 3), ("bb_max", "<f4", 3)])   # (edge_rays reads the root: node 1 of 3)
    box["bb_min"], box["bb_max"] = lo, hi
    eo, ed = edge_rays(box)
    ao = verts[rng.integers(0, len(verts), n_axis)]
    ad = np.zeros((n_axis, 3), np.float32)
    ad[np.arange(n_axis), rng.integers(0, 3, n_axis)] = rng.choice(np.float32([-1, 1]), n_axis)
    aim = (lo + rng.random((n_through, 3), dtype=np.float32) * ext).astype(np.float32)
    out = rng.standard_normal((n_through, 3)).astype(np.float32)
    out /= np.sqrt((out * out).sum(1, keepdims=True))
    to = (c + np.float32(1.5) * np.sqrt((ext * ext).sum()) * out).astype(np.float32)
    td = (aim - to).astype(np.float32)
    pv = verts[rng.integers(0, len(verts), n_plane)]
    ax = rng.integers(0, 3, n_plane)
    po = (c + np.float32(0.75) * ext * rng.choice(np.float32([-1, 1]), (n_plane, 3))).astype(np.float32)
    po[np.arange(n_plane), ax] = pv[np.arange(n_plane), ax]
    pd = ((lo + rng.random((n_plane, 3), dtype=np.float32) * ext).astype(np.float32) - po).astype(np.float32)
    pd[np.arange(n_plane), ax] = 0
    return (np.concatenate([ro, eo, ao, to, po]).astype(np.float32),
            np.concatenate([rd, ed, ad, td, pd]).astype(np.float32))


def mixed_t_max(tris, o, d, rank, seed=3):
    """Per-ray t_max: two thirds +inf; of the other rays, those with members get the t of one of their members
    exactly or the float below it, in turn, the others 10.  Returns (t_max, the lists for t_max = +inf, the lists
    for t_max)."""
    rng = np.random.default_rng(seed)
    off, hits, mn = brute_allhits(tris, o, d, INF, rank, with_mn=True)
    tm = np.full(len(o), INF, np.float32)
    cnt = np.diff(off.astype(np.int64))
    for k in range(0, len(o), 3):
        if cnt[k] == 0:
            tm[k] = 10
            continue
        t = hits["t"][int(off[k]) + int(rng.integers(0, cnt[k]))]
        tm[k] = t if k % 2 == 0 else np.nextafter(t, np.float32(0))
    return tm, (off, hits), cut(off, hits, mn, tm)


# ---------------------------------------------------------------- the stack scene
def stack_scene(K, dup_every=8):
    """K parallel triangles over the square [0, 8]^2, triangle k in the plane z = 0.1 k -- except that every
    dup_every-th one repeats the triangle before it exactly (equal t for every ray: the tie goes to the smaller
    id) -- dealt in a shuffled order, and two pins that keep the mesh box's depth."""
    z = np.arange(K, dtype=np.float64) * 0.1
    dup = (np.arange(K) % dup_every == dup_every - 1)
    z[dup] = z[np.nonzero(dup)[0] - 1]
    base = np.array([[-1, -1], [17, -1], [-1, 17]], np.float32)        # covers the square
    t = np.zeros((K + 2, 3, 3), np.float32)
    t[:K, :, :2] = base
    t[:K, :, 2] = z.astype(np.float32)[:, None]
    t[K] = [(-2, -2, -1), (-1.9, -2, -1), (-2, -1.9, -1)]
    t[K + 1] = [(18, 18, 0.1 * K + 1), (17.9, 18, 0.1 * K + 1), (18, 17.9, 0.1 * K + 1)]
    t[:K] = t[np.random.default_rng(K).permutation(K)]
    v = np.zeros((3 * (K + 2), 8), np.float32)
    v[:, :3] = t.reshape(-1, 3)
    v[:, 5] = -1
    return rt.Scene(v, np.arange(3 * (K + 2), dtype=np.uint32), np.zeros(K + 2, np.uint32),
                    np.zeros(1, rt.MATERIAL_DTYPE))


def stack_rays(n_z=64, n_oblique=64, seed=5):
    """(o, d) piercing the stack scene from z = -0.5: n_z rays along +z and n_oblique oblique ones, inside the
    square."""
    rng = np.random.default_rng(seed)
    n = n_z + n_oblique
    o = np.concatenate([rng.uniform(1, 7, (n, 2)), np.full((n, 1), -0.5)], 1).astype(np.float32)
    d = np.zeros((n, 3), np.float32)
    d[:, 2] = 1
    d[n_z:, :2] = rng.uniform(-0.002, 0.002, (n_oblique, 2))
    return o, d
