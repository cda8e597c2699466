"""Scenes and host helpers for the walk-only tree's model (oracle.lib.walk_tree): lattices of identical
triangles at power-of-two coordinates, whose plane costs are exact in fp32 and tie, and what the CPU and the GPU
tests both ask of a walk tree."""
import numpy as np

import raytracebvh_amd as rt
from oracle import lib as orc

SEED = 0x5EED0004
IDENTITY = (np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32))


def scene_of_triangles(P):
    """An rt.Scene of the (n, 3, 3) float32 triangles P: a synthetic scene's normals, indices and materials (each
    vertex belongs to one triangle there) with these positions."""
    P = np.asarray(P, np.float32)
    base = rt.synthetic(len(P), seed=SEED)
    v = base.vertices.copy()
    idx = base.indices.reshape(-1, 3)
    for k in range(3):
        v[idx[:, k], :3] = P[:, k]
    return rt.Scene(v, base.indices, base.mat_indices, base.materials)


def lattice_scene(nx, ny, nz, step=1.0, size=0.5, origin=(1.0, 1.0, 1.0), seed=None):
    """nx * ny * nz copies of the triangle (0, 0, 0), (size, size, 0), (0, size, size), whose box is a cube, one at
    every point origin + step * (i, j, k): with power-of-two step, size and origin every box, centroid, area and
    cost of DESIGN.md 6c is exact in fp32, the planes between two lattice layers tie, and so do the axes of a cubic
    block.  seed: the triangles dealt in a shuffled order."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    at = (np.asarray(origin, np.float32) + np.float32(step) * g.astype(np.float32)).astype(np.float32)
    if seed is not None:
        at = at[np.random.default_rng(seed).permutation(len(at))]
    tri = np.array([(0, 0, 0), (size, size, 0), (0, size, size)], np.float32)
    return scene_of_triangles(at[:, None, :] + tri[None])


def identical_scene(n=600):
    """n copies of one triangle: every centroid equal, so every range splits in halves."""
    base = rt.synthetic(n, seed=SEED)
    v = base.vertices.copy()
    idx = base.indices.reshape(-1, 3)
    for k in range(3):
        v[idx[:, k]] = v[idx[0, k]]
    return rt.Scene(v, base.indices, base.mat_indices, base.materials)


def oracle_tree(s, wvp):
    """The oracle's built tree of scene s (the library's tree, bit for bit: tests/test_gpu_parity.py)."""
    return orc.build(orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob), wvp)


def leaf_ranges(nodes):
    """(first, last, order): the leaf range of every node of a tree in the oracle's layout, and its internal nodes
    with parents before children."""
    T = (len(nodes) + 1) // 2
    cl, cr = nodes["child_l"].astype(np.int64), nodes["child_r"].astype(np.int64)
    first, last = np.arange(2 * T - 1), np.arange(2 * T - 1)
    order, st = [], [T]
    while st:
        x = st.pop()
        order.append(x)
        st.extend(c for c in (cl[x], cr[x]) if c >= T)
    for x in reversed(order):
        first[x], last[x] = min(first[cl[x]], first[cr[x]]), max(last[cl[x]], last[cr[x]])
    return first, last, order


def check_tree_over_the_same_leaves(wt, built, K=512):
    """`wt` is a binary tree over the leaves of `built`: T - 1 internal nodes from the root, every leaf once, parent
    links that match, every box the union of its children's (so nested, bit for bit: min and max are exact), the
    nodes of more than K leaves the built tree's own, and below a subtree root exactly the built subtree's ids.
    Returns every internal node's depth (the root: 0), indexed by node."""
    T = (len(built) + 1) // 2
    cl, cr, par = wt["child_l"].astype(np.int64), wt["child_r"].astype(np.int64), wt["parent"].astype(np.int64)
    assert par[T] == 0xFFFFFFFF
    depth = np.full(2 * T - 1, -1)
    depth[T] = 0
    seen = np.zeros(2 * T - 1, np.int64)
    order, st = [], [T]
    while st:
        x = st.pop()
        order.append(x)
        seen[x] += 1
        assert len(order) <= T - 1
        for c in (cl[x], cr[x]):
            assert 0 <= c < 2 * T - 1 and par[c] == x
            if c >= T:
                depth[c] = depth[x] + 1
                st.append(c)
            else:
                seen[c] += 1
    np.testing.assert_array_equal(seen, 1, "every node and every leaf exactly once")
    with np.errstate(invalid="ignore"):
        for x in reversed(order):
            lo, hi = np.fmin(wt["bb_min"][cl[x]], wt["bb_min"][cr[x]]), np.fmax(wt["bb_max"][cl[x]], wt["bb_max"][cr[x]])
            fin = np.isfinite(lo) & np.isfinite(hi)   # (a box of NaN corners alone stays +-inf in the model)
            np.testing.assert_array_equal(wt["bb_min"][x][fin], lo[fin])
            np.testing.assert_array_equal(wt["bb_max"][x][fin], hi[fin])
    for f in ("bb_min", "bb_max"):
        np.testing.assert_array_equal(wt[f][:T].view(np.uint32), built[f][:T].view(np.uint32))
    bf, bl, border = leaf_ranges(built)
    wf, wl, _ = leaf_ranges(wt)
    for x in border:
        n = bl[x] - bf[x] + 1
        if n > K:
            assert (cl[x], cr[x], par[x]) == (built["child_l"][x], built["child_r"][x], built["parent"][x])
        elif x == T or bl[built["parent"][x]] - bf[built["parent"][x]] + 1 > K:   # a subtree root: the same leaves
            assert (wf[x], wl[x]) == (bf[x], bl[x])
    return depth


def summed_area(wt):
    """The sum of the internal nodes' half areas (float64): the SAH cost of walking the tree, up to constants."""
    T = (len(wt) + 1) // 2
    d = (wt["bb_max"][T:] - wt["bb_min"][T:]).astype(np.float64)
    return float((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]).sum())


def halves_area(built, K=512):
    """summed_area of the tree that keeps the built tree's top and splits every subtree of <= K leaves in halves of
    the sorted order all the way down."""
    T = (len(built) + 1) // 2
    first, last, order = leaf_ranges(built)
    lo, hi = built["bb_min"][:T].astype(np.float64), built["bb_max"][:T].astype(np.float64)

    def area(a, b):
        d = hi[a:b + 1].max(0) - lo[a:b + 1].min(0)
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]

    def halves(a, b):
        m = b - a + 1
        if m < 2:
            return 0.0
        return area(a, b) + halves(a, a + m // 2 - 1) + halves(a + m // 2, b)

    total = 0.0
    for x in order:
        n = last[x] - first[x] + 1
        p = built["parent"][x]
        if n > K:
            total += area(first[x], last[x])
        elif x == T or last[p] - first[p] + 1 > K:
            total += halves(first[x], last[x])
    return total


def budget_scene(filler=520, peeled=200):
    """A subtree root deep in the built tree over leaves whose cheapest planes peel a few at a time, so that the
    rebuild's level budget refuses planes.  The mesh box is [0, 2^50]^3 (two pins at its corners).
    Thirty small triangles, one at every point whose CPUTests Morton code has a single bit set, make a chain of thirty
    levels above the cell at the origin (code 0, [0, 2^40)^3).  That cell holds `filler` identical triangles and then,
    later in the index order that breaks the codes' tie, `peeled` triangles at x = 2^39 * 1.5^-i, half as wide as
    that, one unit high and flat in z: the Karras tree splits the cell's leaves by index at 512, so the last filler -
    512 + peeled leaves are a subtree root at depth 31 with 33 levels to spend, and every SAH plane there cuts off
    the few widest: 32 levels of them, the last ones refused."""
    E = np.float32(2.0 ** 50)
    tris = []

    def small(at, w=1.0):
        x, y, z = at
        tris.append([(x, y, z), (x + w, y, z), (x, y + w, z)])

    small((0.0, 0.0, 0.0))
    for _ in range(filler - 1):
        small((4.0, 4.0, 4.0))
    for i in range(peeled):
        x = 2.0 ** 39 * 1.5 ** -i
        tris.append([(x, 8.0, 8.0), (x + x / 2, 8.0, 8.0), (x, 9.0, 8.0)])
    for bit in range(30):   # code bit 3j + 2 is x's bit j, 3j + 1 y's, 3j z's: inside cell 2^j on that axis
        at = [0.0, 0.0, 0.0]
        at[2 - bit % 3] = (2.0 ** (bit // 3) + 0.25) * 2.0 ** 40
        small(at, 2.0 ** 30)
    tris.append([(E, E, E), (E - 2.0 ** 30, E, E), (E, E - 2.0 ** 30, E)])
    return scene_of_triangles(np.array(tris, np.float32))
