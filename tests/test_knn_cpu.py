"""k-nearest queries without a GPU: the ABI's names and constants, Context.knn's argument checks (which run before
the library is touched), the brute force (tests/knn_ref.py) and its edges, and -- on the oracle's tree -- the lemma
the GPU walk leans on: a nearer-first walk that carries a k-list and prunes on box distance <= the worst entry
returns the brute-force list."""
import bisect
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import knn_ref as kr
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Test", "Rect", "Image_Test"]


def camera(name):
    m = np.eye(4, dtype=np.float32)
    if name == "affine":
        m[:3, :3] = np.array([[1.5, 0.2, 0], [-0.1, 0.8, 0.3], [0, 0.25, 1.2]], np.float32)
        m[3, :3] = (0.5, -1.0, 2.0)
    return m


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in ("identity", "affine")],
                ids=lambda p: "-".join(p))
def case(request):
    """A golden scene in BVH space, the tests' 704 points and every (point, triangle) dist2 (computed once)."""
    scene, cam = request.param
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
    pts = nr.sample_points(tris)[0]
    dist2, finite = kr.dist2_matrix(tris, pts)
    return scene, cam, tris, pts, dist2, finite


# ---------------------------------------------------------------- the ABI
def test_exports_and_constants():
    L = rt.lib()
    for name in ("rtbvh_knn_async", "rtbvh_knn_host", "rtbvh_knn_counts"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.KNN_SORT, rt.KNN_COUNT, rt.KNN_MAX_K) == (1 << 1, 1 << 2, 32)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    assert re.search(r"RTBVH_KNN_SORT = 1u << 1\b", header) and re.search(r"RTBVH_KNN_COUNT = 1u << 2\b", header)
    assert re.search(r"^#define RTBVH_KNN_MAX_K 32$", header, re.M)
    for name in ("rtbvh_knn_async", "rtbvh_knn_host", "rtbvh_knn_counts"):
        assert re.search(rf"^rtbvh_status {name}\s*\(rtbvh_ctx\*", header, re.M), name
    assert re.search(r"rtbvh_within_\*, rtbvh_knn_\*,", header)   # the calls that are NOT_READY after a vertex update
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_bad_arguments_are_rejected_before_the_library_is_called():
    import torch
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    f32 = np.float32
    ok = np.zeros((4, 3), f32)
    for k in (0, 33, -1, 2.5, None, "4", True):
        with pytest.raises(ValueError):
            ctx.knn(ok, k)
    bad = [np.zeros((4, 5), f32), np.zeros((4, 2), f32), np.zeros(4, f32), np.zeros((4, 3), np.float64),
           np.zeros((4, 4), np.int32), np.zeros((2, 4, 3), f32), np.zeros((8, 4), f32)[::2], np.zeros((4, 6), f32)[:, :3],
           np.zeros((2, 2), rt.POINT_DTYPE), np.zeros(8, rt.POINT_DTYPE)[::2], [[0, 0, 0]], None,
           torch.zeros((4, 4)), torch.zeros((4, 3)), torch.zeros((4, 4), dtype=torch.float64)]
    for b in bad:
        with pytest.raises(ValueError):
            ctx.knn(b, 4)
    with pytest.raises(ValueError):
        ctx.knn(ok, 4, max_dist2=np.zeros(3, f32))               # 4 points, 3 bounds
    with pytest.raises(ValueError):
        ctx.knn(np.zeros((4, 4), f32), 4, max_dist2=1.0)         # the bound is the fourth column
    with pytest.raises(ValueError):
        ctx.knn(np.zeros(4, rt.POINT_DTYPE), 4, max_dist2=1.0)
    for out in (np.zeros((3, 4), rt.PAIR_DTYPE), np.zeros((4, 5), rt.PAIR_DTYPE), np.zeros(16, rt.PAIR_DTYPE),
                np.zeros((4, 4, 2), f32), np.zeros((4, 4), np.uint64), np.zeros((4, 8), rt.PAIR_DTYPE)[:, ::2],
                np.zeros((8, 4), rt.PAIR_DTYPE)[::2]):
        with pytest.raises(ValueError):
            ctx.knn(ok, 4, out=out)


# ---------------------------------------------------------------- the brute force
def test_k_of_one_is_the_closest_point_answer(case):
    _, _, tris, pts, dist2, finite = case
    want = nr.brute(tris, pts)
    tri, d = kr.select_k(dist2, finite, 1)
    assert tri.shape == d.shape == (len(pts), 1) and tri.dtype == np.uint32 and d.dtype == np.float32
    np.testing.assert_array_equal(tri[:, 0], want["tri"])
    np.testing.assert_array_equal(nr.bits(d[:, 0]), nr.bits(want["dist2"]))
    # ... bounded too, and the points that get no walk
    b = np.where(np.arange(len(pts)) % 2 == 0, want["dist2"], np.nextafter(want["dist2"], np.float32(0))).astype(np.float32)
    want = nr.brute(tris, pts, b)
    tri, d = kr.select_k(dist2, finite, 1, b)
    np.testing.assert_array_equal(tri[:, 0], want["tri"])
    np.testing.assert_array_equal(nr.bits(d[:, 0]), nr.bits(want["dist2"]))
    for bound in (-1.0, np.nan, -np.inf):
        tri, d = kr.select_k(dist2[:8], finite[:8], 3, bound)
        assert (tri == kr.NONE).all() and (d == -1).all()
    bad = pts[:3].copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    tri, d = kr.brute_k(tris, bad, 3)
    assert (tri == kr.NONE).all() and (d == -1).all()


def test_k_at_least_the_triangle_count_lists_every_triangle_in_order(case):
    _, _, tris, pts, dist2, finite = case
    T = len(tris)
    for k in (T, T + 20):
        tri, d = kr.select_k(dist2[:64], finite[:64], k)
        assert tri.shape == (64, k)
        assert (tri[:, T:] == kr.NONE).all() and (d[:, T:] == -1).all()
        for i in range(64):
            order = np.lexsort((np.arange(T), dist2[i]))          # by dist2, then by id
            np.testing.assert_array_equal(tri[i, :T], order)
            np.testing.assert_array_equal(nr.bits(d[i, :T]), nr.bits(dist2[i][order]))


@pytest.mark.parametrize("k", [1, 5, 32])
def test_the_bounds_edges(case, k):
    """max_dist2 equal to the j-th distance keeps exactly the members <= it; the next float below drops them."""
    _, _, tris, pts, dist2, finite = case
    T = len(tris)
    j = min(k, T)
    dj = np.sort(dist2, axis=1)[:, j - 1]
    tri, d = kr.select_k(dist2, finite, k, dj)
    members = np.minimum((dist2 <= dj[:, None]).sum(1), k)
    assert (members >= j).all()
    np.testing.assert_array_equal((tri != kr.NONE).sum(1), members)
    np.testing.assert_array_equal((d != -1).sum(1), members)
    assert (np.where(d == -1, np.float32(0), d) <= dj[:, None]).all()
    free_tri, free_d = kr.select_k(dist2, finite, k)
    np.testing.assert_array_equal(tri[:, :j], free_tri[:, :j])    # ... the unbounded list's first j
    pos = dj > 0
    assert pos.any()
    below = np.nextafter(dj, np.float32(0))
    tri, d = kr.select_k(dist2[pos], finite[pos], k, below[pos])
    want = np.minimum((dist2[pos] < dj[pos, None]).sum(1), k)
    assert (want < j).all()
    np.testing.assert_array_equal((tri != kr.NONE).sum(1), want)
    assert (np.where(d == -1, np.float32(0), d) < dj[pos, None]).all()


TIE_KS = {"Test": (1, 4, 8, 32), "Image_Test": (1, 4, 8, 32), "Rect": (1, 4)}


def test_the_tie_break_is_exercised(case):
    """Points whose k-th and (k+1)-th smallest dist2 are equal: there the list's last slot is decided by the id.
    Under the identity camera at least 32 of the 704 points for every k (measured with the restatement alone:
    Test 404 / 223 / 417 / 427, Image_Test 255 / 124 / 139 / 189, Rect 202 / 45); under the other camera the
    counts are printed only."""
    scene, cam, _, _, dist2, _ = case
    s = np.sort(dist2, axis=1)
    counts = {k: int((s[:, k - 1] == s[:, k]).sum()) for k in TIE_KS[scene]}
    print(f"{scene}/{cam}: points with equal k-th and (k+1)-th dist2: {counts}")
    if cam == "identity":
        assert all(c >= 32 for c in counts.values()), counts


# ---------------------------------------------------------------- the lemma, on the oracle's tree
def walk_knn(nodes, bd, d, k, bound):
    """The walk of rtbvh_knn_* for one point, in plain Python: `bd` the point's distance to every node's box, `d`
    its dist2 to every triangle (float32 values as Python floats compare as the floats do).  A sorted list of up to
    k (dist2, id), the worst key (bound, NONE) until it is full; a child, and a leaf's own box, is entered iff its
    distance is <= the worst key's dist2; the nearer child first.  Returns the list and the leaves visited."""
    n = (len(nodes) + 1) // 2
    lst, worst, leaves = [], (bound, kr.NONE), 0
    if not bound >= 0:
        return lst, leaves
    stack = [n if n > 1 else 0]
    index, cl, cr = nodes["index"], nodes["child_l"], nodes["child_r"]
    while stack:
        x = stack.pop()
        if x < n:   # a leaf
            leaves += 1
            t = int(index[x]) // 3
            if bd[x] <= worst[0]:
                cand = (d[t], t)
                if cand < worst:
                    bisect.insort(lst, cand)
                    del lst[k:]
                    if len(lst) == k:
                        worst = lst[-1]
            continue
        l, r = int(cl[x]), int(cr[x])
        lh, rh = bd[l] <= worst[0], bd[r] <= worst[0]
        if lh and rh:
            stack.extend((l, r) if bd[r] < bd[l] else (r, l))   # the nearer one on top
        elif lh or rh:
            stack.append(l if lh else r)
    return lst, leaves


@pytest.mark.parametrize("scene", SCENES)
def test_a_nearer_first_walk_pruned_on_the_worst_entry_is_the_brute_force(scene):
    d = load_scene_fixture(scene)
    wvp = rt.camera_reference(64, 48)[0]
    osc = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    nodes = orc.build(osc, wvp)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    T = len(tris)
    leaf = nr.leaf_data(tris)
    sort_order = nodes["index"][:T] // 3          # the oracle's leaves are in sort order
    np.testing.assert_array_equal(nodes["bb_min"][:T], leaf[3][sort_order])   # the leaf boxes are the records'
    np.testing.assert_array_equal(nodes["bb_max"][:T], leaf[4][sort_order])
    pts = nr.sample_points(tris, seed=21, n_random=40, n_each=8)[0]
    assert len(pts) == 64
    dist2, finite = kr.dist2_matrix(tris, pts)
    bd = nr.box_dist2(pts[:, None, :], nodes["bb_min"][None], nodes["bb_max"][None])
    visited = 0
    for k in (1, 5, 32):
        j = min(k, T)
        dj = np.sort(dist2, axis=1)[:, j - 1]
        cyc = np.arange(len(pts)) % 4   # half the j-th distance, exactly it, the float below it, 4 times it
        bounded = np.where(cyc == 0, np.float32(.5) * dj, np.where(cyc == 1, dj, np.where(
            cyc == 2, np.nextafter(dj, np.float32(0)), np.float32(4) * dj))).astype(np.float32)
        for bound in (np.full(len(pts), np.inf, np.float32), bounded):
            tri, dd = kr.select_k(dist2, finite, k, bound)
            for i in range(len(pts)):
                got, leaves = walk_knn(nodes, bd[i].tolist(), dist2[i].tolist(), k, float(bound[i]))
                visited += leaves
                m = int((tri[i] != kr.NONE).sum())
                assert [t for _, t in got] == tri[i, :m].tolist(), (k, i)
                assert [x for x, _ in got] == dd[i, :m].tolist(), (k, i)
    assert 0 < visited < 6 * 64 * T   # ... and the walk did prune
