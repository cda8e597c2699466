"""Radius queries without a GPU: the ABI's names and layouts, Context.within's argument checks, the brute force
(tests/within_ref.py) against the closest-point restatement, and -- on the oracle's tree -- the two properties the
GPU walk leans on: pruning on the box distance skips no member, and a left-first depth-first walk meets the
triangles in the build's sort order."""
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests import within_ref as wr
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]


def camera(name):
    return rt.camera_reference(64, 48)[0] if name == "reference" else np.eye(4, dtype=np.float32)


# ---------------------------------------------------------------- the ABI
def test_exports_constants_and_sizes():
    L = rt.lib()
    for name in ("rtbvh_within_async", "rtbvh_within_host", "rtbvh_within_counts"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.WITHIN_SORT, rt.WITHIN_COUNT, rt.WITHIN_SIZES, rt.WITHIN_FILL) == (1 << 1, 1 << 2, 1 << 4, 1 << 5)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    for name, bit in (("SORT", 1), ("COUNT", 2), ("SIZES", 4), ("FILL", 5)):
        assert re.search(rf"RTBVH_WITHIN_{name} = 1u << {bit}\b", header), name
    assert rt.PAIR_DTYPE.itemsize == 8 == wr.PAIR_DTYPE.itemsize and rt.PAIR_DTYPE == wr.PAIR_DTYPE
    assert [rt.PAIR_DTYPE.fields[f][1] for f in ("tri", "dist2")] == [0, 4]
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_bad_arguments_are_rejected_before_the_library_is_called():
    import torch
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    f32 = np.float32
    bad = [np.zeros((4, 5), f32), np.zeros((4, 2), f32), np.zeros(4, f32), np.zeros((4, 3), np.float64),
           np.zeros((8, 4), f32)[::2], np.zeros((2, 2), rt.POINT_DTYPE), [[0, 0, 0]], None,
           torch.zeros((4, 4)), torch.zeros((4, 3)), torch.zeros((4, 4), dtype=torch.float64)]
    for b in bad:
        with pytest.raises(ValueError):
            ctx.within(b)
    with pytest.raises(ValueError):
        ctx.within(np.zeros((4, 3), f32), max_dist2=np.zeros(3, f32))    # 4 points, 3 bounds
    with pytest.raises(ValueError):
        ctx.within(np.zeros((4, 4), f32), max_dist2=1.0)                 # the bound is the fourth column
    for mode in (rt.WITHIN_SIZES, rt.WITHIN_FILL):                       # within sets these itself
        with pytest.raises(ValueError):
            ctx.within(np.zeros((4, 3), f32), mode=mode)
    for capacity in (-1, 1.5):
        with pytest.raises(ValueError):
            ctx.within(np.zeros((4, 3), f32), capacity=capacity)


# ---------------------------------------------------------------- the brute force
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_brute_within_against_the_closest_point_restatement(scene, cam):
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
    pts = nr.sample_points(tris)[0]
    T = len(tris)
    rank = np.random.default_rng(7).permutation(T)     # any order: membership does not depend on it
    want = nr.brute(tris, pts)
    dmin = want["dist2"]
    off, pairs = wr.brute_within(tris, pts, dmin, rank)
    assert off.dtype == np.uint64 and off.shape == (len(pts) + 1,) and pairs.dtype == wr.PAIR_DTYPE
    assert off[0] == 0 and off[-1] == len(pairs)
    np.testing.assert_array_equal(np.diff(off).astype(np.int64), want["ties"])   # exactly the minimum's triangles
    np.testing.assert_array_equal(nr.bits(pairs["dist2"]), nr.bits(np.repeat(dmin, want["ties"])))
    first = off[:-1].astype(np.int64)
    np.testing.assert_array_equal(np.minimum.reduceat(pairs["tri"], first), want["tri"])   # the smallest id wins there
    for k in range(len(pts)):                                                    # each list ascending by rank
        r = rank[pairs["tri"][int(off[k]):int(off[k + 1])]]
        assert (np.diff(r) > 0).all()
    pos = dmin > 0
    assert pos.any()
    off0, pairs0 = wr.brute_within(tris, pts[pos], np.nextafter(dmin[pos], np.float32(0)), rank)
    assert off0[-1] == 0 and len(pairs0) == 0
    # no walk: an empty list; +inf: every triangle, in rank order
    for b in (-1.0, np.nan, -np.inf, -1e-30):
        assert wr.brute_within(tris, pts[:8], b, rank)[0][-1] == 0
    bad = pts[:3].copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    assert wr.brute_within(tris, bad, np.inf, rank)[0][-1] == 0
    off, pairs = wr.brute_within(tris, pts[:4], np.inf, rank)
    np.testing.assert_array_equal(off, np.arange(5, dtype=np.uint64) * np.uint64(T))
    np.testing.assert_array_equal(pairs["tri"][:T], np.argsort(rank))
    z = wr.brute_within(tris, tris[:4, 0], -0.0, rank)                           # -0 is +0: the vertex's triangles
    assert (np.diff(z[0]) >= 1).all() and (z[1]["dist2"] == 0).all()


# ---------------------------------------------------------------- the walk's order and pruning, on the oracle's tree
def dfs_within(nodes, leaf, p, bound, out):
    """The left-first depth-first walk of rtbvh_within_* for one point, in plain Python: a child is entered iff its
    box distance is <= bound; a leaf's own box first, then its triangle."""
    n = (len(nodes) + 1) // 2
    a, e1, e2, lo, hi = leaf
    bmin, bmax = nodes["bb_min"], nodes["bb_max"]
    stack = [n if n > 1 else 0]
    while stack:
        k = stack.pop()
        if k < n:   # a leaf
            t = int(nodes["index"][k]) // 3
            if nr.box_dist2(p, lo[t], hi[t]) <= bound:
                d = nr.tri_dist2(p, a[t], e1[t], e2[t], lo[t], hi[t])[0]
                if d <= bound:
                    out.append((t, d))
            continue
        l, r = int(nodes["child_l"][k]), int(nodes["child_r"][k])
        if nr.box_dist2(p, bmin[r], bmax[r]) <= bound:
            stack.append(r)   # below the left one: walked after it
        if nr.box_dist2(p, bmin[l], bmax[l]) <= bound:
            stack.append(l)


@pytest.mark.parametrize("scene", ["Rect", "Test"])
def test_left_first_walk_with_box_pruning_is_the_brute_force_in_sort_order(scene):
    d = load_scene_fixture(scene)
    wvp = rt.camera_reference(64, 48)[0]
    osc = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    nodes = orc.build(osc, wvp)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    T = len(tris)
    leaf = nr.leaf_data(tris)
    sort_order = nodes["index"][:T] // 3          # the oracle's leaves are in sort order
    assert sorted(sort_order.tolist()) == list(range(T))
    np.testing.assert_array_equal(nodes["bb_min"][:T], leaf[3][sort_order])   # the leaf boxes are the records'
    np.testing.assert_array_equal(nodes["bb_max"][:T], leaf[4][sort_order])
    rank = wr.rank_of(sort_order)
    lo, hi = nr.root_box(tris)
    bound = np.float32((np.float32(0.05) * np.float32(np.sqrt(((hi - lo) ** 2).sum()))) ** 2)
    pts = nr.sample_points(tris, seed=21, n_random=40, n_each=8)[0]
    assert len(pts) == 64
    want_off, want = wr.brute_within(tris, pts, bound, rank)
    assert 0 < want_off[-1] < 64 * T   # some lists, and pruning to do
    got, off = [], [0]
    for p in pts:
        dfs_within(nodes, leaf, p, bound, got)
        off.append(len(got))
    pairs = np.zeros(len(got), wr.PAIR_DTYPE)
    pairs["tri"] = [g[0] for g in got]
    pairs["dist2"] = [g[1] for g in got]
    np.testing.assert_array_equal(np.array(off, np.uint64), want_off)
    np.testing.assert_array_equal(wr.pair_bits(pairs), wr.pair_bits(want))
