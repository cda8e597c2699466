"""Clearance queries without a GPU: the ABI's names and Context.clearance's argument checks, and the numpy
restatement of the rule (tests/clearance_ref.py) -- the pruning lemma the GPU walk leans on, the restatement's accuracy
against its own float64 evaluation, the crossing override, the tie to the closest-point query and the bound's edges --
on the three golden scenes under both test cameras."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from raytracebvh_amd import _lib
from tests import clearance_ref as clr
from tests import cross_ref as xr
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Rect", "Test", "Image_Test"]
CAMERAS = ["reference", "identity"]
NAMES = ("rtbvh_clearance_async", "rtbvh_clearance_host", "rtbvh_clearance_counts")
NRANDOM = 512
# random_queries under the identity camera, from the reference alone: the queries that cross a triangle, and those
# with more than one triangle at the minimum
IDENTITY_CROSSING = {"Rect": 110, "Test": 71, "Image_Test": 110}
IDENTITY_TIES = {"Rect": 21, "Test": 229, "Image_Test": 78}
# Worst |sqrt(dist2) in float32 - sqrt(dist2) in float64| over all pairs of the random and the special queries with
# the scene's triangles, without the override, in units of 2^-24 of the root box's diagonal, as measured:
#   Rect 1.243 (identity) 1.772 (reference), Test 1.171 / 1.870, Image_Test 1.417 / 2.796
# The bound is four times the worst of them.
ACCURACY_MEASURED = 2.796
ACCURACY_BOUND = 4 * ACCURACY_MEASURED


def camera(name):
    return rt.camera_reference(64, 48)[0] if name == "reference" else np.eye(4, dtype=np.float32)


class Case:
    """A golden scene under one camera: its triangles, the three query sets in one array -- cross_ref.random_queries,
    the scene's own triangles, cross_ref.special_queries -- and dist2 of every pair, with and without the override
    (once)."""

    def __init__(self, scene, cam):
        d = load_scene_fixture(scene)
        self.tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
        self.T = len(self.tris)
        special, self.names = xr.special_queries(self.tris)
        self.q = np.concatenate([xr.random_queries(self.tris, NRANDOM), self.tris, special])
        self.special = NRANDOM + self.T
        self.valid = clr.valid_queries(self.q)
        self.feature = clr.matrix(self.tris, self.q, override=False)
        k, j = xr.member_pairs(self.tris, self.q)
        self.members = (k, j)
        self.dist = self.feature.copy()
        self.dist[k, j] = np.float32(0)
        lo, hi = nr.root_box(self.tris)
        self.diagonal = float(np.linalg.norm(hi.astype(np.float64) - lo.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def case(scene, cam):
    return Case(scene, cam)


# ---------------------------------------------------------------- 1. the ABI
def test_exports_and_constants():
    L = rt.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.CLEARANCE_SORT, rt.CLEARANCE_COUNT) == (1 << 1, 1 << 2)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    for name, bit in (("SORT", 1), ("COUNT", 2)):
        assert re.search(rf"RTBVH_CLEARANCE_{name} = 1u << {bit}\b", header), name
    for name in NAMES:
        assert re.search(rf"rtbvh_status {name}\s*\(", header), name
    assert re.search(r"\}\s*rtbvh_clearance;", header)
    for name in ("clearance", "clearance_counts"):
        assert callable(getattr(rt.Context, name)), name
    assert rt.CLEARANCE_DTYPE.itemsize == 32
    assert [rt.CLEARANCE_DTYPE.fields[f][1] for f in ("point_q", "dist2", "point_x", "tri")] == [0, 12, 16, 28]
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_make_tris_round_trip():
    """The query buffer is cross()'s: the same packing serves both calls."""
    v = np.random.default_rng(3).random((5, 3, 3)).astype(np.float32)
    t = rt.make_tris(v)
    assert t.dtype == rt.TRI_DTYPE
    np.testing.assert_array_equal(np.stack([t["v0"], t["v1"], t["v2"]], 1), v)
    np.testing.assert_array_equal(rt.make_tris(v.reshape(5, 9)), t)
    kind, got = rt.check_cross_tris(t)
    assert kind == "numpy" and got.ctypes.data == t.ctypes.data


def test_bad_arguments_are_rejected_before_the_library_is_called():
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    t = rt.make_tris(np.zeros((4, 3, 3)))
    for mode in (1, 8, 16, 32, 1 << 6, rt.CLEARANCE_SORT | 1):
        with pytest.raises(ValueError):
            ctx.clearance(t, mode=mode)
    with pytest.raises(ValueError):
        ctx.clearance(t, stream=1)               # a stream goes with the device entry
    for bad in (np.zeros((4, 8), np.float32), np.zeros((4, 3, 4), np.float32), np.zeros((4, 12), np.float64),
                np.zeros(36, np.float32), [[0.0] * 9] * 4, None):
        with pytest.raises(ValueError):
            ctx.clearance(bad)
    import torch
    with pytest.raises(ValueError):
        ctx.clearance(torch.zeros((4, 12)))      # a CPU tensor
    for bound in ("far", None, [1.0, 2.0], np.ones(4, np.float32)):
        with pytest.raises(ValueError):
            ctx.clearance(t, bound)
    L = rt.lib()
    out = np.zeros(4, rt.CLEARANCE_DTYPE)
    cnt = np.zeros(4, np.uint64)
    p, o = ctypes.c_void_p(t.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert L.rtbvh_clearance_async(None, p, 4, 1.0, o, 0, None) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_clearance_host(None, p, 4, 1.0, o, 0) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_clearance_counts(None, ctypes.c_void_p(cnt.ctypes.data)) == _lib.ERR_INVALID_ARG
    assert not out.view(np.uint32).any() and not cnt.any()


def test_not_ready_and_invalid_arg_through_the_host_entry():
    """The checks that come before any device work, on a context that was never given a scene.  A context needs a
    device to exist: where there is none, creating it fails with that status and the NULL-context checks above are
    all a host can ask (tests/test_clearance_gpu.py repeats these on a built context)."""
    try:
        ctx = rt.Context(device=0)
    except rt.RtbvhError as e:
        assert e.status == _lib.ERR_NO_DEVICE
        return
    with ctx:
        L = rt.lib()
        t = rt.make_tris(np.zeros((4, 3, 3)))
        out = np.zeros(4, rt.CLEARANCE_DTYPE)
        p, o = ctypes.c_void_p(t.ctypes.data), ctypes.c_void_p(out.ctypes.data)
        assert L.rtbvh_clearance_host(ctx._h, p, 0, 1.0, o, 0) == _lib.OK                     # n == 0: nothing
        assert L.rtbvh_clearance_host(ctx._h, None, 0, 1.0, None, 0) == _lib.OK
        assert L.rtbvh_clearance_host(ctx._h, p, 4, 1.0, o, 0) == _lib.ERR_NOT_READY
        for mode in (1, 8, 16, 1 << 31):
            assert L.rtbvh_clearance_host(ctx._h, p, 4, 1.0, o, mode) == _lib.ERR_INVALID_ARG, mode
        assert L.rtbvh_clearance_host(ctx._h, None, 4, 1.0, o, 0) == _lib.ERR_INVALID_ARG
        assert L.rtbvh_clearance_host(ctx._h, p, 4, 1.0, None, 0) == _lib.ERR_INVALID_ARG
        assert L.rtbvh_clearance_host(ctx._h, p, 1 << 31, 1.0, o, 0) == _lib.ERR_INVALID_ARG
        assert not out.view(np.uint32).any()
        with pytest.raises(rt.RtbvhError) as e:
            ctx.clearance_counts()
        assert e.value.status == _lib.ERR_NOT_READY


# ---------------------------------------------------------------- 2. the pruning lemma
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_dist2_is_never_below_the_box_box_distance(scene, cam):
    """dist2(q, x) >= bb(q, x's leaf box) for every pair; bb is monotone in the box (a larger box lowers every dk),
    so the same holds for every box of the tree around the leaf: the root box is checked too."""
    c = case(scene, cam)
    lo, hi = nr.leaf_data(c.tris)[3:]
    q = c.q[c.valid]
    d = c.dist[c.valid]
    assert not np.isnan(d).any()
    b = clr.bb(q[:, None], lo[None], hi[None])
    assert int((~(d >= b)).sum()) == 0
    assert int((~(c.feature[c.valid] >= b)).sum()) == 0           # (without the override too)
    rlo, rhi = nr.root_box(c.tris)
    assert (clr.bb(q[:, None], rlo[None, None], rhi[None, None]) <= b).all()
    assert (b > 0).any() and (b == 0).any()                       # the lemma is not empty on these inputs


def walk(nodes, lo, hi, q, dist, bound, limit=1 << 30, deepest=None):
    """k_clearance's walk for one query in plain Python on the oracle's tree: a box is entered iff its box-box
    distance is <= the best dist2 so far, the nearer child first; `dist[position]` is the pair's dist2.  Returns
    (dist2, position) of the best, position -1 for none.  A node whose two children both pass with the stack at
    `limit` loses both.  `deepest`, a list, receives the deepest stack entry stored and the number of nodes lost."""
    n = (len(nodes) + 1) // 2
    cl, cr_ = nodes["child_l"], nodes["child_r"]
    bb = lambda c: clr.bb(q, lo[c], hi[c])
    best, at, deep, lost = np.float32(bound), -1, -1, 0
    stack, node = [], (n if n > 1 else 0)
    while True:
        if node < n:
            if bb(node) <= best and (dist[node] < best or (dist[node] == best and at == -1)):
                best, at = dist[node], node        # (positions differ: the id tie-break is the GPU tests')
        else:
            l, r = int(cl[node]), int(cr_[node])
            bl, br = bb(l), bb(r)
            lh, rh = bl <= best, br <= best
            if lh and rh and len(stack) + 1 >= limit:
                lost += 1
            elif lh or rh:
                swap = lh and rh and br < bl
                if lh and rh:
                    deep = max(deep, len(stack))
                    stack.append(l if swap else r)
                node = r if swap else (l if lh else r)
                continue
        if not stack:
            break
        node = stack.pop()
    if deepest is not None:
        deepest[:] = [deep, lost]
    return best, at


def test_walk_on_the_oracles_tree_finds_the_minimum_and_the_fan_takes_it_deep():
    """The lemma at work on a real tree (Test, reference camera): the pruned walk ends at the brute-force minimum.
    And the scene and queries test_clearance_gpu.py uses for the deep walk: every fan query's walk stores entries at
    and past 16 (trace.hip SB) and loses subtrees at that test's limits of 18 and 8."""
    from oracle import lib as orc
    from tests import collide_ref as cr
    d = load_scene_fixture("Test")
    wvp = camera("reference")
    c = case("Test", "reference")
    nodes = orc.build(orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]), wvp)
    order = nodes["index"][:c.T] // 3
    lo, hi = nodes["bb_min"], nodes["bb_max"]
    for i in list(range(0, NRANDOM, 16)) + [c.special + 2, c.special + 3, c.special + 5]:
        row = c.dist[i][order]
        for bound in (np.inf, np.float32(np.median(row))):
            best, at = walk(nodes, lo, hi, c.q[i], row, bound)
            assert at >= 0 and best == row.min(), i
    s = cr.thick_fan()
    nodes = orc.build(orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob), np.eye(4, dtype=np.float32))
    tris = rw.clip_triangles(s.vertices, s.indices, np.eye(4, dtype=np.float32))
    T = len(tris)
    order = nodes["index"][:T] // 3
    lo, hi = nodes["bb_min"], nodes["bb_max"]
    q = xr.fan_queries()
    dist = clr.matrix(tris, q)
    lost = {18: 0, 8: 0}
    for i in range(len(q)):
        row = dist[i][order]
        deep = []
        best, at = walk(nodes, lo, hi, q[i], row, np.inf, deepest=deep)
        assert best == row.min() and deep[0] >= 16 + 2, i
        for limit in lost:
            cut, at = walk(nodes, lo, hi, q[i], row, np.inf, limit=limit, deepest=deep)
            assert at >= 0 and cut >= best
            lost[limit] += deep[1] > 0
    assert lost[18] and lost[8] == len(q)


# ---------------------------------------------------------------- 3. fp32 against fp64
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_restatement_is_accurate(scene, cam):
    c = case(scene, cam)
    pick = np.r_[0:NRANDOM, c.special:len(c.q)]
    pick = pick[c.valid[pick]]
    d64 = clr.matrix(c.tris, c.q[pick], np.float64, override=False)
    err = np.abs(np.sqrt(c.feature[pick].astype(np.float64)) - np.sqrt(d64)) / c.diagonal * 2.0 ** 24
    print(f"{scene}/{cam}: worst error {err.max():.3f} x 2^-24 of the diagonal")
    assert err.max() <= ACCURACY_BOUND


# ---------------------------------------------------------------- 4. the override
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_crossing_pairs_have_distance_zero_only_by_the_override(scene, cam):
    c = case(scene, cam)
    k, j = c.members
    rnd = k < NRANDOM
    crossing = np.zeros(NRANDOM, bool)
    crossing[k[rnd]] = True
    print(f"{scene}/{cam}: {int(crossing.sum())} of {NRANDOM} random queries cross")
    assert crossing.sum() >= 32 and (~crossing).sum() >= 32
    if cam == "identity":
        assert int(crossing.sum()) == IDENTITY_CROSSING[scene]
    d = clr.pair_dist2(c.q[k], c.tris[j])[0]                      # the rule itself, pair by pair
    assert (d == 0).all() and not np.signbit(d).any()
    np.testing.assert_array_equal(d, c.dist[k, j])
    without = c.feature[k, j]
    assert (without > 0).any()                                    # the feature distance alone misses crossings
    print(f"  feature distance over the crossing pairs: {without.min():.3g} .. {np.sqrt(without.max()) / c.diagonal:.3%}"
          f" of the diagonal")
    assert (clr.pair_dist2(c.q[k], c.tris[j], override=False)[0] == without).all()


# ---------------------------------------------------------------- 5. the tie to the closest-point query
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_a_point_triangle_is_no_farther_than_nearest(scene, cam):
    c = case(scene, cam)
    pts = nr.sample_points(c.tris, n_random=128, n_each=16)[0]
    q = np.repeat(pts[:, None, :], 3, 1)
    got = clr.brute(c.tris, q)
    want = nr.brute(c.tris, pts)
    assert got["found"].all() and want["found"].all()
    assert (got["dist2"] <= want["dist2"]).all()
    # candidates 0..2 are the closest-point formula's bits
    ql, xl = clr.leaf(q[:, None]), clr.leaf(c.tris[None])
    cand = clr.candidates(ql, xl)
    d = nr.tri_dist2(pts[:, None, :], *nr.leaf_data(c.tris))[0]
    for i in range(3):
        np.testing.assert_array_equal(nr.bits(cand[i][0]), nr.bits(d))


# ---------------------------------------------------------------- 6. the bound's edges
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_bound_edges(scene, cam):
    c = case(scene, cam)
    n = NRANDOM
    q, dist = c.q[:n], c.dist[:n]
    free = clr.brute(c.tris, q, dist=dist)
    assert free["found"].all()
    if cam == "identity":
        assert int((free["ties"] > 1).sum()) == IDENTITY_TIES[scene]
    for i in (0, 1, 2, 3, 100, 511):
        own = free["dist2"][i]
        at = clr.brute(c.tris, q[i:i + 1], own, dist=dist[i:i + 1])
        assert at["found"][0] and at["tri"][0] == free["tri"][i] and at["dist2"][0] == own
        if own > 0:
            below = clr.brute(c.tris, q[i:i + 1], np.nextafter(own, np.float32(-1)), dist=dist[i:i + 1])
            assert not below["found"][0] and below["dist2"][0] == -1 and below["tri"][0] == clr.NONE
    zero = clr.brute(c.tris, q, 0.0, dist=dist)
    np.testing.assert_array_equal(zero["found"], free["dist2"] == 0)
    np.testing.assert_array_equal(clr.brute(c.tris, q, -0.0, dist=dist)["found"], zero["found"])
    for bad in (np.nan, -1.0, -np.inf):
        assert not clr.brute(c.tris, q, bad, dist=dist)["found"].any()
    median = np.float32(np.median(free["dist2"]))
    mid = clr.brute(c.tris, q, median, dist=dist)
    assert mid["found"].any() and not mid["found"].all()
    np.testing.assert_array_equal(mid["found"], free["dist2"] <= median)
    for f in ("dist2", "tri", "point_q", "point_x"):
        np.testing.assert_array_equal(mid[f][mid["found"]], free[f][mid["found"]])
    # the special queries: no result for the non-finite ones, a result for the point and the needles
    sp = clr.brute(c.tris, c.q[c.special:], dist=c.dist[c.special:])
    assert dict(zip(c.names, sp["found"].tolist())) == {n_: n_ not in ("NaN", "infinite") for n_ in c.names}
