"""First-k ray queries without a GPU: the ABI's names and constants, Context.khits' argument checks (which run before
the library is touched), the brute force (tests/khits_ref.py) and its edges, that the keys' clamp and tie-break are
exercised by the scenes the GPU tests use, and -- on the oracle's tree -- the lemma the GPU walk leans on (DESIGN.md
5j): a nearer-first walk that carries a k-list and enters a box iff it passes the slab test with the worst entry's
tk as the bound returns the brute-force list."""
import bisect
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import allhits_ref as ar
from tests import containment as cs
from tests import khits_ref as kh
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Test", "Rect", "Image_Test"]
KS = (1, 2, 7, 16)
INF = kh.INF


@pytest.fixture(scope="module", params=SCENES)
def case(request):
    """A golden scene under the identity camera, the tests' 704 rays and every ray's members (computed once)."""
    d = load_scene_fixture(request.param)
    tris = rw.clip_triangles(d["vertices"], d["indices"], np.eye(4, dtype=np.float32))
    o, dd = ar.sample_rays(tris, 400, 48, 200, 40)
    assert len(o) == 704
    lists = kh.members(tris, o, dd)
    for a in lists:
        a.setflags(write=False)
    return request.param, tris, o, dd, lists


@pytest.fixture(scope="module")
def stack():
    s = ar.stack_scene(40)
    tris = rw.clip_triangles(s.vertices, s.indices, np.eye(4, dtype=np.float32))
    o, d = ar.stack_rays()
    return tris, o, d, kh.members(tris, o, d)


# ---------------------------------------------------------------- the ABI
def test_exports_and_constants():
    L = rt.lib()
    for name in ("rtbvh_khits_async", "rtbvh_khits_host", "rtbvh_khits_counts"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.KHITS_SORT, rt.KHITS_COUNT, rt.KHITS_MAX_K) == (1 << 1, 1 << 2, 16)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    assert re.search(r"RTBVH_KHITS_SORT = 1u << 1\b", header) and re.search(r"RTBVH_KHITS_COUNT = 1u << 2\b", header)
    assert re.search(r"^#define RTBVH_KHITS_MAX_K 16$", header, re.M)
    for name in ("rtbvh_khits_async", "rtbvh_khits_host", "rtbvh_khits_counts"):
        assert re.search(rf"^rtbvh_status {name}\s*\(rtbvh_ctx\*", header, re.M), name
    assert re.search(r"rtbvh_signed_\*, rtbvh_khits_\* and", header)   # the calls that are NOT_READY after a vertex update
    assert hasattr(rt.Context, "khits") and hasattr(rt.Context, "khits_counts")
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_bad_arguments_are_rejected_before_the_library_is_called():
    import torch
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    f32 = np.float32
    ok = np.zeros((4, 8), f32)
    for k in (0, 17, -1, 2.5, None, "4", True):
        with pytest.raises(ValueError):
            ctx.khits(ok, k)
    bad = [np.zeros((4, 7), f32), np.zeros((4, 4), f32), np.zeros(8, f32), np.zeros((4, 8), np.float64),
           np.zeros((8, 8), f32)[::2], np.zeros((4, 16), f32)[:, :8], np.zeros((2, 2), rt.RAY_DTYPE),
           np.zeros(8, rt.RAY_DTYPE)[::2], [[0] * 8], None,
           torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.float64), torch.zeros((4, 7))]
    for b in bad:
        with pytest.raises(ValueError):
            ctx.khits(b, 4)
    for out in (np.zeros((3, 4), rt.HIT_DTYPE), np.zeros((4, 5), rt.HIT_DTYPE), np.zeros(16, rt.HIT_DTYPE),
                np.zeros((4, 4, 4), f32), np.zeros((4, 4), np.uint64), np.zeros((4, 8), rt.HIT_DTYPE)[:, ::2],
                np.zeros((8, 4), rt.HIT_DTYPE)[::2], torch.zeros((4, 4, 4))):
        with pytest.raises(ValueError):
            ctx.khits(ok, 4, out=out)
        with pytest.raises(ValueError):
            ctx.khits(np.zeros(4, rt.RAY_DTYPE), 4, out=out)


# ---------------------------------------------------------------- the brute force and its edges
def test_the_list_is_the_first_k_by_key(case):
    _, tris, o, d, lists = case
    off, hits, mn = lists
    key = kh.keys(hits, mn)
    cnt = np.diff(off.astype(np.int64))
    assert cnt.max() >= 2 and (cnt == 0).any()   # (short lists here: the stack scene has the long ones)
    for k in KS:
        got = kh.select_k(lists, k)
        assert got.shape == (704, k) and got.dtype == rt.HIT_DTYPE
        for i in range(704):
            seg = slice(int(off[i]), int(off[i + 1]))
            want = hits[seg][np.argsort(key[seg], kind="stable")][:k]
            m = len(want)
            np.testing.assert_array_equal(ar.hit_words(got[i, :m]), ar.hit_words(want))
            np.testing.assert_array_equal(ar.hit_words(got[i, m:]), ar.hit_words(kh.misses(1, k - m)[0]))


def test_k_above_the_list_length_pads_with_misses_and_keeps_the_set(case):
    _, tris, o, d, lists = case
    off, hits, mn = lists
    cnt = np.diff(off.astype(np.int64))
    got = kh.select_k(lists, 16)
    short = cnt <= 16
    assert short.sum() >= 600
    np.testing.assert_array_equal(kh.found(got).sum(1), np.minimum(cnt, 16))
    f = kh.found(got)
    assert (f[:, :-1] >= f[:, 1:]).all()                                   # the misses are at the end ...
    assert (got["t"][~f] == -1).all() and (got["u"][~f] == 0).all() and (got["v"][~f] == 0).all()
    by_t = ar.order_by_t(off, hits)                                        # ... and the set is allhits'
    for i in np.nonzero(short)[0]:
        seg = by_t[int(off[i]):int(off[i + 1])]
        assert sorted(got["tri"][i, :cnt[i]].tolist()) == sorted(seg["tri"].tolist())
    # slot 0 is a hit iff the list is not empty -- iff the closest-hit query hits (test_allhits_cpu)
    np.testing.assert_array_equal(kh.found(kh.select_k(lists, 1))[:, 0], cnt > 0)


def test_no_walk_rays_get_all_misses(case):
    _, tris, o, d, lists = case
    miss = ar.hit_words(kh.misses(1, 3)[0])
    for tm in (0.0, -0.0, -1.0, np.nan, -np.inf):
        got = kh.select_k(lists, 3, np.float32(tm))
        assert (ar.hit_words(got).reshape(-1, 3, 4) == miss).all(), tm
    o2, d2 = o[:6].copy(), d[:6].copy()
    o2[0, 0], o2[1, 1], d2[2, 2], d2[3] = np.inf, np.nan, -np.inf, 0
    got = kh.brute_k(tris, o2, d2, 3)
    assert (ar.hit_words(got[:4]).reshape(-1, 3, 4) == miss).all()


def test_t_max_at_a_members_t_keeps_it_and_the_float_below_drops_it(case):
    _, tris, o, d, lists = case
    tm, unlimited, cut = ar.mixed_t_max(tris, o, d, np.arange(len(tris)))
    np.testing.assert_array_equal(unlimited[0], lists[0])
    got = kh.select_k(lists, 16, tm)
    cnt = np.diff(cut[0].astype(np.int64))
    cnt_inf = np.diff(lists[0].astype(np.int64))
    assert ((cnt < cnt_inf) & (cnt > 0)).any() and ((cnt == 0) & (cnt_inf > 0)).any()
    np.testing.assert_array_equal(kh.found(got).sum(1), np.minimum(cnt, 16))
    at, below = 0, 0
    for i in range(0, 704, 3):
        if cnt_inf[i] == 0:
            continue
        tri = got["tri"][i][kh.found(got)[i]]
        seg = cut[1][int(cut[0][i]):int(cut[0][i + 1])]
        if cnt[i] <= 16:
            assert sorted(tri.tolist()) == sorted(seg["tri"].tolist())
        full = lists[1][int(lists[0][i]):int(lists[0][i + 1])]
        if i % 2 == 0:      # t_max is a member's t exactly: that member stays, unless its leaf box starts above its t
            full_mn = lists[2][int(lists[0][i]):int(lists[0][i + 1])]
            here = full["t"] == tm[i]
            assert here.any()
            assert set(full["tri"][here & ~(full_mn > tm[i])].tolist()) == set(seg["tri"][seg["t"] == tm[i]].tolist())
            at += int((seg["t"] == tm[i]).any())
        else:               # the float below: it is gone
            assert not (seg["t"] >= np.nextafter(tm[i], INF)).any()
            below += 1
    assert at >= 20 and below >= 20


# ---------------------------------------------------------------- the keys are exercised
def test_hits_below_their_leaf_boxs_entry_exist(case):
    """Members with t < mn, where the key is the box's entry and not t.  Measured with the restatement alone:
    Test 122 of 834, Rect 38 of 872, Image_Test 191 of 799."""
    name, _, _, _, (off, hits, mn) = case
    below = int((hits["t"] < mn).sum())
    print(f"{name}: {below} of {len(hits)} hits have t < mn")
    assert below > 0
    assert (kh.key_t(hits, mn) >= hits["t"]).all() and (kh.key_t(hits, mn) >= mn).all()


def test_the_stack_scene_cuts_between_equal_keys(stack):
    """stack_scene(40): 40-long lists (5,120 hits, 640 with t < mn), every eighth triangle a copy of the one before
    it, so k = 7 cuts between two entries of equal tk for the rays that cross the seventh and eighth at the same
    floats: the id decides.  Measured: 128 rays."""
    tris, o, d, lists = stack
    off, hits, mn = lists
    assert (np.diff(off.astype(np.int64)) == 40).all() and (hits["t"] < mn).sum() > 0
    got = kh.select_k(lists, 8)
    tk = np.zeros((len(o), 8), np.float32)
    for i in range(len(o)):
        seg = slice(int(off[i]), int(off[i + 1]))
        tk[i] = np.sort(kh.key_t(hits[seg], mn[seg]))[:8]
    ties = int((tk[:, 6] == tk[:, 7]).sum())
    print(f"stack_scene(40): {ties} rays with equal 7th and 8th tk")
    assert ties >= 64
    tied = tk[:, 6] == tk[:, 7]
    assert (got["tri"][tied, 6] < got["tri"][tied, 7]).all()
    np.testing.assert_array_equal(ar.hit_words(kh.select_k(lists, 7)), ar.hit_words(np.ascontiguousarray(got[:, :7])))


def test_the_containment_scene_orders_by_id():
    """tests/containment.py: A (id 0) and B (id 1) are coplanar, both leaf boxes start at exactly C on the pixel's
    ray, and both t's round below C with t_B < t_A: the keys tie at C, and A comes first."""
    s = cs.containment_scene(npad=64)
    tris = rw.clip_triangles(s.vertices, s.indices, np.eye(4, dtype=np.float32))
    o = np.float32([[2, -0.5, 0]])
    d = np.float32([[0, 0, 1]])
    off, hits, mn = kh.members(tris, o, d)
    assert sorted(hits["tri"].tolist()) == [0, 1] and (mn == cs.C).all()
    t = dict(zip(hits["tri"].tolist(), hits["t"].tolist()))
    assert t[1] < t[0] < cs.C
    one, two = kh.select_k((off, hits, mn), 1), kh.select_k((off, hits, mn), 2)
    assert one["tri"].tolist() == [[0]] and two["tri"].tolist() == [[0, 1]]
    assert two["t"][0, 1] < two["t"][0, 0]                       # the genuine t's, not the keys'
    assert ar.order_by_t(off, hits)["tri"].tolist() == [1, 0]    # where ALLHITS_BY_T's order differs


# ---------------------------------------------------------------- the lemma, on the oracle's tree
def walk_khits(nodes, base, mn, t, tri, k, tmax, prune=True):
    """The walk of rtbvh_khits_* for one ray, in plain Python: base[x] says whether node x's box passes the first two
    slab conditions, mn[x] is its slab entry, t[j] leaf j's triangle test (-1: rejected), tri[j] its id (float32
    values as Python floats compare as the floats do).  A sorted list of up to k (tk, id, leaf), the worst key
    (tmax, NONE) until it is full; a child's box, and a leaf's own at the leaf, is entered iff base and
    not mn > the worst key's tk; the nearer child first, left on a tie.  prune = False keeps the bound at tmax.
    Returns the list and the leaves visited."""
    n = (len(nodes) + 1) // 2
    none = int(kh.NONE)
    lst, worst, leaves = [], (tmax, none), 0
    cl, cr = nodes["child_l"], nodes["child_r"]

    def enter(x):
        return base[x] and not mn[x] > (worst[0] if prune else tmax)

    stack = [n if n > 1 else 0]
    while stack:
        x = stack.pop()
        if x < n:   # a leaf
            leaves += 1
            if enter(x) and t[x] != -1 and t[x] <= tmax:
                cand = (max(t[x], mn[x]), tri[x])
                if cand < worst[:2]:
                    bisect.insort(lst, cand + (x,))
                    del lst[k:]
                    if len(lst) == k:
                        worst = lst[-1]
            continue
        l, r = int(cl[x]), int(cr[x])
        lh, rh = enter(l), enter(r)
        if lh and rh:
            stack.extend((l, r) if mn[r] < mn[l] else (r, l))   # the nearer one on top
        elif lh or rh:
            stack.append(l if lh else r)
    return lst, leaves


@pytest.mark.parametrize("scene", SCENES)
def test_a_nearer_first_walk_pruned_on_the_worst_key_is_the_brute_force(scene):
    d = load_scene_fixture(scene)
    wvp = rt.camera_reference(64, 48)[0]
    osc = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    nodes = orc.build(osc, wvp)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    T = len(tris)
    lo, hi = nr.leaf_data(tris)[3:]
    leaf_tri = (nodes["index"][:T] // 3).astype(np.int64)          # the oracle's leaves are in sort order
    np.testing.assert_array_equal(nodes["bb_min"][:T], lo[leaf_tri])   # the leaf boxes are the records'
    np.testing.assert_array_equal(nodes["bb_max"][:T], hi[leaf_tri])
    o, dd = ar.sample_rays(tris, 24, 8, 8, 8, seed=21)             # with axis-parallel and in-plane rays
    assert len(o) == 64
    lists = kh.members(tris, o, dd)
    tm_mixed = ar.mixed_t_max(tris, o, dd, np.arange(T))[0]
    walked = ar.walked(o, dd, np.full(64, INF, np.float32))
    pruned = unpruned = 0
    per_ray = []
    for i in range(64):
        oo, di = np.repeat(o[i][None], len(nodes), 0), np.repeat(dd[i][None], len(nodes), 0)
        with np.errstate(all="ignore"):
            inv = (np.float32(1) / di).astype(np.float32)
            base, mn = rw._box(nodes["bb_min"], nodes["bb_max"], oo, inv)
        t = rw.tri_test(tris, leaf_tri, oo[:T], di[:T])[0]
        per_ray.append((base.tolist(), mn.tolist(), t.tolist()))
    for tm in (np.full(64, INF, np.float32), tm_mixed):
        for k in KS:
            want = kh.select_k(lists, k, tm)
            for i in range(64):
                m = int(kh.found(want)[i].sum())
                if not (walked[i] and tm[i] > 0):
                    assert m == 0
                    continue
                base, mn, t = per_ray[i]
                got, leaves = walk_khits(nodes, base, mn, t, leaf_tri.tolist(), k, float(tm[i]))
                pruned += leaves
                unpruned += walk_khits(nodes, base, mn, t, leaf_tri.tolist(), k, float(tm[i]), prune=False)[1]
                assert [x[1] for x in got] == want["tri"][i, :m].tolist(), (k, i)
                assert [t[x[2]] for x in got] == want["t"][i, :m].tolist(), (k, i)
    print(f"{scene}: leaves visited {pruned} pruned, {unpruned} with the bound fixed at t_max")
    assert 0 < pruned < unpruned   # ... and the walk did prune
