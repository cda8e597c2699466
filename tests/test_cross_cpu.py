"""Triangle queries without a GPU: the ABI's names, make_tris, check_cross_tris and Context.cross's argument checks,
the brute force (tests/cross_ref.py), its tie to the self-collision specification, and on the oracle's trees the two
properties the GPU walk leans on -- pruning on (B) skips no member, and a left-first walk meets the members in list
order, so the first one met is the list's head."""
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import collide_ref as cr
from tests import cross_ref as xr
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests import within_ref as wr
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Rect", "Test", "Image_Test"]
CAMERAS = ["reference", "identity"]
NAMES = ("rtbvh_cross_async", "rtbvh_cross_host", "rtbvh_cross_first_async", "rtbvh_cross_first_host",
         "rtbvh_cross_counts")
# the scene's own triangles as queries under the identity camera, entries that share a vertex index removed: twice
# collide's 31, 4,406 and 1,465 pairs
OWN_COUNTS = {"Rect": 62, "Test": 8_812, "Image_Test": 2_930}


def camera(name):
    return rt.camera_reference(64, 48)[0] if name == "reference" else np.eye(4, dtype=np.float32)


def clip_tris(scene, cam):
    d = load_scene_fixture(scene)
    return d, rw.clip_triangles(d["vertices"], d["indices"], camera(cam))


# ---------------------------------------------------------------- 1. the ABI
def test_exports_and_constants():
    L = rt.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.CROSS_SORT, rt.CROSS_COUNT, rt.CROSS_SIZES, rt.CROSS_FILL) == (1 << 1, 1 << 2, 1 << 4, 1 << 5)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    for name, bit in (("SORT", 1), ("COUNT", 2), ("SIZES", 4), ("FILL", 5)):
        assert re.search(rf"RTBVH_CROSS_{name} = 1u << {bit}\b", header), name
    for name in NAMES:
        assert re.search(rf"rtbvh_status {name}\s*\(", header), name
    assert re.search(r"\}\s*rtbvh_tri;", header)
    for name in ("cross", "cross_first", "cross_pairs", "cross_counts"):
        assert callable(getattr(rt.Context, name)), name
    assert rt.TRI_DTYPE.itemsize == 48
    assert [rt.TRI_DTYPE.fields[f][1] for f in ("v0", "v1", "v2")] == [0, 16, 32]
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


# ---------------------------------------------------------------- 2. inputs and arguments
def test_make_tris_packs_vertices():
    v = np.arange(18, dtype=np.float64).reshape(2, 3, 3)
    for given in (v, v.reshape(2, 9), v.astype(np.float32), v.tolist()):
        t = rt.make_tris(given)
        assert t.dtype == rt.TRI_DTYPE and t.shape == (2,)
        for k, f in enumerate(("v0", "v1", "v2")):
            np.testing.assert_array_equal(t[f], v[:, k].astype(np.float32))
        assert not t["reserved0"].any() and not t["reserved1"].any() and not t["reserved2"].any()
    flat = rt.make_tris(v).view(np.float32).reshape(-1, 12)
    np.testing.assert_array_equal(flat[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], v.reshape(2, 9))
    assert rt.make_tris(np.zeros((0, 3, 3))).shape == (0,)
    for bad in (np.zeros((2, 3)), np.zeros((2, 8)), np.zeros((2, 3, 4)), np.zeros(9), np.zeros((2, 2, 3, 3))):
        with pytest.raises(ValueError):
            rt.make_tris(bad)
    import torch
    t = rt.make_tris(torch.from_numpy(v))
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 12) and t.device.type == "cpu"
    np.testing.assert_array_equal(t.numpy(), flat)
    np.testing.assert_array_equal(rt.make_tris(torch.from_numpy(v.reshape(2, 9))).numpy(), flat)
    with pytest.raises(ValueError):
        rt.make_tris(torch.zeros(2, 8))


def test_check_cross_tris():
    t = rt.make_tris(np.random.default_rng(1).random((5, 3, 3)))
    kind, got = rt.check_cross_tris(t)
    assert kind == "numpy" and got.dtype == rt.TRI_DTYPE and got.shape == (5,)
    assert got.ctypes.data == t.ctypes.data                                   # no copy
    kind, got = rt.check_cross_tris(t.view(np.float32).reshape(-1, 12))
    assert kind == "numpy" and got.dtype == rt.TRI_DTYPE and got.shape == (5,)
    f = t.view(np.float32).reshape(-1, 12)
    import torch
    for bad in (f.astype(np.float64), f.reshape(-1), f[:, :9], f.reshape(5, 3, 4), f[::2], t.reshape(5, 1), t[::2],
                np.asfortranarray(f), f.tolist(), None, torch.from_numpy(f),      # a CPU tensor
                torch.zeros((5, 12), dtype=torch.float64), torch.zeros((5, 9)), torch.zeros(60)):
        with pytest.raises(ValueError):
            rt.check_cross_tris(bad)


def test_bad_arguments_are_rejected_before_the_library_is_called():
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    t = rt.make_tris(np.zeros((4, 3, 3)))
    for mode in (rt.CROSS_SIZES, rt.CROSS_FILL, rt.CROSS_SIZES | rt.CROSS_SORT, 1, 8, 1 << 6, 1 << 7):
        with pytest.raises(ValueError):
            ctx.cross(t, mode)
    for mode in (rt.CROSS_SIZES, rt.CROSS_FILL, 1, 8, 1 << 6):
        with pytest.raises(ValueError):
            ctx.cross_first(t, mode)
    for capacity in (-1, 1.5):
        with pytest.raises(ValueError):
            ctx.cross(t, capacity=capacity)
    with pytest.raises(ValueError):
        ctx.cross(t, capacity=4, sizes_only=True)
    with pytest.raises(ValueError):
        ctx.cross(t, stream=1)               # a stream goes with the device entry
    with pytest.raises(ValueError):
        ctx.cross(np.zeros((4, 9), np.float32))
    with pytest.raises(ValueError):
        ctx.cross_first(np.zeros((4, 9), np.float32))
    for out in (np.zeros(4, np.int32), np.zeros(3, np.uint32), np.zeros(8, np.uint32)[::2], [0] * 4):
        with pytest.raises(ValueError):
            ctx.cross_first(t, out=out)
    L = rt.lib()
    off = np.zeros(5, np.uint64)
    ids = np.zeros(4, np.uint32)
    p, o, i = (ctypes.c_void_p(a.ctypes.data) for a in (t, off, ids))
    assert L.rtbvh_cross_async(None, p, 4, o, i, 4, 0, None) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_cross_host(None, p, 4, o, i, 4, 0) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_cross_first_async(None, p, 4, i, 0, None) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_cross_first_host(None, p, 4, i, 0) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_cross_counts(None, o) == _lib.ERR_INVALID_ARG
    assert not off.any() and not ids.any()


# ---------------------------------------------------------------- the brute force
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_golden_scenes_have_something_to_find(scene, cam):
    """What test_cross_gpu.py asserts from the reference before it compares, on the CPU first."""
    d, tris = clip_tris(scene, cam)
    T = len(tris)
    q = xr.random_queries(tris)
    assert q.shape == (512, 3, 3) and q.dtype == np.float32
    st = []
    off, ids = xr.brute_cross(tris, q, np.arange(T), st)
    print(f"{scene}/{cam}: box pairs {st[0]}, members {st[1]}, shape {xr.shape_of(off)}")
    assert 0 < st[1] < st[0] < len(q) * T and int(off[-1]) == st[1] == len(ids)
    if cam == "identity":
        assert xr.shape_of(off) == xr.IDENTITY_COUNTS[scene]
    np.testing.assert_array_equal(xr.first_of(off, ids)[np.diff(off.astype(np.int64)) == 0], xr.NONE)
    # a query is what a leaf record would hold of it: the scene's own triangles give the scene's own leaf floats
    for got, want in zip(nr.leaf_data(rt.make_tris(tris).view(np.float32).reshape(-1, 3, 4)[:, :, :3]),
                         nr.leaf_data(tris)):
        np.testing.assert_array_equal(nr.bits(got), nr.bits(want))


# ---------------------------------------------------------------- 3. the tie to the self-collision specification
@pytest.mark.parametrize("scene", SCENES)
def test_own_triangles_without_neighbours_are_the_symmetric_collide_lists(scene):
    d, tris = clip_tris(scene, "identity")
    T = len(tris)
    rank = np.random.default_rng(9).permutation(T)
    off, ids = xr.brute_cross(tris, tris, rank)
    got = xr.without_neighbours(off, ids, d["indices"])
    want = cr.brute_collide(tris, d["indices"], rank, True, True)
    assert int(got[0][-1]) == OWN_COUNTS[scene]
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    if scene == "Rect":    # a triangle queried with its own floats may or may not list itself: 11 of 12 do here
        owner = np.repeat(np.arange(T), np.diff(off.astype(np.int64)))
        assert int((owner == ids).sum()) == 11


# ---------------------------------------------------------------- 4. fp32 against fp64
def soup(n, extent, seed):
    """n triangles with centres in the unit cube and vertices within `extent` of them (test_collide_cpu.soup)."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3))
    return (c + (rng.random((n, 3, 3)) - 0.5) * extent).astype(np.float32)


def test_float32_and_float64_agree_on_a_random_soup():
    """Random triangles against random triangles: no pair of these seeds is a contact within rounding, so both
    precisions hold the same set."""
    tris, q = soup(2000, 0.06, 11), soup(1500, 0.1, 12)
    st32, st64 = [], []
    k, j = xr.member_pairs(tris, q, np.float32, stages=st32)
    K, J = xr.member_pairs(tris, q, np.float64, stages=st64)
    print(f"soup: {st32[0]} box pairs, {st32[1]} crossing in fp32, {st64[1]} in fp64")
    assert st32[0] > st32[1] > 20
    assert set(zip(k.tolist(), j.tolist())) == set(zip(K.tolist(), J.tolist()))


# ---------------------------------------------------------------- 5. the walk, on the oracle's tree
def walk(nodes, lo, hi, qlo, qhi, member, first=False, limit=1 << 30, deepest=None):
    """k_cross's walk for one query in plain Python: left first, a child is entered iff its box meets the query's
    (B); at a leaf `member(position)` decides.  The positions listed, in order; with `first` the walk ends at the
    first one.  A node whose two children both pass with the stack at `limit` loses both.  `deepest`, a list,
    receives the deepest stack entry stored."""
    n = (len(nodes) + 1) // 2
    cl, cr_ = nodes["child_l"], nodes["child_r"]
    meets = lambda c: bool(((qlo <= hi[c]) & (lo[c] <= qhi)).all())
    out, deep = [], -1
    stack, node = [], (n if n > 1 else 0)
    while True:
        if node < n:
            if meets(node) and member(node):
                out.append(node)
                if first:
                    break
        else:
            l, r = int(cl[node]), int(cr_[node])
            lh, rh = meets(l), meets(r)
            if lh and rh and len(stack) + 1 >= limit:
                pass
            elif lh or rh:
                if lh and rh:
                    deep = max(deep, len(stack))
                    stack.append(r)
                node = l if lh else r
                continue
        if not stack:
            break
        node = stack.pop()
    if deepest is not None:
        deepest[:] = [deep]
    return out


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_walk_on_the_oracles_trees_lists_the_brute_force_in_order(scene, cam):
    d, tris = clip_tris(scene, cam)
    wvp = camera(cam)
    nodes = orc.build(orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]), wvp)
    T = len(tris)
    order = nodes["index"][:T] // 3                # the oracle's leaves are in sort order
    rank = wr.rank_of(order)
    lo, hi = nodes["bb_min"], nodes["bb_max"]
    q = np.concatenate([xr.random_queries(tris, 128), tris[::max(1, T // 64)]])
    off, ids = xr.brute_cross(tris, q, rank)
    assert int(off[-1]) > 0
    want = cr.lists(off, ids)
    head = xr.first_of(off, ids)
    qlo, qhi = nr.leaf_data(q)[3:]
    k, j = xr.member_pairs(tris, q)
    members = [set() for _ in range(len(q))]
    for a, b in zip(k.tolist(), rank[j].tolist()):
        members[a].add(b)
    for i in range(len(q)):
        got = walk(nodes, lo, hi, qlo[i], qhi[i], members[i].__contains__)
        assert order[got].tolist() == want[i].tolist(), i
        one = walk(nodes, lo, hi, qlo[i], qhi[i], members[i].__contains__, first=True)
        assert (order[one].tolist() or [int(xr.NONE)]) == [int(head[i])], i


def test_the_fan_queries_take_the_walk_past_the_lds_part_of_the_stack():
    """The scene and queries test_cross_gpu.py uses for the deep walk: every query's walk stores entries at and past
    16 (trace.hip SB), and with the limit of that test it loses subtrees, keeping a sub-sequence of its list."""
    s = cr.thick_fan()
    nodes = orc.build(orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob), np.eye(4, dtype=np.float32))
    lo, hi = nodes["bb_min"], nodes["bb_max"]
    q = xr.fan_queries()
    qlo, qhi = nr.leaf_data(q)[3:]
    for i in range(len(q)):
        deep = []
        full = walk(nodes, lo, hi, qlo[i], qhi[i], lambda p: True, deepest=deep)
        assert deep[0] >= 16 + 2
        cut = walk(nodes, lo, hi, qlo[i], qhi[i], lambda p: True, limit=8)
        assert 0 < len(cut) < len(full) and [p for p in full if p in set(cut)] == cut


# ---------------------------------------------------------------- 6. exact touching
def test_exact_touching_counts_and_a_lift_off_the_plane_does_not():
    v, idx, q, members = xr.touching_case()
    tris = v[idx].reshape(-1, 3, 3)
    assert (tris[..., 2] == 0).all() and (q[0, 0] == np.float32([0.5, -0.25, 0.0])).all()
    assert (q[1] - q[0] == np.float32([0, 0, 2.0 ** -20])).all()
    for dtype in (np.float32, np.float64):
        k, j = xr.member_pairs(tris, q, dtype)
        assert list(zip(k.tolist(), j.tolist())) == [(0, 0)]
    off, ids = xr.brute_cross(tris, q, np.array([1, 0]))
    assert cr.lists(off, ids)[0].tolist() == members[0] and cr.lists(off, ids)[1].tolist() == members[1]
    assert xr.first_of(off, ids).tolist() == [0, int(xr.NONE)]
