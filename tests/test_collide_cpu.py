"""Self-collision queries without a GPU: the ABI's names, Context.collide's argument checks, the brute force
(tests/collide_ref.py) and its properties, and on the oracle's trees the two properties the GPU walk leans on --
pruning on (B) skips no partner, and the subtrees the leaf-range skip drops hold nothing an owner lists."""
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import collide_ref as cr
from tests import deep_scenes as ds
from tests import nearest_ref as nr
from tests import overlap_ref as ovr
from tests import ray_walk_ref as rw
from tests import signed_ref as sr
from tests import within_ref as wr
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Rect", "Test", "Image_Test"]
CAMERAS = ["reference", "identity"]
# box pairs, after (N), after (X) under the identity camera
IDENTITY_COUNTS = {"Rect": [54, 48, 31], "Test": [15_530, 8_082, 4_406], "Image_Test": [26_064, 9_090, 1_465]}


def camera(name):
    return rt.camera_reference(64, 48)[0] if name == "reference" else np.eye(4, dtype=np.float32)


# ---------------------------------------------------------------- the ABI
def test_exports_and_constants():
    L = rt.lib()
    for name in ("rtbvh_collide_async", "rtbvh_collide_host", "rtbvh_collide_counts"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.COLLIDE_COUNT, rt.COLLIDE_TRIANGLE, rt.COLLIDE_SIZES, rt.COLLIDE_FILL, rt.COLLIDE_SYMMETRIC) == \
        (1 << 2, 1 << 3, 1 << 4, 1 << 5, 1 << 6)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    for name, bit in (("COUNT", 2), ("TRIANGLE", 3), ("SIZES", 4), ("FILL", 5), ("SYMMETRIC", 6)):
        assert re.search(rf"RTBVH_COLLIDE_{name} = 1u << {bit}\b", header), name
    for name in ("rtbvh_collide_async", "rtbvh_collide_host", "rtbvh_collide_counts"):
        assert re.search(rf"rtbvh_status {name}\(", header), name
    for name in ("collide", "collide_pairs", "collide_counts"):
        assert callable(getattr(rt.Context, name)), name
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_bad_arguments_are_rejected_before_the_library_is_called():
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    ctx.num_tris = 4
    for mode in (rt.COLLIDE_SIZES, rt.COLLIDE_FILL, rt.COLLIDE_SIZES | rt.COLLIDE_TRIANGLE, 1, 2, 1 << 7, 1 << 8):
        with pytest.raises(ValueError):
            ctx.collide(mode)
    for capacity in (-1, 1.5):
        with pytest.raises(ValueError):
            ctx.collide(capacity=capacity)
    with pytest.raises(ValueError):
        ctx.collide(capacity=4, sizes_only=True)
    with pytest.raises(ValueError):
        ctx.collide(stream=1)   # a stream goes with the device entry
    L = rt.lib()
    off = np.zeros(5, np.uint64)
    assert L.rtbvh_collide_async(None, off.ctypes.data_as(ctypes.c_void_p), None, 0, 0, None) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_collide_host(None, off.ctypes.data_as(ctypes.c_void_p), None, 0, 0) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_collide_counts(None, off.ctypes.data_as(ctypes.c_void_p)) == _lib.ERR_INVALID_ARG


# ---------------------------------------------------------------- the brute force
def soup(n=2000, extent=0.06, seed=11):
    """n triangles with centres in the unit cube and vertices within `extent` of them; no shared indices."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3))
    return (c + (rng.random((n, 3, 3)) - 0.5) * extent).astype(np.float32), np.arange(3 * n)


def test_reference_is_symmetric_and_independent_of_the_numbering():
    tris, idx = soup(600, 0.15, seed=3)
    x, y = cr.member_pairs(tris, idx, True)
    assert len(x) > 20
    leaf = nr.leaf_data(tris)[:3]
    np.testing.assert_array_equal(cr.triangles_cross(x, y, leaf), cr.triangles_cross(y, x, leaf))
    perm = np.random.default_rng(4).permutation(len(tris))          # triangle perm[i] becomes triangle i
    px, py = cr.member_pairs(tris[perm], idx, True)
    a, b = perm[px], perm[py]
    got = set(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))
    assert got == set(zip(x.tolist(), y.tolist()))
    # both ownership rules hold the same pairs; the symmetric lists are the default ones plus their mirror
    rank = np.random.default_rng(5).permutation(len(tris))
    off_d, ids_d = cr.csr((x, y), rank, len(tris))
    off_s, ids_s = cr.csr((x, y), rank, len(tris), True)
    assert off_d[-1] == len(x) and off_s[-1] == 2 * len(x)
    mirror = [[] for _ in range(len(tris))]
    for i, l in enumerate(cr.lists(off_d, ids_d)):
        assert (rank[l] > rank[i]).all() and (np.diff(rank[l]) > 0).all()
        for j in l.tolist():
            mirror[j].append(i)
    for i, (d, s) in enumerate(zip(cr.lists(off_d, ids_d), cr.lists(off_s, ids_s))):
        both = np.array(sorted(mirror[i] + d.tolist(), key=lambda t: rank[t]), np.uint32)
        np.testing.assert_array_equal(s, both)


def test_float32_and_float64_agree_on_a_random_soup():
    tris, idx = soup()
    st32, st64 = [], []
    x, y = cr.member_pairs(tris, idx, True, np.float32, st32)
    X, Y = cr.member_pairs(tris, idx, True, np.float64, st64)
    print(f"soup: {st32[0]} box pairs, {st32[2]} crossing in fp32, {st64[2]} in fp64")
    assert st32[0] > st32[2] > 20
    assert set(zip(x.tolist(), y.tolist())) == set(zip(X.tolist(), Y.tolist()))


def test_two_crossing_quads_give_the_four_pairs():
    v, idx = cr.crossing_quads()
    tris = v[idx].reshape(-1, 3, 3)
    st = []
    x, y = cr.member_pairs(tris, idx, True, stages=st)
    assert list(zip(x.tolist(), y.tolist())) == [(0, 2), (0, 3), (1, 2), (1, 3)]
    assert st == [6, 4, 4]                      # the two quads' own triangle pairs fall to (N)
    off, ids = cr.brute_collide(tris, idx, np.array([2, 0, 3, 1]), True)   # sort order: 1, 3, 0, 2
    assert off.tolist() == [0, 1, 3, 3, 4] and ids.tolist() == [2, 3, 2, 0]
    off, ids = cr.brute_collide(tris, idx, np.array([2, 0, 3, 1]), True, True)
    assert off.tolist() == [0, 2, 4, 6, 8] and ids.tolist() == [3, 2, 3, 2, 1, 0, 1, 0]
    # the lattice's cells are copies of it
    v, idx = cr.lattice(9)
    x, y = cr.member_pairs(v[idx].reshape(-1, 3, 3), idx, True)
    lx, ly = cr.lattice_pairs(9)
    assert list(zip(x.tolist(), y.tolist())) == list(zip(lx.tolist(), ly.tolist()))


def two_shells(subdiv, shift):
    """Two icospheres of radius 1, the second moved by `shift` along x, with its own vertex range."""
    v, f = sr.icosphere(subdiv)
    v2 = v.copy()
    v2[:, 0] += np.float32(shift)
    return np.concatenate([v, v2]), np.concatenate([f, f + len(v)]).reshape(-1)


def test_interpenetrating_icospheres_meet_along_their_circle():
    shift = 0.25
    v, idx = two_shells(3, shift)
    tris = v[idx].reshape(-1, 3, 3)
    assert len(tris) == 2 * 1280
    x, y = cr.member_pairs(tris, idx, True)
    assert len(x) > 100
    assert ((x < 1280) & (y >= 1280)).all()                    # every pair joins one shell to the other
    edge = np.sqrt((((tris - np.roll(tris, 1, 1)).astype(np.float64)) ** 2).sum(-1)).max()
    # the circle: x = shift / 2, radius sqrt(1 - shift^2 / 4) about the x axis
    p = tris[np.unique(np.concatenate([x, y]))].astype(np.float64)
    rho = np.sqrt(p[..., 1] ** 2 + p[..., 2] ** 2)
    dist = np.sqrt((p[..., 0] - shift / 2) ** 2 + (rho - np.sqrt(1 - shift ** 2 / 4)) ** 2).min(1)
    print(f"shells: {len(x)} pairs, farthest listed triangle {dist.max():.4f} from the circle, edge {edge:.4f}")
    assert (dist <= edge).all()


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_golden_scenes_have_something_to_find(scene, cam):
    """What test_collide_gpu.py asserts from the reference before it compares, on the CPU first."""
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
    T = len(tris)
    st = []
    cr.member_pairs(tris, d["indices"], True, stages=st)
    print(f"{scene}/{cam}: box pairs {st[0]}, after (N) {st[1]}, after (X) {st[2]}")
    assert 0 < st[2] < st[1] < st[0] < T * (T - 1) // 2
    if cam == "identity":
        assert st == IDENTITY_COUNTS[scene]


# ---------------------------------------------------------------- the walk, on the oracle's tree
def walk(nodes, lo, hi, k, symmetric, skip, limit=1 << 30):
    """k_collide's walk for the leaf at position k in plain Python, (B) only: the positions listed, in order, and the
    deepest stack entry stored.  A child is entered iff its box meets leaf k's; without `symmetric` a leaf must lie
    behind k, and with `skip` a left child whose Karras id (where its leaf range ends) is <= k is not entered."""
    n = (len(nodes) + 1) // 2
    cl, cr_ = nodes["child_l"], nodes["child_r"]
    meets = lambda c: bool(((lo[k] <= hi[c]) & (lo[c] <= hi[k])).all())
    out, deepest = [], -1
    if n == 1 or (not symmetric and k + 1 == n):
        return out, deepest
    stack, node = [], n
    while True:
        if node < n:
            if (node != k if symmetric else node > k) and meets(node):
                out.append(node)
        else:
            l, r = int(cl[node]), int(cr_[node])
            g = l - n if l >= n else l
            lh = (symmetric or not skip or g > k) and meets(l)
            rh = meets(r)
            if lh and rh and len(stack) + 1 >= limit:
                pass
            elif lh or rh:
                if lh and rh:
                    deepest = max(deepest, len(stack))
                    stack.append(r)
                node = l if lh else r
                continue
        if not stack:
            return out, deepest
        node = stack.pop()


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_walk_lemma_on_the_oracles_trees(scene, cam):
    d = load_scene_fixture(scene)
    wvp = camera(cam)
    nodes = orc.build(orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]), wvp)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    T = len(tris)
    order = nodes["index"][:T] // 3                # the oracle's leaves are in sort order
    rank = wr.rank_of(order)
    lo, hi = nodes["bb_min"], nodes["bb_max"]
    leaf = nr.leaf_data(tris)
    np.testing.assert_array_equal(lo[:T], leaf[3][order])
    np.testing.assert_array_equal(hi[:T], leaf[4][order])
    # the leaf ranges the skip leans on: a left child's range ends at its own Karras id, a right child's where its
    # parent's does
    first, last = ds.leaf_ranges(nodes)
    cl, cr_ = nodes["child_l"][T:].astype(np.int64), nodes["child_r"][T:].astype(np.int64)
    end = lambda c: np.where(c >= T, last[np.maximum(c - T, 0)], c)
    np.testing.assert_array_equal(end(cl), np.where(cl >= T, cl - T, cl))
    np.testing.assert_array_equal(end(cr_), last)
    assert first[0] == 0 and last[0] == T - 1
    # every ancestor box of a member's partner meets the owner's leaf box
    x, y = cr.member_pairs(tris, d["indices"])
    px, py = rank[x], rank[y]
    own, par = np.minimum(px, py), np.maximum(px, py)
    up = nodes["parent"].astype(np.int64)
    for a, b in ((own, par), (par, own)):          # (the symmetric walk reaches the owner from the partner too)
        at = b.copy()
        while (at != T).any():
            at = np.where(at == T, T, up[at])
            assert ovr.boxes_meet(lo[a], hi[a], lo[at], hi[at]).all()
    # the walk itself, with and without the skip, against the brute force: the same lists
    want = cr.lists(*cr.csr((x, y), rank, T))
    want_s = cr.lists(*cr.csr((x, y), rank, T, True))
    ix = np.asarray(d["indices"], np.int64).reshape(-1, 3)
    for k in range(0, T, max(1, T // 200)):
        t = int(order[k])
        drop = lambda pos: [p for p in pos if not np.isin(ix[order[p]], ix[t]).any()]   # (N)
        got = {}
        for skip in (True, False):
            got[skip], _ = walk(nodes, lo, hi, k, False, skip)
        assert got[True] == got[False]
        assert order[drop(got[True])].tolist() == want[t].tolist(), k
        assert order[drop(walk(nodes, lo, hi, k, True, True)[0])].tolist() == want_s[t].tolist(), k


def test_the_fan_takes_the_walk_past_the_lds_part_of_the_stack():
    """The scene test_collide_gpu.py uses for the deep walk: some leaf's walk stores entries at and past 16 (trace.hip
    SB), and with the limit of that test it loses subtrees."""
    s = cr.thick_fan()
    nodes = orc.build(orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob), np.eye(4, dtype=np.float32))
    T = s.num_tris
    lo, hi = nodes["bb_min"], nodes["bb_max"]
    deepest = max(walk(nodes, lo, hi, k, sym, True)[1] for k in range(T) for sym in (False, True))
    assert deepest >= 16 + 2
    full = [walk(nodes, lo, hi, k, False, True)[0] for k in range(T)]
    cut = [walk(nodes, lo, hi, k, False, True, limit=8)[0] for k in range(T)]
    assert sum(map(len, cut)) < sum(map(len, full))
    assert all(set(c) <= set(f) for c, f in zip(cut, full))
