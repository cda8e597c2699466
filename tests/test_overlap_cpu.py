"""Box-overlap queries without a GPU: the ABI's names and layouts, Context.overlap's argument checks, the brute force
(tests/overlap_ref.py) and its properties, on the oracle's tree the two properties the GPU walk leans on -- pruning
on (B) skips no member, and a left-first depth-first walk meets the triangles in the build's sort order -- and the
sanity check of the fp32 triangle-box test (T) against its float64 evaluation."""
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import nearest_ref as nr
from tests import overlap_ref as ovr
from tests import ray_walk_ref as rw
from tests import within_ref as wr
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]


def camera(name):
    return rt.camera_reference(64, 48)[0] if name == "reference" else np.eye(4, dtype=np.float32)


def lists(off, ids):
    return [ids[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]


def is_subsequence(short, long):
    it = iter(long.tolist())
    return all(x in it for x in short.tolist())


# ---------------------------------------------------------------- the ABI
def test_exports_constants_and_sizes():
    L = rt.lib()
    for name in ("rtbvh_overlap_async", "rtbvh_overlap_host", "rtbvh_overlap_counts"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.OVERLAP_SORT, rt.OVERLAP_COUNT, rt.OVERLAP_TRIANGLE, rt.OVERLAP_SIZES, rt.OVERLAP_FILL) == \
        (1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 5)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    for name, bit in (("SORT", 1), ("COUNT", 2), ("TRIANGLE", 3), ("SIZES", 4), ("FILL", 5)):
        assert re.search(rf"RTBVH_OVERLAP_{name} = 1u << {bit}\b", header), name
    assert rt.BOX_DTYPE.itemsize == 32
    assert [rt.BOX_DTYPE.fields[f][1] for f in ("lo", "reserved0", "hi", "reserved1")] == [0, 12, 16, 28]
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_make_boxes_packs_both_corners():
    lo = np.arange(12, dtype=np.float32).reshape(4, 3)
    b = rt.make_boxes(lo, lo + 1)
    assert b.dtype == rt.BOX_DTYPE and b.shape == (4,)
    np.testing.assert_array_equal(b["lo"], lo)
    np.testing.assert_array_equal(b["hi"], lo + 1)
    assert not b["reserved0"].any() and not b["reserved1"].any()
    np.testing.assert_array_equal(b.view(np.float32).reshape(4, 8)[:, 4:7], lo + 1)
    with pytest.raises(ValueError):
        rt.make_boxes(lo, lo[:3])
    kind, got = rt.check_overlap_boxes(lo, lo + 1)
    assert kind == "numpy" and got.tobytes() == b.tobytes()
    kind, got = rt.check_overlap_boxes(b.view(np.float32).reshape(4, 8))
    assert kind == "numpy" and got.dtype == rt.BOX_DTYPE and got.tobytes() == b.tobytes()


def test_bad_arguments_are_rejected_before_the_library_is_called():
    import torch
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    f32 = np.float32
    bad = [np.zeros((4, 7), f32), np.zeros((4, 3), f32), np.zeros((4, 4), f32), np.zeros(8, f32),
           np.zeros((4, 8), np.float64), np.zeros((8, 8), f32)[::2], np.zeros((2, 2), rt.BOX_DTYPE), [[0] * 8], None,
           torch.zeros((4, 8)), torch.zeros((4, 6)), torch.zeros((4, 8), dtype=torch.float64)]
    for b in bad:
        with pytest.raises(ValueError):
            ctx.overlap(b)
    ok = np.zeros((4, 3), f32)
    for lo, hi in ((ok, np.zeros((3, 3), f32)), (ok, np.zeros((4, 3), np.float64)), (np.zeros((4, 8), f32), ok),
                   (np.zeros(4, rt.BOX_DTYPE), ok), (ok, [[0, 0, 0]] * 4)):
        with pytest.raises(ValueError):
            ctx.overlap(lo, lo if hi is None else hi)
    for mode in (rt.OVERLAP_SIZES, rt.OVERLAP_FILL, 1, 1 << 6, 1 << 8):   # overlap sets the first two itself
        with pytest.raises(ValueError):
            ctx.overlap(ok, ok, mode=mode)
    for capacity in (-1, 1.5):
        with pytest.raises(ValueError):
            ctx.overlap(ok, ok, capacity=capacity)
    with pytest.raises(ValueError):
        ctx.overlap(ok, ok, capacity=4, sizes_only=True)


# ---------------------------------------------------------------- the brute force
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_brute_overlap_properties(scene, cam):
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
    T = len(tris)
    rank = np.random.default_rng(7).permutation(T)     # any order: membership does not depend on it
    lo, hi = nr.root_box(tris)
    # a box around the whole root box: every triangle, in rank order, in both modes' (B); (T) keeps them all too
    # only where it does not separate, so the plain mode is the one asserted on
    pad = np.float32(1)
    off, ids = ovr.brute_overlap(tris, [lo - pad, lo - pad], [hi + pad, hi + pad], rank)
    assert off.dtype == np.uint64 and ids.dtype == np.uint32
    np.testing.assert_array_equal(off, np.arange(3, dtype=np.uint64) * np.uint64(T))
    np.testing.assert_array_equal(ids[:T], np.argsort(rank))
    np.testing.assert_array_equal(ids[T:], np.argsort(rank))
    # TRIANGLE lists: subsequences of the plain lists, strictly shorter somewhere
    qlo, qhi = ovr.sample_boxes(tris, 5)
    assert len(qlo) == 512 + 3 * 64
    cls = np.arange(len(qlo)) % 4
    assert (qlo[cls == 1] == qhi[cls == 1]).all() and (qlo[cls == 2, 0] == qhi[cls == 2, 0]).all()
    assert (qlo[cls == 0] < qhi[cls == 0]).all() and (qlo[cls == 3] < qhi[cls == 3]).all()
    off_b, ids_b = ovr.brute_overlap(tris, qlo, qhi, rank)
    off_t, ids_t = ovr.brute_overlap(tris, qlo, qhi, rank, triangle=True)
    assert off_b[0] == 0 == off_t[0] and off_b[-1] == len(ids_b) and off_t[-1] == len(ids_t)
    assert 0 < off_t[-1] < off_b[-1] < len(qlo) * T
    for lb, lt in zip(lists(off_b, ids_b), lists(off_t, ids_t)):
        assert (np.diff(rank[lb]) > 0).all()                    # each list ascending by rank
        assert is_subsequence(lt, lb)
    # a NaN, an infinity or qlo > qhi: nothing, in both modes
    blo, bhi = np.repeat(lo[None] - pad, 6, 0), np.repeat(hi[None] + pad, 6, 0)
    blo[0, 0], bhi[1, 1], blo[2, 2], bhi[3, 0] = np.nan, np.nan, -np.inf, np.inf
    blo[4, 1] = bhi[4, 1] + pad
    blo[5], bhi[5] = bhi[5].copy(), blo[5].copy()
    for tri in (False, True):
        assert ovr.brute_overlap(tris, blo, bhi, rank, tri)[0][-1] == 0
    # a point box on vertex 0 of a triangle lists that triangle in both modes
    pick = np.arange(0, T, max(1, T // 32))
    for tri in (False, True):
        off, ids = ovr.brute_overlap(tris, tris[pick, 0], tris[pick, 0], rank, tri)
        for t, l in zip(pick, lists(off, ids)):
            assert t in l
    # -0 and +0 bounds behave alike
    zlo, zhi = qlo[:64].copy(), qhi[:64].copy()
    zlo[:, 0], zhi[:, 1] = 0.0, 0.0
    zlo[:, 1] = np.minimum(zlo[:, 1], 0)
    zhi[:, 0] = np.maximum(zhi[:, 0], 0)
    nlo, nhi = zlo.copy(), zhi.copy()
    nlo[:, 0], nhi[:, 1] = -0.0, -0.0
    for tri in (False, True):
        p, m = ovr.brute_overlap(tris, zlo, zhi, rank, tri), ovr.brute_overlap(tris, nlo, nhi, rank, tri)
        np.testing.assert_array_equal(p[0], m[0])
        np.testing.assert_array_equal(p[1], m[1])


# ---------------------------------------------------------------- the walk's order and pruning, on the oracle's tree
def dfs_overlap(nodes, leaf, qlo, qhi, triangle, out):
    """The left-first depth-first walk of rtbvh_overlap_* for one box, in plain Python: a child is entered iff its
    box passes (B); a leaf's own box first, then (T)."""
    n = (len(nodes) + 1) // 2
    a, e1, e2, lo, hi = leaf
    bmin, bmax = nodes["bb_min"], nodes["bb_max"]
    if not ovr.valid_boxes(qlo, qhi):
        return
    stack = [n if n > 1 else 0]
    while stack:
        k = stack.pop()
        if k < n:   # a leaf
            t = int(nodes["index"][k]) // 3
            if ovr.boxes_meet(qlo, qhi, lo[t], hi[t]) and (not triangle or ovr.triangle_meets(qlo, qhi, a[t], e1[t], e2[t])):
                out.append(t)
            continue
        l, r = int(nodes["child_l"][k]), int(nodes["child_r"][k])
        if ovr.boxes_meet(qlo, qhi, bmin[r], bmax[r]):
            stack.append(r)   # below the left one: walked after it
        if ovr.boxes_meet(qlo, qhi, bmin[l], bmax[l]):
            stack.append(l)


@pytest.mark.parametrize("triangle", [False, True])
@pytest.mark.parametrize("scene", ["Rect", "Test"])
def test_left_first_walk_pruned_on_box_overlap_is_the_brute_force_in_sort_order(scene, triangle):
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
    qlo, qhi = ovr.sample_boxes(tris, 21, n_random=40, n_each=8)
    assert len(qlo) == 64
    want_off, want = ovr.brute_overlap(tris, qlo, qhi, rank, triangle)
    assert 0 < want_off[-1] < 64 * T   # some lists, and pruning to do
    got, off = [], [0]
    for lo, hi in zip(qlo, qhi):
        dfs_overlap(nodes, leaf, lo, hi, triangle, got)
        off.append(len(got))
    np.testing.assert_array_equal(np.array(off, np.uint64), want_off)
    np.testing.assert_array_equal(np.array(got, np.uint32), want)


# ---------------------------------------------------------------- (T) in fp32 against its float64 evaluation
@pytest.mark.parametrize("cam", ["identity", "affine"])
@pytest.mark.parametrize("scene", SCENES)
def test_triangle_test_agrees_with_its_float64_evaluation_on_fat_boxes(scene, cam):
    """The pairs that pass (B), fat boxes only (classes 0 and 3: a point or flat box placed on the mesh is a contact
    by construction).  Memberships may differ on at most 0.1% of them, and (T) must reject at least one.  Measured
    with these fixtures and seed 5: 0 differences in 74,117 pairs; (T) rejects 1.6-41% a case."""
    d = load_scene_fixture(scene)
    m = np.eye(4, dtype=np.float32)
    if cam == "affine":
        m[:3, :3] = np.array([[1.5, 0.2, 0], [-0.1, 0.8, 0.3], [0, 0.25, 1.2]], np.float32)
        m[3, :3] = (0.5, -1.0, 2.0)
    tris = rw.clip_triangles(d["vertices"], d["indices"], m)
    qlo, qhi = ovr.sample_boxes(tris, 5)
    fat = np.isin(np.arange(len(qlo)) % 4, (0, 3))
    qlo, qhi = qlo[fat], qhi[fat]
    k, j = ovr.box_pairs(tris, qlo, qhi)
    assert len(k) > 1000
    a, e1, e2 = nr.leaf_data(tris)[:3]
    m32 = ovr.triangle_meets(qlo[k], qhi[k], a[j], e1[j], e2[j])
    a64, e164, e264 = nr.leaf_data(tris, np.float64)[:3]
    m64 = ovr.triangle_meets(qlo[k], qhi[k], a64[j], e164[j], e264[j], np.float64)
    differ = int((m32 != m64).sum())
    rejected = int((~m32).sum())
    print(f"{scene}/{cam}: {len(k)} (B) pairs, (T) rejects {rejected} ({100 * rejected / len(k):.1f}%), "
          f"fp32 and fp64 differ on {differ}")
    assert differ <= len(k) // 1000
    assert rejected >= 1
