"""Split region queries without a GPU: the split field's names and values, region_split and Context.region's argument
checks, and on the oracle's tree the model of tests/region_split_ref.py -- the expansion into at most K ordered pieces
and the piece walks -- whose lists, laid end to end, are the brute force in the build's sort order, with the step
identity the counts rely on."""
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import hostile_scenes as hs
from tests import ray_walk_ref as rw
from tests import region_ref as rr
from tests import region_split_ref as rs
from tests import within_ref as wr
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]
KS = [2, 4, 64, 4096]


def camera(name):
    return rt.camera_reference(64, 48)[0] if name == "reference" else np.eye(4, dtype=np.float32)


# ---------------------------------------------------------------- the ABI and the Python checks
def test_exports_constants_and_header():
    L = rt.lib()
    assert "rtbvh_region_split_counts" in _lib.EXPORTS and hasattr(L, "rtbvh_region_split_counts")
    assert (rt.REGION_SPLIT_SHIFT, rt.REGION_SPLIT_AUTO, rt.REGION_SPLIT_MAX_PIECES) == (16, 15 << 16, 1 << 20)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    assert re.search(r"RTBVH_REGION_SPLIT_SHIFT = 16\b", header)
    assert re.search(r"RTBVH_REGION_SPLIT_AUTO = 15u << 16\b", header)
    assert re.search(r"#define RTBVH_REGION_SPLIT_MAX_PIECES \(1u << 20\)", header)
    assert re.search(r"rtbvh_status rtbvh_region_split_counts\(rtbvh_ctx\* ctx, uint64_t out\[4\]\);", header)
    for name, bit in (("COUNT", 2), ("TRIANGLE", 3), ("SIZES", 4), ("FILL", 5), ("NO_ACCEPT", 6)):   # (unmoved)
        assert re.search(rf"RTBVH_REGION_{name} = 1u << {bit}\b", header), name
    # the field keeps clear of the rejected bits 0, 1, 7, 8, 31 and of the five mode bits
    assert rt.REGION_SPLIT_AUTO & (1 | 2 | 1 << 7 | 1 << 8 | 1 << 31 | 0x7C) == 0
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_region_split_bits():
    for v in range(1, 13):
        assert rt.region_split(1 << v) == v << 16
        assert rt.region_split(np.int64(1 << v)) == v << 16
    for bad in (0, 1, 3, 6, 4095, 8192, 1 << 13, 1 << 14, 1 << 15, -2, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            rt.region_split(bad)


def test_auto_k_formula():
    assert rs.auto_k(1) == 4096 and rs.auto_k(256) == 4096 and rs.auto_k(257) == 2048
    assert rs.auto_k(293) == 2048 and rs.auto_k(4096) == 256
    assert rs.auto_k(1 << 19) == 2 and rs.auto_k((1 << 19) + 1) == 1 and rs.auto_k(6_800_000) == 1
    assert rs.auto_k(1, 6) == 64 and rs.auto_k(1 << 15, 6) == 32      # an explicit field is clamped alike


def test_bad_arguments_are_rejected_before_the_library_is_called():
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    ok = np.zeros(4, rt.REGION_DTYPE)
    split = rt.region_split(64)
    for mode in (rt.REGION_SIZES, rt.REGION_FILL, 1, 2, 1 << 7, 1 << 8):   # with and without a split field
        for field in (0, split, rt.REGION_SPLIT_AUTO):
            with pytest.raises(ValueError):
                ctx.region(ok, mode=mode | field)
    for mode in (13 << 16, 14 << 16, 1 << 20, 1 << 15, 1 << 31, split | 1 << 31):
        with pytest.raises(ValueError):
            ctx.region(ok, mode=mode)
    with pytest.raises(ValueError):
        ctx.region(np.zeros((4, 23), np.float32), mode=split)
    with pytest.raises(ValueError):
        ctx.region(ok, mode=split, capacity=-1)


# ---------------------------------------------------------------- the model, on the oracle's tree
def check_model(osc, wvp, tris, seed, finite_only=None):
    nodes = orc.build(osc, wvp)
    T = len(tris)
    tree = rs.Tree(nodes, tris)
    assert sorted(tree.order.tolist()) == list(range(T))
    rank = wr.rank_of(tree.order)
    regions = rr.sample_regions(tris if finite_only is None else tris[finite_only], seed, n_each=4)
    accepted = 0
    for triangle in (False, True):
        want = rr.brute_region(tris, regions, rank, triangle)
        assert 0 < want[0][-1] < len(regions) * T
        plain = {acc: rs.plain_steps(tree, regions, triangle, acc) for acc in (True, False)}
        for accept in (True, False):
            for K in KS:
                off, ids, st, pieces = rs.split_lists(tree, regions, triangle, K, accept)
                np.testing.assert_array_equal(off, want[0])
                np.testing.assert_array_equal(ids, want[1])
                assert st["overflow"] == 0
                for items in pieces:
                    assert len(items) <= K
                    spans = [rs.leaf_span(tree, it) for it in items]
                    assert all(a <= b for a, b in spans)
                    assert all(spans[i][1] < spans[i + 1][0] for i in range(len(spans) - 1))   # strictly increasing
                    if not (accept and tree.nan_free):
                        assert all(it[0] != "range" for it in items)
                split_steps = st["tests"] + st["internal"] + st["leaf"]
                plain_total = plain[accept]["internal"] + plain[accept]["leaf"]
                if accept:
                    assert split_steps <= plain_total
                    accepted += st["accepted"]
                else:   # every entered node is tested once, by the expansion or by a piece
                    assert st["accepted"] == 0
                    assert st["tests"] + st["internal"] == plain[False]["internal"]
                    assert st["leaf"] == plain[False]["leaf"]
                if K >= 64 and T > 64:
                    assert st["pieces"] > len(regions)                  # something was cut
                    assert st["longest"] < plain_total
    return tree, accepted


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_split_lists_are_the_brute_force_in_sort_order(scene, cam):
    d = load_scene_fixture(scene)
    wvp = camera(cam)
    osc = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    tree, accepted = check_model(osc, wvp, tris, 21)
    assert tree.nan_free and accepted > 0


@pytest.mark.parametrize("cam", hs.CAMERAS)
@pytest.mark.parametrize("variant", list(hs.VARIANTS))
def test_split_lists_on_hostile_scenes(variant, cam):
    h = hs.hostile(variant)
    wvp = hs.camera(cam)[0]
    tris = h.tris(wvp)
    tree, accepted = check_model(hs.oracle_scene(h.scene), wvp, tris, 23, hs.finite_part(tris, h.labels))
    assert tree.nan_free == (variant not in hs.NONFINITE_VARIANTS)
    assert (accepted == 0) == (not tree.nan_free)                       # a tree with a NaN leaf box takes no accepts


def test_k_far_above_the_leaf_count_ends_in_leaves():
    d = load_scene_fixture("Rect")
    wvp = camera("identity")
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    nodes = orc.build(orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]), wvp)
    tree = rs.Tree(nodes, tris)
    assert tree.T < 64
    lo, hi = (np.asarray(x, np.float32) for x in (tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)))
    whole = rt.box_region(lo - 1, hi + 1)
    _, ids, st, pieces = rs.split_lists(tree, whole, False, 4096, accept=False)
    assert [it[0] for it in pieces[0]] == ["leaf"] * tree.T and st["internal"] == 0 and st["tests"] == tree.T - 1
    np.testing.assert_array_equal(ids, tree.order)
    _, ids, st, pieces = rs.split_lists(tree, whole, False, 4096, accept=True)
    assert pieces[0] == [("range", 0, tree.T)] and st["tests"] == 0 and st["leaf"] == 0   # the root taken whole
    np.testing.assert_array_equal(ids, tree.order)


def test_a_chain_grows_by_one_piece_a_round():
    """The 36-level fan (tests/deep_scenes.py): the expansion ends, within its rounds, and the lists are exact."""
    from tests import deep_scenes as ds
    s = ds.fan_scene()
    wvp = np.eye(4, dtype=np.float32)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    nodes = orc.build(hs.oracle_scene(s), wvp)
    tree = rs.Tree(nodes, tris)
    rank = wr.rank_of(tree.order)
    regions = rr.sample_regions(tris, 9, n_each=4)
    want = rr.brute_region(tris, regions, rank, True)
    for K in KS:
        off, ids, st, _ = rs.split_lists(tree, regions, True, K)
        np.testing.assert_array_equal(off, want[0])
        np.testing.assert_array_equal(ids, want[1])
