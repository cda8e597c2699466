"""Signed-distance queries without a GPU: the ABI's names and constants, the argument checks of Context.signed,
inside and signed_distance (which run before the library is touched), the brute force (tests/signed_ref.py) against
an analytic answer -- a sphere's inside -- at three scales, its flags, and, on the oracle's tree, the lemma the GPU
walk leans on: a left-first walk that enters a child iff its box passes the any-hit box rule counts exactly the
brute-force crossings."""
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
from tests import signed_ref as sr
from tests.conftest import REPO, load_scene_fixture
from tests.test_knn_cpu import camera

SCENES = ["Test", "Rect", "Image_Test"]
NAMES = ("rtbvh_signed_async", "rtbvh_signed_host", "rtbvh_signed_counts")


# ---------------------------------------------------------------- the ABI
def test_exports_and_constants():
    L = rt.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.SIGNED_SORT, rt.SIGNED_COUNT, rt.SIGNED_VOTE3, rt.SIGNED_INSIDE_ONLY) == (1 << 1, 1 << 2, 1 << 3, 1 << 4)
    assert rt.SIGNED_DTYPE == sr.DTYPE and rt.SIGNED_DTYPE.itemsize == 32
    assert rt.SIGNED_DTYPE.names == ("point", "dist2", "u", "v", "tri", "flags")
    assert [rt.SIGNED_DTYPE.fields[f][1] for f in rt.SIGNED_DTYPE.names] == [0, 12, 16, 20, 24, 28]
    for f in ("point", "dist2", "u", "v", "tri"):   # rtbvh_nearest's fields at rtbvh_nearest's offsets
        assert rt.SIGNED_DTYPE.fields[f] == rt.NEAREST_DTYPE.fields[f]
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    for name, bit in (("SORT", 1), ("COUNT", 2), ("VOTE3", 3), ("INSIDE_ONLY", 4)):
        assert re.search(rf"RTBVH_SIGNED_{name} = 1u << {bit}\b", header), name
    assert re.search(r"\}\s*rtbvh_signed;", header)
    for name in NAMES:
        assert re.search(rf"^rtbvh_status {name}\s*\(rtbvh_ctx\*", header, re.M), name
    # the calls that are NOT_READY after a vertex update
    assert re.search(r"rtbvh_within_\*, rtbvh_knn_\*,", header) and re.search(r"rtbvh_overlap_\*, rtbvh_signed_\*", header)
    for row in ("0.75,    0.5,   0.4375", "-0.5,     0.75, -0.4375", "0.4375, -0.5,  -0.75"):   # the rays, as specified
        assert row in header, row
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive
    np.testing.assert_array_equal(sr.D, np.array([[.75, .5, .4375], [-.5, .75, -.4375], [.4375, -.5, -.75]], np.float32))
    assert np.isfinite(sr.INV).all() and (sr.D != 0).all()


def test_bad_arguments_are_rejected_before_the_library_is_called():
    import torch
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    f32 = np.float32
    ok = np.zeros((4, 3), f32)
    bad = [np.zeros((4, 5), f32), np.zeros((4, 2), f32), np.zeros(4, f32), np.zeros((4, 3), np.float64),
           np.zeros((4, 4), np.int32), np.zeros((2, 4, 3), f32), np.zeros((8, 4), f32)[::2], np.zeros((4, 6), f32)[:, :3],
           np.zeros((2, 2), rt.POINT_DTYPE), np.zeros(8, rt.POINT_DTYPE)[::2], [[0, 0, 0]], None,
           torch.zeros((4, 4)), torch.zeros((4, 3)), torch.zeros((4, 4), dtype=torch.float64)]
    for b in bad:
        for call in (ctx.signed, ctx.inside, ctx.signed_distance):
            with pytest.raises(ValueError):
                call(b)
    for call in (ctx.signed, ctx.signed_distance):
        with pytest.raises(ValueError):
            call(ok, max_dist2=np.zeros(3, f32))               # 4 points, 3 bounds
        with pytest.raises(ValueError):
            call(np.zeros((4, 4), f32), max_dist2=1.0)         # the bound is the fourth column
        with pytest.raises(ValueError):
            call(np.zeros(4, rt.POINT_DTYPE), max_dist2=1.0)
    for out in (np.zeros(3, rt.SIGNED_DTYPE), np.zeros((4, 1), rt.SIGNED_DTYPE), np.zeros(4, rt.NEAREST_DTYPE),
                np.zeros((4, 8), f32), np.zeros(8, rt.SIGNED_DTYPE)[::2], torch.zeros((4, 8))):
        with pytest.raises(ValueError):
            ctx.signed(ok, out=out)


# ---------------------------------------------------------------- analytic ground truth: inside a sphere
def test_inside_an_icosphere_for_every_ray_and_the_vote_at_three_scales():
    """1,280 triangles on the unit sphere, 20,000 points in [-1.3, 1.3]^3; away from the surface the answer is
    |p| < r_in.  Zero disagreements for each ray alone and for the vote, and the same flags with the mesh and the
    points scaled by 64 and by 1/64: the crossing test has no absolute threshold."""
    tris, pts, keep, inside = sr.analytic_case()
    assert tris.shape == (1280, 3, 3) and tris.dtype == np.float32 and len(pts) == 20_000
    left_out = 1 - keep.mean()
    print(f"left out near the surface: {100 * left_out:.2f}% of the points; inside: {int(inside[keep].sum())}")
    assert left_out <= 0.02
    assert inside[keep].sum() > 4000 and (~inside[keep]).sum() > 10_000
    flags = {}
    for scale in (1.0, 64.0, 1 / 64):
        s = np.float32(scale)
        c = np.stack([sr.crossings(tris * s, pts * s, j) for j in range(3)], 1)
        for j in range(3):
            wrong = int((((c[:, j] & 1) == 1) != inside)[keep].sum())
            print(f"scale {scale}: ray {j}: {wrong} wrong of {int(keep.sum())}")
            assert wrong == 0, (scale, j)
        one = sr.pack_flags(np.where(np.arange(3) == 0, c, 0), False)
        three = sr.pack_flags(c, True)
        assert (((one & 1) == 1) == inside)[keep].all() and (((three & 1) == 1) == inside)[keep].all()
        flags[scale] = (one, three)
    for scale in (64.0, 1 / 64):
        np.testing.assert_array_equal(flags[scale][0], flags[1.0][0])
        np.testing.assert_array_equal(flags[scale][1], flags[1.0][1])


# ---------------------------------------------------------------- the lemma, on the oracle's tree
def walk_count(nodes, bpass, x):
    """The ray phase of rtbvh_signed_* for one point and one ray, in plain Python: `bpass` whether each node's box
    passes (B), `x` whether each triangle passes (X).  Left first; a child is entered iff its box passes; a leaf
    counts iff (X) holds (its box was tested at its parent; at the leaf itself where it is the root).  Returns the
    count and the nodes visited."""
    n = (len(nodes) + 1) // 2
    index, cl, cr = nodes["index"], nodes["child_l"], nodes["child_r"]
    if n == 1:
        return int(bpass[0] and x[int(index[0]) // 3]), 1
    stack, count, visited = [n], 0, 0
    while stack:
        k = stack.pop()
        visited += 1
        if k < n:   # a leaf
            count += int(x[int(index[k]) // 3])
            continue
        l, r = int(cl[k]), int(cr[k])
        if bpass[r]:
            stack.append(r)
        if bpass[l]:
            stack.append(l)   # on top: left first
    return count, visited


@pytest.mark.parametrize("cam", ["identity", "affine"])
@pytest.mark.parametrize("scene", SCENES)
def test_a_left_first_walk_on_the_box_rule_counts_the_brute_force(scene, cam):
    d = load_scene_fixture(scene)
    wvp = camera(cam)
    osc = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    nodes = orc.build(osc, wvp)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    T = len(tris)
    leaf = nr.leaf_data(tris)
    sort_order = nodes["index"][:T] // 3          # the oracle's leaves are in sort order
    np.testing.assert_array_equal(nodes["bb_min"][:T], leaf[3][sort_order])   # the leaf boxes are the records'
    np.testing.assert_array_equal(nodes["bb_max"][:T], leaf[4][sort_order])
    pts = nr.sample_points(tris)[0]
    n, M = len(pts), len(nodes)
    assert n == 704
    pp = np.repeat(pts, M, axis=0)
    ni = np.tile(np.arange(M), n)
    visited = crossed = 0
    for j in range(3):
        want = sr.crossings(tris, pts, j)
        bpass = sr.box_pass(nodes["bb_min"][ni], nodes["bb_max"][ni], pp, j).reshape(n, M)
        # (the helper's two forms of (B) are one)
        np.testing.assert_array_equal(sr.box_pass_grid(nodes["bb_min"], nodes["bb_max"], pts, j), bpass)
        x = sr.crossing_matrix(tris, pts, j, with_box=False)
        for i in range(n):
            got, v = walk_count(nodes, bpass[i].tolist(), x[i].tolist())
            visited += v
            assert got == want[i], (j, i)
        crossed += int(want.sum())
    print(f"{scene}/{cam}: {crossed} crossings, {visited / (3 * n):.1f} nodes a walk of {M}")
    assert crossed > 0 and visited < 3 * n * M   # ... and the walk did prune


# ---------------------------------------------------------------- flags, the no-walk rules
def test_flags_packing_and_saturation():
    c = np.array([[0, 0, 0], [1, 0, 0], [2, 1, 1], [255, 256, 257], [300, 299, 1], [1, 2, 2], [254, 3, 4]], np.int64)
    one = sr.pack_flags(np.where(np.arange(3) == 0, c, 0), False)
    three = sr.pack_flags(c, True)
    assert one.dtype == three.dtype == np.uint32
    assert one.tolist() == [0, 1 | 2 | 1 << 8, 2 << 8, 1 | 2 | 255 << 8, 255 << 8, 1 | 2 | 1 << 8, 254 << 8]
    assert three.tolist() == [0, 2 | 1 << 8, 1 | 4 | 8 | 2 << 8 | 1 << 16 | 1 << 24,
                              1 | 2 | 8 | 255 << 8 | 255 << 16 | 255 << 24, 1 | 4 | 8 | 255 << 8 | 255 << 16 | 1 << 24,
                              2 | 1 << 8 | 2 << 16 | 2 << 24, 4 | 254 << 8 | 3 << 16 | 4 << 24]
    assert ((one | three) & 0xF0 == 0).all()
    for j in range(3):   # 300 copies of one triangle across ray j: byte 255, the parity of the true count
        tris, pts, counts = sr.stack_case(j)
        assert tris.shape == (300, 3, 3) and counts.tolist() == [300, 299, 255, 254, 0]
        np.testing.assert_array_equal(sr.crossings(tris, pts, j), counts)
        f = sr.brute(tris, pts, vote3=True)["flags"]
        np.testing.assert_array_equal(f >> (8 * (j + 1)) & 255, [255, 255, 255, 254, 0])
        np.testing.assert_array_equal(f >> (j + 1) & 1, [0, 1, 1, 0, 0])
        if j == 0:
            f1 = sr.brute(tris, pts, inside_only=True)["flags"]
            assert f1.tolist() == [255 << 8, 1 | 2 | 255 << 8, 1 | 2 | 255 << 8, 254 << 8, 0]


def test_the_no_walk_rules_and_negative_zero_bounds():
    tris, pts, keep, inside = sr.analytic_case(n=64)
    free = sr.brute(tris, pts, vote3=True)
    assert (free["tri"] != sr.NONE).all() and free["flags"].any()
    # a bound that gives no closest-point walk, and INSIDE_ONLY: "no result", the rays still cast
    for got in (sr.brute(tris, pts, np.float32(-1), vote3=True), sr.brute(tris, pts, np.float32(np.nan), vote3=True),
                sr.brute(tris, pts, vote3=True, inside_only=True)):
        np.testing.assert_array_equal(got["flags"], free["flags"])
        assert (got["tri"] == sr.NONE).all() and (got["dist2"] == -1).all()
        assert not got["point"].any() and not got["u"].any() and not got["v"].any()
    # a non-finite coordinate: no rays either
    bad = pts[:6].copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3] = np.nan, np.inf, -np.inf, np.nan
    got = sr.brute(tris, bad, vote3=True)
    assert (got["flags"][:4] == 0).all() and (got["tri"][:4] == sr.NONE).all() and (got["dist2"][:4] == -1).all()
    np.testing.assert_array_equal(got[4:].view(np.uint32), free[4:6].view(np.uint32))
    # a per-point bound is a narrow band: exactly dist2 keeps the result, the float below drops it, the flags stay
    d = free["dist2"]
    band = sr.brute(tris, pts, np.where(np.arange(64) % 2 == 0, d, np.nextafter(d, np.float32(0))).astype(np.float32))
    assert (band["tri"][0::2] == free["tri"][0::2]).all() and (band["tri"][1::2][d[1::2] > 0] == sr.NONE).all()
    np.testing.assert_array_equal(band["flags"], sr.brute(tris, pts)["flags"])
    # -0 counts as +0: a point on a vertex is found at dist2 == 0
    on = tris[:8, 0]
    for zero in (np.float32(0), np.float32(-0.0)):
        got = sr.brute(tris, on, zero)
        assert (got["tri"] != sr.NONE).all() and (nr.bits(got["dist2"]) == 0).all()
