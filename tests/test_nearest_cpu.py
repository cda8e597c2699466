"""Closest-point queries without a GPU: the ABI's names and layouts, Context.nearest's argument checks (which run
before the library is touched), and the two properties of the numpy restatement (tests/nearest_ref.py) that the
GPU tests lean on -- the containment that makes the walk's pruning exact, and its accuracy."""
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from raytracebvh_amd import _lib
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]


def camera(name):
    return rt.camera_reference(64, 48)[0] if name == "reference" else np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    """A golden scene in BVH space, the tests' points, and the restated (point, triangle) distances (computed once)."""
    scene, cam = request.param
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
    pts, first_vertex = nr.sample_points(tris)
    a, e1, e2, lo, hi = nr.leaf_data(tris)
    dist2 = nr.tri_dist2(pts[:, None, :], a[None], e1[None], e2[None], lo[None], hi[None])[0]
    return tris, pts, first_vertex, dist2


# ---------------------------------------------------------------- the ABI
def test_exports_and_constants():
    L = rt.lib()
    for name in ("rtbvh_nearest_async", "rtbvh_nearest_host", "rtbvh_nearest_counts"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.NEAREST_SORT, rt.NEAREST_COUNT) == (1 << 1, 1 << 2)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    assert re.search(r"RTBVH_NEAREST_SORT = 1u << 1\b", header) and re.search(r"RTBVH_NEAREST_COUNT = 1u << 2\b", header)
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_record_layouts():
    assert rt.POINT_DTYPE.itemsize == 16 == ctypes.sizeof(_lib.Point)
    assert rt.NEAREST_DTYPE.itemsize == 32 == ctypes.sizeof(_lib.Nearest)
    for dt, st in ((rt.POINT_DTYPE, _lib.Point), (rt.NEAREST_DTYPE, _lib.Nearest)):
        assert list(dt.names) == [f[0] for f in st._fields_]
        for name in dt.names:
            assert dt.fields[name][1] == getattr(st, name).offset, name
    assert [rt.NEAREST_DTYPE.fields[f][1] for f in ("point", "dist2", "u", "v", "tri", "reserved")] == [0, 12, 16, 20, 24, 28]
    assert [rt.POINT_DTYPE.fields[f][1] for f in ("point", "max_dist2")] == [0, 12]


def test_make_points():
    p = rt.make_points([[1, 2, 3], [4, 5, 6]], [7, 8])
    assert p.dtype == rt.POINT_DTYPE and p["point"].tolist() == [[1, 2, 3], [4, 5, 6]] and p["max_dist2"].tolist() == [7, 8]
    assert np.isinf(rt.make_points(np.zeros((3, 3)))["max_dist2"]).all()
    import torch
    t = rt.make_points(torch.arange(6, dtype=torch.float64).reshape(2, 3), 2.5)
    assert t.dtype == torch.float32 and t.tolist() == [[0, 1, 2, 2.5], [3, 4, 5, 2.5]]


def test_bad_arguments_are_rejected_before_the_library_is_called():
    import torch
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    f32 = np.float32
    bad = [np.zeros((4, 5), f32), np.zeros((4, 2), f32), np.zeros(4, f32), np.zeros((4, 3), np.float64),
           np.zeros((4, 4), np.int32), np.zeros((2, 4, 3), f32), np.zeros((8, 4), f32)[::2], np.zeros((4, 6), f32)[:, :3],
           np.zeros((2, 2), rt.POINT_DTYPE), np.zeros(8, rt.POINT_DTYPE)[::2], [[0, 0, 0]], None,
           torch.zeros((4, 4)), torch.zeros((4, 3)), torch.zeros((4, 4), dtype=torch.float64)]
    for b in bad:
        with pytest.raises(ValueError):
            ctx.nearest(b)
    with pytest.raises(ValueError):
        ctx.nearest(np.zeros((4, 3), f32), max_dist2=np.zeros(3, f32))    # 4 points, 3 bounds
    with pytest.raises(ValueError):
        ctx.nearest(np.zeros((4, 4), f32), max_dist2=1.0)                 # the bound is the fourth column
    with pytest.raises(ValueError):
        ctx.nearest(np.zeros(4, rt.POINT_DTYPE), max_dist2=1.0)
    for out in (np.zeros(3, rt.NEAREST_DTYPE), np.zeros((4, 8), f32), np.zeros(8, rt.NEAREST_DTYPE)[::2]):
        with pytest.raises(ValueError):
            ctx.nearest(np.zeros((4, 3), f32), out=out)
    kind, pts = rt.check_nearest_points(np.ones((4, 3), f32), 2.0)
    assert kind == "numpy" and pts.dtype == rt.POINT_DTYPE and (pts["max_dist2"] == 2).all()
    kind, pts = rt.check_nearest_points(np.ones((4, 4), f32))
    assert pts.dtype == rt.POINT_DTYPE and pts.shape == (4,)


# ---------------------------------------------------------------- the restatement
def test_points_include_mesh_vertices_and_shared_minima(case):
    tris, pts, first_vertex, dist2 = case
    verts = pts[first_vertex:first_vertex + 64]
    assert all((tris.reshape(-1, 3) == v).all(1).any() for v in verts)
    ties = (dist2 == dist2.min(1, keepdims=True)).sum(1)
    assert (ties > 1).sum() >= 32   # shared vertices and edges: the id tie-break is exercised


def test_clamped_distance_is_never_below_the_leaf_box_distance(case):
    """dist2 >= bd2 of the leaf's own box for every (point, triangle) pair: what makes the pruning exact
    (DESIGN.md 5d).  (Without the clamp 33 to 485 of these pairs fail in each of the six cases.)"""
    tris, pts, _, dist2 = case
    _, _, _, lo, hi = nr.leaf_data(tris)
    bd2 = nr.box_dist2(pts[:, None, :], lo[None], hi[None])
    assert not np.isnan(dist2).any()
    assert int((dist2 < bd2).sum()) == 0
    # ... and so against any box that contains the leaf box: the root's
    rlo, rhi = nr.root_box(tris)
    assert (dist2 >= nr.box_dist2(pts, rlo, rhi)[:, None]).all()


MEASURED_WORST = 98.5   # in units of 2^-24 of the root box's diagonal, see below


def test_restatement_is_accurate(case):
    """The float32 winner's distance against the smallest distance of a float64 evaluation of the same formulas,
    in units of 2^-24 of the root box's diagonal.  The computation is deterministic.  Measured on these inputs:
    Test 0.72 (reference camera) and 1.05 (identity), Image_Test 2.53 and 3.65, Rect 98.45 and 34.46 -- Rect's
    worst points are centroids and edge midpoints of its twelve large triangles, which lie on the surface to
    within rounding: there the barycentrics come from cancelling products and the square root magnifies what is
    left.  The bound is 4 times the worst, 98.45."""
    tris, pts, _, dist2 = case
    a, e1, e2, lo, hi = nr.leaf_data(tris, np.float64)
    d64 = nr.tri_dist2(pts.astype(np.float64)[:, None, :], a[None], e1[None], e2[None], lo[None], hi[None])[0]
    rlo, rhi = nr.root_box(tris)
    diag = float(np.sqrt(((rhi.astype(np.float64) - rlo) ** 2).sum()))
    err = np.abs(np.sqrt(dist2.min(1).astype(np.float64)) - np.sqrt(d64.min(1))) / diag * 2.0 ** 24
    print(f"worst error: {err.max():.2f} x 2^-24 of the diagonal")
    assert err.max() <= 4 * MEASURED_WORST


def test_brute_force_answers(case):
    """brute(): the (dist2, id) minimum, the bound's edges, and the points that get no result."""
    tris, pts, _, dist2 = case
    want = nr.brute(tris, pts)
    assert want["found"].all()
    np.testing.assert_array_equal(want["dist2"], dist2.min(1))
    np.testing.assert_array_equal(want["tri"], np.argmin(dist2, 1))   # (argmin: the first, smallest id)
    d = want["dist2"]
    pos = d > 0
    assert nr.brute(tris, pts, d)["found"].all()
    assert not nr.brute(tris, pts[pos], np.nextafter(d[pos], np.float32(0)))["found"].any()
    for b in (-1.0, np.nan, -np.inf):
        assert not nr.brute(tris, pts[:8], b)["found"].any()
    bad = pts[:3].copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    r = nr.brute(tris, bad)
    assert not r["found"].any() and (r["tri"] == nr.NONE).all() and (r["dist2"] == -1).all()
