"""Region queries without a GPU: the ABI's names and layouts, the helpers and Context.region's argument checks, the
brute force (tests/region_ref.py), and on the oracle's tree what the GPU walk leans on -- pruning on m <= 0 skips no
member, taking a subtree with M <= 0 whole lists members only while no leaf box holds a NaN (and lists a non-member
when that guard is ignored), a left-first walk meets the triangles in the build's sort order -- that six axis planes
are the box query's (B), and the sanity check of the fp32 plane value against its float64 evaluation."""
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import deep_scenes as ds
from tests import hostile_scenes as hs
from tests import nearest_ref as nr
from tests import overlap_ref as ovr
from tests import ray_walk_ref as rw
from tests import region_ref as rr
from tests import within_ref as wr
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]
U = 2.0 ** -24
GAMMA4 = 4 * U / (1 - 4 * U)     # the forward bound of s: three products and three sums


def camera(name):
    return rt.camera_reference(64, 48)[0] if name == "reference" else np.eye(4, dtype=np.float32)


def lists(off, ids):
    return [ids[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]


# ---------------------------------------------------------------- the ABI and the helpers
def test_exports_constants_and_sizes():
    L = rt.lib()
    for name in ("rtbvh_region_async", "rtbvh_region_host", "rtbvh_region_counts"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.REGION_COUNT, rt.REGION_TRIANGLE, rt.REGION_SIZES, rt.REGION_FILL, rt.REGION_NO_ACCEPT) == \
        (1 << 2, 1 << 3, 1 << 4, 1 << 5, 1 << 6)
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    for name, bit in (("COUNT", 2), ("TRIANGLE", 3), ("SIZES", 4), ("FILL", 5), ("NO_ACCEPT", 6)):
        assert re.search(rf"RTBVH_REGION_{name} = 1u << {bit}\b", header), name
    assert "RTBVH_REGION_SORT" not in header
    assert re.search(r"typedef struct rtbvh_region \{\s*float plane\[6\]\[4\];", header)
    assert rt.REGION_DTYPE.itemsize == 96 and rt.REGION_DTYPE.fields["plane"][0].shape == (6, 4)
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_helpers_shapes_and_dtypes():
    import torch
    f32 = np.float32
    p = np.arange(2 * 3 * 4, dtype=f32).reshape(2, 3, 4) + 1
    r = rt.make_regions(p)
    assert r.dtype == rt.REGION_DTYPE and r.shape == (2,)
    np.testing.assert_array_equal(r["plane"][:, :3], p)
    assert not r["plane"][:, 3:].any()                              # zero-padded: the unused planes
    assert rt.make_regions(p[0]).shape == (1,)                      # one region's (P, 4)
    t = rt.make_regions(torch.from_numpy(p))
    assert tuple(t.shape) == (2, 24) and t.dtype == torch.float32
    np.testing.assert_array_equal(t.numpy().reshape(2, 6, 4), r["plane"])
    for bad in (np.zeros((2, 7, 4), f32), np.zeros((2, 3, 3), f32), np.zeros(5, f32)):
        with pytest.raises(ValueError):
            rt.make_regions(bad)
    lo, hi = np.array([[-1, -2, -3], [0, 0, 0]], f32), np.array([[1, 2, 3], [4, 5, 6]], f32)
    b = rt.box_region(lo, hi)
    assert b.dtype == rt.REGION_DTYPE and b.shape == (2,)
    np.testing.assert_array_equal(b["plane"][0], [[-1, 0, 0, -1], [1, 0, 0, -1], [0, -1, 0, -2], [0, 1, 0, -2],
                                                  [0, 0, -1, -3], [0, 0, 1, -3]])
    with pytest.raises(ValueError):
        rt.box_region(lo, hi[:1])
    s = rt.slab_region([[0, 0, 1], [1, 0, 0]], [1, 2], 3)
    assert s.dtype == rt.REGION_DTYPE and s.shape == (2,)
    np.testing.assert_array_equal(s["plane"][0, :2], [[0, 0, -1, 1], [0, 0, 1, -3]])
    np.testing.assert_array_equal(s["plane"][1, :2], [[-1, 0, 0, 2], [1, 0, 0, -3]])
    assert not s["plane"][:, 2:].any()
    fp = rt.frustum_planes(rt.camera_reference(64, 48)[0])
    assert fp.shape == (6, 4) and fp.dtype == f32 and np.isfinite(fp).all()
    ident = rt.frustum_planes(np.eye(4, dtype=f32))                 # -1 <= x, y <= 1, 0 <= z <= 1
    np.testing.assert_array_equal(ident, [[-1, 0, 0, -1], [1, 0, 0, -1], [0, -1, 0, -1], [0, 1, 0, -1],
                                          [0, 0, -1, 0], [0, 0, 1, -1]])
    kind, got = rt.check_region_planes(p)
    assert kind == "numpy" and got.tobytes() == r.tobytes()
    kind, got = rt.check_region_planes(r.view(f32).reshape(2, 24))
    assert kind == "numpy" and got.dtype == rt.REGION_DTYPE and got.tobytes() == r.tobytes()


def test_bad_arguments_are_rejected_before_the_library_is_called():
    import torch
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    f32 = np.float32
    bad = [np.zeros((4, 23), f32), np.zeros((4, 7, 4), f32), np.zeros((4, 6, 3), f32), np.zeros(24, f32),
           np.zeros((4, 24), np.float64), np.zeros((8, 24), f32)[::2], np.zeros((2, 2), rt.REGION_DTYPE), [[0] * 24],
           None, torch.zeros((4, 24)), torch.zeros((4, 8)), torch.zeros((4, 24), dtype=torch.float64)]
    for b in bad:
        with pytest.raises(ValueError):
            ctx.region(b)
    ok = np.zeros(4, rt.REGION_DTYPE)
    for mode in (rt.REGION_SIZES, rt.REGION_FILL, 1, 2, 1 << 7, 1 << 8):   # region sets the first two itself
        with pytest.raises(ValueError):
            ctx.region(ok, mode=mode)
    for capacity in (-1, 1.5):
        with pytest.raises(ValueError):
            ctx.region(ok, capacity=capacity)
    with pytest.raises(ValueError):
        ctx.region(ok, capacity=4, sizes_only=True)


# ---------------------------------------------------------------- the brute force
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_brute_region_properties(scene, cam):
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
    T = len(tris)
    rank = np.random.default_rng(7).permutation(T)     # any order: membership does not depend on it
    regions = rr.sample_regions(tris, 5)
    n = len(regions)
    assert n == 6 * 48 + 5 and regions.dtype == rt.REGION_DTYPE
    off_b, ids_b = rr.brute_region(tris, regions, rank)
    off_v, ids_v = rr.brute_region(tris, regions, rank, triangle=True)
    assert off_b.dtype == np.uint64 and ids_b.dtype == np.uint32
    assert off_b[0] == 0 == off_v[0] and off_b[-1] == len(ids_b) and off_v[-1] == len(ids_v)
    assert 0 < off_v[-1] < off_b[-1] < n * T                      # (V) rejects something; pruning to do
    cb, cv = np.diff(off_b).astype(np.int64), np.diff(off_v).astype(np.int64)
    for lb, lv in zip(lists(off_b, ids_b), lists(off_v, ids_v)):
        assert (np.diff(rank[lb]) > 0).all()                      # each list ascending by rank
        assert set(lv.tolist()) <= set(lb.tolist())
    S = rr.SPECIAL
    for c in (cb, cv):
        assert c[S["whole"]] == T and c[S["zero"]] == T           # every triangle: the unused planes hold everywhere
        assert c[S["never"]] == 0 and c[S["nan"]] == 0 and c[S["inf"]] == 0
    np.testing.assert_array_equal(lists(off_b, ids_b)[S["whole"]], np.argsort(rank))
    cls = np.arange(6 * 48) // 48
    for k in range(6):
        assert cv[:6 * 48][cls == k].sum() > 0, k                 # every class lists something
    assert (cb[:6 * 48][cls == 5] > T // 4).any()                 # some regions hold much of the scene
    # a zero-thickness slab through a vertex lists that vertex's triangles (class 3), in both modes
    assert (cv[:6 * 48][cls == 3] >= 1).all()


# ---------------------------------------------------------------- the walk, on the oracle's tree
def dfs_region(nodes, ranges, order, leaf, planes6, triangle, nan_free, out, stats, accept=True):
    """trace.hip k_region's walk for one region in plain Python: the root's own box first; a child is entered iff
    m <= 0 on every plane; an internal child with M <= 0 on every plane is taken whole (its leaf range, in order)
    while `nan_free` -- at once when it is the left child or stands behind an accepted or pruned left child, else it
    waits on the stack as an ordinary node; a leaf tests its own box, then (V)."""
    n = (len(nodes) + 1) // 2
    a, e1, e2, lo, hi = leaf
    bmin, bmax = nodes["bb_min"], nodes["bb_max"]
    first, last = ranges
    if not np.isfinite(planes6).all():
        return

    def leaf_test(k):
        stats["leaf"] += 1
        t = int(order[k])
        if rr.box_enter(planes6, lo[t], hi[t]) and (not triangle or rr.vertices_pass(planes6, a[t], e1[t], e2[t], lo[t], hi[t])):
            out.append(t)

    def take(x):
        stats["accepted"] += 1
        stats["accepted_ids"] += int(last[x - n] - first[x - n] + 1)
        out.extend(int(t) for t in order[first[x - n]:last[x - n] + 1])

    if n == 1:
        return leaf_test(0)
    if not rr.box_enter(planes6, bmin[n], bmax[n]):
        return
    if accept and nan_free and rr.box_inside(planes6, bmin[n], bmax[n]):
        return take(n)
    stack = [n]
    while stack:
        k = stack.pop()
        if k < n:
            leaf_test(k)
            continue
        stats["internal"] += 1
        l, r = int(nodes["child_l"][k]), int(nodes["child_r"][k])
        lh, rh = rr.box_enter(planes6, bmin[l], bmax[l]), rr.box_enter(planes6, bmin[r], bmax[r])
        la = bool(lh and accept and nan_free and l >= n and rr.box_inside(planes6, bmin[l], bmax[l]))
        ra = bool(rh and accept and nan_free and r >= n and rr.box_inside(planes6, bmin[r], bmax[r]) and (la or not lh))
        if la:
            take(l)
        if ra:
            take(r)
        if rh and not ra:
            stack.append(r)   # below the left one: walked after it
        if lh and not la:
            stack.append(l)


def walk_all(nodes, tris, regions, triangle, accept=True, ignore_guard=False):
    T = len(tris)
    leaf = nr.leaf_data(tris)
    order = nodes["index"][:T] // 3
    ranges = ds.leaf_ranges(nodes) if T > 1 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    nan_free = ignore_guard or not (np.isnan(leaf[3]).any() or np.isnan(leaf[4]).any())
    got, off = [], [0]
    stats = dict(internal=0, leaf=0, accepted=0, accepted_ids=0)
    for p in rr.as_planes(regions):
        dfs_region(nodes, ranges, order, leaf, p, triangle, nan_free, got, stats, accept)
        off.append(len(got))
    return np.array(off, np.uint64), np.array(got, np.uint32), stats


def check_walk(osc, wvp, tris, seed, finite_only=None):
    nodes = orc.build(osc, wvp)
    T = len(tris)
    order = nodes["index"][:T] // 3
    assert sorted(order.tolist()) == list(range(T))
    rank = wr.rank_of(order)
    regions = rr.sample_regions(tris if finite_only is None else tris[finite_only], seed, n_each=4)
    out = {}
    for triangle in (False, True):
        want = rr.brute_region(tris, regions, rank, triangle)
        assert 0 < want[0][-1] < len(regions) * T
        off, ids, st = walk_all(nodes, tris, regions, triangle)
        np.testing.assert_array_equal(off, want[0])
        np.testing.assert_array_equal(ids, want[1])
        off, ids, st_no = walk_all(nodes, tris, regions, triangle, accept=False)
        np.testing.assert_array_equal(off, want[0])
        np.testing.assert_array_equal(ids, want[1])
        assert st_no["accepted"] == 0
        assert st["internal"] + st["leaf"] <= st_no["internal"] + st_no["leaf"]
        out[triangle] = (st, st_no)
    return out


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_pruned_accepting_walk_is_the_brute_force_in_sort_order(scene, cam):
    d = load_scene_fixture(scene)
    wvp = camera(cam)
    osc = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    for st, st_no in check_walk(osc, wvp, tris, 21).values():
        assert st["accepted"] > 0 and st["accepted_ids"] > 0       # the accept is exercised
        assert st["internal"] + st["leaf"] < st_no["internal"] + st_no["leaf"]


@pytest.mark.parametrize("cam", hs.CAMERAS)
@pytest.mark.parametrize("variant", list(hs.VARIANTS))
def test_walk_on_hostile_scenes(variant, cam):
    h = hs.hostile(variant)
    wvp = hs.camera(cam)[0]
    tris = h.tris(wvp)
    stats = check_walk(hs.oracle_scene(h.scene), wvp, tris, 23, hs.finite_part(tris, h.labels))
    nan_leaf = np.isnan(np.stack(nr.leaf_data(tris)[3:])).any()
    assert nan_leaf == (variant in hs.NONFINITE_VARIANTS)
    for st, _ in stats.values():
        assert (st["accepted"] == 0) == bool(nan_leaf)             # the guard: no accepts on a tree with a NaN leaf box


def test_the_nan_guard_is_needed():
    s = rr.nan_triangle_scene()
    wvp = np.eye(4, dtype=np.float32)
    with np.errstate(all="ignore"):
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        nodes = orc.build(hs.oracle_scene(s), wvp)
    T = len(tris)
    assert T == 33
    assert np.isfinite(nodes["bb_min"][T]).all() and np.isfinite(nodes["bb_max"][T]).all()   # node boxes drop the NaN
    fin = tris[np.isfinite(tris).all((1, 2))]
    lo, hi = nr.root_box(fin)
    whole = rt.box_region(lo - 1, hi + 1)
    rank = wr.rank_of(nodes["index"][:T] // 3)
    for triangle in (False, True):
        want = rr.brute_region(tris, whole, rank, triangle)
        assert int(want[0][-1]) == T - 1                           # the NaN triangle fails (B)
        off, ids, st = walk_all(nodes, tris, whole, triangle)
        np.testing.assert_array_equal(ids, want[1])
        assert st["accepted"] == 0 and st["leaf"] == T - 1         # every leaf but the NaN one, pruned at its parent
        off, ids, st = walk_all(nodes, tris, whole, triangle, ignore_guard=True)
        assert len(ids) == T and st["accepted"] == 1 and st["leaf"] == 0   # a non-member listed: the guard is needed


# ---------------------------------------------------------------- six axis planes are the box query's (B)
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_axis_planes_equal_overlap(scene, cam):
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
    rank = np.random.default_rng(11).permutation(len(tris))
    qlo, qhi = ovr.sample_boxes(tris, 5)
    walk = ovr.valid_boxes(qlo, qhi)
    assert walk.all()
    want = ovr.brute_overlap(tris, qlo, qhi, rank)
    got = rr.brute_region(tris, rt.box_region(qlo, qhi), rank)
    assert want[0][-1] > 0
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


# ---------------------------------------------------------------- fp32 against float64
def value_and_bound(planes, x):
    """s in fp32 and in float64 of the same floats, and gamma_4 (|n_x x| + |n_y y| + |n_z z| + |d|)."""
    p64, x64 = np.asarray(planes, np.float64), np.asarray(x, np.float64)
    mag = (np.abs(p64[..., :3] * x64)).sum(-1) + np.abs(p64[..., 3])
    return rr.plane_value(planes, x), rr.plane_value(planes, x, np.float64), GAMMA4 * mag


@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("scene", SCENES)
def test_plane_value_agrees_with_its_float64_evaluation_outside_the_bound(scene, cam):
    """Every (plane, vertex) pair of the sampled regions' used planes and the scene's vertices.  Measured with these
    fixtures and seed 5: see DESIGN.md 5o for the pairs inside the bound."""
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], camera(cam))
    planes = rr.as_planes(rr.sample_regions(tris, 5)[:6 * 48]).reshape(-1, 4)
    planes = planes[(planes != 0).any(1)]
    verts = np.unique(tris.reshape(-1, 3), axis=0)
    s32, s64, bound = value_and_bound(planes[:, None], verts[None])
    outside = np.abs(s64) > bound
    inside = int((~outside).sum())
    print(f"{scene}/{cam}: {s32.size} (plane, vertex) pairs, {inside} inside the bound")
    assert outside.sum() > s32.size // 2
    assert ((s32 <= 0) == (s64 <= 0))[outside].all()


@pytest.mark.parametrize("scene", SCENES)
def test_frustum_lists_hold_every_triangle_with_a_vertex_well_inside(scene):
    """The reference camera's frustum over the scene in object space (a context built with an identity camera)."""
    d = load_scene_fixture(scene)
    tris = rw.clip_triangles(d["vertices"], d["indices"], np.eye(4, dtype=np.float32))
    planes = rt.frustum_planes(rt.camera_reference(64, 48)[0])
    region = rt.make_regions(planes)
    T = len(tris)
    rank = np.arange(T)
    off, ids = rr.brute_region(tris, region, rank, triangle=True)
    a, e1, e2, lo, hi = nr.leaf_data(tris)
    well = np.zeros(T, bool)
    for v in rr.clamped_vertices(a, e1, e2, lo, hi):
        _, s64, bound = value_and_bound(planes[None], v[:, None])
        well |= (s64 < -bound).all(1)
    assert well.sum() > 0
    assert set(np.nonzero(well)[0].tolist()) <= set(ids.tolist())
    off_b, ids_b = rr.brute_region(tris, region, rank)
    assert set(ids.tolist()) <= set(ids_b.tolist())
