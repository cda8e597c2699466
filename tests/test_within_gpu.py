"""Radius queries on the GPU (rtbvh_within_async / rtbvh_within_host through Context.within and the raw entries)
against the brute force over all triangles (tests/within_ref.py), ordered by the build's sort order
(Context.read_sorted).  The set and its order are specified independently of the walk, so every comparison is
bit-exact: offsets as integers, pairs as (id, dist2 bits) uint32 words."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests import within_ref as wr
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform
from tests.test_query_gpu import random_rays, tiny_scene

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]
OK, NOT_READY, INVALID_ARG, OVERFLOW = (rt._lib.OK, rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG,
                                        rt._lib.ERR_STACK_OVERFLOW)
INF = np.float32(np.inf)
SIZES, FILL, SORT, COUNT = rt.WITHIN_SIZES, rt.WITHIN_FILL, rt.WITHIN_SORT, rt.WITHIN_COUNT
GUARD = 1024                  # pairs behind `capacity`, filled with PATTERN
PATTERN = 0x5A5AA5A5


def camera(name):
    if name == "reference":
        return rt.camera_reference(W, H)
    return np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)


def fixture_scene(name):
    d = load_scene_fixture(name)
    return rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])


def built(scene, wvp, wv, **kw):
    ctx = rt.Context(device=0, **kw)
    ctx.set_scene(scene)
    ctx.set_camera(wvp, wv)
    ctx.build()
    return ctx


def radius2(tris, fraction):
    """(fraction x the root box's diagonal)^2 in float32."""
    lo, hi = nr.root_box(tris)
    return np.float32((np.float32(fraction) * np.float32(np.sqrt(((hi - lo) ** 2).sum()))) ** 2)


def assert_within_equal(got, want, what=""):
    """(offsets, pairs) of Context.within against brute_within's: every offset, every pair's id and dist2 bits."""
    off, pairs = got
    assert off.dtype == np.uint64 and pairs.dtype == rt.PAIR_DTYPE, what
    np.testing.assert_array_equal(off, want[0], err_msg=what + " offsets")
    np.testing.assert_array_equal(wr.pair_bits(pairs), wr.pair_bits(want[1]), err_msg=what + " pairs")


def vp(a):
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


class Device:
    """The raw device entry on the context stream with torch tensors for memory: points up, a pairs buffer of
    capacity + GUARD entries filled with PATTERN, offsets and pairs back."""

    def __init__(self, ctx, packed):
        import torch
        self.torch, self.ctx, self.n = torch, ctx, len(packed)
        self.points = torch.from_numpy(packed.view(np.float32).reshape(-1, 4).copy()).cuda()
        self.offsets = torch.full((self.n + 1,), -1, dtype=torch.int64, device="cuda")

    def run(self, capacity, mode=0, offsets=None, null_pairs=False, expect=OK):
        torch = self.torch
        if offsets is not None:
            self.offsets.copy_(torch.from_numpy(offsets.view(np.int64)))
        buf = torch.full((capacity + GUARD, 2), PATTERN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        L = rt.lib()
        st = L.rtbvh_within_async(self.ctx._h, vp(self.points), self.n, vp(self.offsets),
                                  None if null_pairs else vp(buf), capacity, mode, None)
        assert st == OK
        assert L.rtbvh_synchronize(self.ctx._h) == expect
        words = buf.cpu().numpy().view(np.uint32)
        assert (words[capacity:] == np.uint32(PATTERN)).all(), "a write behind capacity"
        return self.offsets.cpu().numpy().view(np.uint64), words[:capacity]


class Case:
    """A golden scene built on the GPU under one camera, the tests' points, bounds around and away from each point's
    nearest distance, and the brute-force lists in the build's sort order (once)."""

    def __init__(self, scene, cam):
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.T = len(self.tris)
        self.pts, self.first_vertex = nr.sample_points(self.tris)
        self.rank = wr.rank_of(self.ctx.read_sorted()[1])
        dmin = nr.brute(self.tris, self.pts)["dist2"]
        self.k = np.arange(len(self.pts)) % 4
        self.r2 = radius2(self.tris, 0.05)
        self.bound = np.where(self.k == 0, np.nextafter(dmin, np.float32(0)),
                              np.where(self.k == 1, dmin, np.where(self.k == 2, self.r2, INF))).astype(np.float32)
        self.dmin = dmin
        self.want = wr.brute_within(self.tris, self.pts, self.bound, self.rank)
        self.total = int(self.want[0][-1])


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def big():
    """Test.obj under the reference camera with 20,011 points in 1.5 x the root box and their lists within 0.05 x
    the diagonal."""
    c = Case("Test", "reference")
    pts = nr.sample_points(c.tris, seed=11, n_random=20_011, n_each=0)[0]
    yield c, pts, wr.brute_within(c.tris, pts, c.r2, c.rank)
    c.ctx.close()


def head(want, n):
    """brute_within's answer for the first n points."""
    return want[0][:n + 1], want[1][:int(want[0][n])]


# ---------------------------------------------------------------- 1. the brute force
def test_matches_brute_force(case):
    cnt = np.diff(case.want[0]).astype(np.int64)
    k = case.k
    # from the reference: the classes hold what they are there for
    assert (cnt[(k == 0) & (case.dmin > 0)] == 0).all() and ((k == 0) & (case.dmin > 0)).any()
    assert (cnt[k == 1] >= 1).all()
    assert (cnt[k == 2] == 0).any() and (cnt[k == 2] >= 7).any()
    assert (cnt[k == 3] == case.T).all()
    got = case.ctx.within(case.pts, case.bound, capacity=case.total)                 # mode 0: one call
    assert got[0].shape == (len(case.pts) + 1,) and got[1].shape == (case.total,)
    assert_within_equal(got, case.want, "mode 0")
    assert_within_equal(case.ctx.within(case.pts, case.bound, mode=SORT | COUNT, capacity=case.total), case.want,
                        "SORT | COUNT")
    c = case.ctx.within_counts()
    assert c["points"] == len(case.pts) and c["pairs"] == case.total
    assert c["leaf_steps"] >= 2 * case.total                                         # two passes, every member's leaf
    assert_within_equal(case.ctx.within(case.pts, case.bound), case.want, "SIZES then FILL")
    packed = rt.make_points(case.pts, case.bound)
    assert_within_equal(case.ctx.within(packed.view(np.float32).reshape(-1, 4), mode=COUNT), case.want, "(N, 4)")
    assert case.ctx.within_counts()["pairs"] == case.total                           # (the FILL call's)
    assert_within_equal(case.ctx.within(packed, mode=SORT), case.want, "POINT_DTYPE, SORT")


# ---------------------------------------------------------------- 2. capacity
def test_capacity_truncates_and_never_writes_behind(case):
    dev = Device(case.ctx, rt.make_points(case.pts, case.bound))
    want_words = wr.pair_bits(case.want[1])
    for capacity in (case.total, case.total // 2, 1, 0):
        for mode in (0, SORT):
            off, words = dev.run(capacity, mode)
            np.testing.assert_array_equal(off, case.want[0], err_msg=f"capacity {capacity}")
            np.testing.assert_array_equal(words, want_words[:capacity], err_msg=f"capacity {capacity}")
    off, _ = dev.run(0, 0, null_pairs=True)                                           # capacity 0: pairs may be NULL
    np.testing.assert_array_equal(off, case.want[0])
    off, _ = dev.run(0, SIZES, null_pairs=True)
    np.testing.assert_array_equal(off, case.want[0])
    # the host entry: min(total, capacity) pairs
    half = case.total // 2
    off, pairs = case.ctx.within(case.pts, case.bound, capacity=half)
    np.testing.assert_array_equal(off, case.want[0])
    np.testing.assert_array_equal(wr.pair_bits(pairs), want_words[:half])
    off, pairs = case.ctx.within(case.pts, case.bound, capacity=case.total + 5)
    assert_within_equal((off, pairs), case.want, "capacity above the total")


# ---------------------------------------------------------------- 3. FILL over foreign offsets
def test_fill_over_offsets_of_a_smaller_bound_writes_prefixes(case):
    small, large = radius2(case.tris, 0.03), radius2(case.tris, 0.08)
    off_s, _ = wr.brute_within(case.tris, case.pts, small, case.rank)
    off_l, pairs_l = wr.brute_within(case.tris, case.pts, large, case.rank)
    cnt_s, cnt_l = np.diff(off_s).astype(np.int64), np.diff(off_l).astype(np.int64)
    assert (cnt_l > cnt_s).any() and (cnt_s > 0).any() and (cnt_l >= cnt_s).all()
    total = int(off_s[-1])
    # segment k holds the first cnt_s[k] pairs of the larger list of point k
    src = np.concatenate([np.arange(int(off_l[k]), int(off_l[k]) + cnt_s[k]) for k in range(len(case.pts))])
    want_words = wr.pair_bits(pairs_l)[src]
    dev = Device(case.ctx, rt.make_points(case.pts, large))
    for capacity in (total, total // 2):
        for mode in (FILL, FILL | SORT):
            off, words = dev.run(capacity, mode, offsets=off_s)
            np.testing.assert_array_equal(off, off_s)                                 # FILL reads them only
            np.testing.assert_array_equal(words, want_words[:capacity], err_msg=f"capacity {capacity}")


# ---------------------------------------------------------------- 4. no-walk points, tiny scenes
def test_special_points_and_bounds(case):
    lo, hi = nr.root_box(case.tris)
    c = ((lo + hi) / 2).astype(np.float32)
    diag = np.float32(np.sqrt(((hi - lo) ** 2).sum()))
    nan = np.float32(np.nan)
    bad = np.array([[nan, c[1], c[2]], [c[0], nan, c[2]], [c[0], c[1], nan], [nan] * 3, [INF, c[1], c[2]],
                    [c[0], -INF, c[2]], [c[0], c[1], INF], [-INF] * 3], np.float32)
    far = (c + np.float32(1e6) * diag * np.array([[1, 0, 0], [0, -1, 0], [.6, .48, -.64]], np.float32)).astype(np.float32)
    pts = np.concatenate([bad, far, c[None]])
    want = wr.brute_within(case.tris, pts, INF, case.rank)
    cnt = np.diff(want[0]).astype(np.int64)
    assert (cnt[:len(bad)] == 0).all() and (cnt[len(bad):] == case.T).all()
    assert_within_equal(case.ctx.within(pts), want)
    assert_within_equal(case.ctx.within(pts, mode=SORT | COUNT, capacity=int(want[0][-1])), want, "SORT | COUNT")
    assert case.ctx.within_counts()["points"] == len(pts)
    want = wr.brute_within(case.tris, pts, case.r2, case.rank)       # far points: walked, nothing within
    assert (np.diff(want[0])[len(bad):len(bad) + len(far)] == 0).all()
    assert_within_equal(case.ctx.within(pts, case.r2), want, "bounded")
    n = 32
    for b in (np.float32(-1), nan, -INF, np.float32(-1e-30)):       # no walk: empty lists
        off, pairs = case.ctx.within(case.pts[:n], b)
        assert (off == 0).all() and off.shape == (n + 1,) and len(pairs) == 0, f"bound {b}"
        off, pairs = case.ctx.within(case.pts[:n], b, capacity=8)
        assert (off == 0).all() and len(pairs) == 0, f"bound {b}, mode 0"
    verts = case.pts[case.first_vertex:case.first_vertex + 64]      # on vertices with bound 0 and -0
    want = wr.brute_within(case.tris, verts, np.float32(0), case.rank)
    assert (np.diff(want[0]) >= 1).all() and (want[1]["dist2"] == 0).all()
    for zero in (np.float32(0), np.float32(-0.0)):
        assert_within_equal(case.ctx.within(verts, zero), want, "on a vertex, bound 0")


@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = tiny_scene(ntris)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = wr.rank_of(ctx.read_sorted()[1])
        pts = nr.sample_points(tris, seed=ntris, n_random=300, n_each=16, scale=3.0)[0]
        d = nr.brute(tris, pts)["dist2"]
        k = np.arange(len(d)) % 3
        bound = np.where(k == 0, d, np.where(k == 1, np.nextafter(d, np.float32(0)), INF)).astype(np.float32)
        want = wr.brute_within(tris, pts, bound, rank)
        assert (np.diff(want[0])[k == 2] == ntris).all() and (np.diff(want[0])[(k == 1) & (d > 0)] == 0).all()
        assert_within_equal(ctx.within(pts, bound), want)
        assert_within_equal(ctx.within(pts, bound, mode=SORT, capacity=int(want[0][-1])), want, "SORT, mode 0")


# ---------------------------------------------------------------- 5. sizes: claims, partial waves, scan tiles, refill
@pytest.mark.parametrize("n", [1, 63, 65, 257, 20_011])
def test_sizes(big, n):
    c, pts, want = big
    w = head(want, n)
    assert_within_equal(c.ctx.within(pts[:n], c.r2), w)
    assert_within_equal(c.ctx.within(pts[:n], c.r2, mode=SORT | COUNT, capacity=len(w[1])), w, "SORT | COUNT")
    counts = c.ctx.within_counts()
    assert counts["points"] == n and counts["pairs"] == len(w[1])
    off, pairs = c.ctx.within(pts[:0], c.r2)
    assert off.tolist() == [0] and pairs.shape == (0,)


def test_more_points_than_the_grid_has_lanes():
    s = fixture_scene("Rect")
    wvp, wv = rt.camera_reference(W, H)
    n = 600_000   # > 524,288 lanes of the persistent grid: refills; 293 scan tiles
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        pts = nr.sample_points(tris, seed=17, n_random=n, n_each=0)[0]
        r2 = radius2(tris, 0.05)
        want = wr.brute_within(tris, pts, r2, wr.rank_of(ctx.read_sorted()[1]))
        cnt = np.diff(want[0])
        assert (cnt == 0).any() and (cnt >= 3).any()
        assert_within_equal(ctx.within(pts, r2, capacity=int(want[0][-1])), want)
        assert_within_equal(ctx.within(pts, r2, mode=SORT), want, "SORT")


# ---------------------------------------------------------------- 6. both tree forms
def test_records_and_node_box_trees_agree():
    s = rt.synthetic(70_000, seed=0x5EED0004)
    T = 70_000
    wvp, wv = rt.camera_reference(W, H)
    with built(s, wvp, wv, flags=rt.FLAG_AUTO_WALK) as auto, built(s, wvp, wv) as plain:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        pts = nr.sample_points(tris, seed=3, n_random=384, n_each=43)[0][:512]
        assert len(pts) == 512
        r2 = radius2(tris, 0.02)
        sa, sp = auto.read_sorted()[1], plain.read_sorted()[1]
        np.testing.assert_array_equal(sa, sp)
        want = wr.brute_within(tris, pts, r2, wr.rank_of(sp))
        total = int(want[0][-1])
        assert total > 512
        o, d = random_rays(plain.read_bvh(), 2000, seed=3)
        rays = rt.make_rays(o, d)
        for c in (auto, plain):   # counting ray and closest-point queries first: their counts must survive
            c.query(rays, rt.QUERY_COUNT)
            c.nearest(pts, mode=rt.NEAREST_COUNT)
        ray_counts, near_counts = plain.query_counts(), plain.nearest_counts()
        assert auto.query_counts() == ray_counts and auto.nearest_counts() == near_counts
        a, p = (c.within(pts, r2, mode=COUNT, capacity=total) for c in (auto, plain))
        np.testing.assert_array_equal(a[0], p[0])
        np.testing.assert_array_equal(wr.pair_bits(a[1]), wr.pair_bits(p[1]))
        assert_within_equal(a, want)
        ca, cp = auto.within_counts(), plain.within_counts()
        print("radius query steps per point (two passes):", {k: v / 512 for k, v in ca.items()})
        assert ca == cp   # the same visits on both forms
        assert ca["points"] == 512 and ca["pairs"] == total
        assert 0 < ca["leaf_steps"] < 512 * T // 8 and ca["internal_steps"] > 0
        for c in (auto, plain):
            assert_within_equal(c.within(pts, r2, mode=SORT), want, "SORT")
            assert c.query_counts() == ray_counts and c.nearest_counts() == near_counts
            c.query(rays[:100], rt.QUERY_COUNT)
            c.nearest(pts[:50], mode=rt.NEAREST_COUNT)
            assert c.query_counts()["rays"] == 100 and c.nearest_counts()["points"] == 50
            assert c.within_counts() == ca            # ... and they leave these alone


# ---------------------------------------------------------------- 7. device tensors and streams
def test_device_tensors_on_two_streams(big):
    import torch
    c, pts, want = big
    n = len(pts)
    total = int(want[0][-1])
    m = 4096
    want_b = wr.brute_within(c.tris, pts[:m], radius2(c.tris, 0.08), c.rank)
    p1 = torch.from_numpy(rt.make_points(pts, c.r2).view(np.float32).reshape(n, 4)).cuda()
    p2 = rt.make_points(torch.from_numpy(pts[:m]).cuda(), float(radius2(c.tris, 0.08)))
    o, dd = random_rays(c.ctx.read_bvh(), 4096, seed=5)
    rays = torch.from_numpy(rt.make_rays(o, dd).view(np.float32).reshape(-1, 8)).cuda()
    hits_want = c.ctx.query(rt.make_rays(o, dd))
    near_want = c.ctx.nearest(pts[:m])
    pn = torch.from_numpy(rt.make_points(pts[:m]).view(np.float32).reshape(m, 4)).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    o1, r1 = c.ctx.within(p1, mode=COUNT, capacity=total + 7, stream=s1)   # back to back, one context, two streams
    hits = c.ctx.query(rays, stream=s2)
    o2, r2 = c.ctx.within(p2, mode=SORT, stream=s1)                        # capacity=None: sized from the total
    near = c.ctx.nearest(pn, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert o1.is_cuda and o1.dtype == torch.int64 and tuple(o1.shape) == (n + 1,)
    assert r1.is_cuda and r1.dtype == torch.float32 and tuple(r1.shape) == (total + 7, 2)
    np.testing.assert_array_equal(o1.cpu().numpy().view(np.uint64), want[0])
    np.testing.assert_array_equal(r1[:total].cpu().numpy().view(np.uint32), wr.pair_bits(want[1]))
    np.testing.assert_array_equal(r1[:total, 0].view(torch.int32).cpu().numpy(), want[1]["tri"].view(np.int32))
    assert tuple(r2.shape) == (int(want_b[0][-1]), 2)
    np.testing.assert_array_equal(o2.cpu().numpy().view(np.uint64), want_b[0])
    np.testing.assert_array_equal(r2.cpu().numpy().view(np.uint32), wr.pair_bits(want_b[1]))
    np.testing.assert_array_equal(hits.cpu().numpy().view(np.uint32), hits_want.view(np.uint32).reshape(-1, 4))
    np.testing.assert_array_equal(near.cpu().numpy().view(np.uint32), near_want.view(np.uint32).reshape(-1, 8))
    assert c.ctx.within_counts()["points"] == n and c.ctx.within_counts()["pairs"] == total
    # the current stream (torch's default one) and a side stream made current; capacity given and not
    o3, r3 = c.ctx.within(p2)
    np.testing.assert_array_equal(o3.cpu().numpy(), o2.cpu().numpy())
    np.testing.assert_array_equal(r3.cpu().numpy().view(np.uint32), r2.cpu().numpy().view(np.uint32))
    s1.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        o4, r4 = c.ctx.within(p2, capacity=r2.shape[0])
    s1.synchronize()
    np.testing.assert_array_equal(o4.cpu().numpy(), o2.cpu().numpy())
    np.testing.assert_array_equal(r4.cpu().numpy().view(np.uint32), r2.cpu().numpy().view(np.uint32))
    with pytest.raises(ValueError):
        c.ctx.within(p1[:, :3])
    c.ctx.synchronize()


# ---------------------------------------------------------------- 8. animated geometry
@pytest.mark.parametrize("flags", [0, rt.FLAG_AUTO_WALK], ids=["plain", "auto"])
def test_after_update_refit_and_rebuild(flags):
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    P = deform(s.vertices[:, :3], 0.7)
    v = s.vertices.copy()
    v[:, :3] = P
    tris = rw.clip_triangles(v, s.indices, wvp)
    pts = nr.sample_points(tris, seed=9, n_random=384, n_each=43)[0]
    r2 = radius2(tris, 0.05)
    with built(s, wvp, wv, flags=flags) as ctx:
        old_order = ctx.read_sorted()[1].copy()
        before = ctx.within(pts, r2)
        ctx.update_vertices(P)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.within(pts, r2)
        assert e.value.status == NOT_READY
        ctx.refit()
        np.testing.assert_array_equal(ctx.read_sorted()[1], old_order)   # a refit keeps the order
        want = wr.brute_within(tris, pts, r2, wr.rank_of(old_order))
        refit = ctx.within(pts, r2)
        assert_within_equal(refit, want, "after the refit")
        assert not (np.array_equal(before[0], refit[0]) and np.array_equal(before[1], refit[1]))
        ctx.build()   # another tree over the same geometry: the same sets, in the new order
        new_order = ctx.read_sorted()[1]
        rebuilt = ctx.within(pts, r2)
        assert_within_equal(rebuilt, wr.brute_within(tris, pts, r2, wr.rank_of(new_order)), "after the rebuild")
        np.testing.assert_array_equal(rebuilt[0], refit[0])
        for k in range(len(pts)):
            a, b = (x[1][int(x[0][k]):int(x[0][k + 1])] for x in (refit, rebuilt))
            np.testing.assert_array_equal(np.sort(wr.pair_bits(a).view(np.uint64).ravel()),
                                          np.sort(wr.pair_bits(b).view(np.uint64).ravel()))


# ---------------------------------------------------------------- 9. errors, the stack limit
def test_errors():
    import torch
    pts = rt.make_points(np.zeros((4, 3), np.float32))
    off = np.zeros(5, np.uint64)
    pairs = np.zeros(64, rt.PAIR_DTYPE)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.within(pts)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.within_counts()
        assert e.value.status == NOT_READY
        o, p = ctx.within(pts[:0])                  # n == 0 is OK even before a build
        assert o.tolist() == [0] and p.shape == (0,)
        ctx.build()
        h = ctx._h
        dp = torch.from_numpy(pts.view(np.float32).reshape(-1, 4).copy()).cuda()
        doff = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        dpairs = torch.zeros((64, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for mode in (1, 8, 64, 1 << 8, 1 << 31, SIZES | FILL, SORT | 8):
            assert L.rtbvh_within_async(h, vp(dp), 4, vp(doff), vp(dpairs), 64, mode, None) == INVALID_ARG, mode
            assert L.rtbvh_within_host(h, vp(pts), 4, vp(off), vp(pairs), 64, mode) == INVALID_ARG, mode
        assert L.rtbvh_within_async(h, None, 4, vp(doff), vp(dpairs), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_within_async(h, vp(dp), 4, None, vp(dpairs), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_within_async(h, vp(dp), 4, vp(doff), None, 64, 0, None) == INVALID_ARG
        assert L.rtbvh_within_async(h, vp(dp), 4, vp(doff), None, 64, FILL, None) == INVALID_ARG
        assert L.rtbvh_within_async(h, vp(dp), 1 << 31, vp(doff), vp(dpairs), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_within_host(h, vp(pts), 4, None, vp(pairs), 64, 0) == INVALID_ARG
        assert L.rtbvh_within_host(h, vp(pts), 4, vp(off), None, 64, 0) == INVALID_ARG
        assert L.rtbvh_within_host(h, vp(pts), 1 << 31, vp(off), vp(pairs), 64, 0) == INVALID_ARG
        assert L.rtbvh_within_counts(h, None) == INVALID_ARG
        ctx.synchronize()
        assert (doff.cpu().numpy() == -1).all()     # nothing was written by the rejected calls
        # NULL pairs are fine with capacity 0 and under SIZES; n == 0 writes offsets[0] only where there is one
        assert L.rtbvh_within_async(h, vp(dp), 4, vp(doff), None, 0, 0, None) == OK
        assert L.rtbvh_within_async(h, vp(dp), 4, vp(doff), None, 64, SIZES, None) == OK
        assert L.rtbvh_within_async(h, None, 0, None, None, 0, 0, None) == OK
        ctx.synchronize()
        assert doff.cpu().numpy().tolist() == [0, 12, 24, 36, 48]   # (the SIZES call: Rect's 12 triangles each)
        doff.fill_(-1)
        torch.cuda.synchronize()
        assert L.rtbvh_within_async(h, None, 0, vp(doff), None, 0, 0, None) == OK
        ctx.synchronize()
        assert doff.cpu().numpy().tolist() == [0, -1, -1, -1, -1]
        with pytest.raises(rt.RtbvhError) as e:
            ctx.within_counts()                     # still no counting radius query
        assert e.value.status == NOT_READY
        d = load_scene_fixture("Rect")              # and the context still answers
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(W, H)[0])
        assert_within_equal(ctx.within(pts), wr.brute_within(tris, pts["point"], INF, wr.rank_of(ctx.read_sorted()[1])))
        ctx.synchronize()


def test_stack_limit_reports_overflow_and_keeps_genuine_pairs():
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    pts = nr.sample_points(tris, seed=13)[0]
    r2 = radius2(tris, 0.05)
    n = len(pts)
    with built(s, wvp, wv, stack_limit=2) as ctx:
        want = wr.brute_within(tris, pts, r2, wr.rank_of(ctx.read_sorted()[1]))
        cap = int(want[0][-1])
        dev = Device(ctx, rt.make_points(pts, r2))
        off, words = dev.run(cap, 0, expect=OVERFLOW)   # (its guard region: untouched)
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK   # once per new overflow
        # offsets are consistent, and a walk that lost subtrees lists a subsequence of the point's true list
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
        total = int(off[-1])
        assert 0 < total < cap
        assert (words[total:] == PATTERN).all()     # the fill pass wrote what the sizes pass counted, no more
        assert (words[:total, 0] != PATTERN).all()  # ... and no less (an id is below T)
        true_words = wr.pair_bits(want[1]).view(np.uint64).ravel()
        got_words = np.ascontiguousarray(words[:total]).view(np.uint64).ravel()
        assert len(np.intersect1d(got_words, true_words)) > 0
        for k in range(n):
            g = got_words[int(off[k]):int(off[k + 1])]
            t = true_words[int(want[0][k]):int(want[0][k + 1])]
            idx = {w: i for i, w in enumerate(t.tolist())}
            where = [idx.get(w, -1) for w in g.tolist()]
            assert -1 not in where and where == sorted(where), k
