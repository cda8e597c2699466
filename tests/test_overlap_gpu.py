"""Box-overlap queries on the GPU (rtbvh_overlap_async / rtbvh_overlap_host through Context.overlap and the raw
entries) against the brute force over all triangles (tests/overlap_ref.py), ordered by the build's sort order
(Context.read_sorted).  The set and its order are specified independently of the walk, in both modes (leaf boxes
only, and with the triangle-box test), so every comparison is bit-exact: offsets and ids as integers."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import nearest_ref as nr
from tests import overlap_ref as ovr
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
SIZES, FILL, SORT, COUNT, TRI = (rt.OVERLAP_SIZES, rt.OVERLAP_FILL, rt.OVERLAP_SORT, rt.OVERLAP_COUNT,
                                 rt.OVERLAP_TRIANGLE)
MODES = [0, TRI]
MODE_IDS = ["boxes", "triangles"]
GUARD = 1024                  # ids behind `capacity`, filled with PATTERN
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


def assert_overlap_equal(got, want, what=""):
    """(offsets, ids) of Context.overlap against brute_overlap's: every offset and every id."""
    off, ids = got
    assert off.dtype == np.uint64 and ids.dtype == np.uint32, what
    np.testing.assert_array_equal(off, want[0], err_msg=what + " offsets")
    np.testing.assert_array_equal(ids, want[1], err_msg=what + " ids")


def vp(a):
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def shrunk(qlo, qhi):
    """Boxes with the same centres and half the extents."""
    q = (qhi - qlo) * np.float32(0.25)
    return (qlo + q).astype(np.float32), (qhi - q).astype(np.float32)


class Device:
    """The raw device entry on the context stream with torch tensors for memory: boxes up, an ids buffer of
    capacity + GUARD words filled with PATTERN, offsets and ids back."""

    def __init__(self, ctx, packed):
        import torch
        self.torch, self.ctx, self.n = torch, ctx, len(packed)
        self.boxes = torch.from_numpy(packed.view(np.float32).reshape(-1, 8).copy()).cuda()
        self.offsets = torch.full((self.n + 1,), -1, dtype=torch.int64, device="cuda")

    def run(self, capacity, mode=0, offsets=None, null_ids=False, expect=OK):
        torch = self.torch
        if offsets is not None:
            self.offsets.copy_(torch.from_numpy(offsets.view(np.int64)))
        buf = torch.full((capacity + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        L = rt.lib()
        st = L.rtbvh_overlap_async(self.ctx._h, vp(self.boxes), self.n, vp(self.offsets),
                                   None if null_ids else vp(buf), capacity, mode, None)
        assert st == OK
        assert L.rtbvh_synchronize(self.ctx._h) == expect
        words = buf.cpu().numpy().view(np.uint32)
        assert (words[capacity:] == np.uint32(PATTERN)).all(), "a write behind capacity"
        return self.offsets.cpu().numpy().view(np.uint64), words[:capacity]


class Case:
    """A golden scene built on the GPU under one camera, the tests' boxes and the brute-force lists of both modes
    in the build's sort order (once)."""

    def __init__(self, scene, cam):
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.T = len(self.tris)
        self.qlo, self.qhi = ovr.sample_boxes(self.tris, 5)
        self.boxes = rt.make_boxes(self.qlo, self.qhi)
        self.rank = wr.rank_of(self.ctx.read_sorted()[1])
        self.want = {m: ovr.brute_overlap(self.tris, self.qlo, self.qhi, self.rank, m == TRI) for m in MODES}

    def total(self, m):
        return int(self.want[m][0][-1])


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def big():
    """Test.obj under the reference camera with 20,011 boxes around points in 1.5 x the root box, and their lists
    in both modes."""
    c = Case("Test", "reference")
    qlo, qhi = ovr.sample_boxes(c.tris, 11, n_random=20_011, n_each=0)
    yield c, qlo, qhi, {m: ovr.brute_overlap(c.tris, qlo, qhi, c.rank, m == TRI) for m in MODES}
    c.ctx.close()


def head(want, n):
    """brute_overlap's answer for the first n boxes."""
    return want[0][:n + 1], want[1][:int(want[0][n])]


# ---------------------------------------------------------------- 1. the brute force
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_matches_brute_force(case, m):
    want, total = case.want[m], case.total(m)
    cnt = np.diff(want[0]).astype(np.int64)
    assert 0 < total < len(case.qlo) * case.T and (cnt == 0).any() and (cnt >= 2).any()   # from the reference
    assert case.total(TRI) < case.total(0)                                                # (T) rejects something
    got = case.ctx.overlap(case.boxes, mode=m, capacity=total)                            # mode 0: one call
    assert got[0].shape == (len(case.qlo) + 1,) and got[1].shape == (total,)
    assert_overlap_equal(got, want, "one call")
    assert_overlap_equal(case.ctx.overlap(case.boxes, mode=m | SORT | COUNT, capacity=total), want, "SORT | COUNT")
    c = case.ctx.overlap_counts()
    assert c["boxes"] == len(case.qlo) and c["ids"] == total
    assert c["leaf_steps"] >= 2 * total                                              # two passes, every member's leaf
    assert_overlap_equal(case.ctx.overlap(case.boxes, mode=m), want, "SIZES then FILL")
    flat = case.boxes.view(np.float32).reshape(-1, 8)
    assert_overlap_equal(case.ctx.overlap(flat, mode=m | COUNT), want, "(N, 8)")
    assert case.ctx.overlap_counts()["ids"] == total                                 # (the FILL call's)
    assert_overlap_equal(case.ctx.overlap(case.boxes, mode=m | SORT), want, "BOX_DTYPE, SORT")
    assert_overlap_equal(case.ctx.overlap(case.qlo, case.qhi, mode=m), want, "two (N, 3) arrays")
    np.testing.assert_array_equal(case.ctx.overlap(case.boxes, mode=m, sizes_only=True), want[0])
    junk = case.boxes.copy()                                                         # the reserved words are ignored
    junk["reserved0"], junk["reserved1"] = 0xFFFFFFFF, 0x7FC00000
    assert_overlap_equal(case.ctx.overlap(junk, mode=m, capacity=total), want, "reserved words")


# ---------------------------------------------------------------- 2. capacity
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_capacity_truncates_and_never_writes_behind(case, m):
    want, total = case.want[m], case.total(m)
    dev = Device(case.ctx, case.boxes)
    for capacity in (total, total // 2, 1, 0):
        for mode in (m, m | SORT):
            off, words = dev.run(capacity, mode)
            np.testing.assert_array_equal(off, want[0], err_msg=f"capacity {capacity}")
            np.testing.assert_array_equal(words, want[1][:capacity], err_msg=f"capacity {capacity}")
    off, _ = dev.run(0, m, null_ids=True)                                             # capacity 0: ids may be NULL
    np.testing.assert_array_equal(off, want[0])
    off, _ = dev.run(0, m | SIZES, null_ids=True)
    np.testing.assert_array_equal(off, want[0])
    # the host entry: min(total, capacity) ids
    half = total // 2
    off, ids = case.ctx.overlap(case.boxes, mode=m, capacity=half)
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(ids, want[1][:half])
    assert_overlap_equal(case.ctx.overlap(case.boxes, mode=m, capacity=total + 5), want, "capacity above the total")


# ---------------------------------------------------------------- 3. FILL over foreign offsets
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_fill_over_offsets_of_smaller_boxes_writes_prefixes(case, m):
    slo, shi = shrunk(case.qlo, case.qhi)
    off_s, _ = ovr.brute_overlap(case.tris, slo, shi, case.rank, m == TRI)
    off_l, ids_l = case.want[m]
    cnt_s, cnt_l = np.diff(off_s).astype(np.int64), np.diff(off_l).astype(np.int64)
    assert (cnt_l > cnt_s).any() and (cnt_s > 0).any()
    if m == 0:
        assert (cnt_l >= cnt_s).all()          # (B) is monotone in the query box; (T) within rounding only
    total = int(off_s[-1])
    # segment k holds the first cnt_s[k] ids of the larger list of box k (all of it where that is shorter)
    want_words = np.full(total, PATTERN, np.uint32)
    for k in range(len(case.qlo)):
        take = min(cnt_s[k], cnt_l[k])
        want_words[int(off_s[k]):int(off_s[k]) + take] = ids_l[int(off_l[k]):int(off_l[k]) + take]
    dev = Device(case.ctx, case.boxes)
    for capacity in (total, total // 2):
        for mode in (m | FILL, m | FILL | SORT):
            off, words = dev.run(capacity, mode, offsets=off_s)
            np.testing.assert_array_equal(off, off_s)                                 # FILL reads them only
            np.testing.assert_array_equal(words, want_words[:capacity], err_msg=f"capacity {capacity}")


# ---------------------------------------------------------------- 4. no-walk boxes, tiny scenes
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_invalid_degenerate_and_far_boxes(case, m):
    lo, hi = nr.root_box(case.tris)
    diag = np.float32(np.sqrt(((hi - lo) ** 2).sum()))
    nan = np.float32(np.nan)
    blo, bhi = np.repeat(lo[None], 10, 0), np.repeat(hi[None], 10, 0)
    blo[0, 0], blo[1, 1], bhi[2, 2], bhi[3, 0] = nan, nan, nan, nan
    blo[4, 0], blo[5, 2], bhi[6, 1], bhi[7, 0] = -INF, INF, INF, -INF
    blo[8, 1] = np.nextafter(bhi[8, 1], INF)                        # qlo > qhi on one axis, by one ulp
    blo[9], bhi[9] = hi, lo                                         # ... and on all three
    assert not ovr.valid_boxes(blo, bhi).any()
    off, ids = case.ctx.overlap(blo, bhi, mode=m | COUNT)
    assert off.tolist() == [0] * 11 and len(ids) == 0
    c = case.ctx.overlap_counts()
    assert c == {"boxes": 10, "ids": 0, "internal_steps": 0, "leaf_steps": 0}        # not walked
    off, ids = case.ctx.overlap(blo, bhi, mode=m | SORT, capacity=8)
    assert off.tolist() == [0] * 11 and len(ids) == 0
    # far outside the scene: walked (the root's step), nothing listed
    centre = ((lo + hi) / 2).astype(np.float32)
    far = (centre + np.float32(1e4) * diag * np.array([[1, 0, 0], [0, -1, 0], [.6, .48, -.64]], np.float32)).astype(np.float32)
    off, ids = case.ctx.overlap(far - diag, far + diag, mode=m | COUNT)
    assert off.tolist() == [0] * 4 and len(ids) == 0
    c = case.ctx.overlap_counts()
    assert c["boxes"] == 3 and c["ids"] == 0 and c["internal_steps"] + c["leaf_steps"] >= 3
    # mixed with valid boxes, and the whole root box: every triangle in sort order (boxes mode)
    mlo, mhi = np.concatenate([blo, far - diag, lo[None], case.qlo[:50]]), np.concatenate([bhi, far + diag, hi[None], case.qhi[:50]])
    want = ovr.brute_overlap(case.tris, mlo, mhi, case.rank, m == TRI)
    assert (np.diff(want[0])[:13] == 0).all()
    if m == 0:
        assert int(np.diff(want[0])[13]) == case.T
    assert_overlap_equal(case.ctx.overlap(mlo, mhi, mode=m), want, "mixed")
    assert_overlap_equal(case.ctx.overlap(mlo, mhi, mode=m | SORT, capacity=int(want[0][-1])), want, "mixed, SORT")
    # finite bounds whose extent overflows: (T)'s half-extents are +inf, its radii +inf or NaN, and nothing separates
    huge = np.full((2, 3), np.float32(3e38))
    want = ovr.brute_overlap(case.tris, -huge, huge, case.rank, m == TRI)
    assert np.diff(want[0]).tolist() == [case.T, case.T]
    assert_overlap_equal(case.ctx.overlap(-huge, huge, mode=m), want, "overflowing extent")
    # point boxes on vertices list the vertex's triangles; -0 and +0 bounds alike
    v = case.tris[::max(1, case.T // 64), 0]
    want = ovr.brute_overlap(case.tris, v, v, case.rank, m == TRI)
    assert (np.diff(want[0]) >= 1).all()
    assert_overlap_equal(case.ctx.overlap(v, v.copy(), mode=m), want, "point boxes on vertices")
    zlo, zhi = case.qlo[:64].copy(), case.qhi[:64].copy()
    zlo[:, 0], zhi[:, 1] = 0.0, 0.0
    zlo[:, 1], zhi[:, 0] = np.minimum(zlo[:, 1], 0), np.maximum(zhi[:, 0], 0)
    want = ovr.brute_overlap(case.tris, zlo, zhi, case.rank, m == TRI)
    assert_overlap_equal(case.ctx.overlap(zlo, zhi, mode=m), want, "+0 bounds")
    zlo[:, 0], zhi[:, 1] = -0.0, -0.0
    assert_overlap_equal(case.ctx.overlap(zlo, zhi, mode=m), want, "-0 bounds")


@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = tiny_scene(ntris)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = wr.rank_of(ctx.read_sorted()[1])
        qlo, qhi = ovr.sample_boxes(tris, ntris, n_random=300, n_each=16)
        lo, hi = nr.root_box(tris)
        qlo, qhi = np.concatenate([qlo, lo[None]]), np.concatenate([qhi, hi[None]])
        for m in MODES:
            want = ovr.brute_overlap(tris, qlo, qhi, rank, m == TRI)
            cnt = np.diff(want[0])
            assert (cnt == 0).any() and (m == TRI or cnt[-1] == ntris)
            assert_overlap_equal(ctx.overlap(qlo, qhi, mode=m), want)
            assert_overlap_equal(ctx.overlap(qlo, qhi, mode=m | SORT, capacity=int(want[0][-1])), want, "SORT, one call")


# ---------------------------------------------------------------- 5. sizes: claims, partial waves, scan tiles, refill
@pytest.mark.parametrize("n", [1, 63, 65, 257, 20_011])
def test_sizes(big, n):
    c, qlo, qhi, want = big
    for m in MODES:
        w = head(want[m], n)
        assert_overlap_equal(c.ctx.overlap(qlo[:n], qhi[:n], mode=m), w)
        assert_overlap_equal(c.ctx.overlap(qlo[:n], qhi[:n], mode=m | SORT | COUNT, capacity=len(w[1])), w, "SORT | COUNT")
        counts = c.ctx.overlap_counts()
        assert counts["boxes"] == n and counts["ids"] == len(w[1])
    off, ids = c.ctx.overlap(qlo[:0], qhi[:0])
    assert off.tolist() == [0] and ids.shape == (0,)
    off, ids = c.ctx.overlap(qlo[:0], qhi[:0], capacity=4)
    assert off.tolist() == [0] and ids.shape == (0,)


def test_more_boxes_than_the_grid_has_lanes():
    s = fixture_scene("Rect")
    wvp, wv = rt.camera_reference(W, H)
    n = 600_000   # > 524,288 lanes of the persistent grid: refills; 293 scan tiles
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        qlo, qhi = ovr.sample_boxes(tris, 17, n_random=n, n_each=0)
        rank = wr.rank_of(ctx.read_sorted()[1])
        want = ovr.brute_overlap(tris, qlo, qhi, rank)
        cnt = np.diff(want[0])
        assert (cnt == 0).any() and (cnt >= 3).any()
        boxes = rt.make_boxes(qlo, qhi)
        assert_overlap_equal(ctx.overlap(boxes, capacity=int(want[0][-1])), want)
        assert_overlap_equal(ctx.overlap(boxes, mode=SORT), want, "SORT")
        want = ovr.brute_overlap(tris, qlo, qhi, rank, True)
        assert_overlap_equal(ctx.overlap(boxes, mode=TRI | SORT, capacity=int(want[0][-1])), want, "TRIANGLE | SORT")


# ---------------------------------------------------------------- 6. both tree forms
def test_records_and_node_box_trees_agree():
    s = rt.synthetic(70_000, seed=0x5EED0004)
    T = 70_000
    wvp, wv = rt.camera_reference(W, H)
    with built(s, wvp, wv, flags=rt.FLAG_AUTO_WALK) as auto, built(s, wvp, wv) as plain:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        qlo, qhi = (x[:512] for x in ovr.sample_boxes(tris, 3, n_random=384, n_each=43))
        assert len(qlo) == 512
        q = (qhi - qlo) * np.float32(0.375)          # a quarter of the extents: short lists on 70,000 triangles
        qlo, qhi = (qlo + q).astype(np.float32), (qhi - q).astype(np.float32)
        boxes = rt.make_boxes(qlo, qhi)
        sa, sp = auto.read_sorted()[1], plain.read_sorted()[1]
        np.testing.assert_array_equal(sa, sp)
        pts = nr.sample_points(tris, seed=3, n_random=384, n_each=43)[0][:512]
        o, d = random_rays(plain.read_bvh(), 2000, seed=3)
        rays = rt.make_rays(o, d)
        r2 = np.float32(1e-4)
        for c in (auto, plain):   # counting queries of the other kinds first: their counts must survive
            c.query(rays, rt.QUERY_COUNT)
            c.nearest(pts, mode=rt.NEAREST_COUNT)
            c.within(pts, r2, mode=rt.WITHIN_COUNT)
            c.allhits(rays, mode=rt.ALLHITS_COUNT)
        others = lambda c: (c.query_counts(), c.nearest_counts(), c.within_counts(), c.allhits_counts())
        before = others(plain)
        assert others(auto) == before
        for m in MODES:
            want = ovr.brute_overlap(tris, qlo, qhi, wr.rank_of(sp), m == TRI)
            total = int(want[0][-1])
            assert total > 512
            a, p = (c.overlap(boxes, mode=m | COUNT, capacity=total) for c in (auto, plain))
            np.testing.assert_array_equal(a[0], p[0])
            np.testing.assert_array_equal(a[1], p[1])
            assert_overlap_equal(a, want)
            ca, cp = auto.overlap_counts(), plain.overlap_counts()
            print("box query steps per box (two passes):", {k: v / 512 for k, v in ca.items()})
            assert ca == cp   # the same visits on both forms
            assert ca["boxes"] == 512 and ca["ids"] == total
            assert 0 < ca["leaf_steps"] < 512 * T // 8 and ca["internal_steps"] > 0
            for c in (auto, plain):
                assert_overlap_equal(c.overlap(boxes, mode=m | SORT), want, "SORT")
                assert others(c) == before
        for c in (auto, plain):
            c.query(rays[:100], rt.QUERY_COUNT)
            c.nearest(pts[:50], mode=rt.NEAREST_COUNT)
            c.within(pts[:40], r2, mode=rt.WITHIN_COUNT)
            c.allhits(rays[:30], mode=rt.ALLHITS_COUNT)
            assert c.query_counts()["rays"] == 100 and c.nearest_counts()["points"] == 50
            assert c.within_counts()["points"] == 40 and c.allhits_counts()["rays"] == 30
            assert c.overlap_counts() == ca            # ... and they leave these alone


# ---------------------------------------------------------------- 7. device tensors and streams
def test_device_tensors_on_two_streams(big):
    import torch
    c, qlo, qhi, want_all = big
    want = want_all[0]
    n = len(qlo)
    total = int(want[0][-1])
    m = 4096
    slo, shi = shrunk(qlo[:m], qhi[:m])
    want_b = ovr.brute_overlap(c.tris, slo, shi, c.rank, True)
    b1 = torch.from_numpy(rt.make_boxes(qlo, qhi).view(np.float32).reshape(n, 8)).cuda()
    b2 = rt.make_boxes(torch.from_numpy(slo).cuda(), torch.from_numpy(shi).cuda())
    assert b2.is_cuda and tuple(b2.shape) == (m, 8) and b2.dtype == torch.float32
    o, dd = random_rays(c.ctx.read_bvh(), 4096, seed=5)
    rays = torch.from_numpy(rt.make_rays(o, dd).view(np.float32).reshape(-1, 8)).cuda()
    hits_want = c.ctx.query(rt.make_rays(o, dd))
    pts = ((qlo[:m] + qhi[:m]) * np.float32(0.5)).astype(np.float32)
    near_want = c.ctx.nearest(pts)
    pn = torch.from_numpy(rt.make_points(pts).view(np.float32).reshape(m, 4)).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    o1, r1 = c.ctx.overlap(b1, mode=COUNT, capacity=total + 7, stream=s1)   # back to back, one context, two streams
    hits = c.ctx.query(rays, stream=s2)
    o2, r2 = c.ctx.overlap(b2, mode=SORT | TRI, stream=s1)                  # capacity=None: sized from the total
    near = c.ctx.nearest(pn, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert o1.is_cuda and o1.dtype == torch.int64 and tuple(o1.shape) == (n + 1,)
    assert r1.is_cuda and r1.dtype == torch.int32 and tuple(r1.shape) == (total + 7,)
    np.testing.assert_array_equal(o1.cpu().numpy().view(np.uint64), want[0])
    np.testing.assert_array_equal(r1[:total].cpu().numpy().view(np.uint32), want[1])
    assert tuple(r2.shape) == (int(want_b[0][-1]),)
    np.testing.assert_array_equal(o2.cpu().numpy().view(np.uint64), want_b[0])
    np.testing.assert_array_equal(r2.cpu().numpy().view(np.uint32), want_b[1])
    np.testing.assert_array_equal(hits.cpu().numpy().view(np.uint32), hits_want.view(np.uint32).reshape(-1, 4))
    np.testing.assert_array_equal(near.cpu().numpy().view(np.uint32), near_want.view(np.uint32).reshape(-1, 8))
    assert c.ctx.overlap_counts()["boxes"] == n and c.ctx.overlap_counts()["ids"] == total
    # the current stream (torch's default one) and a side stream made current; capacity given and not
    o3, r3 = c.ctx.overlap(b2, mode=TRI)
    np.testing.assert_array_equal(o3.cpu().numpy(), o2.cpu().numpy())
    np.testing.assert_array_equal(r3.cpu().numpy(), r2.cpu().numpy())
    s1.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        o4, r4 = c.ctx.overlap(b2, mode=TRI, capacity=r2.shape[0])
        o5 = c.ctx.overlap(b2, mode=TRI, sizes_only=True)
    s1.synchronize()
    np.testing.assert_array_equal(o4.cpu().numpy(), o2.cpu().numpy())
    np.testing.assert_array_equal(r4.cpu().numpy(), r2.cpu().numpy())
    np.testing.assert_array_equal(o5.cpu().numpy(), o2.cpu().numpy())
    with pytest.raises(ValueError):
        c.ctx.overlap(b1[:, :7])
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
    qlo, qhi = ovr.sample_boxes(tris, 9, n_random=384, n_each=43)
    with built(s, wvp, wv, flags=flags) as ctx:
        old_order = ctx.read_sorted()[1].copy()
        for m in MODES:
            before = ctx.overlap(qlo, qhi, mode=m)
            ctx.update_vertices(P)
            with pytest.raises(rt.RtbvhError) as e:
                ctx.overlap(qlo, qhi, mode=m)
            assert e.value.status == NOT_READY
            ctx.refit()
            np.testing.assert_array_equal(ctx.read_sorted()[1], old_order)   # a refit keeps the order
            want = ovr.brute_overlap(tris, qlo, qhi, wr.rank_of(old_order), m == TRI)
            refit = ctx.overlap(qlo, qhi, mode=m)
            assert_overlap_equal(refit, want, "after the refit")
            assert not (np.array_equal(before[0], refit[0]) and np.array_equal(before[1], refit[1]))
            ctx.build()   # another tree over the same geometry: the same sets, in the new order
            new_order = ctx.read_sorted()[1].copy()
            rebuilt = ctx.overlap(qlo, qhi, mode=m)
            assert_overlap_equal(rebuilt, ovr.brute_overlap(tris, qlo, qhi, wr.rank_of(new_order), m == TRI),
                                 "after the rebuild")
            np.testing.assert_array_equal(rebuilt[0], refit[0])
            for k in range(len(qlo)):
                a, b = (x[1][int(x[0][k]):int(x[0][k + 1])] for x in (refit, rebuilt))
                np.testing.assert_array_equal(np.sort(a), np.sort(b))
            ctx.update_vertices(s.vertices[:, :3].copy())   # back to the scene's geometry for the next mode
            ctx.build()
            old_order = ctx.read_sorted()[1].copy()


# ---------------------------------------------------------------- 9. errors, the stack limit
def test_errors():
    import torch
    big = np.float32(3e38)
    boxes = rt.make_boxes(np.full((4, 3), -big, np.float32), np.full((4, 3), big, np.float32))
    off = np.zeros(5, np.uint64)
    ids = np.zeros(64, np.uint32)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.overlap(boxes)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.overlap_counts()
        assert e.value.status == NOT_READY
        o, p = ctx.overlap(boxes[:0])               # n == 0 is OK even before a build
        assert o.tolist() == [0] and p.shape == (0,)
        ctx.build()
        h = ctx._h
        db = torch.from_numpy(boxes.view(np.float32).reshape(-1, 8).copy()).cuda()
        doff = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        dids = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for mode in (1, 64, 128, 1 << 8, 1 << 31, SIZES | FILL, SIZES | FILL | TRI, SORT | 1, TRI | 64):
            assert L.rtbvh_overlap_async(h, vp(db), 4, vp(doff), vp(dids), 64, mode, None) == INVALID_ARG, mode
            assert L.rtbvh_overlap_host(h, vp(boxes), 4, vp(off), vp(ids), 64, mode) == INVALID_ARG, mode
        assert L.rtbvh_overlap_async(h, None, 4, vp(doff), vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_overlap_async(h, vp(db), 4, None, vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_overlap_async(h, vp(db), 4, vp(doff), None, 64, 0, None) == INVALID_ARG
        assert L.rtbvh_overlap_async(h, vp(db), 4, vp(doff), None, 64, FILL, None) == INVALID_ARG
        assert L.rtbvh_overlap_async(h, vp(db), 1 << 31, vp(doff), vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_overlap_host(h, vp(boxes), 4, None, vp(ids), 64, 0) == INVALID_ARG
        assert L.rtbvh_overlap_host(h, vp(boxes), 4, vp(off), None, 64, 0) == INVALID_ARG
        assert L.rtbvh_overlap_host(h, vp(boxes), 1 << 31, vp(off), vp(ids), 64, 0) == INVALID_ARG
        assert L.rtbvh_overlap_counts(h, None) == INVALID_ARG
        ctx.synchronize()
        assert (doff.cpu().numpy() == -1).all() and (dids.cpu().numpy() == -1).all()   # nothing was written
        assert not off.any() and not ids.any()
        # NULL ids are fine with capacity 0 and under SIZES; n == 0 writes offsets[0] only where there is one
        assert L.rtbvh_overlap_async(h, vp(db), 4, vp(doff), None, 0, 0, None) == OK
        assert L.rtbvh_overlap_async(h, vp(db), 4, vp(doff), None, 64, SIZES, None) == OK
        assert L.rtbvh_overlap_async(h, None, 0, None, None, 0, 0, None) == OK
        ctx.synchronize()
        assert doff.cpu().numpy().tolist() == [0, 12, 24, 36, 48]   # (the SIZES call: Rect's 12 triangles each)
        doff.fill_(-1)
        torch.cuda.synchronize()
        assert L.rtbvh_overlap_async(h, None, 0, vp(doff), None, 0, 0, None) == OK
        ctx.synchronize()
        assert doff.cpu().numpy().tolist() == [0, -1, -1, -1, -1]
        with pytest.raises(rt.RtbvhError) as e:
            ctx.overlap_counts()                    # still no counting box query
        assert e.value.status == NOT_READY
        d = load_scene_fixture("Rect")              # and the context still answers
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(W, H)[0])
        assert_overlap_equal(ctx.overlap(boxes), ovr.brute_overlap(tris, boxes["lo"], boxes["hi"],
                                                                   wr.rank_of(ctx.read_sorted()[1])))
        ctx.synchronize()


@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_stack_limit_reports_overflow_and_keeps_genuine_ids(m):
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    qlo, qhi = ovr.sample_boxes(tris, 13)
    n = len(qlo)
    with built(s, wvp, wv, stack_limit=2) as ctx:
        want = ovr.brute_overlap(tris, qlo, qhi, wr.rank_of(ctx.read_sorted()[1]), m == TRI)
        cap = int(want[0][-1])
        dev = Device(ctx, rt.make_boxes(qlo, qhi))
        off, words = dev.run(cap, m, expect=OVERFLOW)   # (its guard region: untouched)
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK   # once per new overflow
        # offsets are consistent, and a walk that lost subtrees lists a subsequence of the box's true list
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
        total = int(off[-1])
        assert 0 < total < cap
        assert (words[total:] == PATTERN).all()     # the fill pass wrote what the sizes pass counted, no more
        assert (words[:total] < len(tris)).all()    # ... and no less (an id is below T)
        for k in range(n):
            g = words[int(off[k]):int(off[k + 1])]
            t = want[1][int(want[0][k]):int(want[0][k + 1])]
            idx = {w: i for i, w in enumerate(t.tolist())}
            where = [idx.get(w, -1) for w in g.tolist()]
            assert -1 not in where and where == sorted(where), k
