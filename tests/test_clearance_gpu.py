"""Clearance queries on the GPU (rtbvh_clearance_async / _host through Context.clearance and the raw entries)
against the brute force over all (query, triangle) pairs (tests/clearance_ref.py).  The answer is specified
independently of the tree and of the walk, so every comparison is of bytes: all 32 of every record."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import clearance_ref as clr
from tests import collide_ref as cr
from tests import cross_ref as xr
from tests import hostile_scenes as hs
from tests import nearest_ref as nr
from tests import overlap_ref as ovr
from tests import ray_walk_ref as rw
from tests import within_ref as wr
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Rect", "Test", "Image_Test"]
CAMERAS = ["reference", "identity"]
OK, NOT_READY, INVALID_ARG, OVERFLOW = (rt._lib.OK, rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG,
                                        rt._lib.ERR_STACK_OVERFLOW)
SORT, COUNT = rt.CLEARANCE_SORT, rt.CLEARANCE_COUNT
NONE = 0xFFFFFFFF
NRANDOM = 512
INF = np.float32(np.inf)
IDENTITY_TIES = {"Rect": 21, "Test": 229, "Image_Test": 78}   # random queries with several triangles at the minimum
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


def to_device(q):
    import torch
    return torch.from_numpy(rt.make_tris(q).view(np.float32).reshape(-1, 12)).cuda()


def records(got):
    """A result of either entry as a CLEARANCE_DTYPE array."""
    if hasattr(got, "is_cuda"):
        import torch
        assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 2 and got.shape[1] == 8
        got = got.cpu().numpy().view(rt.CLEARANCE_DTYPE).reshape(-1)
    assert got.dtype == rt.CLEARANCE_DTYPE
    return got


def assert_records_equal(got, want, what=""):
    got = records(got)
    want = clr.records(want) if isinstance(want, dict) else want
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, first {bad[0]}: got {got[bad[0]]}, "
                             f"want {want[bad[0]]}")


def subset(b, sl):
    return {k: v[sl] for k, v in b.items()}


def vp(a):
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


class Case:
    """A golden scene built on the GPU under one camera, the three query sets in one array -- cross_ref.random_queries,
    the scene's own triangles, cross_ref.special_queries -- the dist2 of every pair and the brute-force answers under
    the four bounds (once)."""

    def __init__(self, scene, cam, **kw):
        self.name, self.cam = scene, cam
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv, **kw)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.T = len(self.tris)
        special, self.names = xr.special_queries(self.tris)
        self.q = np.concatenate([xr.random_queries(self.tris, NRANDOM), self.tris, special])
        self.dist = clr.matrix(self.tris, self.q)
        free = clr.brute(self.tris, self.q, INF, dist=self.dist)
        self.median = np.float32(np.median(free["dist2"][:NRANDOM]))
        self.bounds = {"inf": INF, "zero": np.float32(0), "median": self.median, "nan": np.float32(np.nan)}
        self.want = {k: free if k == "inf" else clr.brute(self.tris, self.q, b, dist=self.dist)
                     for k, b in self.bounds.items()}


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. the brute force
def test_the_reference_has_something_to_find(case):
    """From the reference alone, before anything is compared: results and no results under the narrow bounds, ties
    for the id tie-break, crossing and free queries."""
    free, zero, mid = case.want["inf"], case.want["zero"], case.want["median"]
    rnd = slice(0, NRANDOM)
    assert free["found"][rnd].all() and not case.want["nan"]["found"].any()
    assert 32 <= int(zero["found"][rnd].sum()) <= NRANDOM - 32
    assert 0 < int(mid["found"][rnd].sum()) < NRANDOM
    ties = int((free["ties"][rnd] > 1).sum())
    assert ties > 0
    if case.cam == "identity":
        assert ties == IDENTITY_TIES[case.name]
    sp = dict(zip(case.names, free["found"][NRANDOM + case.T:].tolist()))
    assert sp == {n: n not in ("NaN", "infinite") for n in case.names}


@pytest.mark.parametrize("bound", ["inf", "zero", "median", "nan"])
def test_matches_brute_force(case, bound):
    import torch
    ctx, q, want, b = case.ctx, case.q, case.want[bound], case.bounds[bound]
    t, d = rt.make_tris(q), to_device(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = ctx.clearance(t, b)
    assert got.dtype == rt.CLEARANCE_DTYPE and got.shape == (len(q),)
    assert_records_equal(got, want, "host")
    assert_records_equal(ctx.clearance(q, b, SORT), want, "host, vertices in, SORT")
    dev = ctx.clearance(d, b, stream=side)
    dev_sorted = ctx.clearance(d, b, SORT, stream=side)
    side.synchronize()
    assert tuple(dev.shape) == (len(q), 8)
    assert_records_equal(dev, want, "device, side stream")
    assert_records_equal(dev_sorted, want, "device, side stream, SORT")
    tri = dev[:, 7].view(torch.int32).cpu().numpy()
    np.testing.assert_array_equal(tri.view(np.uint32), want["tri"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 512])
def test_query_counts_around_a_wave(case, n):
    import torch
    ctx = case.ctx
    q = case.q[:n]
    t, d = rt.make_tris(q), to_device(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for name, b in case.bounds.items():
        want = subset(case.want[name], slice(0, n))
        assert_records_equal(ctx.clearance(t, b), want, f"host, {name}")
        assert_records_equal(ctx.clearance(t, b, SORT), want, f"host, SORT, {name}")
        got = ctx.clearance(d, b, stream=side), ctx.clearance(d, b, SORT, stream=side)
        side.synchronize()
        assert_records_equal(got[0], want, f"device, {name}")
        assert_records_equal(got[1], want, f"device, SORT, {name}")


# ---------------------------------------------------------------- 2. counts
def test_counts(case):
    ctx, q = case.ctx, case.q
    t = rt.make_tris(q)
    lo, hi = q[:NRANDOM].min(1), q[:NRANDOM].max(1)
    ctx.overlap(lo, hi, rt.OVERLAP_COUNT)                # a counting query of another kind: its counts must survive
    other = ctx.overlap_counts()
    seen = {}
    for name in ("inf", "median", "zero", "nan"):
        want = case.want[name]
        for mode in (COUNT, COUNT | SORT):
            assert_records_equal(ctx.clearance(t, case.bounds[name], mode), want, name)
            c = ctx.clearance_counts()
            assert c["queries"] == len(q) and c["found"] == int(want["found"].sum())
            if name == "nan":
                assert c["internal_steps"] == 0 and c["leaf_steps"] == 0      # no walk
            else:
                assert c["leaf_steps"] > 0 and (c["internal_steps"] > 0 or case.T == 1)
            seen.setdefault(name, c)
            assert (c["queries"], c["found"]) == (seen[name]["queries"], seen[name]["found"])
    assert seen["zero"]["leaf_steps"] <= seen["median"]["leaf_steps"] <= seen["inf"]["leaf_steps"]
    last = ctx.clearance_counts()
    ctx.clearance(t[:7], INF)                            # a call without COUNT leaves the words alone
    assert ctx.clearance_counts() == last
    assert ctx.overlap_counts() == other


# ---------------------------------------------------------------- 3. the ties to cross and nearest
def test_where_cross_lists_anything_the_distance_is_zero(case):
    ctx, q = case.ctx, case.q
    t = rt.make_tris(q)
    off, ids = ctx.cross(t)
    off = off.astype(np.int64)
    free, zero = ctx.clearance(t), ctx.clearance(t, 0.0)
    listed = np.diff(off) > 0
    assert listed.any() and not listed.all()
    assert (free["dist2"][listed] == 0).all()
    head = np.array([ids[off[k]:off[k + 1]].min() for k in np.nonzero(listed)[0]], np.uint32)
    assert (free["tri"][listed] <= head).all()
    assert not listed[zero["tri"] == NONE].any()         # nothing at distance 0: nothing crossed


def test_a_point_triangle_is_no_farther_than_nearest(case):
    ctx = case.ctx
    pts = nr.sample_points(case.tris, n_random=256, n_each=32)[0]
    q = np.repeat(pts[:, None, :], 3, 1)
    got = ctx.clearance(rt.make_tris(q))
    near = ctx.nearest(rt.make_points(pts))
    assert (got["tri"] != NONE).all() and (near["tri"] != NONE).all()
    assert (got["dist2"] <= near["dist2"]).all()
    assert_records_equal(got, clr.brute(case.tris, q), "point triangles")


# ---------------------------------------------------------------- 4. both tree forms
def test_records_and_node_box_trees_agree(case):
    """A certified-only context's multi-kernel build writes the topology and node boxes, a plain one the records:
    the same bytes and the same counted steps."""
    q = case.q
    t = rt.make_tris(q)
    with built(case.scene, case.wvp, case.wv, flags=rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD) as nbox:
        np.testing.assert_array_equal(nbox.read_sorted()[1], case.ctx.read_sorted()[1])
        for name in ("inf", "median"):
            for mode in (COUNT, COUNT | SORT):
                a, p = nbox.clearance(t, case.bounds[name], mode), case.ctx.clearance(t, case.bounds[name], mode)
                assert a.tobytes() == p.tobytes()
                assert_records_equal(a, case.want[name], f"node boxes, {name}")
                assert nbox.clearance_counts() == case.ctx.clearance_counts()   # the same visits on both forms
        assert_records_equal(nbox.clearance(to_device(q), case.median), case.want["median"], "node boxes, device")


# ---------------------------------------------------------------- 5. a moving mesh
@pytest.mark.parametrize("flags", [0, rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD], ids=["records", "node boxes"])
def test_after_update_and_refit(flags):
    s = fixture_scene("Image_Test")
    wvp, wv = rt.camera_reference(W, H)
    P = deform(s.vertices[:, :3], 0.7)
    v = s.vertices.copy()
    v[:, :3] = P
    still_tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    moved_tris = rw.clip_triangles(v, s.indices, wvp)
    q = xr.random_queries(still_tris, 256)
    t, d = rt.make_tris(q), to_device(q)
    still, moved = clr.brute(still_tris, q), clr.brute(moved_tris, q)
    bound = np.float32(np.median(moved["dist2"]))
    moved_near = clr.brute(moved_tris, q, bound)
    assert clr.records(still).tobytes() != clr.records(moved).tobytes()
    with built(s, wvp, wv, flags=flags) as ctx:
        assert_records_equal(ctx.clearance(t), still, "before")
        ctx.update_vertices(P)
        for call in (lambda: ctx.clearance(t), lambda: ctx.clearance(d)):
            with pytest.raises(rt.RtbvhError) as e:
                call()
            assert e.value.status == NOT_READY
        ctx.refit()
        assert_records_equal(ctx.clearance(t), moved, "after the refit")
        assert_records_equal(ctx.clearance(d, bound, SORT), moved_near, "after the refit, device, a bound")
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK


# ---------------------------------------------------------------- 6. a deep tree, the stack limit
def fan_case(stack_limit=0):
    s = cr.thick_fan()
    wvp, wv = camera("identity")
    ctx = built(s, wvp, wv, stack_limit=stack_limit)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    return ctx, tris, xr.fan_queries()


def raw_device(ctx, q, bound, mode=0):
    """The raw device entry on the context stream and the status of the synchronising call behind it."""
    import torch
    d = to_device(q)
    out = torch.full((len(q), 8), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert rt.lib().rtbvh_clearance_async(ctx._h, vp(d), len(q), ctypes.c_float(bound), vp(out), mode, None) == OK
    return rt.lib().rtbvh_synchronize(ctx._h), records(out)


def test_fan_walks_past_the_lds_part_of_the_stack():
    """The walks of these queries store entries past 16, the LDS part: with a limit of 18 entries they still lose
    subtrees, and without one they give the brute force."""
    ctx, tris, q = fan_case()
    want = clr.brute(tris, q)
    assert want["found"].all()
    with ctx:
        assert_records_equal(ctx.clearance(rt.make_tris(q)), want, "host")
        assert_records_equal(ctx.clearance(to_device(q), mode=SORT), want, "device")
        st, got = raw_device(ctx, q, INF)
        assert st == OK
        assert_records_equal(got, want, "raw device entry")
    ctx, _, _ = fan_case(stack_limit=18)
    with ctx:
        st, _ = raw_device(ctx, q, INF)
        assert st == OVERFLOW                             # a push at entry 17 was refused: the walk was that deep


def test_stack_limit_reports_overflow_and_keeps_genuine_pairs():
    ctx, tris, q = fan_case(stack_limit=8)
    with ctx:
        st, got = raw_device(ctx, q, INF)
        assert st == OVERFLOW
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK   # once per new overflow
        found = got["tri"] != NONE
        assert found.any()
        assert (got["dist2"][~found] == -1).all()
        tri = got["tri"][found].astype(np.int64)
        assert (tri < len(tris)).all()
        d, cq, cx = clr.pair_dist2(q[found], tris[tri])   # each a genuine pair: that triangle's own distance
        np.testing.assert_array_equal(nr.bits(got["dist2"][found]), nr.bits(d))
        np.testing.assert_array_equal(nr.bits(got["point_q"][found]), nr.bits(cq))
        np.testing.assert_array_equal(nr.bits(got["point_x"][found]), nr.bits(cx))
        want = clr.brute(tris, q)
        assert (got["dist2"][found] >= want["dist2"][found]).all()            # never better than the best


# ---------------------------------------------------------------- 7. hostile geometry
@pytest.mark.parametrize("cam", hs.CAMERAS)
@pytest.mark.parametrize("variant", list(hs.VARIANTS))
def test_hostile_scenes(variant, cam):
    h = hs.hostile(variant, 12)
    wvp, wv = hs.camera(cam)
    tris = h.tris(wvp)
    inp = hs.Inputs(tris, h.labels)
    q = np.concatenate([inp.queries, tris[::3]])
    dist = clr.matrix(tris, q)
    free = clr.brute(tris, q, INF, dist=dist)
    valid = clr.valid_queries(q)
    assert valid.any() and free["found"][valid].any()
    finite = free["dist2"][free["found"] & np.isfinite(free["dist2"])]
    bound = np.float32(np.median(finite))
    near = clr.brute(tris, q, bound, dist=dist)
    for flags in (0, rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD):
        with built(h.scene, wvp, wv, flags=flags) as ctx:
            assert_records_equal(ctx.clearance(rt.make_tris(q)), free, f"{variant}, inf")
            assert_records_equal(ctx.clearance(to_device(q), bound, SORT), near, f"{variant}, a bound")
            assert_records_equal(ctx.clearance(rt.make_tris(q), 0.0), clr.brute(tris, q, 0.0, dist=dist),
                                 f"{variant}, zero")


# ---------------------------------------------------------------- 8. one triangle
def ctx_vertices(v):
    """Bare positions as the (V, 8) vertex records clip_triangles reads."""
    out = np.zeros((len(v), 8), np.float32)
    out[:, :3] = v
    return out


def test_a_scene_of_one_triangle():
    a = np.array([[-3, -2, 0], [4, -1, 1], [0, 5, 2]], np.float32)
    b = np.array([[0, 0, -3], [1, 1, 4], [0.5, 2, -2]], np.float32)           # pierces a
    q = np.stack([b, b + np.float32(40), b + np.float32([0, 0, 8]), a])
    for cam in CAMERAS:
        wvp, wv = camera(cam)
        with built(cr.scene_of(a, np.arange(3)), wvp, wv) as ctx:
            tris = rw.clip_triangles(ctx_vertices(a), np.arange(3), wvp)
            qq = q if cam == "identity" else np.concatenate([tris, xr.random_queries(tris, 16)])
            want = clr.brute(tris, qq)
            if cam == "identity":
                assert want["dist2"][0] == 0 and want["dist2"][1] > want["dist2"][2] > 0
            assert_records_equal(ctx.clearance(rt.make_tris(qq)), want, cam)
            assert_records_equal(ctx.clearance(to_device(qq), mode=SORT | COUNT), want, cam)
            c = ctx.clearance_counts()
            assert c["queries"] == len(qq) and c["internal_steps"] == 0 and c["leaf_steps"] == len(qq)
            bound = np.float32(np.median(want["dist2"]))
            assert_records_equal(ctx.clearance(rt.make_tris(qq), bound), clr.brute(tris, qq, bound), cam)


# ---------------------------------------------------------------- 9. plumbing
def test_a_side_stream_behind_an_overlap_call():
    """An overlap on one stream, then a clearance on another: they share the query scratch, and the library orders
    them."""
    import torch
    c = Case("Test", "reference")
    with c.ctx:
        q = c.q[:NRANDOM]
        want = subset(c.want["median"], slice(0, NRANDOM))
        rank = wr.rank_of(c.ctx.read_sorted()[1])
        lo, hi = q.min(1), q.max(1)
        boxes = torch.from_numpy(rt.make_boxes(lo, hi).view(np.float32).reshape(-1, 8)).cuda()
        box_want = ovr.brute_overlap(c.tris, lo, hi, rank)
        d = to_device(q)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        b = c.ctx.overlap(boxes, capacity=int(box_want[0][-1]), stream=s2)
        r1 = c.ctx.clearance(d, c.median, COUNT, stream=s1)
        b2 = c.ctx.overlap(boxes, capacity=int(box_want[0][-1]), stream=s2)
        r2 = c.ctx.clearance(d, c.median, SORT, stream=s1)
        s1.synchronize()
        s2.synchronize()
        assert r1.is_cuda and r1.dtype == torch.float32 and tuple(r1.shape) == (len(q), 8)
        assert_records_equal(r1, want, "a side stream")
        assert_records_equal(r2, want, "a side stream, SORT")
        for got in (b, b2):
            np.testing.assert_array_equal(got[0].cpu().numpy().view(np.uint64), box_want[0])
            np.testing.assert_array_equal(got[1].cpu().numpy().view(np.uint32), box_want[1])
        with torch.cuda.stream(s1):                                # a side stream made current
            r3 = c.ctx.clearance(d, c.median)
        s1.synchronize()
        assert_records_equal(r3, want, "the current stream")
        assert c.ctx.clearance_counts()["queries"] == len(q)
        c.ctx.synchronize()


def test_errors_and_empty_inputs():
    import torch
    L = rt.lib()
    d = load_scene_fixture("Rect")
    wvp, wv = rt.camera_reference(W, H)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    q = xr.random_queries(tris, 12)
    t = rt.make_tris(q)
    out = np.zeros(12, rt.CLEARANCE_DTYPE)
    one = ctypes.c_float(1.0)
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(wvp, wv)
        h = ctx._h
        dt = to_device(q)
        dout = torch.full((12, 8), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        # n == 0 before a build: OK, nothing touched
        assert L.rtbvh_clearance_async(h, None, 0, one, None, 0, None) == OK
        assert L.rtbvh_clearance_async(h, vp(dt), 0, one, vp(dout), 0, None) == OK
        assert L.rtbvh_clearance_host(h, None, 0, one, None, 0) == OK
        assert L.rtbvh_clearance_host(h, vp(t), 0, one, vp(out), 0) == OK
        assert ctx.clearance(t[:0]).shape == (0,)
        for call in (lambda: ctx.clearance(t), lambda: ctx.clearance(dt), ctx.clearance_counts):
            with pytest.raises(rt.RtbvhError) as e:
                call()
            assert e.value.status == NOT_READY
        assert L.rtbvh_clearance_async(h, vp(dt), 12, one, vp(dout), 0, None) == NOT_READY
        assert L.rtbvh_clearance_host(h, vp(t), 12, one, vp(out), 0) == NOT_READY
        ctx.build()
        for mode in (1, 8, 16, 32, 64, 1 << 8, 1 << 31, COUNT | 1, SORT | 16):
            assert L.rtbvh_clearance_async(h, vp(dt), 12, one, vp(dout), mode, None) == INVALID_ARG, mode
            assert L.rtbvh_clearance_host(h, vp(t), 12, one, vp(out), mode) == INVALID_ARG, mode
        big = 1 << 31
        assert L.rtbvh_clearance_async(h, vp(dt), big, one, vp(dout), 0, None) == INVALID_ARG
        assert L.rtbvh_clearance_host(h, vp(t), big, one, vp(out), 0) == INVALID_ARG
        assert L.rtbvh_clearance_async(h, None, 12, one, vp(dout), 0, None) == INVALID_ARG
        assert L.rtbvh_clearance_async(h, vp(dt), 12, one, None, 0, None) == INVALID_ARG
        assert L.rtbvh_clearance_host(h, None, 12, one, vp(out), 0) == INVALID_ARG
        assert L.rtbvh_clearance_host(h, vp(t), 12, one, None, 0) == INVALID_ARG
        assert L.rtbvh_clearance_counts(h, None) == INVALID_ARG
        ctx.synchronize()
        assert (dout.cpu().numpy() == -1).all() and not out.view(np.uint32).any()   # nothing was written
        with pytest.raises(rt.RtbvhError) as e:
            ctx.clearance_counts()                  # still no counting clearance query
        assert e.value.status == NOT_READY
        want = clr.brute(tris, q)
        assert_records_equal(ctx.clearance(t), want)      # and the context still answers
        for bad in (np.nan, -1.0, -np.inf):               # no result, no walk
            got = ctx.clearance(t, bad, COUNT)
            assert (got["tri"] == NONE).all() and (got["dist2"] == -1).all() and not got["point_q"].any()
            c = ctx.clearance_counts()
            assert (c["queries"], c["found"], c["internal_steps"], c["leaf_steps"]) == (12, 0, 0, 0)
        assert_records_equal(ctx.clearance(t, -0.0), clr.brute(tris, q, 0.0), "-0 counts as +0")
        ctx.update_vertices(d["vertices"][:, :3].copy())
        assert L.rtbvh_clearance_async(h, vp(dt), 12, one, vp(dout), 0, None) == NOT_READY
        assert L.rtbvh_clearance_host(h, vp(t), 12, one, vp(out), 0) == NOT_READY
        ctx.refit()
        assert_records_equal(ctx.clearance(t, mode=SORT), want)
        ctx.synchronize()
