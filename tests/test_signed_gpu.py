"""Signed-distance queries on the GPU (rtbvh_signed_async / rtbvh_signed_host through Context.signed, inside and
signed_distance) against the brute force over all triangles of the numpy restatement (tests/signed_ref.py on
tests/nearest_ref.py and tests/ray_walk_ref.py), and against an analytic answer on a sphere.  The record is specified
independently of the tree, so every comparison is bit-exact: records are compared as uint32 views."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests import signed_ref as sr
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform
from tests.test_query_gpu import random_rays, tiny_scene

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]
SORT, COUNT, VOTE3, INSIDE_ONLY = rt.SIGNED_SORT, rt.SIGNED_COUNT, rt.SIGNED_VOTE3, rt.SIGNED_INSIDE_ONLY
NOT_READY, INVALID_ARG, OVERFLOW = rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG, rt._lib.ERR_STACK_OVERFLOW


def camera(name):
    if name == "reference":
        return rt.camera_reference(W, H)
    return np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)


def fixture_scene(name):
    d = load_scene_fixture(name)
    return rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])


def scene_of(tris):
    """A scene of (T, 3, 3) triangles with one material (the positions are the BVH's under an identity camera)."""
    T = len(tris)
    v = np.zeros((3 * T, 8), np.float32)
    v[:, :3] = tris.reshape(-1, 3)
    v[:, 5] = -1
    return rt.Scene(v, np.arange(3 * T, dtype=np.uint32), np.zeros(T, np.uint32), np.zeros(1, rt.MATERIAL_DTYPE))


def built(scene, wvp, wv, **kw):
    ctx = rt.Context(device=0, **kw)
    ctx.set_scene(scene)
    ctx.set_camera(wvp, wv)
    ctx.build()
    return ctx


def assert_records_equal(got, want, what=""):
    """Two SIGNED_DTYPE arrays, every field bit for bit."""
    assert got.dtype == rt.SIGNED_DTYPE and want.dtype == sr.DTYPE and got.shape == want.shape, what
    for f in rt.SIGNED_DTYPE.names:
        np.testing.assert_array_equal(got[f].view(np.uint32), want[f].view(np.uint32), err_msg=f"{what} {f}")


class Case:
    """A scene built on the GPU under one camera, points, and their three crossing counts (computed once)."""

    def __init__(self, scene, wvp, wv, pts=None, **kw):
        self.scene = scene
        self.ctx = built(scene, wvp, wv, **kw)
        self.tris = rw.clip_triangles(scene.vertices, scene.indices, wvp)
        self.T = len(self.tris)
        self.pts = nr.sample_points(self.tris)[0] if pts is None else pts(self.tris)
        self.finite = np.isfinite(self.pts).all(1)
        self.c = np.stack([sr.crossings(self.tris, self.pts, j) for j in range(3)], 1)
        self._near = {}

    def near(self, bound=np.inf, key="free"):
        if key not in self._near:
            self._near[key] = nr.brute(self.tris, self.pts, bound)
        return self._near[key]

    def want(self, mode=0, bound=np.inf, key="free", sel=slice(None)):
        n = len(self.pts)
        near = nr.no_result(n) if mode & INSIDE_ONLY else self.near(bound, key)
        return sr.assemble(near, self.c, self.finite, bool(mode & VOTE3))[sel]


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    scene, cam = request.param
    c = Case(fixture_scene(scene), *camera(cam))
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def big():
    """Test.obj under the reference camera with 20,011 points in 1.5 x the root box."""
    c = Case(fixture_scene("Test"), *camera("reference"),
             pts=lambda tris: nr.sample_points(tris, seed=11, n_random=20_011, n_each=0)[0])
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. the golden scenes
def test_matches_brute_force(case):
    n = len(case.pts)
    assert n == 704 and case.c.sum() > 0
    near = case.ctx.nearest(case.pts)
    for mode in (0, VOTE3, INSIDE_ONLY, INSIDE_ONLY | VOTE3, SORT | COUNT | VOTE3, SORT, COUNT):
        want = case.want(mode)
        got = case.ctx.signed(case.pts, mode=mode)
        assert_records_equal(got, want, f"mode {mode}")
        if not mode & INSIDE_ONLY:   # the closest-point query's answer, on the same context
            for f in ("point", "dist2", "u", "v", "tri"):
                np.testing.assert_array_equal(got[f].view(np.uint32), near[f].view(np.uint32), err_msg=f)
        if mode & COUNT:
            c = case.ctx.signed_counts()
            assert c["points"] == n and c["inside"] == int((want["flags"] & 1).sum())
            assert c["leaf_steps"] > 0 and c["internal_steps"] > 0
    # the (N, 4) and POINT_DTYPE forms are the (N, 3) one
    packed = rt.make_points(case.pts)
    assert_records_equal(case.ctx.signed(packed, mode=VOTE3), case.want(VOTE3), "POINT_DTYPE")
    assert_records_equal(case.ctx.signed(packed.view(np.float32).reshape(-1, 4)), case.want(0), "(N, 4)")
    # the conveniences
    np.testing.assert_array_equal(case.ctx.inside(case.pts), (case.want(0)["flags"] & 1).astype(bool))
    np.testing.assert_array_equal(case.ctx.inside(case.pts, vote3=True), (case.want(VOTE3)["flags"] & 1).astype(bool))
    sd = case.ctx.signed_distance(case.pts)
    assert sd.dtype == np.float32
    w = case.want(0)
    np.testing.assert_array_equal(nr.bits(sd), nr.bits(np.where(w["flags"] & 1, -np.sqrt(w["dist2"]), np.sqrt(w["dist2"]))))


def test_per_point_bounds_make_a_band_and_the_rays_are_still_cast(case):
    d = case.near()["dist2"]
    k = np.arange(len(d)) % 4   # exactly the distance, the float below it, -1, NaN
    bound = np.where(k == 0, d, np.where(k == 1, np.nextafter(d, np.float32(0)), np.where(k == 2, np.float32(-1),
                                                                                         np.float32(np.nan)))).astype(np.float32)
    want = case.want(VOTE3, bound, "band")
    assert (want["tri"][k == 0] != sr.NONE).all() and (want["tri"][(k == 1) & (d > 0)] == sr.NONE).all()
    assert (want["tri"][k >= 2] == sr.NONE).all()
    np.testing.assert_array_equal(want["flags"], case.want(VOTE3)["flags"])   # whatever the bound
    assert_records_equal(case.ctx.signed(case.pts, bound, mode=VOTE3), want)
    assert_records_equal(case.ctx.signed(case.pts, bound, mode=SORT | COUNT), case.want(0, bound, "band"), "SORT | COUNT")
    assert case.ctx.signed_counts()["points"] == len(d)
    sd = case.ctx.signed_distance(case.pts, bound)
    np.testing.assert_array_equal(np.isnan(sd), want["tri"] == sr.NONE)
    for zero in (np.float32(0), np.float32(-0.0)):   # -0 counts as +0: a vertex is found at dist2 == 0
        first = len(case.pts) - 192
        got = case.ctx.signed(case.pts[first:first + 64], zero)
        assert (got["tri"] != sr.NONE).all() and (nr.bits(got["dist2"]) == 0).all()
    # non-finite coordinates: no walk of either kind
    bad = case.pts[:8].copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3] = np.nan, np.inf, -np.inf, np.nan
    got = case.ctx.signed(bad, mode=VOTE3 | SORT)
    assert_records_equal(got, sr.brute(case.tris, bad, vote3=True), "non-finite")
    assert (got["flags"][:4] == 0).all() and (got["tri"][:4] == sr.NONE).all()


# ---------------------------------------------------------------- 2. the analytic answer
def test_inside_an_icosphere():
    tris, pts, keep, inside = sr.analytic_case()
    assert len(tris) == 1280 and len(pts) == 20_000 and keep.mean() >= 0.98
    eye = np.eye(4, dtype=np.float32)
    with built(scene_of(tris), eye, eye) as ctx:
        for vote3 in (False, True):
            got = ctx.inside(pts, vote3=vote3)
            assert got.dtype == bool and got.shape == (len(pts),)
            wrong = int((got != inside)[keep].sum())
            print(f"vote3 {vote3}: {wrong} wrong of {int(keep.sum())}")
            assert wrong == 0
        rec = ctx.signed(pts, mode=VOTE3 | SORT)
        for j in range(3):   # each ray alone
            assert (((rec["flags"] >> (j + 1) & 1) == 1) == inside)[keep].all(), j
        sd = ctx.signed_distance(pts)
        r = np.sqrt((pts.astype(np.float64) ** 2).sum(1))
        assert (np.sign(sd) == np.sign(r - 1))[keep].all()
        np.testing.assert_array_equal(nr.bits(np.abs(sd)), nr.bits(np.sqrt(ctx.nearest(pts)["dist2"])))
        assert (np.abs(np.abs(sd) - np.abs(r - 1))[keep] < 0.01).all()   # (the facets are within 0.004 of the sphere)
        import torch
        dev = rt.make_points(torch.from_numpy(pts).cuda())
        ti, tsd = ctx.inside(dev, vote3=True), ctx.signed_distance(dev)
        torch.cuda.synchronize()
        assert ti.is_cuda and ti.dtype == torch.bool and tsd.is_cuda and tsd.dtype == torch.float32
        np.testing.assert_array_equal(ti.cpu().numpy(), ctx.inside(pts, vote3=True))
        np.testing.assert_array_equal(nr.bits(tsd.cpu().numpy()), nr.bits(sd))


# ---------------------------------------------------------------- 3. tiny trees
@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    """The root of a one-triangle tree is the leaf: its box is tested at the leaf.  Points on both sides of each
    triangle along each D_j (the ray from one side crosses it), and random ones around."""
    s = tiny_scene(ntris)
    wvp, wv = camera(cam)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    cen = (tris[:, 0] + tris[:, 1] + tris[:, 2]) / np.float32(3)
    ext = np.float32(np.abs(tris - cen[:, None]).max())
    along = [cen[k] + np.float32(sgn * f) * ext * sr.D[j] for k in range(ntris) for j in range(3) for sgn in (-1, 1)
             for f in (0.25, 1, 8)]
    pts = np.concatenate([np.array(along, np.float32), nr.sample_points(tris, seed=ntris, n_random=300, n_each=16,
                                                                         scale=3.0)[0]])
    want = sr.brute(tris, pts, vote3=True)
    c = want["flags"] >> 8
    assert ((c & 255) > 0).any() and ((c >> 8 & 255) > 0).any() and ((c >> 16) > 0).any()   # every ray crosses somewhere
    assert (want["flags"] >> 8 == 0).any()                                                  # ... and some point none
    with built(s, wvp, wv) as ctx:
        assert_records_equal(ctx.signed(pts, mode=VOTE3), want)
        assert_records_equal(ctx.signed(pts, mode=SORT | COUNT), sr.brute(tris, pts), "SORT | COUNT")
        assert ctx.signed_counts()["leaf_steps"] >= len(pts)
        assert_records_equal(ctx.signed(pts, mode=INSIDE_ONLY | VOTE3), sr.brute(tris, pts, vote3=True, inside_only=True))


# ---------------------------------------------------------------- 4. both tree forms
def test_records_and_node_box_trees_agree():
    s = rt.synthetic(70_000, seed=0x5EED0004)
    T = 70_000
    wvp, wv = rt.camera_reference(W, H)
    with built(s, wvp, wv, flags=rt.FLAG_AUTO_WALK) as auto, built(s, wvp, wv) as plain:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        pts = nr.sample_points(tris, seed=3, n_random=384, n_each=43)[0][:512]
        assert len(pts) == 512
        o, d = random_rays(plain.read_bvh(), 2000, seed=3)
        rays = rt.make_rays(o, d)
        for c in (auto, plain):   # counting queries of the other kinds first: their counts must survive
            c.query(rays, rt.QUERY_COUNT)
            c.nearest(pts[:300], mode=rt.NEAREST_COUNT)
            c.knn(pts[:200], 4, mode=rt.KNN_COUNT)
        ray_counts, near_counts, knn_counts = plain.query_counts(), plain.nearest_counts(), plain.knn_counts()
        assert auto.query_counts() == ray_counts and ray_counts["rays"] == 2000
        assert auto.nearest_counts() == near_counts and near_counts["points"] == 300
        assert auto.knn_counts() == knn_counts and knn_counts["points"] == 200
        a, p = auto.signed(pts, mode=COUNT | VOTE3), plain.signed(pts, mode=COUNT | VOTE3)
        assert a.tobytes() == p.tobytes()
        want = sr.brute(tris, pts, vote3=True)
        assert_records_equal(a, want)
        ca, cp = auto.signed_counts(), plain.signed_counts()
        print("signed-distance steps per point:", {key: v / 512 for key, v in ca.items()})
        assert ca == cp   # the same visits on both forms
        assert ca["points"] == 512 and ca["inside"] == int((want["flags"] & 1).sum())
        assert 0 < ca["leaf_steps"] < 512 * T // 8 and ca["internal_steps"] > 0
        for c in (auto, plain):
            assert c.signed(pts, mode=SORT | VOTE3).tobytes() == a.tobytes()
            assert c.query_counts() == ray_counts       # the last counting RAY query's, still
            assert c.nearest_counts() == near_counts    # ... the last counting closest-point query's
            assert c.knn_counts() == knn_counts         # ... and the last counting k-nearest query's
            c.query(rays[:100], rt.QUERY_COUNT)
            c.nearest(pts[:100], mode=rt.NEAREST_COUNT)
            c.knn(pts[:100], 4, mode=rt.KNN_COUNT)
            assert c.query_counts()["rays"] == 100 and c.nearest_counts()["points"] == 100
            assert c.knn_counts()["points"] == 100
            assert c.signed_counts() == ca              # ... and those queries leave these alone


# ---------------------------------------------------------------- 5. sizes: claims, segment ends, partial waves
@pytest.mark.parametrize("n", [1, 63, 65, 257, 20_011])
def test_sizes(big, n):
    want = big.want(0, sel=slice(0, n))
    assert_records_equal(big.ctx.signed(big.pts[:n]), want)
    assert_records_equal(big.ctx.signed(big.pts[:n], mode=SORT | COUNT | VOTE3), big.want(VOTE3, sel=slice(0, n)), "SORT")
    counts = big.ctx.signed_counts()
    assert counts["points"] == n and counts["inside"] == int((big.want(VOTE3, sel=slice(0, n))["flags"] & 1).sum())
    got = big.ctx.signed(big.pts[:0])
    assert got.shape == (0,) and got.dtype == rt.SIGNED_DTYPE
    assert big.ctx.inside(big.pts[:0]).shape == (0,) and big.ctx.signed_distance(big.pts[:0]).shape == (0,)


# ---------------------------------------------------------------- 6. device tensors and streams
def test_device_tensors_on_two_streams(big):
    import torch
    c = big
    n = len(c.pts)
    d = c.near()["dist2"]
    bound = np.where(np.arange(n) % 2 == 0, d, np.float32(.5) * d).astype(np.float32)
    want_b = sr.assemble(nr.brute(c.tris, c.pts[:4096], bound[:4096]), c.c[:4096], c.finite[:4096], True)
    near_want = c.ctx.nearest(c.pts[:4096])
    p1 = torch.from_numpy(rt.make_points(c.pts).view(np.float32).reshape(n, 4)).cuda()
    p2 = rt.make_points(torch.from_numpy(c.pts[:4096]).cuda(), torch.from_numpy(bound[:4096]).cuda())
    p3 = rt.make_points(torch.from_numpy(c.pts[:4096]).cuda())
    o, dd = random_rays(c.ctx.read_bvh(), 4096, seed=5)
    rays = torch.from_numpy(rt.make_rays(o, dd).view(np.float32).reshape(-1, 8)).cuda()
    hits_want = c.ctx.query(rt.make_rays(o, dd))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    r1 = c.ctx.signed(p1, mode=COUNT, stream=s1)   # back to back, one context, two streams
    hits = c.ctx.query(rays, stream=s2)
    r2 = c.ctx.signed(p2, mode=SORT | VOTE3, stream=s1)
    near = c.ctx.nearest(p3, stream=s2)
    ins = c.ctx.inside(p3, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert r1.is_cuda and r1.dtype == torch.float32 and tuple(r1.shape) == (n, 8)

    def words(t):
        return t.cpu().numpy().view(np.uint32)

    np.testing.assert_array_equal(words(r1), c.want(0).view(np.uint32).reshape(-1, 8))
    np.testing.assert_array_equal(words(r2), want_b.view(np.uint32).reshape(-1, 8))
    np.testing.assert_array_equal(words(hits), hits_want.view(np.uint32).reshape(-1, 4))
    np.testing.assert_array_equal(words(near), near_want.view(np.uint32).reshape(-1, 8))
    np.testing.assert_array_equal(ins.cpu().numpy(), (c.want(0)["flags"][:4096] & 1).astype(bool))
    np.testing.assert_array_equal(r1[:, 7].contiguous().view(torch.int32).cpu().numpy(), c.want(0)["flags"].view(np.int32))
    assert c.ctx.signed_counts()["points"] == n
    # `out` reuse, on the current stream (torch's default one) and on a side stream; whatever it held is overwritten
    out = torch.full((4096, 8), 7.0, dtype=torch.float32, device="cuda")
    assert c.ctx.signed(p2, mode=VOTE3, out=out) is out
    np.testing.assert_array_equal(words(out), words(r2))
    out.fill_(-3.0)
    s1.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        c.ctx.signed(p2, mode=VOTE3, out=out)
    s1.synchronize()
    np.testing.assert_array_equal(words(out), words(r2))
    for bad in (torch.empty((4096, 7), dtype=torch.float32, device="cuda"),
                torch.empty((4095, 8), dtype=torch.float32, device="cuda"),
                torch.empty((4096, 8), dtype=torch.float64, device="cuda"),
                torch.empty((4096, 16), dtype=torch.float32, device="cuda")[:, ::2],
                torch.empty((4096, 8), dtype=torch.float32)):
        with pytest.raises(ValueError):
            c.ctx.signed(p2, out=bad)
    for call in (c.ctx.signed, c.ctx.inside, c.ctx.signed_distance):
        with pytest.raises(ValueError):
            call(p1[:, :3])
    c.ctx.synchronize()


def test_the_conveniences_own_their_temporary_on_the_side_stream(big):
    """inside and signed_distance keep a record tensor of their own.  It must belong to the stream the work runs on:
    allocated on the current stream and dropped on return, its block would go to the next allocation there while the
    side stream still uses it.  So: call them on a side stream, then allocate and fill tensors of the record's size
    on the current stream before anything synchronises."""
    import torch
    c = big
    n = len(c.pts)
    p1 = torch.from_numpy(rt.make_points(c.pts).view(np.float32).reshape(n, 4)).cuda()
    torch.cuda.synchronize()
    w3, w1 = c.want(VOTE3), c.want(0)
    want_sd = np.where(w1["flags"] & 1, -np.sqrt(w1["dist2"]), np.sqrt(w1["dist2"])).astype(np.float32)
    side = torch.cuda.Stream()
    for stream in (side, side.cuda_stream):   # a torch stream, and its raw handle
        for _ in range(3):
            side.wait_stream(torch.cuda.current_stream())
            ins = c.ctx.inside(p1, vote3=True, stream=stream)
            sd = c.ctx.signed_distance(p1, stream=stream)
            junk = [torch.full((n, 8), float("nan"), device="cuda") for _ in range(6)]   # on the current stream
            assert ins.is_cuda and sd.is_cuda
            side.synchronize()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(ins.cpu().numpy(), (w3["flags"] & 1).astype(bool))
            np.testing.assert_array_equal(nr.bits(sd.cpu().numpy()), nr.bits(want_sd))
            del junk, ins, sd
    c.ctx.synchronize()


# ---------------------------------------------------------------- 7. saturation
@pytest.mark.parametrize("j", [0, 1, 2])
def test_a_stack_of_300_triangles_saturates_the_byte_and_keeps_the_parity(j):
    tris, pts, counts = sr.stack_case(j)
    eye = np.eye(4, dtype=np.float32)
    with built(scene_of(tris), eye, eye) as ctx:
        got = ctx.signed(pts, mode=VOTE3)
        assert_records_equal(got, sr.brute(tris, pts, vote3=True))
        np.testing.assert_array_equal(got["flags"] >> (8 * (j + 1)) & 255, [255, 255, 255, 254, 0])
        np.testing.assert_array_equal(got["flags"] >> (j + 1) & 1, counts & 1)
        if j == 0:
            np.testing.assert_array_equal(ctx.inside(pts), [False, True, True, False, False])


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
    with built(s, wvp, wv, flags=flags) as ctx:
        before = ctx.signed(pts, mode=VOTE3)
        ctx.update_vertices(P)
        for call in (lambda: ctx.signed(pts), lambda: ctx.inside(pts), lambda: ctx.signed_distance(pts)):
            with pytest.raises(rt.RtbvhError) as e:
                call()
            assert e.value.status == NOT_READY
        ctx.refit()
        refit = ctx.signed(pts, mode=VOTE3)
        assert_records_equal(refit, sr.brute(tris, pts, vote3=True), "after the refit")
        assert before.tobytes() != refit.tobytes()
        ctx.build()   # another tree over the same geometry: the answer does not depend on it
        assert ctx.signed(pts, mode=VOTE3).tobytes() == refit.tobytes()


# ---------------------------------------------------------------- 9. errors, the stack limit
def test_errors():
    pts = rt.make_points(np.zeros((4, 3), np.float32))
    out = np.zeros(4, rt.SIGNED_DTYPE)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.signed(pts)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.signed_counts()
        assert e.value.status == NOT_READY
        assert ctx.signed(pts[:0]).shape == (0,)   # n == 0 is OK even before a build
        ctx.build()
        for mode in (1, 1 << 5, 1 << 8, 1 << 31, SORT | 1, VOTE3 | 1 << 5):
            with pytest.raises(rt.RtbvhError) as e:
                ctx.signed(pts, mode=mode)
            assert e.value.status == INVALID_ARG
        assert L.rtbvh_signed_async(ctx._h, None, 4, None, 0, None) == INVALID_ARG
        assert L.rtbvh_signed_async(ctx._h, None, 0, None, 0, None) == rt._lib.OK
        assert L.rtbvh_signed_host(ctx._h, pts.ctypes.data, 4, None, 0) == INVALID_ARG
        assert L.rtbvh_signed_host(ctx._h, None, 4, out.ctypes.data, 0) == INVALID_ARG
        assert L.rtbvh_signed_host(ctx._h, pts.ctypes.data, 1 << 31, out.ctypes.data, 0) == INVALID_ARG
        assert L.rtbvh_signed_async(ctx._h, pts.ctypes.data, 1 << 31, out.ctypes.data, 0, None) == INVALID_ARG
        assert L.rtbvh_signed_counts(ctx._h, None) == INVALID_ARG
        assert L.rtbvh_signed_async(None, pts.ctypes.data, 4, out.ctypes.data, 0, None) == INVALID_ARG
        ctx.signed(pts)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.signed_counts()                     # still no counting signed-distance query
        assert e.value.status == NOT_READY
        got = ctx.signed(pts, mode=COUNT | VOTE3)   # and the context still answers
        d = load_scene_fixture("Rect")
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(W, H)[0])
        assert_records_equal(got, sr.brute(tris, pts["point"], vote3=True))
        assert ctx.signed_counts()["points"] == 4
        ctx.synchronize()


def test_stack_limit_reports_overflow_once_and_keeps_genuine_distances():
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    pts = nr.sample_points(tris, seed=13)[0]
    want = sr.brute(tris, pts, vote3=True)
    with built(s, wvp, wv, stack_limit=2) as ctx:
        out = np.zeros(len(pts), rt.SIGNED_DTYPE)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.signed(pts, mode=VOTE3, out=out)    # the host entry is synchronous: it reports at once
        assert e.value.status == OVERFLOW
        ctx.synchronize()               # once per new overflow
    f = out["tri"] != sr.NONE
    assert f.any() and (out["dist2"][~f] == -1).all()
    a, e1, e2, lo, hi = (x[out["tri"][f].astype(np.int64)] for x in nr.leaf_data(tris))
    d, u, v, q = nr.tri_dist2(pts[f], a, e1, e2, lo, hi)
    np.testing.assert_array_equal(nr.bits(out["dist2"][f]), nr.bits(d))    # a genuine triangle's distance ...
    np.testing.assert_array_equal(nr.bits(out["point"][f]), nr.bits(q))    # ... and closest point
    assert (out["dist2"][f] >= want["dist2"][f]).all()                     # never below the true one
    lost = (out["flags"] >> 8 & 255).astype(np.int64) - (want["flags"] >> 8 & 255)
    assert (lost <= 0).all()                                               # a walk may lose crossings, never add one
