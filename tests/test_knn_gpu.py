"""k-nearest queries on the GPU (rtbvh_knn_async / rtbvh_knn_host through Context.knn) against the brute force over
all triangles of the numpy restatement (tests/knn_ref.py on tests/nearest_ref.py).  The answer is specified
independently of the tree -- the k smallest (dist2, triangle id) within the bound, in order -- so every comparison
is bit-exact: dist2 is compared as uint32 views."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import knn_ref as kr
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform
from tests.test_query_gpu import random_rays, tiny_scene

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]
KS = [1, 2, 4, 5, 8, 9, 16, 17, 32]   # both sides of every edge of the kernel's list tiers (4, 8, 16, 32)
MODES = [0, rt.KNN_COUNT, rt.KNN_SORT, rt.KNN_SORT | rt.KNN_COUNT]
NOT_READY, INVALID_ARG, OVERFLOW = rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG, rt._lib.ERR_STACK_OVERFLOW
INF = np.float32(np.inf)


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


def assert_knn_equal(got, want, what=""):
    """got: an (n, k) PAIR_DTYPE array; want: knn_ref's (tri, dist2).  Both fields, bit for bit."""
    tri, dist2 = want
    assert got.dtype == rt.PAIR_DTYPE and got.shape == tri.shape, what
    np.testing.assert_array_equal(got["tri"], tri, err_msg=what + " tri")
    np.testing.assert_array_equal(nr.bits(got["dist2"]), nr.bits(dist2), err_msg=what + " dist2")


def cycled_bounds(dj):
    """Per point, cycled: half the j-th distance, exactly it, the float below it, 4 times it."""
    c = np.arange(len(dj)) % 4
    return np.where(c == 0, np.float32(.5) * dj, np.where(c == 1, dj, np.where(c == 2, np.nextafter(dj, np.float32(0)),
                                                                              np.float32(4) * dj))).astype(np.float32)


class Case:
    """A golden scene built on the GPU under one camera, the tests' points and every (point, triangle) dist2 (once)."""

    def __init__(self, scene, cam):
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.T = len(self.tris)
        self.pts, self.first_vertex = nr.sample_points(self.tris)
        self.d, self.finite = kr.dist2_matrix(self.tris, self.pts)

    def want(self, k, bound=np.inf, sel=slice(None)):
        return kr.select_k(self.d[sel], self.finite[sel], k, bound)


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def big():
    """Test.obj under the reference camera with 20,011 points in 1.5 x the root box and their k = 5 answers."""
    c = Case("Test", "reference")
    pts = nr.sample_points(c.tris, seed=11, n_random=20_011, n_each=0)[0]
    yield c, pts, kr.brute_k(c.tris, pts, 5)
    c.ctx.close()


# ---------------------------------------------------------------- 1. the brute force
@pytest.mark.parametrize("k", KS)
def test_matches_brute_force(case, k):
    n = len(case.pts)
    assert n == 704
    want = case.want(k)
    found = int((want[0] != kr.NONE).sum())
    assert found == n * min(k, case.T)
    for mode in MODES:
        got = case.ctx.knn(case.pts, k, mode=mode)
        assert_knn_equal(got, want, f"mode {mode}")
        if mode & rt.KNN_COUNT:
            c = case.ctx.knn_counts()
            assert c["points"] == n and c["found"] == found
            assert c["leaf_steps"] >= found and c["internal_steps"] > 0
    # the (N, 4) and POINT_DTYPE forms are the (N, 3) one
    packed = rt.make_points(case.pts)
    assert_knn_equal(case.ctx.knn(packed, k), want, "POINT_DTYPE")
    assert_knn_equal(case.ctx.knn(packed.view(np.float32).reshape(-1, 4), k), want, "(N, 4)")
    if k == 1:   # the closest-point query's answer
        near = case.ctx.nearest(case.pts)
        got = case.ctx.knn(case.pts, 1)
        np.testing.assert_array_equal(got["tri"][:, 0], near["tri"])
        np.testing.assert_array_equal(nr.bits(got["dist2"][:, 0]), nr.bits(near["dist2"]))
    if k == 32 and case.T == 12:   # Rect: every triangle, then 20 slots of none
        got = case.ctx.knn(case.pts, 32)
        assert (got["tri"][:, :12] != kr.NONE).all() and (np.sort(got["tri"][:, :12], 1) == np.arange(12)).all()
        assert (got["tri"][:, 12:] == kr.NONE).all() and (got["dist2"][:, 12:] == -1).all()


# ---------------------------------------------------------------- 2. max_dist2
@pytest.mark.parametrize("k", KS)
def test_max_dist2_around_the_last_of_each_list(case, k):
    j = min(k, case.T)
    dj = case.want(j)[1][:, j - 1]
    bound = cycled_bounds(dj)
    want = case.want(k, bound)
    nfound = (want[0] != kr.NONE).sum(1)
    c = np.arange(len(dj)) % 4
    pos = dj > 0
    assert (pos & (c == 0)).any() and (pos & (c == 2)).any()
    assert (nfound[pos & ((c == 0) | (c == 2))] < j).all()      # half and the float below: the j-th is out
    assert (nfound[(c == 1) | (c == 3)] >= j).all()              # exactly it and 4 times it: it is in
    assert_knn_equal(case.ctx.knn(case.pts, k, bound), want)
    assert_knn_equal(case.ctx.knn(case.pts, k, bound, mode=rt.KNN_SORT | rt.KNN_COUNT), want, "SORT | COUNT")
    counts = case.ctx.knn_counts()
    assert counts["points"] == len(dj) and counts["found"] == int(nfound.sum())


def test_bounds_that_give_no_walk_and_no_limit(case):
    n, k = 32, 5
    for b in (np.float32(-1), np.float32(np.nan), -INF, np.float32(-1e-30)):
        got = case.ctx.knn(case.pts[:n], k, b)
        assert (got["tri"] == kr.NONE).all() and (got["dist2"] == -1).all(), f"bound {b}"
        assert_knn_equal(got, case.want(k, b, slice(0, n)), f"bound {b}")
    assert_knn_equal(case.ctx.knn(case.pts[:n], k, INF), case.want(k, np.inf, slice(0, n)), "bound +inf")
    # points exactly on vertices with bound 0: the triangles that share the vertex, dist2 == 0
    sel = slice(case.first_vertex, case.first_vertex + 64)
    for zero in (np.float32(0), np.float32(-0.0)):
        for k in (1, 8):
            got = case.ctx.knn(case.pts[sel], k, zero)
            assert (got["tri"][:, 0] != kr.NONE).all()
            f = got["tri"] != kr.NONE
            assert (nr.bits(got["dist2"][f]) == 0).all() and (got["dist2"][~f] == -1).all()
            assert_knn_equal(got, case.want(k, np.float32(0), sel), f"on a vertex, bound {zero}")


# ---------------------------------------------------------------- 3. special points, tiny scenes
def test_special_points(case):
    lo, hi = nr.root_box(case.tris)
    c = ((lo + hi) / 2).astype(np.float32)
    diag = np.float32(np.sqrt(((hi - lo) ** 2).sum()))
    nan = np.float32(np.nan)
    bad = np.array([[nan, c[1], c[2]], [c[0], nan, c[2]], [c[0], c[1], nan], [nan] * 3, [INF, c[1], c[2]],
                    [c[0], -INF, c[2]], [c[0], c[1], INF], [-INF] * 3], np.float32)
    far = (c + np.float32(1e6) * diag * np.array([[1, 0, 0], [0, -1, 0], [.6, .48, -.64]], np.float32)).astype(np.float32)
    pts = np.concatenate([bad, far, c[None]])
    for k in (1, 8, 32):
        want = kr.brute_k(case.tris, pts, k)
        assert (want[0][:len(bad)] == kr.NONE).all() and (want[0][len(bad):, :min(k, case.T)] != kr.NONE).all()
        assert_knn_equal(case.ctx.knn(pts, k), want, f"k {k}")
        assert_knn_equal(case.ctx.knn(pts, k, mode=rt.KNN_SORT | rt.KNN_COUNT), want, f"k {k} SORT | COUNT")
        counts = case.ctx.knn_counts()
        assert counts["points"] == len(pts) and counts["found"] == (len(far) + 1) * min(k, case.T)


@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = tiny_scene(ntris)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        pts = nr.sample_points(tris, seed=ntris, n_random=300, n_each=16, scale=3.0)[0]
        d, finite = kr.dist2_matrix(tris, pts)
        for k in (1, 2, 3):
            want = kr.select_k(d, finite, k)
            assert ((want[0] != kr.NONE).sum(1) == min(k, ntris)).all()
            assert_knn_equal(ctx.knn(pts, k), want, f"k {k}")
            dj = want[1][:, min(k, ntris) - 1]
            bound = np.where(np.arange(len(dj)) % 2 == 0, dj, np.nextafter(dj, np.float32(0))).astype(np.float32)
            assert_knn_equal(ctx.knn(pts, k, bound, mode=rt.KNN_SORT), kr.select_k(d, finite, k, bound), f"k {k} bounded")


# ---------------------------------------------------------------- 4. both tree forms
def test_records_and_node_box_trees_agree():
    s = rt.synthetic(70_000, seed=0x5EED0004)
    T, k = 70_000, 8
    wvp, wv = rt.camera_reference(W, H)
    with built(s, wvp, wv, flags=rt.FLAG_AUTO_WALK) as auto, built(s, wvp, wv) as plain:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        pts = nr.sample_points(tris, seed=3, n_random=384, n_each=43)[0][:512]
        assert len(pts) == 512
        o, d = random_rays(plain.read_bvh(), 2000, seed=3)
        rays = rt.make_rays(o, d)
        for c in (auto, plain):   # counting ray and closest-point queries first: their counts must survive
            c.query(rays, rt.QUERY_COUNT)
            c.nearest(pts[:300], mode=rt.NEAREST_COUNT)
        ray_counts, near_counts = plain.query_counts(), plain.nearest_counts()
        assert auto.query_counts() == ray_counts and ray_counts["rays"] == 2000
        assert auto.nearest_counts() == near_counts and near_counts["points"] == 300
        a, p = auto.knn(pts, k, mode=rt.KNN_COUNT), plain.knn(pts, k, mode=rt.KNN_COUNT)
        assert a.tobytes() == p.tobytes()
        assert_knn_equal(a, kr.brute_k(tris, pts, k))
        ca, cp = auto.knn_counts(), plain.knn_counts()
        print("k-nearest steps per point:", {key: v / 512 for key, v in ca.items()})
        assert ca == cp   # the same visits on both forms
        assert ca["points"] == 512 and ca["found"] == 512 * k
        assert 0 < ca["leaf_steps"] < 512 * T // 8 and ca["internal_steps"] > 0
        for c in (auto, plain):
            assert c.knn(pts, k, mode=rt.KNN_SORT).tobytes() == a.tobytes()
            assert c.query_counts() == ray_counts       # the last counting RAY query's, still
            assert c.nearest_counts() == near_counts    # ... and the last counting closest-point query's
            c.query(rays[:100], rt.QUERY_COUNT)
            c.nearest(pts[:100], mode=rt.NEAREST_COUNT)
            assert c.query_counts()["rays"] == 100 and c.nearest_counts()["points"] == 100
            assert c.knn_counts() == ca                 # ... and those queries leave these alone
        # the queries left the build's state alone: the AUTO context still traces the oracle's rows
        auto.trace(W, H, 1)
        fb = auto.read_framebuffer()
        assert auto.stats()["walk_state"] == 2   # (the certified walks: the build wrote node boxes, no records)
        osc = orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob)
        ofb = orc.trace(osc, orc.build(osc, wvp), wvp, wv, W, H, 1, row_begin=0, row_end=16)[0]
        np.testing.assert_array_equal(fb[0:16].view(np.uint32), ofb.view(np.uint32))


# ---------------------------------------------------------------- 5. sizes: claims, segment ends, partial waves
@pytest.mark.parametrize("n", [1, 63, 65, 257, 20_011])
def test_sizes(big, n):
    c, pts, want = big
    w = (want[0][:n], want[1][:n])
    assert_knn_equal(c.ctx.knn(pts[:n], 5), w)
    assert_knn_equal(c.ctx.knn(pts[:n], 5, mode=rt.KNN_SORT | rt.KNN_COUNT), w, "SORT")
    assert c.ctx.knn_counts()["points"] == n and c.ctx.knn_counts()["found"] == 5 * n
    got = c.ctx.knn(pts[:0], 5)
    assert got.shape == (0, 5) and got.dtype == rt.PAIR_DTYPE


# ---------------------------------------------------------------- 6. device tensors and streams
def test_device_tensors_on_two_streams(big):
    import torch
    c, pts, want = big
    n, k = len(pts), 5
    d5 = want[1][:, k - 1]
    bound = np.where(np.arange(n) % 2 == 0, d5, np.float32(.5) * d5).astype(np.float32)
    want_b = kr.brute_k(c.tris, pts[:4096], k, bound[:4096])
    near_want = c.ctx.nearest(pts[:4096])
    p1 = torch.from_numpy(rt.make_points(pts).view(np.float32).reshape(n, 4)).cuda()
    p2 = rt.make_points(torch.from_numpy(pts[:4096]).cuda(), torch.from_numpy(bound[:4096]).cuda())
    p3 = rt.make_points(torch.from_numpy(pts[:4096]).cuda())
    o, dd = random_rays(c.ctx.read_bvh(), 4096, seed=5)
    rays = torch.from_numpy(rt.make_rays(o, dd).view(np.float32).reshape(-1, 8)).cuda()
    hits_want = c.ctx.query(rt.make_rays(o, dd))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    r1 = c.ctx.knn(p1, k, mode=rt.KNN_COUNT, stream=s1)   # back to back, one context, two streams
    hits = c.ctx.query(rays, stream=s2)
    r2 = c.ctx.knn(p2, k, mode=rt.KNN_SORT, stream=s1)
    near = c.ctx.nearest(p3, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert r1.is_cuda and r1.dtype == torch.float32 and tuple(r1.shape) == (n, k, 2)

    def pairs(t):
        return t.cpu().numpy().view(rt.PAIR_DTYPE).reshape(t.shape[0], t.shape[1])

    assert_knn_equal(pairs(r1), want)
    assert_knn_equal(pairs(r2), want_b)
    np.testing.assert_array_equal(hits.cpu().numpy().view(np.uint32), hits_want.view(np.uint32).reshape(-1, 4))
    np.testing.assert_array_equal(near.cpu().numpy().view(np.uint32), near_want.view(np.uint32).reshape(-1, 8))
    np.testing.assert_array_equal(r1[..., 0].contiguous().view(torch.int32).cpu().numpy(), want[0].view(np.int32))
    assert c.ctx.knn_counts()["points"] == n
    # `out` reuse, on the current stream (torch's default one) and on a side stream; whatever it held is overwritten
    out = torch.full((4096, k, 2), 7.0, dtype=torch.float32, device="cuda")
    assert c.ctx.knn(p2, k, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), r2.cpu().numpy().view(np.uint32))
    out[..., 0] = torch.tensor([-1], dtype=torch.int32, device="cuda").view(torch.float32)   # "none" in every slot
    out[..., 1] = -1.0
    s1.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        c.ctx.knn(p2, k, out=out)
    s1.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), r2.cpu().numpy().view(np.uint32))
    for bad in (torch.empty((4096, k), dtype=torch.float32, device="cuda"),
                torch.empty((4096, k + 1, 2), dtype=torch.float32, device="cuda"),
                torch.empty((4096, k, 2), dtype=torch.float64, device="cuda"),
                torch.empty((4096, k, 4), dtype=torch.float32, device="cuda")[..., ::2]):
        with pytest.raises(ValueError):
            c.ctx.knn(p2, k, out=bad)
    with pytest.raises(ValueError):
        c.ctx.knn(p1[:, :3], k)
    c.ctx.synchronize()


# ---------------------------------------------------------------- 7. animated geometry
@pytest.mark.parametrize("flags", [0, rt.FLAG_AUTO_WALK], ids=["plain", "auto"])
def test_after_update_refit_and_rebuild(flags):
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    P = deform(s.vertices[:, :3], 0.7)
    v = s.vertices.copy()
    v[:, :3] = P
    tris = rw.clip_triangles(v, s.indices, wvp)
    pts = nr.sample_points(tris, seed=9, n_random=384, n_each=43)[0]
    k = 8
    with built(s, wvp, wv, flags=flags) as ctx:
        before = ctx.knn(pts, k)
        ctx.update_vertices(P)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.knn(pts, k)
        assert e.value.status == NOT_READY
        ctx.refit()
        refit = ctx.knn(pts, k)
        assert_knn_equal(refit, kr.brute_k(tris, pts, k), "after the refit")
        assert before.tobytes() != refit.tobytes()
        ctx.build()   # another tree over the same geometry: the answer does not depend on it
        assert ctx.knn(pts, k).tobytes() == refit.tobytes()


# ---------------------------------------------------------------- 8. errors, the stack limit
def test_errors():
    pts = rt.make_points(np.zeros((4, 3), np.float32))
    out = np.zeros((4, 33), rt.PAIR_DTYPE)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.knn(pts, 4)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.knn_counts()
        assert e.value.status == NOT_READY
        assert ctx.knn(pts[:0], 4).shape == (0, 4)   # n == 0 is OK even before a build
        ctx.build()
        for mode in (1, 8, 1 << 8, 1 << 31, rt.KNN_SORT | 16):
            with pytest.raises(rt.RtbvhError) as e:
                ctx.knn(pts, 4, mode=mode)
            assert e.value.status == INVALID_ARG
        for k in (0, 33):
            assert L.rtbvh_knn_host(ctx._h, pts.ctypes.data, 4, k, out.ctypes.data, 0) == INVALID_ARG
            assert L.rtbvh_knn_async(ctx._h, pts.ctypes.data, 4, k, out.ctypes.data, 0, None) == INVALID_ARG
        assert L.rtbvh_knn_async(ctx._h, None, 4, 4, None, 0, None) == INVALID_ARG
        assert L.rtbvh_knn_async(ctx._h, None, 0, 4, None, 0, None) == rt._lib.OK
        assert L.rtbvh_knn_host(ctx._h, pts.ctypes.data, 4, 4, None, 0) == INVALID_ARG
        assert L.rtbvh_knn_host(ctx._h, None, 4, 4, out.ctypes.data, 0) == INVALID_ARG
        assert L.rtbvh_knn_host(ctx._h, pts.ctypes.data, 1 << 31, 4, out.ctypes.data, 0) == INVALID_ARG
        assert L.rtbvh_knn_counts(ctx._h, None) == INVALID_ARG
        with pytest.raises(rt.RtbvhError) as e:
            ctx.knn_counts()                        # still no counting k-nearest query
        assert e.value.status == NOT_READY
        got = ctx.knn(pts, 4)                       # and the context still answers
        d = load_scene_fixture("Rect")
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(W, H)[0])
        assert_knn_equal(got, kr.brute_k(tris, pts["point"], 4))
        ctx.synchronize()


def test_stack_limit_reports_overflow_and_keeps_genuine_lists():
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    pts = nr.sample_points(tris, seed=13)[0]
    k = 8
    want_tri, want_d = kr.brute_k(tris, pts, k)
    with built(s, wvp, wv, stack_limit=2) as ctx:
        out = np.zeros((len(pts), k), rt.PAIR_DTYPE)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.knn(pts, k, out=out)    # the host entry is synchronous: it reports at once
        assert e.value.status == OVERFLOW
        ctx.synchronize()               # once per new overflow
    # a walk that lost subtrees ends with the best list it found
    f = out["tri"] != kr.NONE
    assert f.any()
    assert (f[:, :-1] >= f[:, 1:]).all()                                   # the none-slots are at the end ...
    assert (out["dist2"][~f] == -1).all()                                  # ... and hold -1
    rows = np.broadcast_to(np.arange(len(pts))[:, None], f.shape)[f]
    a, e1, e2, lo, hi = (x[out["tri"][f].astype(np.int64)] for x in nr.leaf_data(tris))
    d = nr.tri_dist2(pts[rows], a, e1, e2, lo, hi)[0]
    np.testing.assert_array_equal(nr.bits(out["dist2"][f]), nr.bits(d))    # every pair a genuine (tri, dist2)
    key = nr.bits(out["dist2"]).astype(np.uint64) << np.uint64(32) | out["tri"].astype(np.uint64)
    both = f[:, :-1] & f[:, 1:]
    assert (key[:, :-1] < key[:, 1:])[both].all()                          # ascending in (dist2, tri): no id twice
    assert (out["dist2"][f] >= want_d[f]).all()                            # slot j never below the true j-th
