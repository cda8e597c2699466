"""Closest-point queries on the GPU (rtbvh_nearest_async / rtbvh_nearest_host through Context.nearest) against the
brute force over all triangles of the numpy restatement (tests/nearest_ref.py).  The answer is specified
independently of the tree, so every comparison is bit-exact: point, dist2, u and v are compared as uint32 views."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform
from tests.test_query_gpu import random_rays, tiny_scene

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]
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


def assert_nearest_equal(got, want, what=""):
    """got: a NEAREST_DTYPE array; want: nearest_ref.brute's dict.  All five fields, bit for bit."""
    np.testing.assert_array_equal(got["tri"], want["tri"], err_msg=what + " tri")
    np.testing.assert_array_equal(got["dist2"] != -1, want["found"], err_msg=what + " found mask")
    for f in ("dist2", "u", "v", "point"):
        np.testing.assert_array_equal(nr.bits(got[f]), nr.bits(want[f]), err_msg=what + " " + f)
    assert (got["reserved"] == 0).all()


def take(want, sel):
    return {k: v[sel] for k, v in want.items()}


class Case:
    """A golden scene built on the GPU under one camera, the tests' points and their brute-force answers (once)."""

    def __init__(self, scene, cam):
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.pts, self.first_vertex = nr.sample_points(self.tris)
        self.want = nr.brute(self.tris, self.pts)


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def big():
    """Test.obj under the reference camera with 20,011 points in 1.5 x the root box and their answers."""
    c = Case("Test", "reference")
    pts = nr.sample_points(c.tris, seed=11, n_random=20_011, n_each=0)[0]
    yield c, pts, nr.brute(c.tris, pts)
    c.ctx.close()


# ---------------------------------------------------------------- 1. the brute force
def test_matches_brute_force(case):
    assert case.want["found"].all()
    assert (case.want["ties"][case.first_vertex:] > 1).sum() >= 32   # minima that several triangles share
    got = case.ctx.nearest(case.pts)
    assert got.dtype == rt.NEAREST_DTYPE and got.shape == (len(case.pts),)
    assert_nearest_equal(got, case.want)
    # counting and sorting do not change the answer; the (N, 4) and POINT_DTYPE forms are the (N, 3) one
    assert_nearest_equal(case.ctx.nearest(case.pts, mode=rt.NEAREST_COUNT), case.want, "COUNT")
    packed = rt.make_points(case.pts)
    assert_nearest_equal(case.ctx.nearest(packed, mode=rt.NEAREST_SORT | rt.NEAREST_COUNT), case.want, "SORT | COUNT")
    assert_nearest_equal(case.ctx.nearest(packed.view(np.float32).reshape(-1, 4)), case.want, "(N, 4)")
    c = case.ctx.nearest_counts()
    assert c["points"] == len(case.pts) and c["found"] == len(case.pts)


# ---------------------------------------------------------------- 2. max_dist2
def test_max_dist2_around_each_answer(case):
    d = case.want["dist2"]
    k = np.arange(len(d)) % 4
    bound = np.where(k == 0, np.float32(.5) * d, np.where(k == 1, d, np.where(k == 2, np.nextafter(d, np.float32(0)),
                                                                             np.float32(4) * d))).astype(np.float32)
    want = nr.brute(case.tris, case.pts, bound)
    pos = d > 0   # (a point on the surface: every bound >= 0 finds it)
    assert (pos & (k == 0)).any() and (pos & (k == 2)).any()
    assert not want["found"][pos & ((k == 0) | (k == 2))].any()
    for f in ("tri", "dist2", "u", "v", "point"):   # d exactly and 4 d: the unbounded answer
        sel = (k == 1) | (k == 3)
        np.testing.assert_array_equal(nr.bits(want[f][sel]), nr.bits(case.want[f][sel]))
    assert_nearest_equal(case.ctx.nearest(case.pts, bound), want)
    assert_nearest_equal(case.ctx.nearest(case.pts, bound, mode=rt.NEAREST_SORT), want, "SORT")
    # no walk: a negative, NaN or -inf bound; +inf is no limit; -0 is 0
    n = 32
    for b in (np.float32(-1), np.float32(np.nan), -INF, np.float32(-1e-30)):
        got = case.ctx.nearest(case.pts[:n], b)
        assert_nearest_equal(got, nr.no_result(n), f"bound {b}")
    assert_nearest_equal(case.ctx.nearest(case.pts[:n], INF), take(case.want, slice(0, n)), "bound +inf")
    # points exactly on vertices with bound 0: found, dist2 == 0
    verts = case.pts[case.first_vertex:case.first_vertex + 64]
    for zero in (np.float32(0), np.float32(-0.0)):
        got = case.ctx.nearest(verts, zero)
        assert (got["dist2"] == 0).all() and (got["tri"] != nr.NONE).all()
        assert_nearest_equal(got, nr.brute(case.tris, verts, zero), "on a vertex, bound 0")


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
    want = nr.brute(case.tris, pts)
    assert not want["found"][:len(bad)].any() and want["found"][len(bad):].all()
    assert_nearest_equal(case.ctx.nearest(pts), want)
    assert_nearest_equal(case.ctx.nearest(pts, mode=rt.NEAREST_SORT | rt.NEAREST_COUNT), want, "SORT | COUNT")
    assert case.ctx.nearest_counts()["points"] == len(pts) and case.ctx.nearest_counts()["found"] == len(far) + 1


@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = tiny_scene(ntris)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        pts = nr.sample_points(tris, seed=ntris, n_random=300, n_each=16, scale=3.0)[0]
        want = nr.brute(tris, pts)
        assert_nearest_equal(ctx.nearest(pts), want)
        assert len(set(want["tri"].tolist())) == ntris
        d = want["dist2"]
        bound = np.where(np.arange(len(d)) % 2 == 0, d, np.nextafter(d, np.float32(0))).astype(np.float32)
        assert_nearest_equal(ctx.nearest(pts, bound, mode=rt.NEAREST_SORT), nr.brute(tris, pts, bound), "bounded")


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
        for c in (auto, plain):   # a counting ray query first: its counts must survive the closest-point queries
            c.query(rays, rt.QUERY_COUNT)
        ray_counts = plain.query_counts()
        assert auto.query_counts() == ray_counts and ray_counts["rays"] == 2000
        a, p = auto.nearest(pts, mode=rt.NEAREST_COUNT), plain.nearest(pts, mode=rt.NEAREST_COUNT)
        np.testing.assert_array_equal(a.view(np.uint32), p.view(np.uint32))
        assert_nearest_equal(a, nr.brute(tris, pts))
        ca, cp = auto.nearest_counts(), plain.nearest_counts()
        print("closest-point steps per point:", {k: v / 512 for k, v in ca.items()})
        assert ca == cp   # the same visits on both forms
        assert ca["points"] == 512 and ca["found"] == 512
        assert 0 < ca["leaf_steps"] < 512 * T // 8 and ca["internal_steps"] > 0
        for c in (auto, plain):
            np.testing.assert_array_equal(c.nearest(pts, mode=rt.NEAREST_SORT).view(np.uint32), a.view(np.uint32))
            assert c.query_counts() == ray_counts       # the last counting RAY query's, still
            c.query(rays[:100], rt.QUERY_COUNT)
            assert c.query_counts()["rays"] == 100
            assert c.nearest_counts() == ca             # ... and a ray query leaves these alone
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
    assert_nearest_equal(c.ctx.nearest(pts[:n]), take(want, slice(0, n)))
    assert_nearest_equal(c.ctx.nearest(pts[:n], mode=rt.NEAREST_SORT | rt.NEAREST_COUNT), take(want, slice(0, n)), "SORT")
    assert c.ctx.nearest_counts()["points"] == n
    assert c.ctx.nearest(pts[:0]).shape == (0,)


# ---------------------------------------------------------------- 6. device tensors and streams
def test_device_tensors_on_two_streams(big):
    import torch
    c, pts, want = big
    n = len(pts)
    d = want["dist2"]
    bound = np.where(np.arange(n) % 2 == 0, d, np.float32(.5) * d).astype(np.float32)
    want_b = nr.brute(c.tris, pts[:4096], bound[:4096])
    p1 = torch.from_numpy(rt.make_points(pts).view(np.float32).reshape(n, 4)).cuda()
    p2 = rt.make_points(torch.from_numpy(pts[:4096]).cuda(), torch.from_numpy(bound[:4096]).cuda())
    o, dd = random_rays(c.ctx.read_bvh(), 4096, seed=5)
    rays = torch.from_numpy(rt.make_rays(o, dd).view(np.float32).reshape(-1, 8)).cuda()
    hits_want = c.ctx.query(rt.make_rays(o, dd))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    r1 = c.ctx.nearest(p1, mode=rt.NEAREST_COUNT, stream=s1)   # back to back, one context, two streams
    hits = c.ctx.query(rays, stream=s2)
    r2 = c.ctx.nearest(p2, mode=rt.NEAREST_SORT, stream=s1)
    s1.synchronize()
    s2.synchronize()
    assert r1.is_cuda and r1.dtype == torch.float32 and tuple(r1.shape) == (n, 8)
    assert_nearest_equal(r1.cpu().numpy().view(rt.NEAREST_DTYPE).reshape(-1), want)
    assert_nearest_equal(r2.cpu().numpy().view(rt.NEAREST_DTYPE).reshape(-1), want_b)
    np.testing.assert_array_equal(hits.cpu().numpy().view(np.uint32), hits_want.view(np.uint32).reshape(-1, 4))
    np.testing.assert_array_equal(r1[:, 6].view(torch.int32).cpu().numpy(), want["tri"].view(np.int32))
    assert c.ctx.nearest_counts()["points"] == n
    # `out` reuse, on the current stream (torch's default one) and on a side stream
    out = torch.full((4096, 8), 7.0, dtype=torch.float32, device="cuda")
    assert c.ctx.nearest(p2, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), r2.cpu().numpy().view(np.uint32))
    out.fill_(7.0)
    s1.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        c.ctx.nearest(p2, out=out)
    s1.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), r2.cpu().numpy().view(np.uint32))
    with pytest.raises(ValueError):
        c.ctx.nearest(p2, out=torch.empty((4096, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        c.ctx.nearest(p1[:, :3])
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
    with built(s, wvp, wv, flags=flags) as ctx:
        before = ctx.nearest(pts)
        ctx.update_vertices(P)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.nearest(pts)
        assert e.value.status == NOT_READY
        ctx.refit()
        refit = ctx.nearest(pts)
        assert_nearest_equal(refit, nr.brute(tris, pts), "after the refit")
        assert not np.array_equal(before.view(np.uint32), refit.view(np.uint32))
        ctx.build()   # another tree over the same geometry: the answer does not depend on it
        np.testing.assert_array_equal(ctx.nearest(pts).view(np.uint32), refit.view(np.uint32))


# ---------------------------------------------------------------- 8. errors, the stack limit
def test_errors():
    pts = rt.make_points(np.zeros((4, 3), np.float32))
    out = np.zeros(4, rt.NEAREST_DTYPE)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.nearest(pts)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.nearest_counts()
        assert e.value.status == NOT_READY
        assert ctx.nearest(pts[:0]).shape == (0,)   # n == 0 is OK even before a build
        ctx.build()
        for mode in (1, 8, 1 << 8, 1 << 31, rt.NEAREST_SORT | 16):
            with pytest.raises(rt.RtbvhError) as e:
                ctx.nearest(pts, mode=mode)
            assert e.value.status == INVALID_ARG
        assert L.rtbvh_nearest_async(ctx._h, None, 4, None, 0, None) == INVALID_ARG
        assert L.rtbvh_nearest_async(ctx._h, None, 0, None, 0, None) == rt._lib.OK
        assert L.rtbvh_nearest_host(ctx._h, pts.ctypes.data, 4, None, 0) == INVALID_ARG
        assert L.rtbvh_nearest_host(ctx._h, pts.ctypes.data, 1 << 31, out.ctypes.data, 0) == INVALID_ARG
        assert L.rtbvh_nearest_counts(ctx._h, None) == INVALID_ARG
        with pytest.raises(rt.RtbvhError) as e:
            ctx.nearest_counts()                    # still no counting closest-point query
        assert e.value.status == NOT_READY
        got = ctx.nearest(pts)                      # and the context still answers
        d = load_scene_fixture("Rect")
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(W, H)[0])
        assert_nearest_equal(got, nr.brute(tris, pts["point"]))
        ctx.synchronize()


def test_stack_limit_reports_overflow_and_keeps_genuine_results():
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    pts = nr.sample_points(tris, seed=13)[0]
    want = nr.brute(tris, pts)
    with built(s, wvp, wv, stack_limit=2) as ctx:
        out = np.zeros(len(pts), rt.NEAREST_DTYPE)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.nearest(pts, out=out)   # the host entry is synchronous: it reports at once
        assert e.value.status == OVERFLOW
        ctx.synchronize()               # once per new overflow
        # a walk that lost subtrees ends with the best it found: a genuine triangle distance, never below the answer
        f = out["tri"] != nr.NONE
        assert f.any()
        a, e1, e2, lo, hi = (x[out["tri"][f].astype(np.int64)] for x in nr.leaf_data(tris))
        d, u, v, q = nr.tri_dist2(pts[f], a, e1, e2, lo, hi)
        for name, w in (("dist2", d), ("u", u), ("v", v), ("point", q)):
            np.testing.assert_array_equal(nr.bits(out[name][f]), nr.bits(w), err_msg=name)
        assert (out["dist2"][f] >= want["dist2"][f]).all() and (out["dist2"][~f] == -1).all()
