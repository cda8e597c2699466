"""Ray queries on the GPU (rtbvh_query_async / rtbvh_query_host through Context.query) against the CPU oracle's
counters and the numpy restatement of findCollision (tests/ray_walk_ref.py, itself pinned to the oracle by
tests/test_query_cpu.py).  Every comparison is bit-exact: t, u and v are compared as uint32 views."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_query_cpu import BACKGROUND, primary_rays

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
BIG = 100_003


def root_box(nodes):
    n = (len(nodes) + 1) // 2
    root = nodes[n if n > 1 else 0]
    return root["bb_min"].astype(np.float32), root["bb_max"].astype(np.float32)


def random_rays(nodes, count, seed=7):
    """Origins uniform in the root box, directions unit normals."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(nodes)
    o = (lo + rng.random((count, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    d = rng.standard_normal((count, 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    return o, d.astype(np.float32)


def edge_rays(nodes):
    """16 hand-made rays; the last six are degenerate (a zero or NaN direction, a NaN origin): misses."""
    lo, hi = root_box(nodes)
    c = ((lo + hi) / 2).astype(np.float32)
    far = (hi + (hi - lo) + 1).astype(np.float32)
    nan = np.float32(np.nan)
    o = [c] * 6 + [far, far, (lo - 1).astype(np.float32), np.array([c[0], c[1], lo[2] - 10], np.float32)]
    d = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
         c - far, far - c, c - (lo - 1), [0, 0, 1]]
    o += [c, c, c, np.array([nan, c[1], c[2]], np.float32), np.array([nan] * 3, np.float32), c]
    d += [[0, 0, 0], [nan, nan, nan], [nan, 0, 1], [0, 0, 1], [0, 0, 1], [0, nan, 0]]
    return np.array(o, np.float32), np.array(d, np.float32)


def assert_hits_equal(got, want, what=""):
    """got: a HIT_DTYPE array; want: the restatement's dict."""
    np.testing.assert_array_equal(got["t"] != -1, want["hit"], err_msg=what + " hit mask")
    for f in ("t", "u", "v"):
        np.testing.assert_array_equal(rw.bits(got[f]), rw.bits(want[f]), err_msg=what + " " + f)
    np.testing.assert_array_equal(got["tri"], want["tri"], err_msg=what + " tri")


def assert_genuine(got, tris, o, d, t_max=None):
    """Every reported hit is what the restated triangle test returns for its triangle, within t_max."""
    h = got["t"] != -1
    assert (got["tri"][~h] == 0xFFFFFFFF).all() and (got["u"][~h] == 0).all() and (got["v"][~h] == 0).all()
    t, u, v = rw.tri_test(tris, got["tri"][h].astype(np.int64), o[h], d[h])
    np.testing.assert_array_equal(rw.bits(got["t"][h]), rw.bits(t))
    np.testing.assert_array_equal(rw.bits(got["u"][h]), rw.bits(u))
    np.testing.assert_array_equal(rw.bits(got["v"][h]), rw.bits(v))
    if t_max is not None:
        assert (got["t"][h] <= t_max[h]).all()


class Case:
    """A reference scene built on the GPU and by the oracle, its rays and their restated answers (computed once)."""

    def __init__(self, name):
        d = load_scene_fixture(name)
        self.scene = rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
        self.oscene = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
        self.wvp, self.wv = rt.camera_reference(W, H)
        self.ctx = rt.Context(device=0)
        self.ctx.set_scene(self.scene)
        self.ctx.set_camera(self.wvp, self.wv)
        self.ctx.build()
        self.nodes = orc.build(self.oscene, self.wvp)
        self.tris = rw.clip_triangles(d["vertices"], d["indices"], self.wvp)
        ro, rd = random_rays(self.nodes, 4096)
        eo, ed = edge_rays(self.nodes)
        self.o, self.d = np.concatenate([ro, eo]), np.concatenate([rd, ed])
        self.want = rw.walk(self.nodes, self.tris, self.o, self.d)
        # t_max around each ray's own closest t: 0.5 t, t exactly, the float below t (misses: 10)
        t = self.want["t"]
        k = np.arange(len(t)) % 3
        below = np.nextafter(t, np.float32(0))
        self.t_max = np.where(self.want["hit"], np.where(k == 0, np.float32(.5) * t, np.where(k == 1, t, below)),
                              np.float32(10)).astype(np.float32)
        self.want_tmax = rw.walk(self.nodes, self.tris, self.o, self.d, t_max=self.t_max)


@pytest.fixture(scope="module", params=SCENES)
def case(request):
    c = Case(request.param)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def big():
    """Test.obj with 100,003 random rays and their restated closest hits."""
    c = Case("Test")
    o, d = random_rays(c.nodes, BIG, seed=11)
    want = rw.walk(c.nodes, c.tris, o, d)
    yield c, o, d, want
    c.ctx.close()


# ---------------------------------------------------------------- 1. the oracle, directly
def test_primary_and_reflect_rays_match_oracle_counters(case):
    _, _, st0, refl, _ = orc.trace(case.oscene, case.nodes, case.wvp, case.wv, W, H, 0, want_records=True)
    fb0 = orc.trace(case.oscene, case.nodes, case.wvp, case.wv, W, H, 0)[0]
    _, _, st1 = orc.trace(case.oscene, case.nodes, case.wvp, case.wv, W, H, 1)
    o, d = primary_rays(W, H)
    hits = case.ctx.query(rt.make_rays(o, d), rt.QUERY_COUNT)
    assert case.ctx.query_counts() == {"rays": W * H, "hits": st0["hits"], "internal_visits": st0["internal_visits"],
                                       "leaf_visits": st0["leaf_visits"]}
    np.testing.assert_array_equal((hits["t"] != -1).reshape(H, W), (fb0 != BACKGROUND).any(-1))
    rec = refl.reshape(-1, 14)
    live = rec[:, 0] > 0
    hits = case.ctx.query(rt.make_rays(rec[live, 1:4], rec[live, 4:7]), rt.QUERY_COUNT)
    assert case.ctx.query_counts() == {"rays": st1["bounce"], "hits": st1["hits"] - st0["hits"],
                                       "internal_visits": st1["internal_visits"] - st0["internal_visits"],
                                       "leaf_visits": st1["leaf_visits"] - st0["leaf_visits"]}
    assert int((hits["t"] != -1).sum()) == st1["hits"] - st0["hits"]


# ---------------------------------------------------------------- 2. the restatement
def test_closest_hit_matches_restatement(case):
    assert case.want["hit"][:4096].any() and not case.want["hit"][:4096].all()   # both outcomes covered
    assert not case.want["hit"][-6:].any()                                       # the degenerate rays miss
    got = case.ctx.query(rt.make_rays(case.o, case.d))
    assert_hits_equal(got, case.want)
    # counting does not change the answer, and counts what the restatement visits
    got = case.ctx.query(rt.make_rays(case.o, case.d), rt.QUERY_COUNT)
    assert_hits_equal(got, case.want, "COUNT")
    assert case.ctx.query_counts() == {"rays": len(case.o), "hits": int(case.want["hit"].sum()),
                                       "internal_visits": int(case.want["internal"].sum()),
                                       "leaf_visits": int(case.want["leaf"].sum())}


# ---------------------------------------------------------------- 3. t_max
def test_t_max_matches_restatement(case):
    got = case.ctx.query(rt.make_rays(case.o, case.d, case.t_max))
    assert_hits_equal(got, case.want_tmax, "t_max")
    lost = case.want["hit"] & ~case.want_tmax["hit"]
    assert lost.any()   # rays whose t_max is below their only hit became misses
    np.testing.assert_array_equal((got["t"] == -1)[lost], True)
    # t_max == t exactly keeps the hit (unless a box on the way enters later than t by rounding, which the
    # restatement prunes too: most rays, not every ray)
    at = case.want["hit"] & (np.arange(len(case.o)) % 3 == 1)
    assert (rw.bits(got["t"][at]) == rw.bits(case.want["t"][at])).mean() > .9
    assert (got["t"][case.want["hit"]] <= case.t_max[case.want["hit"]]).all()


# ---------------------------------------------------------------- 4. any-hit
@pytest.mark.parametrize("limited", [False, True], ids=["inf", "t_max"])
def test_any_hit_mask_and_triangles(case, limited):
    t_max = case.t_max if limited else np.full(len(case.o), np.inf, np.float32)
    want = case.want_tmax if limited else case.want
    rays = rt.make_rays(case.o, case.d, t_max)
    got = case.ctx.query(rays, rt.QUERY_ANY)
    np.testing.assert_array_equal(got["t"] != -1, want["hit"])
    np.testing.assert_array_equal(got["t"] != -1, case.ctx.query(rays)["t"] != -1)
    assert_genuine(got, case.tris, case.o, case.d, t_max)
    ref = rw.walk(case.nodes, case.tris, case.o, case.d, t_max=t_max, any_hit=True)
    np.testing.assert_array_equal(ref["hit"], want["hit"])
    got = case.ctx.query(rays, rt.QUERY_ANY | rt.QUERY_COUNT)
    counts = case.ctx.query_counts()
    assert counts["rays"] == len(case.o) and counts["hits"] == int(want["hit"].sum())


# ---------------------------------------------------------------- 5. sizes and edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(big, n):
    c, o, d, want = big
    got = c.ctx.query(rt.make_rays(o[:n], d[:n]))
    assert got.shape == (n,)
    assert_hits_equal(got, {k: v[:n] for k, v in want.items()})
    import torch
    dev = c.ctx.query(torch.from_numpy(rt.make_rays(o[:n], d[:n]).view(np.float32).reshape(-1, 8)).cuda())
    assert tuple(dev.shape) == (n, 4)
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), got.view(np.uint32).reshape(-1, 4))


def test_100003_rays(big):
    c, o, d, want = big
    assert_hits_equal(c.ctx.query(rt.make_rays(o, d)), want)


# ---------------------------------------------------------------- 7. SORT
def test_sort_returns_identical_hits(big):
    c, o, d, want = big
    rays = rt.make_rays(o, d)
    assert_hits_equal(c.ctx.query(rays, rt.QUERY_SORT), want, "SORT")
    got = c.ctx.query(rays, rt.QUERY_SORT | rt.QUERY_COUNT)
    assert_hits_equal(got, want, "SORT | COUNT")
    assert c.ctx.query_counts()["internal_visits"] == int(want["internal"].sum())
    assert_hits_equal(c.ctx.query(rays[:65], rt.QUERY_SORT), {k: v[:65] for k, v in want.items()}, "SORT 65")


def tiny_scene(ntris):
    """ntris triangles facing -z, with one material."""
    v = np.zeros((3 * ntris, 8), np.float32)
    for k in range(ntris):
        v[3 * k:3 * k + 3, :3] = np.array([[-3, -2, 0], [4, -1, 1], [0, 5, 2]], np.float32) + np.float32(6 * k)
    v[:, 5] = -1
    return rt.Scene(v, np.arange(3 * ntris, dtype=np.uint32), np.zeros(ntris, np.uint32), np.zeros(1, rt.MATERIAL_DTYPE))


@pytest.mark.parametrize("ntris", [1, 2])
def test_one_and_two_triangle_scenes(ntris):
    s = tiny_scene(ntris)
    wvp, wv = rt.camera_reference(W, H)
    rng = np.random.default_rng(ntris)
    with rt.Context(device=0) as ctx:
        ctx.set_scene(s)
        ctx.set_camera(wvp, wv)
        ctx.build()
        nodes = ctx.read_bvh()
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        lo, hi = root_box(nodes)
        ext = hi - lo + 1
        o = (lo - ext + rng.random((500, 3), dtype=np.float32) * 3 * ext).astype(np.float32)
        aim = (lo + rng.random((500, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
        d = (aim - o).astype(np.float32)   # not unit: t is in units of |d|
        want = rw.walk(nodes, tris, o, d)
        assert want["hit"].any() and not want["hit"].all()
        assert_hits_equal(ctx.query(rt.make_rays(o, d)), want)
        got = ctx.query(rt.make_rays(o, d), rt.QUERY_ANY)
        np.testing.assert_array_equal(got["t"] != -1, want["hit"])
        assert_genuine(got, tris, o, d)


def test_errors():
    d = load_scene_fixture("Rect")
    rays = rt.make_rays(np.zeros((4, 3)), np.ones((4, 3)))
    with rt.Context(device=0) as ctx:
        ctx.set_scene(rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.query(rays)
        assert e.value.status == rt._lib.ERR_NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.query_counts()
        assert e.value.status == rt._lib.ERR_NOT_READY
        assert ctx.query(rays[:0]).shape == (0,)   # n == 0 is OK even before a build
        ctx.build()
        for mode in (8, 1 << 31, rt.QUERY_ANY | 16):
            with pytest.raises(rt.RtbvhError) as e:
                ctx.query(rays, mode)
            assert e.value.status == rt._lib.ERR_INVALID_ARG
        L = rt.lib()
        assert L.rtbvh_query_async(ctx._h, None, 4, None, 0, None) == rt._lib.ERR_INVALID_ARG
        assert L.rtbvh_query_async(ctx._h, None, 0, None, 0, None) == rt._lib.OK
        assert L.rtbvh_query_host(ctx._h, rays.ctypes.data, 1 << 31, rays.ctypes.data, 0) == rt._lib.ERR_INVALID_ARG
        assert ctx.query(rays).shape == (4,)   # and the context still answers
        ctx.synchronize()


# ---------------------------------------------------------------- 6. both tree forms
def test_records_and_node_box_trees_agree():
    s = rt.synthetic(70_000, seed=0x5EED0004)
    wvp, wv = rt.camera_reference(W, H)
    with rt.Context(device=0, flags=rt.FLAG_AUTO_WALK) as auto, rt.Context(device=0) as plain:
        for c in (auto, plain):
            c.set_scene(s)
            c.set_camera(wvp, wv)
            c.build()
        nodes = plain.read_bvh()
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        o, d = random_rays(nodes, 20_000, seed=3)
        rays = rt.make_rays(o, d)
        a, p = auto.query(rays, rt.QUERY_COUNT), plain.query(rays, rt.QUERY_COUNT)
        np.testing.assert_array_equal(a.view(np.uint32), p.view(np.uint32))
        assert auto.query_counts() == plain.query_counts()
        want = rw.walk(nodes, tris, o, d)
        assert want["hit"].any() and not want["hit"].all()
        assert_hits_equal(a, want)
        assert auto.query_counts()["internal_visits"] == int(want["internal"].sum())
        anyh = auto.query(rays, rt.QUERY_ANY)
        np.testing.assert_array_equal(anyh["t"] != -1, want["hit"])
        assert_genuine(anyh, tris, o, d)
        # the query left the build's state alone: the AUTO context still traces the oracle's frame
        auto.trace(W, H, 1)
        fb = auto.read_framebuffer()
        assert auto.stats()["walk_state"] == 2   # (the certified walks: the build wrote node boxes, no records)
        osc = orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob)
        ofb = orc.trace(osc, orc.build(osc, wvp), wvp, wv, W, H, 1, row_begin=0, row_end=16)[0]
        np.testing.assert_array_equal(fb[0:16].view(np.uint32), ofb.view(np.uint32))


# ---------------------------------------------------------------- 8. streams and torch
def test_two_streams_and_device_tensors(case):
    import torch
    n = len(case.o)
    r1 = torch.from_numpy(rt.make_rays(case.o, case.d).view(np.float32).reshape(n, 8)).cuda()
    r2 = torch.from_numpy(rt.make_rays(case.o, case.d, case.t_max).view(np.float32).reshape(n, 8)).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    h1 = case.ctx.query(r1, rt.QUERY_COUNT, stream=s1)   # back to back, one context, two streams
    h2 = case.ctx.query(r2, rt.QUERY_SORT, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert h1.is_cuda and h1.dtype == torch.float32 and tuple(h1.shape) == (n, 4)
    for h, want in ((h1, case.want), (h2, case.want_tmax)):
        got = h.cpu().numpy().view(rt.HIT_DTYPE).reshape(-1)
        assert_hits_equal(got, want)
        tri = h[:, 3].view(torch.int32).cpu().numpy()
        np.testing.assert_array_equal(tri, want["tri"].view(np.int32))
    assert case.ctx.query_counts()["internal_visits"] == int(case.want["internal"].sum())
    # the current stream (here torch's default one) and the numpy path give the same bits
    h3 = case.ctx.query(r1)
    np.testing.assert_array_equal(h3.cpu().numpy().view(np.uint32), h1.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(case.ctx.query(rt.make_rays(case.o, case.d)).view(np.uint32).reshape(n, 4),
                                  h1.cpu().numpy().view(np.uint32))
    with torch.cuda.stream(s1):
        h4 = case.ctx.query(r2, out=torch.empty((n, 4), dtype=torch.float32, device="cuda"))
    s1.synchronize()
    np.testing.assert_array_equal(h4.cpu().numpy().view(np.uint32), h2.cpu().numpy().view(np.uint32))
    case.ctx.synchronize()


def test_query_after_async_rebuild_sees_the_new_tree(case):
    import torch
    n = len(case.o)
    rays = torch.from_numpy(rt.make_rays(case.o, case.d).view(np.float32).reshape(n, 8)).cuda()
    wvp2, wv2 = rt.camera_look(rt.camera_orbit(rt.EYE_REFERENCE, rt.KEY_LEFT), W, H)
    s1 = torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    try:
        before = case.ctx.query(rays, stream=s1)   # outstanding while the build is enqueued
        case.ctx.set_camera(wvp2, wv2)
        case.ctx.build(sync=False)
        moved = case.ctx.query(rays, stream=s1)
        s1.synchronize()
        with rt.Context(device=0) as fresh:
            fresh.set_scene(case.scene)
            fresh.set_camera(wvp2, wv2)
            fresh.build()
            want = fresh.query(rt.make_rays(case.o, case.d))
        np.testing.assert_array_equal(moved.cpu().numpy().view(np.uint32), want.view(np.uint32).reshape(n, 4))
        assert_hits_equal(before.cpu().numpy().view(rt.HIT_DTYPE).reshape(-1), case.want, "before the rebuild")
        assert not np.array_equal(before.cpu().numpy(), moved.cpu().numpy())
    finally:
        case.ctx.set_camera(case.wvp, case.wv)
        case.ctx.build()


# ---------------------------------------------------------------- 9. the stack limit
def test_stack_limit_reports_overflow_and_keeps_genuine_hits():
    import torch
    d = load_scene_fixture("Test")
    wvp, wv = rt.camera_reference(W, H)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    with rt.Context(device=0, stack_limit=2) as ctx:
        ctx.set_scene(rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]))
        ctx.set_camera(wvp, wv)
        ctx.build()
        po, pd = primary_rays(W, H)
        ro, rd = random_rays(ctx.read_bvh(), 4096)
        o, dd = np.concatenate([po, ro]), np.concatenate([pd, rd])
        rays = torch.from_numpy(rt.make_rays(o, dd).view(np.float32).reshape(-1, 8)).cuda()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        hits = ctx.query(rays, stream=s)   # enqueued: no error yet
        with pytest.raises(rt.RtbvhError) as e:
            ctx.synchronize()              # the next synchronising call reports it, as after a trace
        assert e.value.status == rt._lib.ERR_STACK_OVERFLOW
        ctx.synchronize()                  # once per new overflow
        got = hits.cpu().numpy().view(rt.HIT_DTYPE).reshape(-1)
        assert (got["t"] != -1).any()
        assert_genuine(got, tris, o, dd)
        out = np.zeros(len(o), rt.HIT_DTYPE)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.query(rt.make_rays(o, dd), out=out)   # the host entry is synchronous: it reports at once
        assert e.value.status == rt._lib.ERR_STACK_OVERFLOW
        np.testing.assert_array_equal(out.view(np.uint32), got.view(np.uint32))
