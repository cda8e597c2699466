"""First-k ray queries on the GPU (rtbvh_khits_async / rtbvh_khits_host through Context.khits) against the brute force
over all triangles of the numpy restatement (tests/khits_ref.py on tests/allhits_ref.py).  The answer is specified
independently of the tree -- the k members with the smallest (max(t, leaf-box entry), triangle id), in order, each
as its genuine {t, u, v, tri} -- so every comparison is bit-exact: hits as four uint32 words.  Tolerance: none."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import allhits_ref as ar
from tests import khits_ref as kh
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform
from tests.test_query_gpu import tiny_scene

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["identity", "affine"]
KS = [1, 2, 7, 16]
OK, NOT_READY, INVALID_ARG, OVERFLOW = (rt._lib.OK, rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG,
                                        rt._lib.ERR_STACK_OVERFLOW)
INF = kh.INF
SORT, COUNT = rt.KHITS_SORT, rt.KHITS_COUNT


def camera(name):
    m = np.eye(4, dtype=np.float32)
    if name == "affine":
        m[:3, :3] = np.array([[1.5, 0.2, 0], [-0.1, 0.8, 0.3], [0, 0.25, 1.2]], np.float32)
        m[3, :3] = (0.5, -1.0, 2.0)
    elif name == "reference":
        return rt.camera_reference(W, H)
    return m, np.eye(4, dtype=np.float32)


def fixture_scene(name):
    d = load_scene_fixture(name)
    return rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])


def built(scene, wvp, wv, **kw):
    ctx = rt.Context(device=0, **kw)
    ctx.set_scene(scene)
    ctx.set_camera(wvp, wv)
    ctx.build()
    return ctx


def assert_khits_equal(got, want, what=""):
    """got: an (n, k) HIT_DTYPE array; want: khits_ref's.  Every slot's four words."""
    assert got.dtype == rt.HIT_DTYPE and got.shape == want.shape, what
    np.testing.assert_array_equal(ar.hit_words(got), ar.hit_words(want), err_msg=what)


def as_hits(t):
    """An (n, k, 4) float32 device tensor as the (n, k) HIT_DTYPE array."""
    return np.ascontiguousarray(t.cpu().numpy()).view(rt.HIT_DTYPE).reshape(t.shape[0], t.shape[1])


class Case:
    """A golden scene built on the GPU under one camera, the tests' 704 rays and every ray's members (once)."""

    def __init__(self, scene, cam, rays=None):
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.T = len(self.tris)
        self.o, self.d = rays(self.tris) if rays else ar.sample_rays(self.tris, 400, 48, 200, 40)
        self.n = len(self.o)
        self.lists = kh.members(self.tris, self.o, self.d)
        for a in self.lists:
            a.setflags(write=False)
        self.cnt = np.diff(self.lists[0].astype(np.int64))

    def want(self, k, t_max=INF):
        return kh.select_k(self.lists, k, t_max)


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def big():
    """Test.obj under the reference camera with 20,011 rays and their members."""
    c = Case("Test", "reference", lambda tris: ar.sample_rays(tris, 20_011 - 16, 0, 0, seed=11))
    assert c.n == 20_011
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. the brute force
@pytest.mark.parametrize("k", KS)
def test_matches_brute_force(case, k):
    assert case.n == 704
    rays = rt.make_rays(case.o, case.d)
    want = case.want(k)
    nfound = int(kh.found(want).sum())
    assert nfound == int(np.minimum(case.cnt, k).sum()) > 0
    for mode in (0, SORT, COUNT, SORT | COUNT):
        got = case.ctx.khits(rays, k, mode=mode)
        assert_khits_equal(got, want, f"mode {mode}")
        if mode & COUNT:
            c = case.ctx.khits_counts()
            assert c["rays"] == case.n and c["found"] == nfound
            assert c["leaf_steps"] >= nfound and c["internal_steps"] > 0
    assert_khits_equal(case.ctx.khits(rays.view(np.float32).reshape(-1, 8), k), want, "(N, 8)")
    # the GPU's own other queries: slot 0 is a hit iff the closest-hit query hits ...
    closest = case.ctx.query(rays)
    np.testing.assert_array_equal(kh.found(want)[:, 0], closest["t"] != -1)
    # ... and where no member's t is below its leaf box's entry, the list is the first k of ALLHITS_BY_T's
    off, hits, mn = case.lists
    clamped = np.zeros(case.n, bool)
    clamped[np.repeat(np.arange(case.n), case.cnt)[hits["t"] < mn]] = True
    assert (~clamped & (case.cnt > 0)).sum() >= 100
    aoff, ahits = case.ctx.allhits(rays, mode=rt.ALLHITS_BY_T)
    np.testing.assert_array_equal(aoff, off)
    got = case.ctx.khits(rays, k)
    for i in np.nonzero(~clamped)[0]:
        m = min(k, case.cnt[i])
        assert got[i, :m].tobytes() == ahits[int(aoff[i]):int(aoff[i]) + m].tobytes(), i
        assert not kh.found(got)[i, m:].any()


# ---------------------------------------------------------------- 2. t_max
@pytest.mark.parametrize("k", KS)
def test_mixed_t_max(case, k):
    tm, _, cut = ar.mixed_t_max(case.tris, case.o, case.d, np.arange(case.T))
    cnt = np.diff(cut[0].astype(np.int64))
    assert ((cnt < case.cnt) & (cnt > 0)).any() and ((cnt == 0) & (case.cnt > 0)).any()
    want = case.want(k, tm)
    np.testing.assert_array_equal(kh.found(want).sum(1), np.minimum(cnt, k))
    rays = rt.make_rays(case.o, case.d, tm)
    assert_khits_equal(case.ctx.khits(rays, k), want)
    assert_khits_equal(case.ctx.khits(rays, k, mode=SORT | COUNT), want, "SORT | COUNT")
    c = case.ctx.khits_counts()
    assert c["rays"] == case.n and c["found"] == int(kh.found(want).sum())


# ---------------------------------------------------------------- 3. rays that are not walked
def test_no_walk_rays(case):
    k = 3
    hit = np.nonzero(case.cnt > 0)[0][:12]
    assert len(hit) == 12
    o, d = case.o[hit].copy(), case.d[hit].copy()
    nan, inf = np.float32(np.nan), INF
    o[0, 0], o[1, 1], o[2, 2], o[3] = nan, inf, -inf, nan
    d[4, 0], d[5, 1], d[6, 2], d[7] = nan, inf, -inf, 0
    tm = np.full(12, INF, np.float32)
    tm[8:12] = [0, -1, nan, -0.0]
    miss = kh.misses(12, k)
    want = kh.select_k(kh.members(case.tris, o, d), k, tm)
    assert_khits_equal(want, miss, "the restatement")
    for mode in (0, SORT | COUNT):
        assert_khits_equal(case.ctx.khits(rt.make_rays(o, d, tm), k, mode=mode), miss, f"mode {mode}")
    c = case.ctx.khits_counts()
    assert c == {"rays": 12, "found": 0, "internal_steps": 0, "leaf_steps": 0}
    # ... and beside rays that are: every slot of every ray is written
    o2, d2 = np.concatenate([o, case.o[hit]]), np.concatenate([d, case.d[hit]])
    tm2 = np.concatenate([tm, np.full(12, INF, np.float32)])
    out = np.zeros((24, k), rt.HIT_DTYPE)
    out["t"], out["tri"] = 7, 7
    assert case.ctx.khits(rt.make_rays(o2, d2, tm2), k, out=out) is out
    assert_khits_equal(out, kh.select_k(kh.members(case.tris, o2, d2), k, tm2))
    assert kh.found(out)[12:, 0].all()


# ---------------------------------------------------------------- 4. the stack: long lists, ties at the cut
@pytest.fixture(scope="module")
def stack40():
    s = ar.stack_scene(40)
    wvp, wv = camera("identity")
    ctx = built(s, wvp, wv)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    o, d = ar.stack_rays()
    yield ctx, o, d, kh.members(tris, o, d)
    ctx.close()


@pytest.mark.parametrize("k", [1, 7, 15, 16])
def test_stack_scene(stack40, k):
    ctx, o, d, lists = stack40
    off, hits, mn = lists
    assert (np.diff(off.astype(np.int64)) == 40).all() and (hits["t"] < mn).sum() >= 100
    want = kh.select_k(lists, k)
    assert kh.found(want).all()
    # (k = 7 and 15 cut between a triangle and its copy, equal keys but for the id: tests/test_khits_cpu.py counts them)
    rays = rt.make_rays(o, d)
    assert_khits_equal(ctx.khits(rays, k), want)
    assert_khits_equal(ctx.khits(rays, k, mode=SORT), want, "SORT")
    tm = np.where(np.arange(len(o)) % 2 == 0, np.float32(1.75), np.float32(0.95)).astype(np.float32)   # 13 and 5 planes or so
    want = kh.select_k(lists, k, tm)
    assert not kh.found(want)[:, -1].all() or k < 5
    assert_khits_equal(ctx.khits(rt.make_rays(o, d, tm), k), want, "t_max")


def test_stack_scene_200_long_insert_chains():
    s = ar.stack_scene(200)
    wvp, wv = camera("identity")
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    o, d = ar.stack_rays(32, 32)
    # from below (the list fills in ascending order only by the walk's order) and from above (every later plane
    # is nearer: each insertion moves the whole list)
    o2 = o.copy()
    o2[:, 2] = 0.1 * 200 + 0.5
    o, d = np.concatenate([o, o2]), np.concatenate([d, -d])
    lists = kh.members(tris, o, d)
    assert (np.diff(lists[0].astype(np.int64)) == 200).all()
    want = kh.select_k(lists, 16)
    with built(s, wvp, wv) as ctx:
        assert_khits_equal(ctx.khits(rt.make_rays(o, d), 16, mode=COUNT), want)
        c = ctx.khits_counts()
        assert c["found"] == 16 * len(o) and c["leaf_steps"] < 202 * len(o)   # pruned: not every leaf of every ray
        assert_khits_equal(ctx.khits(rt.make_rays(o, d), 16, mode=SORT), want, "SORT")


# ---------------------------------------------------------------- 5. tiny scenes: T == 1 has no parent box test
@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = tiny_scene(ntris)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        o, d = ar.sample_rays(tris, 300, 24, 300, n_plane=24, seed=ntris)
        # axis rays that start on a vertex and run along the leaf box's face: (T) may accept where (B) rejects
        v = tris.reshape(-1, 3)[:3]
        o = np.concatenate([o, v, v, v]).astype(np.float32)
        d = np.concatenate([d, np.repeat(np.eye(3, dtype=np.float32), 3, 0)]).astype(np.float32)
        lists = kh.members(tris, o, d)
        cnt = np.diff(lists[0].astype(np.int64))
        assert (cnt > 0).any() and (cnt == 0).any() and cnt.max() <= ntris
        tm = ar.mixed_t_max(tris, o, d, np.arange(ntris))[0]
        for k in (1, 2, 3):
            assert_khits_equal(ctx.khits(rt.make_rays(o, d), k), kh.select_k(lists, k), f"k {k}")
            assert_khits_equal(ctx.khits(rt.make_rays(o, d, tm), k, mode=SORT), kh.select_k(lists, k, tm), f"k {k} t_max")


def test_single_leaf_box_is_tested():
    """tests/test_allhits_gpu.py's scene: one flat triangle, and rays whose triangle test accepts where the leaf box
    rejects -- on a one-leaf tree only the leaf step can say so."""
    v = np.zeros((3, 8), np.float32)
    v[:, :3] = [[0, 0, 0], [4, 0, 0.5], [0, 4, 1]]
    v[:, 5] = -1
    s = rt.Scene(v, np.arange(3, dtype=np.uint32), np.zeros(1, np.uint32), np.zeros(1, rt.MATERIAL_DTYPE))
    wvp, wv = camera("identity")
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    o = np.float32([[1, 1, -1], [3, 3, -1], [0, 1, -1], [0, 0, -1]])
    d = np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]])
    want = kh.brute_k(tris, o, d, 2)
    assert kh.found(want).tolist() == [[True, False]] + [[False, False]] * 3
    with built(s, wvp, wv) as ctx:
        assert_khits_equal(ctx.khits(rt.make_rays(o, d), 2), want)


def test_the_containment_scene_orders_by_id():
    from tests import containment as cs
    s = cs.containment_scene(npad=64)
    wvp, wv = cs.identity_camera()
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    o, d = np.float32([[2, -0.5, 0]]), np.float32([[0, 0, 1]])
    with built(s, wvp, wv) as ctx:
        for k in (1, 2, 3):
            want = kh.brute_k(tris, o, d, k)
            assert want["tri"][0, :2].tolist() == [0, 1][:k]
            assert_khits_equal(ctx.khits(rt.make_rays(o, d), k), want, f"k {k}")


# ---------------------------------------------------------------- 6. both tree forms
def test_records_and_node_box_trees_agree():
    s = rt.synthetic(70_000, seed=0x5EED0004)
    wvp, wv = rt.camera_reference(W, H)
    k = 7
    with built(s, wvp, wv, flags=rt.FLAG_AUTO_WALK) as auto, built(s, wvp, wv) as plain:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        o, d = ar.sample_rays(tris, 1500, 84, 400, seed=3)
        assert len(o) == 2000
        rays = rt.make_rays(o, d)
        auto.trace(W, H, 1)
        assert auto.stats()["walk_state"] == 2   # (the certified walks: the build wrote node boxes, no records)
        for c in (auto, plain):   # a counting all-hits query first: its counts must survive
            c.allhits(rays[:300], mode=rt.ALLHITS_COUNT)
        all_counts = plain.allhits_counts()
        a, p = auto.khits(rays, k, mode=COUNT), plain.khits(rays, k, mode=COUNT)
        assert a.tobytes() == p.tobytes()
        ca, cp = auto.khits_counts(), plain.khits_counts()
        print("first-k steps per ray:", {key: v / 2000 for key, v in ca.items()})
        assert ca == cp and ca["rays"] == 2000 and ca["found"] == int(kh.found(a).sum()) > 100
        sel = np.nonzero(kh.found(a)[:, 0])[0][:64]                         # the brute force, for some rays
        assert_khits_equal(np.ascontiguousarray(p[sel]), kh.brute_k(tris, o[sel], d[sel], k))
        for c in (auto, plain):
            assert c.khits(rays, k, mode=SORT).tobytes() == a.tobytes()
            assert c.allhits_counts() == all_counts
            assert c.khits_counts() == ca
        # the all-hits queries' set, where it fits: the same triangles
        off, hits = plain.allhits(rays, mode=rt.ALLHITS_BY_T)
        cnt = np.diff(off.astype(np.int64))
        np.testing.assert_array_equal(kh.found(p).sum(1), np.minimum(cnt, k))
        for i in np.nonzero((cnt > 0) & (cnt <= k))[0][:200]:
            assert sorted(p["tri"][i, :cnt[i]].tolist()) == sorted(hits["tri"][int(off[i]):int(off[i + 1])].tolist())


# ---------------------------------------------------------------- 7. sizes: claims, segment ends, partial waves
@pytest.mark.parametrize("n", [1, 63, 65, 257, 20_011])
def test_sizes(big, n):
    k = 2
    want = np.ascontiguousarray(big.want(k)[:n])
    rays = rt.make_rays(big.o[:n], big.d[:n])
    assert_khits_equal(big.ctx.khits(rays, k), want)
    assert_khits_equal(big.ctx.khits(rays, k, mode=SORT | COUNT), want, "SORT")
    c = big.ctx.khits_counts()
    assert c["rays"] == n and c["found"] == int(kh.found(want).sum())
    got = big.ctx.khits(rays[:0], k)
    assert got.shape == (0, k) and got.dtype == rt.HIT_DTYPE


# ---------------------------------------------------------------- 8. device tensors and streams
def test_device_tensors_on_two_streams(big):
    import torch
    n, k = big.n, 7
    m = 4096
    tm = ar.mixed_t_max(big.tris, big.o[:m], big.d[:m], np.arange(big.T))[0]
    want, want_b = big.want(k), kh.select_k(tuple(kh.members(big.tris, big.o[:m], big.d[:m])), k, tm)
    host = rt.make_rays(big.o, big.d)
    hits_want = big.ctx.query(host[:m])
    all_want = big.ctx.allhits(host[:m], mode=rt.ALLHITS_BY_T)
    r1 = torch.from_numpy(host.view(np.float32).reshape(n, 8).copy()).cuda()
    r2 = rt.make_rays(torch.from_numpy(big.o[:m]).cuda(), torch.from_numpy(big.d[:m]).cuda(), torch.from_numpy(tm).cuda())
    r3 = r1[:m].contiguous()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    g1 = big.ctx.khits(r1, k, mode=COUNT, stream=s1)   # back to back, one context, two streams
    hits = big.ctx.query(r3, stream=s2)
    g2 = big.ctx.khits(r2, k, mode=SORT, stream=s1)
    aoff, ahits = big.ctx.allhits(r3, mode=rt.ALLHITS_BY_T, capacity=len(all_want[1]), stream=s2)
    g3 = big.ctx.khits(r3, 1, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert g1.is_cuda and g1.dtype == torch.float32 and tuple(g1.shape) == (n, k, 4)
    assert_khits_equal(as_hits(g1), want)
    assert_khits_equal(as_hits(g2), want_b)
    assert_khits_equal(as_hits(g3), np.ascontiguousarray(big.want(1)[:m]))
    np.testing.assert_array_equal(hits.cpu().numpy().view(np.uint32), hits_want.view(np.uint32).reshape(-1, 4))
    np.testing.assert_array_equal(aoff.cpu().numpy().view(np.uint64), all_want[0])
    np.testing.assert_array_equal(ahits.cpu().numpy().view(np.uint32), ar.hit_words(all_want[1]))
    np.testing.assert_array_equal(g1[..., 3].contiguous().view(torch.int32).cpu().numpy(), want["tri"].view(np.int32))
    assert big.ctx.khits_counts()["rays"] == n
    # `out` reuse, on the current stream (torch's default one) and on a side stream; whatever it held is overwritten
    out = torch.full((m, k, 4), 7.0, dtype=torch.float32, device="cuda")
    assert big.ctx.khits(r2, k, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), g2.cpu().numpy().view(np.uint32))
    out.fill_(3.0)
    s1.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        big.ctx.khits(r2, k, out=out)
    s1.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), g2.cpu().numpy().view(np.uint32))
    for bad in (torch.empty((m, k), dtype=torch.float32, device="cuda"),
                torch.empty((m, k + 1, 4), dtype=torch.float32, device="cuda"),
                torch.empty((m, k, 4), dtype=torch.float64, device="cuda"),
                torch.empty((m, k, 8), dtype=torch.float32, device="cuda")[..., ::2],
                np.zeros((m, k), rt.HIT_DTYPE)):
        with pytest.raises(ValueError):
            big.ctx.khits(r2, k, out=bad)
    with pytest.raises(ValueError):
        big.ctx.khits(r1[:, :7], k)
    big.ctx.synchronize()


# ---------------------------------------------------------------- 9. animated geometry
@pytest.mark.parametrize("flags", [0, rt.FLAG_AUTO_WALK], ids=["plain", "auto"])
def test_after_update_refit_and_rebuild(flags):
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    P = deform(s.vertices[:, :3], 0.7)
    v = s.vertices.copy()
    v[:, :3] = P
    tris = rw.clip_triangles(v, s.indices, wvp)
    o, d = ar.sample_rays(tris, 384, 16, 96, seed=9)
    rays = rt.make_rays(o, d)
    k = 7
    with built(s, wvp, wv, flags=flags) as ctx:
        before = ctx.khits(rays, k)
        ctx.update_vertices(P)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.khits(rays, k)
        assert e.value.status == NOT_READY
        ctx.refit()
        refit = ctx.khits(rays, k)
        assert_khits_equal(refit, kh.brute_k(tris, o, d, k), "after the refit")
        assert before.tobytes() != refit.tobytes()
        ctx.build()   # another tree over the same geometry: the answer does not depend on it
        assert ctx.khits(rays, k).tobytes() == refit.tobytes()


# ---------------------------------------------------------------- 10. errors, the stack limit
def test_errors():
    rays = rt.make_rays(np.zeros((4, 3), np.float32), np.float32([[0, 0, 1]] * 4))
    out = np.zeros((4, 17), rt.HIT_DTYPE)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.khits(rays, 4)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.khits_counts()
        assert e.value.status == NOT_READY
        assert ctx.khits(rays[:0], 4).shape == (0, 4)   # n == 0 is OK even before a build
        ctx.build()
        for mode in (1, 8, 1 << 8, 1 << 31, SORT | 16):
            with pytest.raises(rt.RtbvhError) as e:
                ctx.khits(rays, 4, mode=mode)
            assert e.value.status == INVALID_ARG
        for k in (0, 17):
            assert L.rtbvh_khits_host(ctx._h, rays.ctypes.data, 4, k, out.ctypes.data, 0) == INVALID_ARG
            assert L.rtbvh_khits_async(ctx._h, rays.ctypes.data, 4, k, out.ctypes.data, 0, None) == INVALID_ARG
        assert L.rtbvh_khits_async(ctx._h, None, 4, 4, None, 0, None) == INVALID_ARG
        assert L.rtbvh_khits_async(ctx._h, None, 0, 4, None, 0, None) == OK
        assert L.rtbvh_khits_host(ctx._h, rays.ctypes.data, 4, 4, None, 0) == INVALID_ARG
        assert L.rtbvh_khits_host(ctx._h, None, 4, 4, out.ctypes.data, 0) == INVALID_ARG
        assert L.rtbvh_khits_host(ctx._h, rays.ctypes.data, 1 << 31, 4, out.ctypes.data, 0) == INVALID_ARG
        assert L.rtbvh_khits_counts(ctx._h, None) == INVALID_ARG
        with pytest.raises(rt.RtbvhError) as e:
            ctx.khits_counts()                      # still no counting first-k query
        assert e.value.status == NOT_READY
        d = load_scene_fixture("Rect")
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(W, H)[0])
        o, dd = ar.sample_rays(tris, 40, 8, 0)
        got = ctx.khits(rt.make_rays(o, dd), 4)     # and the context still answers
        assert_khits_equal(got, kh.brute_k(tris, o, dd, 4))
        ctx.synchronize()


def test_stack_limit_reports_overflow_and_keeps_genuine_ascending_lists():
    s = ar.stack_scene(40)
    wvp, wv = camera("identity")
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    o, d = ar.stack_rays()
    k = 7
    want = kh.brute_k(tris, o, d, k)
    with built(s, wvp, wv, stack_limit=2) as ctx:
        out = np.zeros((len(o), k), rt.HIT_DTYPE)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.khits(rt.make_rays(o, d), k, out=out)   # the host entry is synchronous: it reports at once
        assert e.value.status == OVERFLOW
        ctx.synchronize()                               # once per new overflow
    # a walk that lost subtrees ends with the best list it found
    f = kh.found(out)
    assert f.any()
    assert (f[:, :-1] >= f[:, 1:]).all()                                   # the misses are at the end ...
    np.testing.assert_array_equal(ar.hit_words(out[~f]), ar.hit_words(kh.misses(1, int((~f).sum()))[0]))
    rows = np.broadcast_to(np.arange(len(o))[:, None], f.shape)[f]
    tm = np.full(len(rows), INF, np.float32)
    ok, t, u, v, mn = ar.pair_tests(tris, out["tri"][f].astype(np.int64), o[rows], d[rows], tm, with_mn=True)
    assert ok.all()                                                        # every listed hit a genuine member's
    np.testing.assert_array_equal(ar.hit_words(out[f])[:, :3], np.stack([rw.bits(t), rw.bits(u), rw.bits(v)], 1))
    key = np.full(f.shape, np.uint64(0xFFFFFFFFFFFFFFFF))
    key[f] = kh.keys(out[f], mn)
    assert (key[:, :-1] < key[:, 1:])[f[:, :-1] & f[:, 1:]].all()          # ascending by key: no id twice
    wf = kh.found(want)
    assert wf.all()
    rows = np.broadcast_to(np.arange(len(o))[:, None], wf.shape)[wf]
    mn_w = ar.pair_tests(tris, want["tri"][wf].astype(np.int64), o[rows], d[rows],
                         np.full(len(rows), INF, np.float32), with_mn=True)[4]
    true_key = kh.keys(want[wf], mn_w).reshape(wf.shape)
    assert (key >= true_key).all()                                         # slot j never below the true j-th
