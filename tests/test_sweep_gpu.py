"""Sphere-sweep queries on the GPU (rtbvh_sweep_async / rtbvh_sweep_host through Context.sweep) against the brute force
over all triangles of the numpy restatement (tests/sweep_ref.py).  The answer is specified independently of the tree
-- the member with the smallest (max(t, grown leaf-box entry), triangle id), as its genuine {t, point, tri, feature}
-- so every comparison is bit-exact: records as eight uint32 words.  Tolerance: none."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import allhits_ref as ar
from tests import deep_scenes as ds
from tests import hostile_scenes as hs
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests import sweep_ref as sr
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform
from tests.test_query_gpu import tiny_scene

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["identity", "affine"]
OK, NOT_READY, INVALID_ARG, OVERFLOW = (rt._lib.OK, rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG,
                                        rt._lib.ERR_STACK_OVERFLOW)
INF = sr.INF
NONE = sr.NONE
ANY, SORT, COUNT = rt.SWEEP_ANY, rt.SWEEP_SORT, rt.SWEEP_COUNT
NODE_BOXES = rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD   # a build that writes the topology and node boxes


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


def diagonal(tris):
    lo, hi = nr.root_box(tris)
    return np.float32(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))


def assert_sweeps_equal(got, want, what=""):
    assert got.dtype == rt.SWEEP_HIT_DTYPE and got.shape == want.shape, what
    np.testing.assert_array_equal(sr.hit_words(got), sr.hit_words(want), err_msg=what)


def as_hits(t):
    """An (n, 8) float32 device tensor as the SWEEP_HIT_DTYPE array."""
    return np.ascontiguousarray(t.cpu().numpy()).view(rt.SWEEP_HIT_DTYPE).reshape(-1)


def to_device(sweeps):
    import torch
    return torch.from_numpy(sweeps.view(np.float32).reshape(-1, 8).copy()).cuda()


def assert_any_is_genuine(got, mem, want, what=""):
    """SWEEP_ANY's answer: hit / miss as the default mode's, and every record that triangle's own member record."""
    np.testing.assert_array_equal(got["tri"] != NONE, want["tri"] != NONE, err_msg=what)
    hit = np.nonzero(got["tri"] != NONE)[0]
    at = sr.find(mem, hit, got["tri"][hit])
    assert (at >= 0).all(), what
    assert_sweeps_equal(np.ascontiguousarray(got[hit]), sr.records(mem, at), what)
    assert_sweeps_equal(np.ascontiguousarray(got[got["tri"] == NONE]), sr.misses(int((got["tri"] == NONE).sum())), what)


class Case:
    """A golden scene built on the GPU under one camera, the tests' 704 sweeps and every sweep's members (once)."""

    def __init__(self, scene, cam, rays=None, radii=None):
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.T = len(self.tris)
        self.o, self.d = rays(self.tris) if rays else ar.sample_rays(self.tris, 400, 48, 200, 40)
        self.n = len(self.o)
        radii = radii(self.tris) if radii else (0, 1e-3, 5e-2, 2 * diagonal(self.tris))
        self.r = np.float32(radii)[np.arange(self.n) % len(radii)]
        self.mem = sr.members(self.tris, self.o, self.d, self.r)
        for a in self.mem.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        self.want = sr.select(self.mem)
        self.want.setflags(write=False)
        self.sweeps = rt.make_sweeps(self.o, self.d, self.r)


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def big():
    """Test.obj under the reference camera with 20,011 sweeps (the refill claim, a partial last wave) and their
    members; the largest radius a twentieth of the root diagonal, which keeps the brute force to seconds."""
    c = Case("Test", "reference", lambda tris: ar.sample_rays(tris, 20_011 - 16, 0, 0, seed=11),
             lambda tris: (0, 1e-3, 5e-2, 0.05 * diagonal(tris)))
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. the brute force
def test_matches_brute_force(case):
    assert case.n == 704
    want = case.want
    nhit = int((want["tri"] != NONE).sum())
    assert nhit >= 256 and (want["tri"] == NONE).any()
    assert {1, 2} <= set(want["feature"].tolist())
    walked = sr.walked(case.o, case.d, case.r, np.full(case.n, INF, np.float32))
    big_r = walked & (np.arange(case.n) % 4 == 3)      # every triangle in reach at tk = 0: the smallest id in reach
    assert big_r.sum() >= 170 and (want["feature"][big_r] == 1).all() and (want["tri"][big_r] == 0).sum() >= 170
    for mode in (0, SORT, COUNT, SORT | COUNT):
        got = case.ctx.sweep(case.sweeps, mode=mode)
        assert_sweeps_equal(got, want, f"mode {mode}")
        if mode & COUNT:
            c = case.ctx.sweep_counts()
            assert c["sweeps"] == case.n and c["hits"] == nhit
            assert c["leaf_steps"] >= nhit and c["internal_steps"] > 0
    assert_sweeps_equal(case.ctx.sweep(case.sweeps.view(np.float32).reshape(-1, 8)), want, "(N, 8)")
    for mode in (ANY, ANY | SORT | COUNT):
        assert_any_is_genuine(case.ctx.sweep(case.sweeps, mode=mode), case.mem, want, f"mode {mode}")
    assert case.ctx.sweep_counts()["hits"] == nhit


def test_finite_t_max(case):
    """Every third sweep with members gets the t of one of them exactly (it stays a member unless its grown leaf box
    starts above it) or the float below it (it is gone), the others 10."""
    from tests.test_sweep_cpu import finite_t_max
    tm = finite_t_max(case.mem, case.n)
    mem = sr.members(case.tris, case.o, case.d, case.r, tm)
    want = sr.select(mem)
    assert ((want["tri"] == NONE) & (case.want["tri"] != NONE)).any()
    assert ((want["tri"] != NONE) & (tm != INF)).sum() >= 32
    sweeps = rt.make_sweeps(case.o, case.d, case.r, tm)
    assert_sweeps_equal(case.ctx.sweep(sweeps), want)
    assert_sweeps_equal(case.ctx.sweep(sweeps, mode=SORT | COUNT), want, "SORT | COUNT")
    assert case.ctx.sweep_counts()["hits"] == int((want["tri"] != NONE).sum())
    assert_any_is_genuine(case.ctx.sweep(sweeps, mode=ANY), mem, want, "ANY")


# ---------------------------------------------------------------- 2. sweeps that are not walked
def test_invalid_sweeps_get_the_miss_record_without_a_walk(case):
    hit = np.nonzero(case.want["tri"] != NONE)[0][:12]
    o, d, r = case.o[hit].copy(), case.d[hit].copy(), case.r[hit].copy()
    nan = np.float32(np.nan)
    tm = np.full(12, INF, np.float32)
    o[0, 0], o[1, 1], o[2] = nan, INF, nan
    d[3, 0], d[4, 1], d[5] = nan, -INF, 0
    r[6], r[7], r[8] = -1, nan, INF
    tm[9], tm[10], tm[11] = nan, -1, -INF
    miss = sr.misses(12)
    assert_sweeps_equal(sr.brute(case.tris, o, d, r, tm), miss, "the restatement")
    for mode in (0, ANY, SORT | COUNT):
        assert_sweeps_equal(case.ctx.sweep(rt.make_sweeps(o, d, r, tm), mode=mode), miss, f"mode {mode}")
    assert case.ctx.sweep_counts() == {"sweeps": 12, "hits": 0, "internal_steps": 0, "leaf_steps": 0}
    # ... and beside sweeps that are: every record is written; -0 counts as +0 for r and t_max
    o2, d2 = np.concatenate([o, case.o[hit]]), np.concatenate([d, case.d[hit]])
    r2 = np.concatenate([r, np.where(case.r[hit] == 0, np.float32(-0.0), case.r[hit])]).astype(np.float32)
    tm2 = np.concatenate([tm, np.full(12, INF, np.float32)])
    got = case.ctx.sweep(rt.make_sweeps(o2, d2, r2, tm2))
    assert_sweeps_equal(got, sr.brute(case.tris, o2, d2, r2, tm2))
    assert_sweeps_equal(np.ascontiguousarray(got[12:]), np.ascontiguousarray(case.want[hit]))
    zero = rt.make_sweeps(case.o[hit], case.d[hit], 2 * diagonal(case.tris), -0.0)   # t_max = -0: the overlaps alone
    got = case.ctx.sweep(zero)
    assert_sweeps_equal(got, sr.brute(case.tris, case.o[hit], case.d[hit], 2 * diagonal(case.tris), np.float32(-0.0)))
    assert (got["feature"] == 1).all()


# ---------------------------------------------------------------- 3. device tensors and streams
def test_device_tensors_on_a_side_stream(case):
    import torch
    s1 = torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    dev = to_device(case.sweeps)
    with torch.cuda.stream(s1):
        made = rt.make_sweeps(torch.from_numpy(case.o).cuda(), torch.from_numpy(case.d).cuda(),
                              torch.from_numpy(case.r).cuda())
    g1 = case.ctx.sweep(dev, stream=s1)
    g2 = case.ctx.sweep(made, mode=SORT | COUNT, stream=s1)
    s1.synchronize()
    assert g1.is_cuda and g1.dtype == torch.float32 and tuple(g1.shape) == (case.n, 8)
    assert_sweeps_equal(as_hits(g1), case.want, "device")
    assert_sweeps_equal(as_hits(g2), case.want, "device, make_sweeps, SORT | COUNT")
    np.testing.assert_array_equal(g1[:, 4].contiguous().view(torch.int32).cpu().numpy(), case.want["tri"].view(np.int32))
    assert case.ctx.sweep_counts()["sweeps"] == case.n
    assert case.ctx.sweep(dev[:0]).shape == (0, 8) and case.ctx.sweep(case.sweeps[:0]).shape == (0,)
    with pytest.raises(ValueError):
        case.ctx.sweep(dev[:, :7])
    case.ctx.synchronize()


def test_two_streams_interleaved_with_other_kinds(big):
    import torch
    n, m = big.n, 4096
    rays = rt.make_rays(big.o[:m], big.d[:m])
    pts = rt.make_points(big.o[:m])
    hits_want, near_want = big.ctx.query(rays), big.ctx.nearest(pts)
    khits_want = big.ctx.khits(rays, 3)
    d1, d2 = to_device(big.sweeps), to_device(np.ascontiguousarray(big.sweeps[:m]))
    dr = torch.from_numpy(rays.view(np.float32).reshape(m, 8).copy()).cuda()
    dp = torch.from_numpy(pts.view(np.float32).reshape(m, 4).copy()).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    g1 = big.ctx.sweep(d1, mode=COUNT, stream=s1)        # back to back, one context, two streams
    hits = big.ctx.query(dr, stream=s2)
    g2 = big.ctx.sweep(d2, mode=SORT, stream=s2)
    near = big.ctx.nearest(dp, mode=rt.NEAREST_COUNT, stream=s1)
    g3 = big.ctx.sweep(d2, mode=ANY, stream=s1)
    kh3 = big.ctx.khits(dr, 3, mode=rt.KHITS_COUNT, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert_sweeps_equal(as_hits(g1), big.want)
    assert_sweeps_equal(as_hits(g2), np.ascontiguousarray(big.want[:m]))
    np.testing.assert_array_equal(as_hits(g3)["tri"] != NONE, big.want["tri"][:m] != NONE)
    np.testing.assert_array_equal(hits.cpu().numpy().view(np.uint32), hits_want.view(np.uint32).reshape(-1, 4))
    np.testing.assert_array_equal(near.cpu().numpy().view(np.uint32), near_want.view(np.uint32).reshape(-1, 8))
    np.testing.assert_array_equal(kh3.cpu().numpy().view(np.uint32).reshape(-1, 4), ar.hit_words(khits_want))
    # the count blocks are the kinds' own: a counting nearest and a counting khits left the sweep's alone ...
    c = big.ctx.sweep_counts()
    assert c["sweeps"] == n and c["hits"] == int((big.want["tri"] != NONE).sum())
    near_c, khits_c = big.ctx.nearest_counts(), big.ctx.khits_counts()
    assert near_c["points"] == m and khits_c["rays"] == m
    # ... and the reverse
    big.ctx.sweep(d2, mode=COUNT)
    assert big.ctx.sweep_counts()["sweeps"] == m
    assert big.ctx.nearest_counts() == near_c and big.ctx.khits_counts() == khits_c
    big.ctx.synchronize()


# ---------------------------------------------------------------- 4. both tree forms, T == 1, a moving mesh, sizes
def test_node_box_trees(case):
    """A certified-only context's multi-kernel build writes the topology and node boxes (the NB instances): the
    brute force again, and the same counted steps as on the records."""
    with built(case.scene, case.wvp, case.wv, flags=NODE_BOXES) as nbox:
        np.testing.assert_array_equal(nbox.read_sorted()[1], case.ctx.read_sorted()[1])
        for mode in (COUNT, COUNT | SORT):
            assert_sweeps_equal(nbox.sweep(case.sweeps, mode=mode), case.want, f"node boxes, mode {mode}")
            case.ctx.sweep(case.sweeps, mode=mode)
            assert nbox.sweep_counts() == case.ctx.sweep_counts()
        assert_any_is_genuine(nbox.sweep(case.sweeps, mode=ANY), case.mem, case.want, "node boxes, ANY")
        assert_sweeps_equal(as_hits(nbox.sweep(to_device(case.sweeps))), case.want, "node boxes, device")


def test_auto_walk_build_on_a_larger_mesh():
    """A FLAG_AUTO_WALK context after a trace (walk_state 2: node boxes, no records) and a plain one: the same bytes
    and counted steps on 70,000 triangles, and the brute force for some sweeps."""
    s = rt.synthetic(70_000, seed=0x5EED0004)
    wvp, wv = rt.camera_reference(W, H)
    with built(s, wvp, wv, flags=rt.FLAG_AUTO_WALK) as auto, built(s, wvp, wv) as plain:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        o, d = ar.sample_rays(tris, 1500, 84, 400, seed=3)
        r = (np.float32([0, 1e-4, 1e-3, 1e-2]) * diagonal(tris))[np.arange(len(o)) % 4]
        sweeps = rt.make_sweeps(o, d, r)
        auto.trace(W, H, 1)
        assert auto.stats()["walk_state"] == 2
        a, p = auto.sweep(sweeps, mode=COUNT), plain.sweep(sweeps, mode=COUNT)
        assert a.tobytes() == p.tobytes()
        ca = auto.sweep_counts()
        print("sweep steps per sweep:", {key: v / len(o) for key, v in ca.items()})
        assert ca == plain.sweep_counts() and ca["sweeps"] == len(o) and ca["hits"] == int((a["tri"] != NONE).sum()) > 100
        sel = np.nonzero(a["tri"] != NONE)[0][:48]
        assert_sweeps_equal(np.ascontiguousarray(a[sel]), sr.brute(tris, o[sel], d[sel], r[sel]))
        for c in (auto, plain):
            assert c.sweep(sweeps, mode=SORT).tobytes() == a.tobytes()


@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = tiny_scene(ntris)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        o, d = ar.sample_rays(tris, 300, 24, 300, n_plane=24, seed=ntris)
        r = np.float32([0, 1e-3, 0.3, 1.5])[np.arange(len(o)) % 4]
        want = sr.brute(tris, o, d, r)
        assert (want["tri"] != NONE).any() and (want["tri"] == NONE).any()
        assert len(set(want["feature"].tolist())) >= 5
        assert_sweeps_equal(ctx.sweep(rt.make_sweeps(o, d, r)), want)
        assert_sweeps_equal(ctx.sweep(rt.make_sweeps(o, d, r), mode=SORT | COUNT), want, "SORT | COUNT")
        tm = np.where(np.arange(len(o)) % 2 == 0, np.float32(2), np.float32(0.5)).astype(np.float32)
        assert_sweeps_equal(ctx.sweep(rt.make_sweeps(o, d, r, tm)), sr.brute(tris, o, d, r, tm), "t_max")


@pytest.mark.parametrize("flags", [0, NODE_BOXES], ids=["records", "node boxes"])
def test_after_update_refit_and_rebuild(flags):
    s = fixture_scene("Test")
    wvp, wv = rt.camera_reference(W, H)
    P = deform(s.vertices[:, :3], 0.7)
    v = s.vertices.copy()
    v[:, :3] = P
    tris = rw.clip_triangles(v, s.indices, wvp)
    o, d = ar.sample_rays(tris, 384, 16, 96, seed=9)
    r = (np.float32([0, 1e-3, 1e-2, 1e-1]) * diagonal(tris))[np.arange(len(o)) % 4]
    sweeps = rt.make_sweeps(o, d, r)
    with built(s, wvp, wv, flags=flags) as ctx:
        before = ctx.sweep(sweeps)
        ctx.update_vertices(P)
        for call in (lambda: ctx.sweep(sweeps), lambda: ctx.sweep(to_device(sweeps))):
            with pytest.raises(rt.RtbvhError) as e:
                call()
            assert e.value.status == NOT_READY
        ctx.refit()
        refit = ctx.sweep(sweeps)
        assert_sweeps_equal(refit, sr.brute(tris, o, d, r), "after the refit")
        assert before.tobytes() != refit.tobytes()
        ctx.build()   # another tree over the same geometry: the answer does not depend on it
        assert ctx.sweep(sweeps).tobytes() == refit.tobytes()


@pytest.mark.parametrize("n", [1, 63, 65, 257, 20_011])
def test_sizes(big, n):
    assert big.n == 20_011
    want = np.ascontiguousarray(big.want[:n])
    sweeps = np.ascontiguousarray(big.sweeps[:n])
    assert_sweeps_equal(big.ctx.sweep(sweeps), want)
    assert_sweeps_equal(big.ctx.sweep(sweeps, mode=SORT | COUNT), want, "SORT")
    c = big.ctx.sweep_counts()
    assert c["sweeps"] == n and c["hits"] == int((want["tri"] != NONE).sum())


# ---------------------------------------------------------------- 5. a deep tree, the stack limit
def fan_sweeps(n=256, seed=4):
    """Sweeps along +z (a little oblique) through the fan's window from in front of it: every box of the fan's 36
    levels holds the window, so the walk pushes at every level."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(ds.P[0] - ds.R, ds.P[0] + ds.R, n), rng.uniform(ds.P[1] - ds.R, ds.P[1] + ds.R, n),
                  np.full(n, ds.FRONT_Z + 0.05)], 1).astype(np.float32)
    d = np.stack([rng.uniform(-0.01, 0.01, n), rng.uniform(-0.01, 0.01, n), np.ones(n)], 1).astype(np.float32)
    r = np.float32([0, 0.01, 0.05, 0.5])[np.arange(n) % 4]
    return o, d, r


def test_fan_full_limit_is_exact_and_a_low_limit_reports_overflow_once():
    s, _, _, wvp, wv = ds.fan()
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    o, d, r = fan_sweeps()
    sweeps = rt.make_sweeps(o, d, r)
    mem = sr.members(tris, o, d, r)
    want = sr.select(mem)
    assert (want["tri"] != NONE).sum() >= 128
    with built(s, wvp, wv) as ctx:
        assert_sweeps_equal(ctx.sweep(sweeps), want, "the full stack")
        assert_sweeps_equal(as_hits(ctx.sweep(to_device(sweeps), mode=SORT)), want, "the full stack, device")
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK
    with built(s, wvp, wv, stack_limit=6) as ctx:
        import torch
        dev = to_device(sweeps)
        out = torch.full((len(o), 8), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        vp = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        assert rt.lib().rtbvh_sweep_async(ctx._h, vp(dev), len(o), vp(out), 0, None) == OK
        assert rt.lib().rtbvh_synchronize(ctx._h) == OVERFLOW
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK        # once per new overflow
        got = as_hits(out)
    # a walk that lost subtrees ends with the best member it found: a genuine member's record, never a better key
    hit = np.nonzero(got["tri"] != NONE)[0]
    assert len(hit) > 0
    assert_sweeps_equal(np.ascontiguousarray(got[got["tri"] == NONE]), sr.misses(int((got["tri"] == NONE).sum())))
    at = sr.find(mem, hit, got["tri"][hit])
    assert (at >= 0).all()
    assert_sweeps_equal(np.ascontiguousarray(got[hit]), sr.records(mem, at))
    assert (want["tri"][hit] != NONE).all()
    best = sr.find(mem, hit, want["tri"][hit])
    key = sr.keys(mem["t"], mem["mn"], mem["tri"])
    assert (key[at] >= key[best]).all()


# ---------------------------------------------------------------- 6. hostile geometry
@pytest.mark.parametrize("cam", hs.CAMERAS)
@pytest.mark.parametrize("variant", list(hs.VARIANTS))
def test_hostile_scenes(variant, cam):
    h = hs.hostile(variant, 12)
    wvp, wv = hs.camera(cam)
    tris = h.tris(wvp)
    inp = hs.Inputs(tris, h.labels)
    o, d = inp.ray_o, inp.ray_d
    fin = tris[hs.finite_part(tris, h.labels)]
    r = (np.float32([0, 1e-3, 2e-2, 0.3]) * diagonal(fin))[np.arange(len(o)) % 4]
    want = sr.brute(tris, o, d, r)
    assert (want["tri"] != NONE).sum() >= 100
    tm = np.where(np.arange(len(o)) % 3 == 0, np.float32(0.5), INF).astype(np.float32)
    want_tm = sr.brute(tris, o, d, r, tm)
    for flags in (0, NODE_BOXES):
        with built(h.scene, wvp, wv, flags=flags) as ctx:
            assert_sweeps_equal(ctx.sweep(rt.make_sweeps(o, d, r)), want, f"{variant}")
            assert_sweeps_equal(as_hits(ctx.sweep(to_device(rt.make_sweeps(o, d, r, tm)), mode=SORT)), want_tm,
                                f"{variant}, t_max")
            assert rt.lib().rtbvh_synchronize(ctx._h) == OK


# ---------------------------------------------------------------- 7. the protocol
def test_errors_and_their_precedence():
    """DESIGN.md 5p's order for both entries: mode bits, 2^31, n == 0, NULL arrays, no tree, a stale tree."""
    o = np.zeros((4, 3), np.float32)
    sweeps = rt.make_sweeps(o, np.float32([[0, 0, 1]] * 4), 0.5)
    out = np.zeros(4, rt.SWEEP_HIT_DTYPE)
    L = rt.lib()
    p, q = ctypes.c_void_p(sweeps.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    s = fixture_scene("Rect")
    with rt.Context(device=0) as ctx:
        ctx.set_scene(s)
        ctx.set_camera(*rt.camera_reference(W, H))
        entries = (lambda *a: L.rtbvh_sweep_host(ctx._h, *a), lambda *a: L.rtbvh_sweep_async(ctx._h, *a, None))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.sweep(sweeps)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.sweep_counts()
        assert e.value.status == NOT_READY
        assert ctx.sweep(sweeps[:0]).shape == (0,)       # n == 0 is OK even before a build
        for entry in entries:
            assert entry(None, 4, None, 8) == INVALID_ARG            # (every argument wrong: still INVALID_ARG)
            assert entry(None, 4, q, 0) == INVALID_ARG               # NULL before NOT_READY
            assert entry(p, 4, q, 0) == NOT_READY
        ctx.build()
        for mode in (8, 16, 1 << 8, 1 << 31, SORT | 32):
            with pytest.raises(rt.RtbvhError) as e:
                ctx.sweep(sweeps, mode=mode)
            assert e.value.status == INVALID_ARG
        for entry in entries:
            assert entry(None, 0, None, 8) == INVALID_ARG            # the mode before n == 0
            assert entry(None, 1 << 31, None, 0) == INVALID_ARG      # 2^31 before n == 0 and the NULLs
            assert entry(None, 0, None, 0) == OK
            assert entry(None, 4, q, 0) == INVALID_ARG
            assert entry(p, 4, None, 0) == INVALID_ARG
            assert entry(p, 1 << 31, q, 0) == INVALID_ARG
        assert L.rtbvh_sweep_counts(ctx._h, None) == INVALID_ARG
        assert not out.view(np.uint32).any()
        with pytest.raises(rt.RtbvhError) as e:
            ctx.sweep_counts()                                       # still no counting sweep query
        assert e.value.status == NOT_READY
        ctx.update_vertices(s.vertices[:, :3])
        for entry in entries:
            assert entry(None, 4, q, 0) == INVALID_ARG               # NULL before the stale tree
            assert entry(p, 4, q, 0) == NOT_READY
            assert entry(p, 0, q, 0) == OK
        ctx.refit()
        tris = rw.clip_triangles(s.vertices, s.indices, rt.camera_reference(W, H)[0])
        oo, dd = ar.sample_rays(tris, 40, 8, 0)
        got = ctx.sweep(rt.make_sweeps(oo, dd, 0.01))                # and the context still answers
        assert_sweeps_equal(got, sr.brute(tris, oo, dd, np.float32(0.01)))
        ctx.synchronize()
