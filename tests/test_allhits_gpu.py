"""All-hits ray queries on the GPU (rtbvh_allhits_async / rtbvh_allhits_host through Context.allhits and the raw
entries) against the brute force over all triangles (tests/allhits_ref.py), ordered by the build's sort order
(Context.read_sorted) or by (t, tri).  The set and both orders are specified independently of the walk, so every
comparison is bit-exact: offsets as integers, hits as four uint32 words."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import allhits_ref as ar
from tests import deep_scenes as ds
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform
from tests.test_query_gpu import tiny_scene

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]
OK, NOT_READY, INVALID_ARG, OVERFLOW = (rt._lib.OK, rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG,
                                        rt._lib.ERR_STACK_OVERFLOW)
INF = ar.INF
SORT, COUNT, BY_T, SIZES, FILL = rt.ALLHITS_SORT, rt.ALLHITS_COUNT, rt.ALLHITS_BY_T, rt.ALLHITS_SIZES, rt.ALLHITS_FILL
GUARD = 1024                  # hits behind `capacity`, filled with PATTERN
PATTERN = 0x5A5AA5A5
LANE_MAX, LDS_MAX = 32, 2048  # the ordering pass's thresholds (rtbvh_internal.h ALLHITS_LANE_MAX, ALLHITS_LDS_MAX)


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


def assert_allhits_equal(got, want, what=""):
    """(offsets, hits) of Context.allhits against brute_allhits': every offset, every hit's four words."""
    off, hits = got
    assert off.dtype == np.uint64 and hits.dtype == rt.HIT_DTYPE, what
    np.testing.assert_array_equal(off, want[0], err_msg=what + " offsets")
    np.testing.assert_array_equal(ar.hit_words(hits), ar.hit_words(want[1]), err_msg=what + " hits")


def vp(a):
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


class Device:
    """The raw device entry on the context stream with torch tensors for memory: rays up, a hits buffer of
    capacity + GUARD entries filled with PATTERN, offsets and the hits' words back."""

    def __init__(self, ctx, rays):
        import torch
        self.torch, self.ctx, self.n = torch, ctx, len(rays)
        self.rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        self.offsets = torch.full((self.n + 1,), -1, dtype=torch.int64, device="cuda")

    def run(self, capacity, mode=0, offsets=None, null_hits=False, expect=OK):
        torch = self.torch
        if offsets is not None:
            self.offsets.copy_(torch.from_numpy(offsets.view(np.int64).copy()))
        buf = torch.full((capacity + GUARD, 4), PATTERN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        L = rt.lib()
        st = L.rtbvh_allhits_async(self.ctx._h, vp(self.rays), self.n, vp(self.offsets),
                                   None if null_hits else vp(buf), capacity, mode, None)
        assert st == OK
        assert L.rtbvh_synchronize(self.ctx._h) == expect
        words = buf.cpu().numpy().view(np.uint32)
        assert (words[capacity:] == np.uint32(PATTERN)).all(), "a write behind capacity"
        return self.offsets.cpu().numpy().view(np.uint64), words[:capacity]


class Case:
    """A golden scene built on the GPU under one camera, the tests' rays with mixed t_max, and the brute-force lists
    in the build's sort order (once)."""

    def __init__(self, scene, cam):
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.rank = ar.rank_of(self.ctx.read_sorted()[1])
        self.o, self.d = ar.sample_rays(self.tris, 4096, 64, 256)
        self.n = len(self.o)
        self.tm, self.unlimited, self.want = ar.mixed_t_max(self.tris, self.o, self.d, self.rank)
        self.rays = rt.make_rays(self.o, self.d, self.tm)
        self.total = int(self.want[0][-1])
        for a in self.want + self.unlimited:
            a.setflags(write=False)


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. the brute force, and the equivalent calls
def test_matches_brute_force(case):
    import torch
    cnt = np.diff(case.want[0].astype(np.int64))
    cnt_inf = np.diff(case.unlimited[0].astype(np.int64))
    assert case.n == 4096 + 16 + 64 + 256
    assert (cnt >= 2).sum() >= 50 and (cnt == 0).any() and ((cnt < cnt_inf) & (cnt > 0)).any()
    got = case.ctx.allhits(case.rays, capacity=case.total)                        # mode 0: one call
    assert got[0].shape == (case.n + 1,) and got[1].shape == (case.total,)
    assert_allhits_equal(got, case.want, "mode 0")
    assert_allhits_equal(case.ctx.allhits(case.rays), case.want, "SIZES then FILL")
    assert_allhits_equal(case.ctx.allhits(case.rays.view(np.float32).reshape(-1, 8), mode=SORT), case.want, "SORT")
    assert_allhits_equal(case.ctx.allhits(case.rays, mode=SORT | COUNT, capacity=case.total), case.want, "SORT | COUNT")
    c = case.ctx.allhits_counts()
    assert c["rays"] == case.n and c["hits"] == case.total
    assert c["leaf_steps"] >= 2 * case.total and c["internal_steps"] > 0           # two passes, every member's leaf
    np.testing.assert_array_equal(case.ctx.allhits(case.rays, sizes_only=True), case.want[0])
    # torch: capacity given (one call) and not (sized from the total)
    dr = torch.from_numpy(case.rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    for cap in (case.total + 7, None):
        off, hits = case.ctx.allhits(dr, capacity=cap)
        assert off.is_cuda and off.dtype == torch.int64 and tuple(off.shape) == (case.n + 1,)
        assert hits.is_cuda and hits.dtype == torch.float32 and tuple(hits.shape) == (cap or case.total, 4)
        np.testing.assert_array_equal(off.cpu().numpy().view(np.uint64), case.want[0])
        np.testing.assert_array_equal(hits[:case.total].cpu().numpy().view(np.uint32), ar.hit_words(case.want[1]))
    np.testing.assert_array_equal(case.ctx.allhits(dr, sizes_only=True).cpu().numpy().view(np.uint64), case.want[0])
    # the raw device entry, with a guard behind the hits
    dev = Device(case.ctx, case.rays)
    for mode in (0, SORT):
        off, words = dev.run(case.total, mode)
        np.testing.assert_array_equal(off, case.want[0])
        np.testing.assert_array_equal(words, ar.hit_words(case.want[1]))
    off, _ = dev.run(0, SIZES, null_hits=True)                                     # SIZES, then FILL over them
    np.testing.assert_array_equal(off, case.want[0])
    off, words = dev.run(case.total, FILL)
    np.testing.assert_array_equal(words, ar.hit_words(case.want[1]))


# ---------------------------------------------------------------- 2. capacity
def test_capacity_truncates_and_never_writes_behind(case):
    dev = Device(case.ctx, case.rays)
    want_words = ar.hit_words(case.want[1])
    for capacity in (case.total // 2, 1, 0):
        for mode in (0, SORT):
            off, words = dev.run(capacity, mode)
            np.testing.assert_array_equal(off, case.want[0], err_msg=f"capacity {capacity}")   # the true total
            np.testing.assert_array_equal(words, want_words[:capacity], err_msg=f"capacity {capacity}")
    off, _ = dev.run(0, 0, null_hits=True)                                         # capacity 0: hits may be NULL
    np.testing.assert_array_equal(off, case.want[0])
    half = case.total // 2                                                         # the host entry
    off, hits = case.ctx.allhits(case.rays, capacity=half)
    np.testing.assert_array_equal(off, case.want[0])
    np.testing.assert_array_equal(ar.hit_words(hits), want_words[:half])
    assert_allhits_equal(case.ctx.allhits(case.rays, capacity=case.total + 5), case.want, "capacity above the total")


# ---------------------------------------------------------------- 3. FILL over foreign offsets
def test_fill_over_offsets_of_a_smaller_t_max_writes_prefixes(case):
    off_s = case.want[0]                                       # the mixed t_max: lists cut short
    off_l, hits_l = case.unlimited                             # t_max = +inf
    cnt_s, cnt_l = np.diff(off_s.astype(np.int64)), np.diff(off_l.astype(np.int64))
    assert (cnt_l > cnt_s).any() and (cnt_s > 0).any() and (cnt_l >= cnt_s).all()
    total = int(off_s[-1])
    # segment k holds the first cnt_s[k] hits of the longer list of ray k
    src = np.concatenate([np.arange(int(off_l[k]), int(off_l[k]) + cnt_s[k]) for k in range(case.n)])
    dev = Device(case.ctx, rt.make_rays(case.o, case.d))
    for capacity in (total, total // 2):
        for mode in (FILL, FILL | SORT):
            off, words = dev.run(capacity, mode, offsets=off_s)
            np.testing.assert_array_equal(off, off_s)                              # FILL reads them only
            np.testing.assert_array_equal(words, ar.hit_words(hits_l)[src][:capacity], err_msg=f"capacity {capacity}")
    # BY_T orders exactly what was written: each prefix, by (t, tri)
    off, words = dev.run(total, FILL | BY_T, offsets=off_s)
    np.testing.assert_array_equal(words, ar.hit_words(ar.order_by_t(off_s, hits_l[src])))


# ---------------------------------------------------------------- 4. BY_T
def assert_by_t(off, hits, want, what=""):
    """Every list ascends in (t, tri), and holds the hits of the default-order list `want`."""
    np.testing.assert_array_equal(off, want[0], err_msg=what)
    for k, (g, w) in enumerate(zip(ar.segments(off, hits), ar.segments(*want))):
        keys = ar.hit_keys(g)
        assert (keys[1:] > keys[:-1]).all(), f"{what} ray {k}"
        srt = np.argsort(ar.hit_keys(w))
        np.testing.assert_array_equal(ar.hit_words(g), ar.hit_words(w[srt]), err_msg=f"{what} ray {k}")


def test_by_t_orders_each_list(case):
    got = case.ctx.allhits(case.rays, mode=BY_T, capacity=case.total)              # one call
    assert_by_t(*got, case.want, "BY_T")
    want = (case.want[0], ar.order_by_t(*case.want))
    assert_allhits_equal(got, want, "BY_T against the brute force by (t, tri)")
    assert_allhits_equal(case.ctx.allhits(case.rays, mode=BY_T), want, "SIZES, then BY_T | FILL")
    assert_allhits_equal(case.ctx.allhits(case.rays, mode=BY_T | SORT | COUNT, capacity=case.total), want, "all bits")
    assert case.ctx.allhits_counts()["hits"] == case.total
    # a truncated output: the walk-order prefix, then ordered
    cap = case.total // 2
    k = int(np.searchsorted(case.want[0], cap, side="right")) - 1                  # the ray the cut falls in
    off_cut = np.minimum(case.want[0], np.uint64(cap))
    dev = Device(case.ctx, case.rays)
    off, words = dev.run(cap, BY_T)
    np.testing.assert_array_equal(off, case.want[0])
    np.testing.assert_array_equal(words, ar.hit_words(ar.order_by_t(off_cut, case.want[1][:cap])), err_msg=f"ray {k}")


# ---------------------------------------------------------------- 5. consistency with the closest-hit query
def test_closest_hit_is_a_member_and_empty_means_miss(case):
    hits = case.ctx.query(case.rays)
    any_ = case.ctx.query(case.rays, rt.QUERY_ANY)
    cnt = np.diff(case.want[0].astype(np.int64))
    np.testing.assert_array_equal(cnt > 0, hits["t"] != -1)
    np.testing.assert_array_equal(cnt > 0, any_["t"] != -1)
    keys = ar.hit_keys(case.want[1])
    first = case.want[0][:-1].astype(np.int64)[cnt > 0]
    nearest = np.minimum.reduceat(keys, first) >> np.uint64(32)                      # each list's least t
    np.testing.assert_array_equal(rw.bits(hits["t"][cnt > 0]).astype(np.uint64), nearest)
    words = {tuple(w) for w in ar.hit_words(case.want[1]).tolist()}
    for k in np.nonzero(cnt > 0)[0][::7]:
        seg = ar.hit_words(case.want[1][int(case.want[0][k]):int(case.want[0][k + 1])]).tolist()
        assert ar.hit_words(hits[k:k + 1]).tolist()[0] in seg, k                    # (t, u, v, tri): the same bits
        assert tuple(ar.hit_words(any_[k:k + 1]).tolist()[0]) in words, k


# ---------------------------------------------------------------- 6. the deep fan: the stack's scratch part, long lists
class Fan:
    def __init__(self):
        s, _, _, self.wvp, self.wv = ds.fan()
        self.scene = s
        self.tris = rw.clip_triangles(s.vertices, s.indices, self.wvp)
        rng = np.random.default_rng(64)
        o = np.concatenate([rng.uniform(ds.P[0] - ds.R, ds.P[0] + ds.R, (256, 1)),
                            rng.uniform(ds.P[1] - ds.R, ds.P[1] + ds.R, (256, 1)), np.zeros((256, 1))], 1)
        d = np.tile(np.float32([0, 0, 1]), (256, 1))
        tilt = d + np.float32([0.002, -0.002, 0])
        self.o, self.d = np.concatenate([o, o]).astype(np.float32), np.concatenate([d, tilt]).astype(np.float32)
        self.rays = rt.make_rays(self.o, self.d)


@pytest.fixture(scope="module")
def fan():
    return Fan()


def test_fan_lists_in_both_orders(fan):
    with built(fan.scene, fan.wvp, fan.wv) as ctx:
        rank = ar.rank_of(ctx.read_sorted()[1])
        want = ar.brute_allhits(fan.tris, fan.o, fan.d, INF, rank)
        cnt = np.diff(want[0].astype(np.int64))
        assert cnt.max() > 64 and (cnt > LANE_MAX).sum() >= 20 and (cnt <= LANE_MAX).sum() >= 20
        stacks = rw.walk(ds.fan()[2], fan.tris, fan.o, fan.d)["max_stack"]
        assert (stacks >= 24).any()                                    # past the 16 entries in LDS
        total = int(want[0][-1])
        assert_allhits_equal(ctx.allhits(fan.rays, capacity=total), want)
        assert_allhits_equal(ctx.allhits(fan.rays, mode=SORT), want, "SORT")
        by_t = (want[0], ar.order_by_t(*want))
        assert_allhits_equal(ctx.allhits(fan.rays, mode=BY_T, capacity=total), by_t, "BY_T")
        assert_allhits_equal(ctx.allhits(fan.rays, mode=BY_T | SORT), by_t, "BY_T | SORT, two calls")


def test_fan_overflows_at_the_limit_and_stays_consistent(fan):
    with built(fan.scene, fan.wvp, fan.wv, stack_limit=32) as ctx:
        want = ar.brute_allhits(fan.tris, fan.o, fan.d, INF, ar.rank_of(ctx.read_sorted()[1]))
        cap = int(want[0][-1])
        dev = Device(ctx, fan.rays)
        off, words = dev.run(cap, 0, expect=OVERFLOW)
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK               # once per new overflow
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
        total = int(off[-1])
        assert 0 < total < cap
        assert (words[total:] == PATTERN).all()                       # the fill pass wrote what the sizes pass counted
        assert (words[:total, 3] != PATTERN).all()
        got = np.ascontiguousarray(words[:total]).view(rt.HIT_DTYPE).reshape(-1)
        ray = np.repeat(np.arange(len(fan.o)), np.diff(off.astype(np.int64)))
        t, u, v = rw.tri_test(fan.tris, got["tri"].astype(np.int64), fan.o[ray], fan.d[ray])   # every hit genuine
        np.testing.assert_array_equal(ar.hit_words(got)[:, :3], np.stack([rw.bits(t), rw.bits(u), rw.bits(v)], 1))
        assert (t != -1).all()


# ---------------------------------------------------------------- 7. the stack: the ordering pass's long paths
def test_stack_scene_lists_of_every_length_class():
    K = 2 * LDS_MAX + 104                                              # more than two LDS chunks
    s = ar.stack_scene(K)
    wvp, wv = camera("identity")
    o, d = ar.stack_rays(64, 64)
    tm = np.full(len(o), INF, np.float32)
    # one length on each side of every threshold, by t_max on rays along +z (triangle k at t = 0.5 + 0.1 k; none of
    # the lengths is 7 mod 8, where the next triangle is a duplicate at the same t)
    lengths = [LANE_MAX, LANE_MAX + 1, LDS_MAX, LDS_MAX + 1, 2 * LDS_MAX, 2 * LDS_MAX + 1, 1, 2, 60, 64, 65, 1000]
    tm[:len(lengths)] = [np.float32(0.5 + 0.1 * (m - 1) + 0.05) for m in lengths]
    # rays in the plane of a flat triangle (1 / d.z is infinite: the lemma's exception): no hit
    po = np.float32([[-3, 2, 0.1 * 10], [-3, 5, 0.1 * 500]])
    pd = np.float32([[1, 0.1, 0], [1, -0.05, 0]])
    o, d, tm = np.concatenate([o, po]), np.concatenate([d, pd]), np.concatenate([tm, np.float32([INF, INF])])
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = ar.rank_of(ctx.read_sorted()[1])
        want = ar.brute_allhits(tris, o, d, tm, rank)
        cnt = np.diff(want[0].astype(np.int64))
        assert cnt[:len(lengths)].tolist() == lengths and (cnt[len(lengths):64] == K).all() and (cnt[-2:] == 0).all()
        assert (cnt[64:128] > 2 * LDS_MAX).all()
        by_t = ar.order_by_t(*want)
        t_bits = rw.bits(by_t["t"][int(want[0][20]):int(want[0][21])])
        assert (np.diff(t_bits.astype(np.int64)) == 0).sum() >= K // 8 - 1        # equal t: the smaller id first
        rays = rt.make_rays(o, d, tm)
        total = int(want[0][-1])
        assert_allhits_equal(ctx.allhits(rays, capacity=total), want)
        assert_allhits_equal(ctx.allhits(rays, mode=BY_T, capacity=total), (want[0], by_t), "BY_T")
        assert_allhits_equal(ctx.allhits(rays, mode=BY_T | SORT), (want[0], by_t), "BY_T | SORT, two calls")


# ---------------------------------------------------------------- 8. tiny scenes
@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = tiny_scene(ntris)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = ar.rank_of(ctx.read_sorted()[1])
        o, d = ar.sample_rays(tris, 300, 24, 300, n_plane=24, seed=ntris)
        # axis rays that start on a vertex and run along the leaf box's face: (T) may accept where (B) rejects
        v = tris.reshape(-1, 3)[:3]
        eo = np.concatenate([v, v, v])
        ed = np.repeat(np.eye(3, dtype=np.float32), 3, 0)
        step = (v[[1, 2, 0]] - v).astype(np.float32)                  # from a vertex along an edge, one axis zeroed
        for a in range(3):
            z = step.copy()
            z[:, a] = 0
            eo, ed = np.concatenate([eo, v]), np.concatenate([ed, z])
        o, d = np.concatenate([o, eo]).astype(np.float32), np.concatenate([d, ed]).astype(np.float32)
        tm, _, want = ar.mixed_t_max(tris, o, d, rank)
        cnt = np.diff(want[0].astype(np.int64))
        assert (cnt > 0).any() and (cnt == 0).any() and cnt.max() <= ntris
        rays = rt.make_rays(o, d, tm)
        assert_allhits_equal(ctx.allhits(rays), want)
        assert_allhits_equal(ctx.allhits(rays, mode=SORT | BY_T, capacity=int(want[0][-1])),
                             (want[0], ar.order_by_t(*want)), "SORT | BY_T, mode 0")


def test_single_leaf_box_is_tested():
    """One triangle flat in z = 0 and a ray in its plane's box face: the leaf box [.., 0] x [.., 0] gives the slab
    [+inf, +inf] on an axis where the ray starts on the face and runs along it, so (B) rejects a ray whose triangle
    test accepts -- on a one-leaf tree only the leaf step can say so."""
    v = np.zeros((3, 8), np.float32)
    v[:, :3] = [[0, 0, 0], [4, 0, 0.5], [0, 4, 1]]
    v[:, 5] = -1
    s = rt.Scene(v, np.arange(3, dtype=np.uint32), np.zeros(1, np.uint32), np.zeros(1, rt.MATERIAL_DTYPE))
    wvp, wv = camera("identity")
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    # rays along +z under the triangle; the third starts level with the box's x = 0 face and has d.x = 0
    o = np.float32([[1, 1, -1], [3, 3, -1], [0, 1, -1], [0, 0, -1]])
    d = np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]])
    tm = np.full(4, INF, np.float32)
    ok, t, _, _ = ar.pair_tests(tris, np.zeros(4, np.int64), o, d, tm)
    assert ok.tolist() == [True, False, False, False] and (t[2] != -1 or t[3] != -1)   # (T) alone would accept one
    with built(s, wvp, wv) as ctx:
        want = ar.brute_allhits(tris, o, d, tm, np.zeros(1, np.int64))
        assert want[0].tolist() == [0, 1, 1, 1, 1]
        assert_allhits_equal(ctx.allhits(rt.make_rays(o, d)), want)
        np.testing.assert_array_equal(ctx.query(rt.make_rays(o, d))["t"] != -1, [True, False, True, True])


# ---------------------------------------------------------------- 9. both tree forms
def test_records_and_node_box_trees_agree():
    s = rt.synthetic(70_000, seed=0x5EED0004)
    wvp, wv = rt.camera_reference(W, H)
    with built(s, wvp, wv, flags=rt.FLAG_AUTO_WALK) as auto, built(s, wvp, wv) as plain:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        np.testing.assert_array_equal(auto.read_sorted()[1], plain.read_sorted()[1])
        o, d = ar.sample_rays(tris, 384, 16, 96, seed=3)
        rays = rt.make_rays(o, d)
        auto.trace(W, H, 1)
        assert auto.stats()["walk_state"] == 2   # (the certified walks: the build wrote node boxes, no records)
        a, p = (c.allhits(rays, mode=COUNT) for c in (auto, plain))
        np.testing.assert_array_equal(a[0], p[0])
        np.testing.assert_array_equal(ar.hit_words(a[1]), ar.hit_words(p[1]))
        ca, cp = auto.allhits_counts(), plain.allhits_counts()
        assert ca == cp and ca["rays"] == len(o) and ca["hits"] == len(a[1]) > len(o) // 4
        cnt = np.diff(a[0].astype(np.int64))
        sel = np.nonzero(cnt > 0)[0][:64]                                           # the brute force, for some rays
        want = ar.brute_allhits(tris, o[sel], d[sel], INF, ar.rank_of(plain.read_sorted()[1]))
        np.testing.assert_array_equal(np.diff(want[0].astype(np.int64)), cnt[sel])
        got = np.concatenate([p[1][int(p[0][k]):int(p[0][k + 1])] for k in sel])
        np.testing.assert_array_equal(ar.hit_words(got), ar.hit_words(want[1]))
        for c in (auto, plain):
            b = c.allhits(rays, mode=BY_T | SORT)
            np.testing.assert_array_equal(ar.hit_words(b[1]), ar.hit_words(ar.order_by_t(*p)))


# ---------------------------------------------------------------- 10. animated geometry
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
    with built(s, wvp, wv, flags=flags) as ctx:
        old_order = ctx.read_sorted()[1].copy()
        before = ctx.allhits(rays)
        ctx.update_vertices(P)
        with pytest.raises(rt.RtbvhError) as e:
            ctx.allhits(rays)
        assert e.value.status == NOT_READY
        ctx.refit()
        np.testing.assert_array_equal(ctx.read_sorted()[1], old_order)   # a refit keeps the order
        want = ar.brute_allhits(tris, o, d, INF, ar.rank_of(old_order))
        refit = ctx.allhits(rays)
        assert_allhits_equal(refit, want, "after the refit")
        assert not (np.array_equal(before[0], refit[0]) and np.array_equal(before[1], refit[1]))
        ctx.build()   # another tree over the same geometry: the same sets, and BY_T the same bytes
        by_t = ctx.allhits(rays, mode=BY_T)
        assert_allhits_equal(by_t, (want[0], ar.order_by_t(*want)), "after the rebuild, BY_T")


# ---------------------------------------------------------------- 11. streams, an asynchronous rebuild
def test_two_streams_and_async_rebuild(case):
    import torch
    n = case.n
    r1 = torch.from_numpy(case.rays.view(np.float32).reshape(n, 8).copy()).cuda()
    r2 = torch.from_numpy(rt.make_rays(case.o, case.d).view(np.float32).reshape(n, 8).copy()).cuda()
    total2 = int(case.unlimited[0][-1])
    want_q = case.ctx.query(case.rays)
    wvp2, wv2 = rt.camera_look(rt.camera_orbit(rt.EYE_REFERENCE, rt.KEY_LEFT), W, H)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    try:
        o1, h1 = case.ctx.allhits(r1, mode=COUNT, capacity=case.total + 3, stream=s1)   # back to back, two streams
        q = case.ctx.query(r1, stream=s2)
        o2, h2 = case.ctx.allhits(r2, mode=BY_T | SORT, capacity=total2, stream=s2)
        case.ctx.set_camera(wvp2, wv2)                                  # outstanding while the build is enqueued
        case.ctx.build(sync=False)
        o3, h3 = case.ctx.allhits(r2, stream=s1)                        # sees the new tree
        s1.synchronize()
        s2.synchronize()
        np.testing.assert_array_equal(o1.cpu().numpy().view(np.uint64), case.want[0])
        np.testing.assert_array_equal(h1[:case.total].cpu().numpy().view(np.uint32), ar.hit_words(case.want[1]))
        np.testing.assert_array_equal(o2.cpu().numpy().view(np.uint64), case.unlimited[0])
        np.testing.assert_array_equal(h2.cpu().numpy().view(np.uint32), ar.hit_words(ar.order_by_t(*case.unlimited)))
        np.testing.assert_array_equal(q.cpu().numpy().view(np.uint32), want_q.view(np.uint32).reshape(n, 4))
        assert case.ctx.allhits_counts()["hits"] == case.total
        with built(case.scene, wvp2, wv2) as fresh:
            want = fresh.allhits(rt.make_rays(case.o, case.d))
        np.testing.assert_array_equal(o3.cpu().numpy().view(np.uint64), want[0])
        np.testing.assert_array_equal(h3.cpu().numpy().view(np.uint32), ar.hit_words(want[1]))
        assert not np.array_equal(want[0], case.unlimited[0])
    finally:
        case.ctx.set_camera(case.wvp, case.wv)
        case.ctx.build()


# ---------------------------------------------------------------- 12. errors
def test_errors():
    import torch
    rays = rt.make_rays(np.zeros((4, 3), np.float32) + np.float32([0, 10, 0]), np.tile(np.float32([0, -1, 0]), (4, 1)))
    off = np.zeros(5, np.uint64)
    hits = np.zeros(64, rt.HIT_DTYPE)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.allhits(rays)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.allhits_counts()
        assert e.value.status == NOT_READY
        o, h = ctx.allhits(rays[:0])                # n == 0 is OK even before a build
        assert o.tolist() == [0] and h.shape == (0,)
        ctx.build()
        hd = ctx._h
        dr = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
        doff = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        dhits = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for mode in (1, 64, 1 << 8, 1 << 31, SIZES | FILL, SIZES | BY_T, SORT | 64):
            assert L.rtbvh_allhits_async(hd, vp(dr), 4, vp(doff), vp(dhits), 64, mode, None) == INVALID_ARG, mode
            assert L.rtbvh_allhits_host(hd, vp(rays), 4, vp(off), vp(hits), 64, mode) == INVALID_ARG, mode
        assert L.rtbvh_allhits_async(hd, None, 4, vp(doff), vp(dhits), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_allhits_async(hd, vp(dr), 4, None, vp(dhits), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_allhits_async(hd, vp(dr), 4, vp(doff), None, 64, 0, None) == INVALID_ARG
        assert L.rtbvh_allhits_async(hd, vp(dr), 4, vp(doff), None, 64, FILL, None) == INVALID_ARG
        assert L.rtbvh_allhits_async(hd, vp(dr), 1 << 31, vp(doff), vp(dhits), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_allhits_host(hd, vp(rays), 4, None, vp(hits), 64, 0) == INVALID_ARG
        assert L.rtbvh_allhits_host(hd, vp(rays), 4, vp(off), None, 64, 0) == INVALID_ARG
        assert L.rtbvh_allhits_host(hd, vp(rays), 1 << 31, vp(off), vp(hits), 64, 0) == INVALID_ARG
        assert L.rtbvh_allhits_counts(hd, None) == INVALID_ARG
        ctx.synchronize()
        assert (doff.cpu().numpy() == -1).all()     # nothing was written by the rejected calls
        # NULL hits are fine with capacity 0 and under SIZES; n == 0 writes offsets[0] only where there is one
        assert L.rtbvh_allhits_async(hd, vp(dr), 4, vp(doff), None, 0, 0, None) == OK
        assert L.rtbvh_allhits_async(hd, vp(dr), 4, vp(doff), None, 64, SIZES, None) == OK
        assert L.rtbvh_allhits_async(hd, vp(dr), 4, vp(doff), None, 0, BY_T, None) == OK
        assert L.rtbvh_allhits_async(hd, None, 0, None, None, 0, 0, None) == OK
        ctx.synchronize()
        got = doff.cpu().numpy()
        assert got[0] == 0 and (np.diff(got) == got[1]).all() and got[1] >= 2      # the same ray four times: through the box
        doff.fill_(-1)
        torch.cuda.synchronize()
        assert L.rtbvh_allhits_async(hd, None, 0, vp(doff), None, 0, 0, None) == OK
        ctx.synchronize()
        assert doff.cpu().numpy().tolist() == [0, -1, -1, -1, -1]
        with pytest.raises(rt.RtbvhError) as e:
            ctx.allhits_counts()                    # still no counting all-hits query
        assert e.value.status == NOT_READY
        d = load_scene_fixture("Rect")              # and the context still answers
        tris = rw.clip_triangles(d["vertices"], d["indices"], np.eye(4, dtype=np.float32))
        assert_allhits_equal(ctx.allhits(rays), ar.brute_allhits(tris, rays["origin"], rays["direction"], INF,
                                                                 ar.rank_of(ctx.read_sorted()[1])))
        ctx.synchronize()
