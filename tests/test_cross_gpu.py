"""Triangle queries on the GPU (rtbvh_cross_async / _host and rtbvh_cross_first_async / _host through Context.cross,
Context.cross_first and the raw entries) against the brute force over all (query, triangle) pairs
(tests/cross_ref.py), listed by the build's sort order (Context.read_sorted).  The set, its order and the first
member are specified independently of the walk, so every comparison is bit-exact: offsets and ids as integers."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import collide_ref as cr
from tests import cross_ref as xr
from tests import overlap_ref as ovr
from tests import ray_walk_ref as rw
from tests import within_ref as wr
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Rect", "Test", "Image_Test"]
CAMERAS = ["reference", "identity"]
QUERIES = ["own", "random"]
OK, NOT_READY, INVALID_ARG, OVERFLOW = (rt._lib.OK, rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG,
                                        rt._lib.ERR_STACK_OVERFLOW)
SORT, COUNT, SIZES, FILL = rt.CROSS_SORT, rt.CROSS_COUNT, rt.CROSS_SIZES, rt.CROSS_FILL
OWN_COUNTS = {"Rect": 62, "Test": 8_812, "Image_Test": 2_930}   # identity camera, index-sharing entries removed
GUARD = 1024                  # ids behind `capacity`, filled with PATTERN
PATTERN = 0x5A5AA5A5
NONE = 0xFFFFFFFF


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


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a.view(np.uint32)


def assert_cross_equal(got, want, what=""):
    off, ids = got
    if hasattr(off, "is_cuda"):
        off, ids = host(off), host(ids)
    assert off.dtype == np.uint64 and ids.dtype == np.uint32, what
    np.testing.assert_array_equal(off, want[0], err_msg=what + " offsets")
    np.testing.assert_array_equal(ids, want[1], err_msg=what + " ids")


def vp(a):
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


class Device:
    """The raw device entry on the context stream with torch tensors for memory: an ids buffer of capacity + GUARD
    words filled with PATTERN, offsets and ids back."""

    def __init__(self, ctx, q):
        import torch
        self.torch, self.ctx, self.n = torch, ctx, len(q)
        self.tris = to_device(q)
        self.offsets = torch.full((self.n + 1,), -1, dtype=torch.int64, device="cuda")

    def run(self, capacity, mode=0, offsets=None, null_ids=False, expect=OK):
        torch = self.torch
        if offsets is not None:
            self.offsets.copy_(torch.from_numpy(offsets.view(np.int64)))
        buf = torch.full((capacity + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        L = rt.lib()
        st = L.rtbvh_cross_async(self.ctx._h, vp(self.tris), self.n, vp(self.offsets), None if null_ids else vp(buf),
                                 capacity, mode, None)
        assert st == OK
        assert L.rtbvh_synchronize(self.ctx._h) == expect
        words = buf.cpu().numpy().view(np.uint32)
        assert (words[capacity:] == np.uint32(PATTERN)).all(), "a write behind capacity"
        return self.offsets.cpu().numpy().view(np.uint64), words[:capacity]


class Case:
    """A golden scene built on the GPU under one camera, the two query sets -- the scene's own triangles and
    cross_ref.random_queries -- and their brute-force lists in the build's sort order (once)."""

    def __init__(self, scene, cam, **kw):
        self.name, self.cam = scene, cam
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv, **kw)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.T = len(self.tris)
        self.rank = wr.rank_of(self.ctx.read_sorted()[1])
        self.q = {"own": self.tris, "random": xr.random_queries(self.tris)}
        self.want = {k: xr.brute_cross(self.tris, q, self.rank) for k, q in self.q.items()}

    def total(self, k):
        return int(self.want[k][0][-1])


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. the brute force
@pytest.mark.parametrize("qs", QUERIES)
def test_matches_brute_force(case, qs):
    q, want, total, T = case.q[qs], case.want[qs], case.total(qs), case.T
    n = len(q)
    assert 0 < total < n * T                                      # from the reference: an empty answer cannot pass
    if case.cam == "identity" and qs == "random":
        assert xr.shape_of(want[0]) == xr.IDENTITY_COUNTS[case.name]
    if case.cam == "identity" and qs == "own":
        assert int(xr.without_neighbours(*want, case.scene.indices)[0][-1]) == OWN_COUNTS[case.name]
    ctx = case.ctx
    for what, t in (("host", rt.make_tris(q)), ("device", to_device(q))):
        got = ctx.cross(t, capacity=total)                        # mode 0: one call
        assert tuple(got[0].shape) == (n + 1,) and tuple(got[1].shape) == (total,)
        assert_cross_equal(got, want, what + ", one call")
        assert_cross_equal(ctx.cross(t), want, what + ", SIZES then FILL")
        off = ctx.cross(t, sizes_only=True)
        np.testing.assert_array_equal(host(off) if hasattr(off, "is_cuda") else off, want[0])
        assert_cross_equal(ctx.cross(t, COUNT, capacity=total), want, what + ", COUNT, one call")
        c = ctx.cross_counts()
        assert c["queries"] == n and c["ids"] == total
        assert c["leaf_steps"] >= 2 * total and c["internal_steps"] > 0   # two passes, every member's leaf
        assert_cross_equal(ctx.cross(t, COUNT), want, what + ", COUNT, SIZES then FILL")
        c = ctx.cross_counts()                                    # (the FILL call's)
        assert c["queries"] == n and c["ids"] == total
        assert_cross_equal(ctx.cross(t, SORT, capacity=total), want, what + ", SORT, one call")
        assert_cross_equal(ctx.cross(t, SORT | COUNT), want, what + ", SORT, SIZES then FILL")
        c = ctx.cross_counts()
        assert c["queries"] == n and c["ids"] == total
    p = ctx.cross_pairs(rt.make_tris(q))
    assert p.dtype == np.uint32 and p.shape == (total, 2)
    np.testing.assert_array_equal(p[:, 0], np.repeat(np.arange(n), np.diff(want[0]).astype(np.int64)))
    np.testing.assert_array_equal(p[:, 1], want[1])
    np.testing.assert_array_equal(ctx.cross_pairs(to_device(q)), p)
    for l in cr.lists(*want)[::7]:
        assert (np.diff(case.rank[l]) > 0).all()                  # each list ascending by sort position


# ---------------------------------------------------------------- 2. the tie to the self-collision queries
def test_own_triangles_without_neighbours_are_the_symmetric_collide_lists(case):
    got = case.ctx.cross(rt.make_tris(case.tris))
    off, ids = xr.without_neighbours(*got, case.scene.indices)
    c_off, c_ids = case.ctx.collide(rt.COLLIDE_TRIANGLE | rt.COLLIDE_SYMMETRIC)
    assert int(c_off[-1]) > 0
    assert off.tobytes() == c_off.tobytes() and ids.tobytes() == c_ids.tobytes()


# ---------------------------------------------------------------- 3. the first member
@pytest.mark.parametrize("qs", QUERIES)
def test_cross_first_is_the_head_of_each_list(case, qs):
    q, want = case.q[qs], case.want[qs]
    n = len(q)
    head = xr.first_of(*want)
    found = int((head != NONE).sum())
    assert 0 < found < n or qs == "own"
    ctx = case.ctx
    t, d = rt.make_tris(q), to_device(q)
    got = ctx.cross_first(t)
    assert got.dtype == np.uint32 and got.shape == (n,)
    np.testing.assert_array_equal(got, head)
    np.testing.assert_array_equal(ctx.cross_first(t, SORT), head)
    np.testing.assert_array_equal(host(ctx.cross_first(d)), head)
    np.testing.assert_array_equal(host(ctx.cross_first(d, SORT)), head)
    out = np.full(n, 7, np.uint32)
    assert ctx.cross_first(t, out=out) is out
    np.testing.assert_array_equal(out, head)
    ctx.cross(t, COUNT, sizes_only=True)
    sizes = ctx.cross_counts()
    np.testing.assert_array_equal(ctx.cross_first(t, COUNT), head)
    first = ctx.cross_counts()
    assert first["queries"] == n and first["ids"] == found
    assert 0 < first["leaf_steps"] <= sizes["leaf_steps"] and first["internal_steps"] <= sizes["internal_steps"]
    np.testing.assert_array_equal(ctx.cross_first(t, COUNT | SORT), head)
    assert ctx.cross_counts() == first                            # the same walks in another order


# ---------------------------------------------------------------- 4. capacity
@pytest.mark.parametrize("qs", QUERIES)
def test_capacity_truncates_and_never_writes_behind(case, qs):
    want, total = case.want[qs], case.total(qs)
    dev = Device(case.ctx, case.q[qs])
    for capacity in (total, total - 1, total // 2, 0):
        off, words = dev.run(capacity)
        np.testing.assert_array_equal(off, want[0], err_msg=f"capacity {capacity}")   # offsets[n]: the true total
        np.testing.assert_array_equal(words, want[1][:capacity], err_msg=f"capacity {capacity}")
    off, _ = dev.run(0, null_ids=True)                            # capacity 0: ids may be NULL
    np.testing.assert_array_equal(off, want[0])
    off, _ = dev.run(0, SIZES, null_ids=True)
    np.testing.assert_array_equal(off, want[0])
    half = total // 2                                             # the host entry: min(total, capacity) ids
    off, ids = case.ctx.cross(rt.make_tris(case.q[qs]), capacity=half)
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(ids, want[1][:half])
    assert_cross_equal(case.ctx.cross(rt.make_tris(case.q[qs]), capacity=total + 5), want, "capacity above the total")


def test_fill_over_offsets_of_another_query_set_writes_prefixes(case):
    """The first 512 own triangles under a FILL over the random queries' offsets, and the other way round: segment i
    holds the first ids of query i's list, the rest of it is left alone."""
    n = min(len(case.q["own"]), len(case.q["random"]))
    sets = {k: xr.brute_cross(case.tris, case.q[k][:n], case.rank) for k in QUERIES}
    for src, dst in (("random", "own"), ("own", "random")):
        off_s = sets[src][0]
        off_m, ids_m = sets[dst]
        cnt_s, cnt_m = np.diff(off_s).astype(np.int64), np.diff(off_m).astype(np.int64)
        assert (cnt_s != cnt_m).any() and np.minimum(cnt_s, cnt_m).any()
        total = int(off_s[-1])
        want_words = np.full(total, PATTERN, np.uint32)
        for i in np.nonzero(np.minimum(cnt_s, cnt_m))[0]:
            take = min(cnt_s[i], cnt_m[i])
            want_words[int(off_s[i]):int(off_s[i]) + take] = ids_m[int(off_m[i]):int(off_m[i]) + take]
        dev = Device(case.ctx, case.q[dst][:n])
        for capacity in (total, total // 2):
            off, words = dev.run(capacity, FILL, offsets=off_s)
            np.testing.assert_array_equal(off, off_s)                                 # FILL reads them only
            np.testing.assert_array_equal(words, want_words[:capacity], err_msg=f"capacity {capacity}")


# ---------------------------------------------------------------- 5. special queries
def test_special_queries():
    """One batch on the Test scene: a NaN and an infinite component, a point, needles, a triangle across the whole
    mesh box; one on the flat quad: the exact-touching pair of test_cross_cpu.py beside the non-finite ones."""
    s = fixture_scene("Test")
    wvp, wv = camera("identity")
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        q, names = xr.special_queries(tris)
        want = xr.brute_cross(tris, q, wr.rank_of(ctx.read_sorted()[1]))
        cnt = dict(zip(names, np.diff(want[0]).astype(np.int64).tolist()))
        assert cnt["NaN"] == cnt["infinite"] == cnt["point"] == 0 and cnt["needle"] > 0 and cnt["short needle"] > 0
        assert cnt["spanning"] > 2 * 64                           # far longer than a wave
        head = xr.first_of(*want)
        for t in (rt.make_tris(q), to_device(q)):
            for mode in (0, SORT):
                assert_cross_equal(ctx.cross(t, mode), want, f"mode {mode}")
                assert_cross_equal(ctx.cross(t, mode, capacity=int(want[0][-1])), want, f"mode {mode}, one call")
                got = ctx.cross_first(t, mode)
                np.testing.assert_array_equal(host(got) if hasattr(got, "is_cuda") else got, head)
        assert head[0] == head[1] == head[2] == NONE
        ctx.cross(rt.make_tris(q[:2]), COUNT)                     # no walk for the non-finite ones
        c = ctx.cross_counts()
        assert (c["queries"], c["ids"], c["internal_steps"], c["leaf_steps"]) == (2, 0, 0, 0)
    v, idx, tq, members = xr.touching_case()
    nan = tq[0].copy()
    nan[0, 0] = np.nan
    inf = tq[0].copy()
    inf[2, 2] = np.inf
    q = np.stack([tq[0], nan, tq[1], inf, tq[0]])
    with built(cr.scene_of(v, idx), wvp, wv) as ctx:
        tris = rw.clip_triangles(ctx_vertices(v), idx, wvp)
        want = xr.brute_cross(tris, q, wr.rank_of(ctx.read_sorted()[1]))
        assert cr.lists(*want)[0].tolist() == members[0] and np.diff(want[0]).tolist() == [1, 0, 0, 0, 1]
        assert_cross_equal(ctx.cross(rt.make_tris(q)), want)
        assert_cross_equal(ctx.cross(to_device(q), capacity=2), want)
        np.testing.assert_array_equal(ctx.cross_first(rt.make_tris(q)), [0, NONE, NONE, NONE, 0])


def ctx_vertices(v):
    """Bare positions as the (V, 8) vertex records clip_triangles reads."""
    out = np.zeros((len(v), 8), np.float32)
    out[:, :3] = v
    return out


# ---------------------------------------------------------------- 6. a deep tree, the stack limit
def fan_case(stack_limit=0):
    s = cr.thick_fan()
    wvp, wv = camera("identity")
    ctx = built(s, wvp, wv, stack_limit=stack_limit)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    q = xr.fan_queries()
    return ctx, q, xr.brute_cross(tris, q, wr.rank_of(ctx.read_sorted()[1]))


def test_fan_walks_past_the_lds_part_of_the_stack():
    """tests/test_cross_cpu.py shows that these walks store entries at and past 16, the LDS part."""
    ctx, q, want = fan_case()
    with ctx:
        assert int(want[0][-1]) > 64 * len(q)
        assert_cross_equal(ctx.cross(rt.make_tris(q), capacity=int(want[0][-1])), want, "one call")
        assert_cross_equal(ctx.cross(to_device(q)), want, "SIZES then FILL")
        np.testing.assert_array_equal(ctx.cross_first(rt.make_tris(q)), xr.first_of(*want))


def test_stack_limit_reports_overflow_and_keeps_genuine_ids():
    ctx, q, want = fan_case(stack_limit=8)
    with ctx:
        cap = int(want[0][-1])
        dev = Device(ctx, q)
        off, words = dev.run(cap, expect=OVERFLOW)      # (its guard region: untouched)
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK   # once per new overflow
        # offsets are consistent, and a walk that lost subtrees lists a subsequence of the query's true list
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
        total = int(off[-1])
        assert 0 < total < cap
        assert (words[total:] == PATTERN).all()         # the fill pass wrote what the sizes pass counted, no more
        assert (words[:total] < len(ctx.read_sorted()[1])).all()    # ... and no less (an id is below T)
        for k in range(len(q)):
            g = words[int(off[k]):int(off[k + 1])]
            t = want[1][int(want[0][k]):int(want[0][k + 1])]
            idx = {w: i for i, w in enumerate(t.tolist())}
            where = [idx.get(w, -1) for w in g.tolist()]
            assert -1 not in where and where == sorted(where), k
        # the two-call form loses the same ids
        off2, _ = dev.run(0, SIZES, null_ids=True, expect=OVERFLOW)
        np.testing.assert_array_equal(off2, off)
        _, words2 = dev.run(cap, FILL, offsets=off, expect=OVERFLOW)
        np.testing.assert_array_equal(words2, words)
        # cross_first: the head of the shortened list, and the overflow reported at the next synchronising call
        import torch
        first = torch.full((len(q),), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert rt.lib().rtbvh_cross_first_async(ctx._h, vp(dev.tris), len(q), vp(first), 0, None) == OK
        assert rt.lib().rtbvh_synchronize(ctx._h) == OVERFLOW
        np.testing.assert_array_equal(host(first), xr.first_of(off, words[:total]))


# ---------------------------------------------------------------- 7. both tree forms
def test_records_and_node_box_trees_agree():
    """A certified-only context's multi-kernel build writes the topology and node boxes, a plain one the records:
    the same bytes and the same counted steps."""
    cases = [(fixture_scene("Image_Test"), 3072), (rt.synthetic(12_000, seed=0x5EED0004), 12_000)]
    wvp, wv = rt.camera_reference(W, H)
    for s, T in cases:
        with built(s, wvp, wv, flags=rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD) as nbox, built(s, wvp, wv) as plain:
            sa, sp = nbox.read_sorted()[1], plain.read_sorted()[1]
            np.testing.assert_array_equal(sa, sp)
            tris = rw.clip_triangles(s.vertices, s.indices, wvp)
            assert len(tris) == T
            q = xr.random_queries(tris, 768, seed=8)
            want = xr.brute_cross(tris, q, wr.rank_of(sp))
            total = int(want[0][-1])
            assert total > 0
            head = xr.first_of(*want)
            t = rt.make_tris(q)
            lo, hi = q.min(1), q.max(1)
            for c in (nbox, plain):                 # a counting query of another kind first: its counts must survive
                c.overlap(lo, hi, rt.OVERLAP_COUNT)
            before = plain.overlap_counts()
            for mode in (COUNT, COUNT | SORT):
                a, p = (c.cross(t, mode, capacity=total) for c in (nbox, plain))
                assert a[0].tobytes() == p[0].tobytes() and a[1].tobytes() == p[1].tobytes()
                assert_cross_equal(a, want, f"mode {mode}")
                ca, cp = nbox.cross_counts(), plain.cross_counts()
                assert ca == cp                     # the same visits on both forms
                assert ca["queries"] == len(q) and ca["ids"] == total
                fa, fp = (c.cross_first(t, mode) for c in (nbox, plain))
                assert fa.tobytes() == fp.tobytes()
                np.testing.assert_array_equal(fa, head)
                assert nbox.cross_counts() == plain.cross_counts()
                assert plain.overlap_counts() == before and nbox.overlap_counts() == before


# ---------------------------------------------------------------- 8. a moving mesh
@pytest.mark.parametrize("flags", [0, rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD], ids=["records", "node boxes"])
def test_after_update_and_refit(flags):
    s = fixture_scene("Image_Test")
    wvp, wv = rt.camera_reference(W, H)
    P = deform(s.vertices[:, :3], 0.7)
    v = s.vertices.copy()
    v[:, :3] = P
    still_tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    moved_tris = rw.clip_triangles(v, s.indices, wvp)
    q = xr.random_queries(still_tris)
    t, d = rt.make_tris(q), to_device(q)
    L = rt.lib()
    with built(s, wvp, wv, flags=flags) as ctx:
        order = ctx.read_sorted()[1].copy()
        still = xr.brute_cross(still_tris, q, wr.rank_of(order))
        moved = xr.brute_cross(moved_tris, q, wr.rank_of(order))
        assert not (np.array_equal(still[0], moved[0]) and np.array_equal(still[1], moved[1]))
        assert_cross_equal(ctx.cross(t), still, "before")
        ctx.update_vertices(P)
        for call in (lambda: ctx.cross(t), lambda: ctx.cross(d), lambda: ctx.cross_first(t), lambda: ctx.cross_first(d)):
            with pytest.raises(rt.RtbvhError) as e:
                call()
            assert e.value.status == NOT_READY
        ctx.refit()
        np.testing.assert_array_equal(ctx.read_sorted()[1], order)   # a refit keeps the order
        assert_cross_equal(ctx.cross(t), moved, "after the refit")
        assert_cross_equal(ctx.cross(d, SORT), moved, "after the refit, device")
        np.testing.assert_array_equal(ctx.cross_first(t), xr.first_of(*moved))
        assert L.rtbvh_synchronize(ctx._h) == OK


# ---------------------------------------------------------------- 9. plumbing
def test_errors_and_empty_inputs():
    import torch
    L = rt.lib()
    d = load_scene_fixture("Rect")
    wvp, wv = rt.camera_reference(W, H)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    q = xr.random_queries(tris, 12)
    t = rt.make_tris(q)
    off = np.zeros(13, np.uint64)
    ids = np.zeros(64, np.uint32)
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(wvp, wv)
        h = ctx._h
        dt = to_device(q)
        doff = torch.full((13,), -1, dtype=torch.int64, device="cuda")
        dids = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        # n == 0 before a build: OK, nothing touched (offsets[0] = 0 is written only where offsets are given)
        assert L.rtbvh_cross_async(h, None, 0, None, None, 0, 0, None) == OK
        assert L.rtbvh_cross_async(h, vp(dt), 0, None, vp(dids), 64, FILL, None) == OK
        assert L.rtbvh_cross_first_async(h, None, 0, None, 0, None) == OK
        assert L.rtbvh_cross_first_async(h, vp(dt), 0, vp(dids), 0, None) == OK
        assert L.rtbvh_cross_host(h, None, 0, None, None, 0, 0) == OK
        assert L.rtbvh_cross_first_host(h, None, 0, None, 0) == OK
        ctx.synchronize()
        assert (doff.cpu().numpy() == -1).all() and (dids.cpu().numpy() == -1).all()
        assert L.rtbvh_cross_async(h, vp(dt), 0, vp(doff), None, 0, 0, None) == OK
        ctx.synchronize()
        assert doff.cpu().numpy().tolist() == [0] + [-1] * 12
        doff.fill_(-1)
        off[0] = 9
        assert L.rtbvh_cross_host(h, vp(t), 0, vp(off), None, 0, 0) == OK and off[0] == 0
        assert len(ctx.cross(t[:0])[1]) == 0 and ctx.cross(t[:0])[0].tolist() == [0]
        assert ctx.cross_first(t[:0]).shape == (0,)
        for call in (lambda: ctx.cross(t), lambda: ctx.cross_first(t), ctx.cross_counts):
            with pytest.raises(rt.RtbvhError) as e:
                call()
            assert e.value.status == NOT_READY
        ctx.build()
        for mode in (1, 8, 64, 128, 1 << 8, 1 << 31, SIZES | FILL, SIZES | FILL | SORT, COUNT | 1):
            assert L.rtbvh_cross_async(h, vp(dt), 12, vp(doff), vp(dids), 64, mode, None) == INVALID_ARG, mode
            assert L.rtbvh_cross_host(h, vp(t), 12, vp(off), vp(ids), 64, mode) == INVALID_ARG, mode
        for mode in (1, 8, SIZES, FILL, 64, 1 << 31, SORT | SIZES):
            assert L.rtbvh_cross_first_async(h, vp(dt), 12, vp(dids), mode, None) == INVALID_ARG, mode
            assert L.rtbvh_cross_first_host(h, vp(t), 12, vp(ids), mode) == INVALID_ARG, mode
        big = 1 << 31
        assert L.rtbvh_cross_async(h, vp(dt), big, vp(doff), vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_cross_host(h, vp(t), big, vp(off), vp(ids), 64, 0) == INVALID_ARG
        assert L.rtbvh_cross_first_async(h, vp(dt), big, vp(dids), 0, None) == INVALID_ARG
        assert L.rtbvh_cross_first_host(h, vp(t), big, vp(ids), 0) == INVALID_ARG
        assert L.rtbvh_cross_async(h, None, 12, vp(doff), vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_cross_async(h, vp(dt), 12, None, vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_cross_async(h, vp(dt), 12, vp(doff), None, 64, 0, None) == INVALID_ARG
        assert L.rtbvh_cross_async(h, vp(dt), 12, vp(doff), None, 64, FILL, None) == INVALID_ARG
        assert L.rtbvh_cross_host(h, None, 12, vp(off), vp(ids), 64, 0) == INVALID_ARG
        assert L.rtbvh_cross_host(h, vp(t), 12, None, vp(ids), 64, 0) == INVALID_ARG
        assert L.rtbvh_cross_host(h, vp(t), 12, vp(off), None, 64, 0) == INVALID_ARG
        assert L.rtbvh_cross_first_async(h, None, 12, vp(dids), 0, None) == INVALID_ARG
        assert L.rtbvh_cross_first_async(h, vp(dt), 12, None, 0, None) == INVALID_ARG
        assert L.rtbvh_cross_first_host(h, None, 12, vp(ids), 0) == INVALID_ARG
        assert L.rtbvh_cross_first_host(h, vp(t), 12, None, 0) == INVALID_ARG
        assert L.rtbvh_cross_counts(h, None) == INVALID_ARG
        ctx.synchronize()
        assert (doff.cpu().numpy() == -1).all() and (dids.cpu().numpy() == -1).all()   # nothing was written
        assert not off.any() and not ids.any()
        # NULL ids are fine with capacity 0 and under SIZES
        want = xr.brute_cross(tris, q, wr.rank_of(ctx.read_sorted()[1]))
        assert int(want[0][-1]) > 0
        assert L.rtbvh_cross_async(h, vp(dt), 12, vp(doff), None, 0, 0, None) == OK
        ctx.synchronize()
        np.testing.assert_array_equal(host(doff), want[0])
        doff.fill_(-1)
        assert L.rtbvh_cross_async(h, vp(dt), 12, vp(doff), None, 64, SIZES, None) == OK
        ctx.synchronize()
        np.testing.assert_array_equal(host(doff), want[0])
        with pytest.raises(rt.RtbvhError) as e:
            ctx.cross_counts()                      # still no counting triangle query
        assert e.value.status == NOT_READY
        assert_cross_equal(ctx.cross(t), want)      # and the context still answers
        ctx.update_vertices(d["vertices"][:, :3].copy())
        assert L.rtbvh_cross_async(h, vp(dt), 12, vp(doff), vp(dids), 64, 0, None) == NOT_READY
        assert L.rtbvh_cross_host(h, vp(t), 12, vp(off), vp(ids), 64, 0) == NOT_READY
        assert L.rtbvh_cross_first_async(h, vp(dt), 12, vp(dids), 0, None) == NOT_READY
        assert L.rtbvh_cross_first_host(h, vp(t), 12, vp(ids), 0) == NOT_READY
        ctx.refit()
        assert_cross_equal(ctx.cross(t, SORT), want)
        ctx.synchronize()


def test_a_side_stream_between_an_overlap_and_a_collide_call():
    import torch
    c = Case("Test", "reference")
    with c.ctx:
        q = c.q["random"]
        want, total = c.want["random"], c.total("random")
        lo, hi = q.min(1), q.max(1)
        boxes = torch.from_numpy(rt.make_boxes(lo, hi).view(np.float32).reshape(-1, 8)).cuda()
        box_want = ovr.brute_overlap(c.tris, lo, hi, c.rank)
        col_want = cr.brute_collide(c.tris, c.scene.indices, c.rank, True)
        d = to_device(q)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        b = c.ctx.overlap(boxes, capacity=int(box_want[0][-1]), stream=s2)
        o1, r1 = c.ctx.cross(d, COUNT, capacity=total + 7, stream=s1)
        col = c.ctx.collide(rt.COLLIDE_TRIANGLE, stream=s2, device=True)
        f1 = c.ctx.cross_first(d, SORT, stream=s1)
        o2, r2 = c.ctx.cross(d, stream=s1)                         # capacity=None: sized from the total
        s1.synchronize()
        s2.synchronize()
        assert o1.is_cuda and o1.dtype == torch.int64 and tuple(o1.shape) == (len(q) + 1,)
        assert r1.is_cuda and r1.dtype == torch.int32 and tuple(r1.shape) == (total + 7,)
        assert f1.is_cuda and f1.dtype == torch.int32 and tuple(f1.shape) == (len(q),)
        assert_cross_equal((o1, r1[:total]), want, "one call on a side stream")
        assert_cross_equal((o2, r2), want, "SIZES then FILL on a side stream")
        np.testing.assert_array_equal(host(f1), xr.first_of(*want))
        assert_cross_equal(b, box_want, "the overlap call beside it")
        assert_cross_equal(col, col_want, "the collide call beside it")
        with torch.cuda.stream(s1):                                # a side stream made current
            o3, r3 = c.ctx.cross(d, SORT, capacity=total)
            f3 = c.ctx.cross_first(d)
        s1.synchronize()
        assert_cross_equal((o3, r3), want, "the current stream")
        np.testing.assert_array_equal(host(f3), xr.first_of(*want))
        c.ctx.synchronize()


def test_a_scene_of_one_triangle_is_tested_at_the_leaf():
    a = np.array([[-3, -2, 0], [4, -1, 1], [0, 5, 2]], np.float32)
    b = np.array([[0, 0, -3], [1, 1, 4], [0.5, 2, -2]], np.float32)           # pierces a
    far = b + np.float32(40)
    near = b + np.float32([0, 0, 8])                                          # its box misses a's in z
    q = np.stack([b, far, near, a])
    for cam in CAMERAS:
        wvp, wv = camera(cam)
        with built(cr.scene_of(a, np.arange(3)), wvp, wv) as ctx:
            tris = rw.clip_triangles(ctx_vertices(a), np.arange(3), wvp)
            qq = q if cam == "identity" else np.concatenate([tris, xr.random_queries(tris, 16)])
            want = xr.brute_cross(tris, qq, np.zeros(1, np.int64))
            if cam == "identity":
                assert np.diff(want[0]).tolist()[:3] == [1, 0, 0]
            for t in (rt.make_tris(qq), to_device(qq)):
                assert_cross_equal(ctx.cross(t), want, cam)
                assert_cross_equal(ctx.cross(t, SORT | COUNT, capacity=int(want[0][-1])), want, cam)
                got = ctx.cross_first(t)
                np.testing.assert_array_equal(host(got) if hasattr(got, "is_cuda") else got, xr.first_of(*want))
            c = ctx.cross_counts()
            assert c["queries"] == len(qq) and c["internal_steps"] == 0
