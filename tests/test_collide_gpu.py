"""Self-collision queries on the GPU (rtbvh_collide_async / rtbvh_collide_host through Context.collide and the raw
entries) against the brute force over all pairs of triangles (tests/collide_ref.py), listed by the build's sort order
(Context.read_sorted).  The set and its order are specified independently of the walk, in every mode (leaf boxes
only or with the segment-triangle tests, a pair listed once or by both triangles), so every comparison is bit-exact:
offsets and ids as integers."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import collide_ref as cr
from tests import ray_walk_ref as rw
from tests import within_ref as wr
from tests.conftest import load_scene_fixture
from tests.test_dynamic_gpu import deform
from tests.test_query_gpu import random_rays

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Rect", "Test", "Image_Test"]
CAMERAS = ["reference", "identity"]
OK, NOT_READY, INVALID_ARG, OVERFLOW = (rt._lib.OK, rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG,
                                        rt._lib.ERR_STACK_OVERFLOW)
SIZES, FILL, COUNT, TRI, SYM = (rt.COLLIDE_SIZES, rt.COLLIDE_FILL, rt.COLLIDE_COUNT, rt.COLLIDE_TRIANGLE,
                                rt.COLLIDE_SYMMETRIC)
MODES = [0, TRI, SYM, TRI | SYM]
MODE_IDS = ["boxes", "triangles", "boxes-symmetric", "triangles-symmetric"]
IDENTITY_COUNTS = {"Rect": [54, 48, 31], "Test": [15_530, 8_082, 4_406], "Image_Test": [26_064, 9_090, 1_465]}
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


def brute(tris, indices, rank, stages=None):
    """{mode: (offsets, ids)} of the four modes, from one pass over the pairs; `stages`: collide_ref's counts."""
    st = [[], []]
    pairs = {0: cr.member_pairs(tris, indices, False, stages=st[0]), TRI: cr.member_pairs(tris, indices, True, stages=st[1])}
    if stages is not None:
        stages[:] = st[1]
    return {m: cr.csr(pairs[m & TRI], rank, len(tris), bool(m & SYM)) for m in MODES}


def assert_collide_equal(got, want, what=""):
    off, ids = got
    assert off.dtype == np.uint64 and ids.dtype == np.uint32, what
    np.testing.assert_array_equal(off, want[0], err_msg=what + " offsets")
    np.testing.assert_array_equal(ids, want[1], err_msg=what + " ids")


def vp(a):
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


class Device:
    """The raw device entry on the context stream with torch tensors for memory: an ids buffer of capacity + GUARD
    words filled with PATTERN, offsets and ids back."""

    def __init__(self, ctx, T):
        import torch
        self.torch, self.ctx, self.T = torch, ctx, T
        self.offsets = torch.full((T + 1,), -1, dtype=torch.int64, device="cuda")

    def run(self, capacity, mode=0, offsets=None, null_ids=False, expect=OK):
        torch = self.torch
        if offsets is not None:
            self.offsets.copy_(torch.from_numpy(offsets.view(np.int64)))
        buf = torch.full((capacity + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        L = rt.lib()
        st = L.rtbvh_collide_async(self.ctx._h, vp(self.offsets), None if null_ids else vp(buf), capacity, mode, None)
        assert st == OK
        assert L.rtbvh_synchronize(self.ctx._h) == expect
        words = buf.cpu().numpy().view(np.uint32)
        assert (words[capacity:] == np.uint32(PATTERN)).all(), "a write behind capacity"
        return self.offsets.cpu().numpy().view(np.uint64), words[:capacity]


class Case:
    """A golden scene built on the GPU under one camera and the brute-force lists of the four modes in the build's
    sort order (once)."""

    def __init__(self, scene, cam, **kw):
        self.name, self.cam = scene, cam
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv, **kw)
        self.tris = rw.clip_triangles(self.scene.vertices, self.scene.indices, self.wvp)
        self.T = len(self.tris)
        self.rank = wr.rank_of(self.ctx.read_sorted()[1])
        self.stages = []
        self.want = brute(self.tris, self.scene.indices, self.rank, self.stages)

    def total(self, m):
        return int(self.want[m][0][-1])


@pytest.fixture(scope="module", params=[(s, c) for s in SCENES for c in CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. the brute force
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_matches_brute_force(case, m):
    want, total, T = case.want[m], case.total(m), case.T
    nb, nn, nx = case.stages                                     # from the reference: an empty answer cannot pass
    assert 0 < case.total(TRI) < case.total(0) < T * (T - 1) // 2 and nn < nb
    assert case.total(m | SYM) == 2 * case.total(m & ~SYM) and (nn, nx) == (case.total(0), case.total(TRI))
    if case.cam == "identity":
        assert case.stages == IDENTITY_COUNTS[case.name]
    got = case.ctx.collide(m, capacity=total)                    # mode 0: one call
    assert got[0].shape == (T + 1,) and got[1].shape == (total,)
    assert_collide_equal(got, want, "one call")
    assert_collide_equal(case.ctx.collide(m), want, "SIZES then FILL")
    np.testing.assert_array_equal(case.ctx.collide(m, sizes_only=True), want[0])
    assert_collide_equal(case.ctx.collide(m | COUNT, capacity=total), want, "COUNT, one call")
    c = case.ctx.collide_counts()
    assert c["triangles"] == T and c["entries"] == total
    assert c["leaf_steps"] >= 2 * total and c["internal_steps"] > 0   # two passes, every partner's leaf
    assert_collide_equal(case.ctx.collide(m | COUNT), want, "COUNT, SIZES then FILL")
    c = case.ctx.collide_counts()                                # (the FILL call's)
    assert c["triangles"] == T and c["entries"] == total
    if not m & SYM:
        p = case.ctx.collide_pairs(triangle=bool(m & TRI))
        assert p.dtype == np.uint32 and p.shape == (total, 2)
        np.testing.assert_array_equal(p[:, 0], np.repeat(np.arange(T), np.diff(want[0]).astype(np.int64)))
        np.testing.assert_array_equal(p[:, 1], want[1])
        assert (case.rank[p[:, 0]] < case.rank[p[:, 1]]).all()


@pytest.mark.parametrize("tri", [0, TRI], ids=["boxes", "triangles"])
def test_symmetric_lists_are_the_default_ones_and_their_mirror(case, tri):
    off_d, ids_d = case.ctx.collide(tri)
    off_s, ids_s = case.ctx.collide(tri | SYM)
    owner = np.repeat(np.arange(case.T), np.diff(off_d).astype(np.int64))
    assert_collide_equal((off_s, ids_s), cr.csr((owner, ids_d.astype(np.int64)), case.rank, case.T, True))
    for l in cr.lists(off_s, ids_s)[::7]:
        assert (np.diff(case.rank[l]) > 0).all()               # each list ascending by sort position


# ---------------------------------------------------------------- 2. capacity
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_capacity_truncates_and_never_writes_behind(case, m):
    want, total = case.want[m], case.total(m)
    dev = Device(case.ctx, case.T)
    for capacity in (total, total // 2, 1, 0):
        off, words = dev.run(capacity, m)
        np.testing.assert_array_equal(off, want[0], err_msg=f"capacity {capacity}")
        np.testing.assert_array_equal(words, want[1][:capacity], err_msg=f"capacity {capacity}")
    off, _ = dev.run(0, m, null_ids=True)                        # capacity 0: ids may be NULL
    np.testing.assert_array_equal(off, want[0])
    off, _ = dev.run(0, m | SIZES, null_ids=True)
    np.testing.assert_array_equal(off, want[0])
    half = total // 2                                            # the host entry: min(total, capacity) ids
    off, ids = case.ctx.collide(m, capacity=half)
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(ids, want[1][:half])
    assert_collide_equal(case.ctx.collide(m, capacity=total + 5), want, "capacity above the total")


@pytest.mark.parametrize("sym", [0, SYM], ids=["default", "symmetric"])
def test_fill_over_offsets_of_another_mode_writes_prefixes(case, sym):
    """The offsets of the TRIANGLE lists under a boxes-mode FILL: segment i holds the first ids of triangle i's
    boxes-mode list.  The other way round: the TRIANGLE lists with the rest of each segment left alone."""
    for src, m in ((TRI | sym, sym), (sym, TRI | sym)):
        off_s = case.want[src][0]
        off_m, ids_m = case.want[m]
        cnt_s, cnt_m = np.diff(off_s).astype(np.int64), np.diff(off_m).astype(np.int64)
        assert (cnt_s != cnt_m).any()
        total = int(off_s[-1])
        want_words = np.full(total, PATTERN, np.uint32)
        for i in np.nonzero(np.minimum(cnt_s, cnt_m))[0]:
            take = min(cnt_s[i], cnt_m[i])
            want_words[int(off_s[i]):int(off_s[i]) + take] = ids_m[int(off_m[i]):int(off_m[i]) + take]
        dev = Device(case.ctx, case.T)
        for capacity in (total, total // 2):
            off, words = dev.run(capacity, m | FILL, offsets=off_s)
            np.testing.assert_array_equal(off, off_s)                                 # FILL reads them only
            np.testing.assert_array_equal(words, want_words[:capacity], err_msg=f"capacity {capacity}")


# ---------------------------------------------------------------- 3. tiny and empty scenes
def tiny_cases():
    """name -> (vertices, indices): what each expects comes from the brute force, asserted in the test."""
    a = np.array([[-3, -2, 0], [4, -1, 1], [0, 5, 2]], np.float32)
    b = np.array([[0, 0, -3], [1, 1, 4], [0.5, 2, -2]], np.float32)           # pierces a
    nan = np.concatenate([a, b, b + np.float32(0.25)])
    nan[4, 1] = np.nan
    flat = np.concatenate([a, b, np.array([[0, 0, -3], [0, 0, -3], [1, 1, 4]], np.float32)])   # b's edge, twice
    return {"one": (a, np.arange(3)), "two crossing": (np.concatenate([a, b]), np.arange(6)),
            "two sharing a vertex index": (np.concatenate([a, b]), np.array([0, 1, 2, 3, 4, 0])),
            "a NaN vertex": (nan, np.arange(9)), "a degenerate triangle": (flat, np.arange(9))}


@pytest.mark.parametrize("name", list(tiny_cases()))
@pytest.mark.parametrize("cam", CAMERAS)
def test_tiny_scenes(name, cam):
    v, idx = tiny_cases()[name]
    s = cr.scene_of(v, idx)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        want = brute(tris, idx, wr.rank_of(ctx.read_sorted()[1]))
        totals = [int(want[m][0][-1]) for m in MODES]
        if cam == "identity":
            expect = {"one": [0, 0, 0, 0], "two crossing": [1, 1, 2, 2], "two sharing a vertex index": [0, 0, 0, 0],
                      "a NaN vertex": [2, 1, 4, 2], "a degenerate triangle": [3, 2, 6, 4]}[name]
            assert totals == expect
        for m in MODES:
            assert_collide_equal(ctx.collide(m), want[m], MODE_IDS[MODES.index(m)])
            assert_collide_equal(ctx.collide(m, capacity=totals[MODES.index(m)] + 3), want[m], "one call")
        if name == "one":
            assert ctx.collide()[0].tolist() == [0, 0]


# ---------------------------------------------------------------- 4. both tree forms, and the leaf-range skip
def test_records_and_node_box_trees_agree():
    """A certified-only context's multi-kernel build writes the topology and node boxes, a plain one the records:
    the same bytes.  The default walk prunes by leaf range, the symmetric one cannot: its steps say so, and the
    default lists are the symmetric ones' upper halves."""
    cases = [(fixture_scene("Image_Test"), 3072), (rt.synthetic(12_000, seed=0x5EED0004), 12_000)]
    wvp, wv = rt.camera_reference(W, H)
    for s, T in cases:
        with built(s, wvp, wv, flags=rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD) as nbox, built(s, wvp, wv) as plain:
            sa, sp = nbox.read_sorted()[1], plain.read_sorted()[1]
            np.testing.assert_array_equal(sa, sp)
            tris = rw.clip_triangles(s.vertices, s.indices, wvp)
            assert len(tris) == T
            want = brute(tris, s.indices, wr.rank_of(sp))
            assert int(want[TRI][0][-1]) > 0
            o, d = random_rays(plain.read_bvh(), 500, seed=3)
            rays = rt.make_rays(o, d)
            for c in (nbox, plain):                 # a counting query of another kind first: its counts must survive
                c.query(rays, rt.QUERY_COUNT)
            before = plain.query_counts()
            steps = {}
            for m in MODES:
                total = int(want[m][0][-1])
                a, p = (c.collide(m | COUNT, capacity=total) for c in (nbox, plain))
                np.testing.assert_array_equal(a[0], p[0])
                np.testing.assert_array_equal(a[1], p[1])
                assert_collide_equal(a, want[m], MODE_IDS[MODES.index(m)])
                ca, cp = nbox.collide_counts(), plain.collide_counts()
                assert ca == cp                     # the same visits on both forms
                assert ca["triangles"] == T and ca["entries"] == total
                steps[m] = ca
                assert plain.query_counts() == before and nbox.query_counts() == before
            print(f"T = {T}: steps per triangle (two passes)",
                  {MODE_IDS[MODES.index(m)]: (v["internal_steps"] / T, v["leaf_steps"] / T) for m, v in steps.items()})
            for tri in (0, TRI):
                assert steps[tri]["leaf_steps"] < steps[tri | SYM]["leaf_steps"]
                assert steps[tri]["internal_steps"] < steps[tri | SYM]["internal_steps"]


# ---------------------------------------------------------------- 5. past one workgroup's build, past the grid's lanes
@pytest.mark.parametrize("cells", [2_250, 132_000], ids=["9,000 triangles", "528,000 triangles"])
def test_lattice_of_crossing_quads(cells):
    """Separated cells of one crossing pair of quads each: only triangles of one cell can meet, so the lists are
    known in closed form.  528,000 triangles: more than the 524,288 lanes of the largest persistent grid (refills,
    258 scan tiles)."""
    v, idx = cr.lattice(cells)
    T = 4 * cells
    wvp, wv = camera("identity")
    with built(cr.scene_of(v, idx), wvp, wv) as ctx:
        rank = wr.rank_of(ctx.read_sorted()[1])
        pairs = cr.lattice_pairs(cells)
        for m in ((TRI, SYM) if cells > 10_000 else MODES):
            want = cr.csr(pairs, rank, T, bool(m & SYM))
            assert int(want[0][-1]) == (8 if m & SYM else 4) * cells
            assert_collide_equal(ctx.collide(m, capacity=int(want[0][-1])), want, MODE_IDS[MODES.index(m)])
        assert_collide_equal(ctx.collide(TRI | SYM | COUNT), cr.csr(pairs, rank, T, True), "COUNT")
        c = ctx.collide_counts()
        assert c["triangles"] == T and c["entries"] == 8 * cells


# ---------------------------------------------------------------- 6. a deep tree, the stack limit
def fan_case(stack_limit=0):
    s = cr.thick_fan()
    wvp, wv = camera("identity")
    ctx = built(s, wvp, wv, stack_limit=stack_limit)
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    return ctx, tris, brute(tris, s.indices, wr.rank_of(ctx.read_sorted()[1]))


def test_fan_walks_past_the_lds_part_of_the_stack():
    """tests/test_collide_cpu.py shows that these walks store entries at and past 16, the LDS part."""
    ctx, tris, want = fan_case()
    with ctx:
        assert int(want[0][0][-1]) > len(tris)
        for m in MODES:
            assert_collide_equal(ctx.collide(m, capacity=int(want[m][0][-1])), want[m], MODE_IDS[MODES.index(m)])
            assert_collide_equal(ctx.collide(m), want[m], "SIZES then FILL")


@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_stack_limit_reports_overflow_and_keeps_genuine_ids(m):
    ctx, tris, wants = fan_case(stack_limit=8)
    with ctx:
        want = wants[m]
        cap = int(want[0][-1])
        dev = Device(ctx, len(tris))
        off, words = dev.run(cap, m, expect=OVERFLOW)   # (its guard region: untouched)
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK   # once per new overflow
        # offsets are consistent, and a walk that lost subtrees lists a subsequence of the triangle's true list
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
        total = int(off[-1])
        assert 0 < total < cap
        assert (words[total:] == PATTERN).all()     # the fill pass wrote what the sizes pass counted, no more
        assert (words[:total] < len(tris)).all()    # ... and no less (an id is below T)
        for k in range(len(tris)):
            g = words[int(off[k]):int(off[k + 1])]
            t = want[1][int(want[0][k]):int(want[0][k + 1])]
            idx = {w: i for i, w in enumerate(t.tolist())}
            where = [idx.get(w, -1) for w in g.tolist()]
            assert -1 not in where and where == sorted(where), k


# ---------------------------------------------------------------- 7. a moving mesh
@pytest.mark.parametrize("flags", [0, rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD], ids=["records", "node boxes"])
def test_after_update_refit_and_rebuild(flags):
    s = fixture_scene("Image_Test")
    wvp, wv = rt.camera_reference(W, H)
    P = deform(s.vertices[:, :3], 0.7)
    v = s.vertices.copy()
    v[:, :3] = P
    tris = rw.clip_triangles(v, s.indices, wvp)
    with built(s, wvp, wv, flags=flags) as ctx:
        old_order = ctx.read_sorted()[1].copy()
        still = brute(rw.clip_triangles(s.vertices, s.indices, wvp), s.indices, wr.rank_of(old_order))
        moved = brute(tris, s.indices, wr.rank_of(old_order))
        for m in (TRI, SYM):
            # the deformation changes the member set
            assert not (np.array_equal(still[m][0], moved[m][0]) and np.array_equal(still[m][1], moved[m][1]))
            assert_collide_equal(ctx.collide(m), still[m], "before")
            ctx.update_vertices(P)
            with pytest.raises(rt.RtbvhError) as e:
                ctx.collide(m)
            assert e.value.status == NOT_READY
            ctx.refit()
            np.testing.assert_array_equal(ctx.read_sorted()[1], old_order)   # a refit keeps the order
            assert_collide_equal(ctx.collide(m), moved[m], "after the refit")
            ctx.build()   # another tree over the same geometry: the same set, in the new order
            new_order = ctx.read_sorted()[1].copy()
            assert_collide_equal(ctx.collide(m), brute(tris, s.indices, wr.rank_of(new_order))[m], "after the rebuild")
            ctx.update_vertices(s.vertices[:, :3].copy())   # back to the scene's geometry for the next mode
            ctx.build()
            old_order = ctx.read_sorted()[1].copy()
            still = brute(rw.clip_triangles(s.vertices, s.indices, wvp), s.indices, wr.rank_of(old_order))
            moved = brute(tris, s.indices, wr.rank_of(old_order))


# ---------------------------------------------------------------- 8. device tensors and streams
def test_device_tensors_on_two_streams():
    import torch
    c = Case("Test", "reference")
    with c.ctx:
        T = c.T
        want, want_t = c.want[SYM], c.want[TRI]
        total = c.total(SYM)
        o, dd = random_rays(c.ctx.read_bvh(), 4096, seed=5)
        rays = torch.from_numpy(rt.make_rays(o, dd).view(np.float32).reshape(-1, 8)).cuda()
        hits_want = c.ctx.query(rt.make_rays(o, dd))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        o1, r1 = c.ctx.collide(SYM | COUNT, capacity=total + 7, stream=s1, device=True)   # back to back, two streams
        hits = c.ctx.query(rays, stream=s2)
        o2, r2 = c.ctx.collide(TRI, stream=s1, device=True)                     # capacity=None: sized from the total
        s1.synchronize()
        s2.synchronize()
        assert o1.is_cuda and o1.dtype == torch.int64 and tuple(o1.shape) == (T + 1,)
        assert r1.is_cuda and r1.dtype == torch.int32 and tuple(r1.shape) == (total + 7,)
        np.testing.assert_array_equal(o1.cpu().numpy().view(np.uint64), want[0])
        np.testing.assert_array_equal(r1[:total].cpu().numpy().view(np.uint32), want[1])
        assert tuple(r2.shape) == (c.total(TRI),)
        np.testing.assert_array_equal(o2.cpu().numpy().view(np.uint64), want_t[0])
        np.testing.assert_array_equal(r2.cpu().numpy().view(np.uint32), want_t[1])
        np.testing.assert_array_equal(hits.cpu().numpy().view(np.uint32), hits_want.view(np.uint32).reshape(-1, 4))
        assert c.ctx.collide_counts()["triangles"] == T and c.ctx.collide_counts()["entries"] == total
        # the current stream (torch's default one) and a side stream made current; capacity given and not
        o3, r3 = c.ctx.collide(TRI, device=True)
        np.testing.assert_array_equal(o3.cpu().numpy(), o2.cpu().numpy())
        np.testing.assert_array_equal(r3.cpu().numpy(), r2.cpu().numpy())
        s1.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s1):
            o4, r4 = c.ctx.collide(TRI, capacity=r2.shape[0], device=True)
            o5 = c.ctx.collide(TRI, sizes_only=True, device=True)
        s1.synchronize()
        np.testing.assert_array_equal(o4.cpu().numpy(), o2.cpu().numpy())
        np.testing.assert_array_equal(r4.cpu().numpy(), r2.cpu().numpy())
        np.testing.assert_array_equal(o5.cpu().numpy(), o2.cpu().numpy())
        c.ctx.synchronize()


# ---------------------------------------------------------------- 9. errors
def test_errors():
    import torch
    off = np.zeros(13, np.uint64)
    ids = np.zeros(64, np.uint32)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.collide()
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.collide_counts()
        assert e.value.status == NOT_READY
        ctx.build()
        h = ctx._h
        doff = torch.full((13,), -1, dtype=torch.int64, device="cuda")
        dids = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for mode in (1, 2, 128, 1 << 8, 1 << 31, SIZES | FILL, SIZES | FILL | TRI, SYM | 1, TRI | 2):
            assert L.rtbvh_collide_async(h, vp(doff), vp(dids), 64, mode, None) == INVALID_ARG, mode
            assert L.rtbvh_collide_host(h, vp(off), vp(ids), 64, mode) == INVALID_ARG, mode
        assert L.rtbvh_collide_async(h, None, vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_collide_async(h, vp(doff), None, 64, 0, None) == INVALID_ARG
        assert L.rtbvh_collide_async(h, vp(doff), None, 64, FILL, None) == INVALID_ARG
        assert L.rtbvh_collide_host(h, None, vp(ids), 64, 0) == INVALID_ARG
        assert L.rtbvh_collide_host(h, vp(off), None, 64, 0) == INVALID_ARG
        assert L.rtbvh_collide_counts(h, None) == INVALID_ARG
        ctx.synchronize()
        assert (doff.cpu().numpy() == -1).all() and (dids.cpu().numpy() == -1).all()   # nothing was written
        assert not off.any() and not ids.any()
        # NULL ids are fine with capacity 0 and under SIZES
        d = load_scene_fixture("Rect")
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(W, H)[0])
        want = brute(tris, d["indices"], wr.rank_of(ctx.read_sorted()[1]))
        assert L.rtbvh_collide_async(h, vp(doff), None, 0, 0, None) == OK
        ctx.synchronize()
        np.testing.assert_array_equal(doff.cpu().numpy().view(np.uint64), want[0][0])
        doff.fill_(-1)
        assert L.rtbvh_collide_async(h, vp(doff), None, 64, SIZES | TRI, None) == OK
        ctx.synchronize()
        np.testing.assert_array_equal(doff.cpu().numpy().view(np.uint64), want[TRI][0])
        with pytest.raises(rt.RtbvhError) as e:
            ctx.collide_counts()                    # still no counting self-collision query
        assert e.value.status == NOT_READY
        assert_collide_equal(ctx.collide(TRI), want[TRI])   # and the context still answers
        ctx.update_vertices(d["vertices"][:, :3].copy())
        assert L.rtbvh_collide_async(h, vp(doff), vp(dids), 64, 0, None) == NOT_READY
        assert L.rtbvh_collide_host(h, vp(off), vp(ids), 64, 0) == NOT_READY
        ctx.refit()
        assert_collide_equal(ctx.collide(TRI | SYM), want[TRI | SYM])
        ctx.synchronize()
