"""Region queries on the GPU (rtbvh_region_async / rtbvh_region_host through Context.region and the raw entries)
against the brute force over all triangles (tests/region_ref.py), ordered by the build's sort order
(Context.read_sorted).  The set and its order are specified independently of the walk and of whether it takes
subtrees whole, so every comparison is bit-exact: offsets and ids as integers."""
import ctypes
import functools

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import deep_scenes as ds
from tests import hostile_scenes as hs
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests import region_ref as rr
from tests import within_ref as wr
from tests.conftest import load_scene_fixture

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CAMERAS = ["reference", "identity"]
FORMS = {"records": 0, "node-boxes": rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD}
OK, NOT_READY, INVALID_ARG, OVERFLOW = (rt._lib.OK, rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG,
                                        rt._lib.ERR_STACK_OVERFLOW)
SIZES, FILL, COUNT, TRI, NOACC = (rt.REGION_SIZES, rt.REGION_FILL, rt.REGION_COUNT, rt.REGION_TRIANGLE,
                                  rt.REGION_NO_ACCEPT)
MODES = [0, TRI]
MODE_IDS = ["boxes", "triangles"]
ACCEPTS = [0, NOACC]
ACCEPT_IDS = ["accept", "no-accept"]
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


def assert_region_equal(got, want, what=""):
    off, ids = got
    assert off.dtype == np.uint64 and ids.dtype == np.uint32, what
    np.testing.assert_array_equal(off, want[0], err_msg=what + " offsets")
    np.testing.assert_array_equal(ids, want[1], err_msg=what + " ids")


def vp(a):
    return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


class Device:
    """The raw device entry on the context stream with torch tensors for memory: regions up, an ids buffer of
    capacity + GUARD words filled with PATTERN, offsets and ids back."""

    def __init__(self, ctx, packed):
        import torch
        self.torch, self.ctx, self.n = torch, ctx, len(packed)
        self.regions = torch.from_numpy(packed.view(np.float32).reshape(-1, 24).copy()).cuda()
        self.offsets = torch.full((self.n + 1,), -1, dtype=torch.int64, device="cuda")

    def run(self, capacity, mode=0, offsets=None, null_ids=False, expect=OK):
        torch = self.torch
        if offsets is not None:
            self.offsets.copy_(torch.from_numpy(offsets.view(np.int64)))
        buf = torch.full((capacity + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        L = rt.lib()
        st = L.rtbvh_region_async(self.ctx._h, vp(self.regions), self.n, vp(self.offsets),
                                  None if null_ids else vp(buf), capacity, mode, None)
        assert st == OK
        assert L.rtbvh_synchronize(self.ctx._h) == expect
        words = buf.cpu().numpy().view(np.uint32)
        assert (words[capacity:] == np.uint32(PATTERN)).all(), "a write behind capacity"
        return self.offsets.cpu().numpy().view(np.uint64), words[:capacity]


@functools.lru_cache(maxsize=None)
def reference(scene, cam, order_bytes):
    """(tris, regions, {mode: brute-force lists}) of a golden scene under a camera in a sort order: computed once,
    shared by the tree forms."""
    s = fixture_scene(scene)
    tris = rw.clip_triangles(s.vertices, s.indices, camera(cam)[0])
    regions = rr.sample_regions(tris, 5)
    rank = wr.rank_of(np.frombuffer(order_bytes, np.uint32))
    return tris, regions, {m: rr.brute_region(tris, regions, rank, m == TRI) for m in MODES}


class Case:
    def __init__(self, scene, cam, form):
        self.scene = fixture_scene(scene)
        self.wvp, self.wv = camera(cam)
        self.ctx = built(self.scene, self.wvp, self.wv, flags=FORMS[form])
        self.order = self.ctx.read_sorted()[1].copy()
        self.rank = wr.rank_of(self.order)
        self.tris, self.regions, self.want = reference(scene, cam, self.order.tobytes())
        self.T = len(self.tris)

    def total(self, m):
        return int(self.want[m][0][-1])


@pytest.fixture(scope="module", params=[(s, c, f) for s in SCENES for c in CAMERAS for f in FORMS],
                ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. parity, and the accept exercised
@pytest.mark.parametrize("acc", ACCEPTS, ids=ACCEPT_IDS)
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_matches_brute_force(case, m, acc):
    want, total = case.want[m], case.total(m)
    n = len(case.regions)
    cnt = np.diff(want[0]).astype(np.int64)
    assert 0 < total < n * case.T and (cnt == 0).any() and (cnt == case.T).any()         # from the reference
    mode = m | acc
    got = case.ctx.region(case.regions, mode=mode, capacity=total)                        # one call
    assert got[0].shape == (n + 1,) and got[1].shape == (total,)
    assert_region_equal(got, want, "one call")
    assert_region_equal(case.ctx.region(case.regions, mode=mode), want, "SIZES then FILL")
    flat = case.regions.view(np.float32).reshape(-1, 24)
    assert_region_equal(case.ctx.region(flat, mode=mode | COUNT, capacity=total), want, "(N, 24), COUNT")
    c = case.ctx.region_counts()
    assert c["regions"] == n and c["ids"] == total
    np.testing.assert_array_equal(case.ctx.region(case.regions, mode=mode, sizes_only=True), want[0])
    dev = Device(case.ctx, case.regions)                                                  # the device entry
    off, words = dev.run(total, mode)
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(words, want[1])


@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_accepts_happen_and_save_steps(case, m):
    want, total = case.want[m], case.total(m)
    assert_region_equal(case.ctx.region(case.regions, mode=m | COUNT, capacity=total), want)
    a = case.ctx.region_counts()
    assert_region_equal(case.ctx.region(case.regions, mode=m | COUNT | NOACC, capacity=total), want)
    b = case.ctx.region_counts()
    print("region steps:", a, "without accepts:", b)
    assert a["accepted_subtrees"] > 0 and a["accepted_ids"] > 0 and a["leaf_steps"] > 0
    assert 0 < a["accepted_ids"] <= total
    assert b["accepted_subtrees"] == 0 and b["accepted_ids"] == 0
    assert b["leaf_steps"] >= 2 * total                          # two passes, every member's leaf
    assert a["internal_steps"] + a["leaf_steps"] < b["internal_steps"] + b["leaf_steps"]
    assert a["regions"] == b["regions"] == len(case.regions) and a["ids"] == b["ids"] == total
    # the whole-scene region: the root taken whole, at most one node step and no leaf step
    whole = case.regions[rr.SPECIAL["whole"]:][:1]
    off = case.ctx.region(whole, mode=m | COUNT, sizes_only=True)
    assert off.tolist() == [0, case.T]
    c = case.ctx.region_counts()
    assert c["internal_steps"] <= 1 and c["leaf_steps"] == 0 and c["accepted_subtrees"] == 1
    assert c["accepted_ids"] == case.T == c["ids"]
    off, ids = case.ctx.region(whole, mode=m)
    np.testing.assert_array_equal(ids, case.order)               # every triangle, in sort order


# ---------------------------------------------------------------- 2. capacity and foreign offsets
@pytest.mark.parametrize("acc", ACCEPTS, ids=ACCEPT_IDS)
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_capacity_truncates_and_never_writes_behind(case, m, acc):
    want, total = case.want[m], case.total(m)
    dev = Device(case.ctx, case.regions)
    k = len(case.regions) + rr.SPECIAL["whole"]                  # its list is one accepted range: cut it after one id
    assert int(want[0][k + 1] - want[0][k]) == case.T
    for capacity in (total, total - 1, int(want[0][k]) + 1, 1, 0):
        off, words = dev.run(capacity, m | acc)
        np.testing.assert_array_equal(off, want[0], err_msg=f"capacity {capacity}")       # offsets[-1]: the true total
        np.testing.assert_array_equal(words, want[1][:capacity], err_msg=f"capacity {capacity}")
    off, _ = dev.run(0, m | acc, null_ids=True)                  # capacity 0: ids may be NULL
    np.testing.assert_array_equal(off, want[0])
    off, _ = dev.run(0, m | acc | SIZES, null_ids=True)
    np.testing.assert_array_equal(off, want[0])
    half = total // 2                                            # the host entry: min(total, capacity) ids
    off, ids = case.ctx.region(case.regions, mode=m | acc, capacity=half)
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(ids, want[1][:half])
    assert_region_equal(case.ctx.region(case.regions, mode=m | acc, capacity=total + 5), want, "capacity above the total")


@pytest.mark.parametrize("acc", ACCEPTS, ids=ACCEPT_IDS)
def test_fill_over_smaller_offsets_writes_prefixes(case, acc):
    """FILL of the box lists over the offsets of the (shorter) TRIANGLE lists: segment k holds the first ids of
    region k's box list, whether they come from leaves or from a range, and nothing leaves a segment."""
    off_s = case.want[TRI][0]
    off_l, ids_l = case.want[0]
    cnt_s, cnt_l = np.diff(off_s).astype(np.int64), np.diff(off_l).astype(np.int64)
    assert (cnt_l >= cnt_s).all() and (cnt_l > cnt_s).any() and (cnt_s > 0).any()
    total = int(off_s[-1])
    want_words = np.full(total, PATTERN, np.uint32)
    for k in range(len(case.regions)):
        want_words[int(off_s[k]):int(off_s[k]) + cnt_s[k]] = ids_l[int(off_l[k]):int(off_l[k]) + cnt_s[k]]
    dev = Device(case.ctx, case.regions)
    for capacity in (total, total // 2):
        off, words = dev.run(capacity, FILL | acc, offsets=off_s)
        np.testing.assert_array_equal(off, off_s)                # FILL reads them only
        np.testing.assert_array_equal(words, want_words[:capacity], err_msg=f"capacity {capacity}")
    # offsets that begin behind the capacity, and empty segments: nothing is written
    shifted = (off_s + np.uint64(7)).astype(np.uint64)
    off, words = dev.run(5, FILL | acc, offsets=shifted)
    assert (words == PATTERN).all()
    flat = np.full(len(off_s), 3, np.uint64)
    off, words = dev.run(16, FILL | acc, offsets=flat)
    assert (words == PATTERN).all()


# ---------------------------------------------------------------- 3. tiny scenes
@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = rr.tiny_scene(ntris)
    wvp, wv = camera(cam)
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = wr.rank_of(ctx.read_sorted()[1])
        regions = rr.sample_regions(tris, ntris, n_each=16)
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            cnt = np.diff(want[0])
            assert (cnt == 0).any() and cnt[rr.SPECIAL["whole"]] == ntris
            for acc in ACCEPTS:
                assert_region_equal(ctx.region(regions, mode=m | acc), want)
                assert_region_equal(ctx.region(regions, mode=m | acc | COUNT, capacity=int(want[0][-1])), want, "one call")
                assert ctx.region_counts()["ids"] == int(want[0][-1])


@pytest.mark.parametrize("form", list(FORMS))
def test_nan_triangle_scene(form):
    """The CPU test's scene: finite triangles and one all-NaN triangle under finite node boxes.  The region around
    the root box lists T - 1 triangles, and the walk takes nothing whole."""
    s = rr.nan_triangle_scene()
    wvp, wv = camera("identity")
    with built(s, wvp, wv, flags=FORMS[form]) as ctx:
        with np.errstate(all="ignore"):
            tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        T = len(tris)
        fin = tris[np.isfinite(tris).all((1, 2))]
        lo, hi = nr.root_box(fin)
        rank = wr.rank_of(ctx.read_sorted()[1])
        regions = np.concatenate([rt.box_region(lo - 1, hi + 1), rr.sample_regions(fin, 9, n_each=8)])
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            assert int(want[0][1]) == T - 1
            for acc in ACCEPTS:
                assert_region_equal(ctx.region(regions, mode=m | acc | COUNT), want)
                c = ctx.region_counts()
                assert c["accepted_subtrees"] == 0 and c["accepted_ids"] == 0 and c["leaf_steps"] > 0


# ---------------------------------------------------------------- 4. hostile scenes
HOSTILE = [(v, c, G) for v in hs.VARIANTS for c in hs.CAMERAS for G in (12, 64)]


@pytest.mark.parametrize("case", HOSTILE, ids=lambda p: f"{p[0]}-{p[1]}-G{p[2]}")
def test_hostile_scenes(case):
    variant, cam, G = case
    h = hs.hostile(variant, G)
    wvp, wv = hs.camera(cam)
    tris = h.tris(wvp)
    regions = rr.sample_regions(tris[hs.finite_part(tris, h.labels)], 7, n_each=24)
    nan_leaf = bool(np.isnan(np.stack(nr.leaf_data(tris)[3:])).any())
    forms = list(FORMS) if G == 12 else ["records"]
    for form in forms:
        with built(h.scene, wvp, wv, flags=FORMS[form]) as ctx:
            rank = wr.rank_of(ctx.read_sorted()[1])
            for m in MODES:
                want = rr.brute_region(tris, regions, rank, m == TRI)
                assert want[0][-1] > 0
                assert_region_equal(ctx.region(regions, mode=m | COUNT), want, form)
                c = ctx.region_counts()
                assert (c["accepted_subtrees"] == 0) == nan_leaf, (form, c)          # the guard
                assert_region_equal(ctx.region(regions, mode=m | NOACC, capacity=int(want[0][-1])), want, form + " no accept")


# ---------------------------------------------------------------- 5. the guard follows the tree
@pytest.mark.parametrize("form", list(FORMS))
def test_guard_follows_refit_and_rebuild(form):
    s = fixture_scene("Test")
    wvp, wv = camera("reference")
    P0 = np.ascontiguousarray(s.vertices[:, :3], np.float32)
    P1 = P0.copy()
    P1[s.indices[:3]] = np.nan                                   # triangle 0: all NaN (its vertices' other triangles too)
    v1 = s.vertices.copy()
    v1[:, :3] = P1
    tris0 = rw.clip_triangles(s.vertices, s.indices, wvp)
    with np.errstate(all="ignore"):
        tris1 = rw.clip_triangles(v1, s.indices, wvp)
    assert np.isnan(tris1[0]).all()
    regions = rr.sample_regions(tris0, 5, n_each=24)

    def check(ctx, tris, accepts, what):
        rank = wr.rank_of(ctx.read_sorted()[1])
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            assert_region_equal(ctx.region(regions, mode=m | COUNT), want, what)
            c = ctx.region_counts()
            assert (c["accepted_subtrees"] > 0) == accepts, (what, c)

    with built(s, wvp, wv, flags=FORMS[form]) as ctx:
        check(ctx, tris0, True, "built")
        for again in ("refit", "build"):
            ctx.update_vertices(P1)
            getattr(ctx, again)()
            check(ctx, tris1, False, again + " to NaN positions")
            ctx.update_vertices(P0)
            getattr(ctx, again)()
            check(ctx, tris0, True, again + " back")


# ---------------------------------------------------------------- 6. deep scenes, the stack limit
def fan_slabs():
    """Planes through the fan's window (every fan leaf box holds it, none lies inside a thin slab: the walk enters
    both children at every level) and slabs across its depth."""
    px, py = ds.P
    n = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, -1, 0], [0, 0, 1], [0, 0, 1]], np.float32)
    lo = np.array([px, py, px + py, px - py, 0.03, -1.0], np.float32)
    hi = np.array([px, py + 1, px + py, px - py + 2, 0.2, 400.0], np.float32)
    return rt.slab_region(n, lo, hi)


@pytest.mark.parametrize("form", list(FORMS))
def test_fan_slabs_leave_the_lds_part_of_the_stack(form):
    s, _, nodes, wvp, wv = ds.fan()
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    regions = fan_slabs()
    with built(s, wvp, wv, flags=FORMS[form]) as ctx:
        rank = wr.rank_of(ctx.read_sorted()[1])
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            assert int(np.diff(want[0])[0]) >= 64                # the plane x = P.x meets the whole fan
            for acc in ACCEPTS:
                assert_region_equal(ctx.region(regions, mode=m | acc), want)
                assert_region_equal(ctx.region(regions, mode=m | acc, capacity=int(want[0][-1])), want, "one call")
    # stack_limit = 20, past the 16 entries in LDS and below what the fan needs: reported at synchronize, the
    # lists consistent subsequences
    with built(s, wvp, wv, flags=FORMS[form], stack_limit=20) as ctx:
        rank = wr.rank_of(ctx.read_sorted()[1])
        want = rr.brute_region(tris, regions, rank)
        cap = int(want[0][-1])
        dev = Device(ctx, regions)
        off, words = dev.run(cap, 0, expect=OVERFLOW)
        assert rt.lib().rtbvh_synchronize(ctx._h) == OK          # once per new overflow
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
        total = int(off[-1])
        assert 0 < total < cap
        assert (words[total:] == PATTERN).all() and (words[:total] < len(tris)).all()
        for k in range(len(regions)):
            g = words[int(off[k]):int(off[k + 1])]
            t = want[1][int(want[0][k]):int(want[0][k + 1])]
            idx = {w: i for i, w in enumerate(t.tolist())}
            where = [idx.get(w, -1) for w in g.tolist()]
            assert -1 not in where and where == sorted(where), k
        with pytest.raises(rt.RtbvhError) as e:
            ctx.region(regions)
        assert e.value.status == OVERFLOW


def test_crossing_scene_slabs():
    s, _, nodes, wvp, wv = ds.crossing()
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    rng = np.random.default_rng(2)
    lo, hi = nr.root_box(tris)
    n = np.concatenate([np.eye(3), rng.standard_normal((5, 3))]).astype(np.float32)
    c = (lo + (hi - lo) * rng.random((8, 3))).astype(np.float32)
    d = rr.plane_dots(n, c)
    regions = np.concatenate([rt.slab_region(n, d, d), rt.slab_region(n, d, d + np.float32(0.05) * np.abs(d) + np.float32(0.01))])
    with built(s, wvp, wv) as ctx:
        rank = wr.rank_of(ctx.read_sorted()[1])
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            assert want[0][-1] > 0
            for acc in ACCEPTS:
                assert_region_equal(ctx.region(regions, mode=m | acc), want)


# ---------------------------------------------------------------- 7. device tensors and streams
def test_first_queries_of_a_tree_on_two_streams():
    """The leaf-NaN word is written on the stream of a tree's first region query; a query on another stream right
    behind it must see it (both take subtrees whole, and give the lists)."""
    import torch
    s = fixture_scene("Test")
    wvp, wv = camera("reference")
    with built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = wr.rank_of(ctx.read_sorted()[1])
        regions = rr.sample_regions(tris, 5)
        want = {m: rr.brute_region(tris, regions, rank, m == TRI) for m in MODES}
        r1 = torch.from_numpy(regions.view(np.float32).reshape(-1, 24).copy()).cuda()
        r2 = rt.make_regions(torch.from_numpy(rr.as_planes(regions)).cuda())
        assert r2.is_cuda and tuple(r2.shape) == (len(regions), 24)
        assert torch.equal(r1.view(torch.int32), r2.view(torch.int32))   # (the bits: one region holds a NaN)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for again in range(2):
            s1.wait_stream(torch.cuda.current_stream())
            s2.wait_stream(torch.cuda.current_stream())
            total = int(want[0][0][-1])
            o1, i1 = ctx.region(r1, mode=COUNT, capacity=total + 7, stream=s1)
            o2, i2 = ctx.region(r2, mode=TRI, stream=s2)         # capacity=None: sized from the total
            s1.synchronize()
            s2.synchronize()
            assert o1.dtype == torch.int64 and i1.dtype == torch.int32 and tuple(i1.shape) == (total + 7,)
            np.testing.assert_array_equal(o1.cpu().numpy().view(np.uint64), want[0][0])
            np.testing.assert_array_equal(i1[:total].cpu().numpy().view(np.uint32), want[0][1])
            np.testing.assert_array_equal(o2.cpu().numpy().view(np.uint64), want[TRI][0])
            np.testing.assert_array_equal(i2.cpu().numpy().view(np.uint32), want[TRI][1])
            assert ctx.region_counts()["accepted_subtrees"] > 0
            ctx.synchronize()
            ctx.refit()                                          # a new tree epoch: the word is written again
        with pytest.raises(ValueError):
            ctx.region(r1[:, :23])


# ---------------------------------------------------------------- 8. errors
def test_errors():
    import torch
    big = np.float32(3e38)
    regions = rt.box_region(np.full((4, 3), -big, np.float32), np.full((4, 3), big, np.float32))
    off = np.zeros(5, np.uint64)
    ids = np.zeros(64, np.uint32)
    L = rt.lib()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.region(regions)
        assert e.value.status == NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.region_counts()
        assert e.value.status == NOT_READY
        o, p = ctx.region(regions[:0])               # n == 0 is OK even before a build
        assert o.tolist() == [0] and p.shape == (0,)
        ctx.build()
        h = ctx._h
        dr = torch.from_numpy(regions.view(np.float32).reshape(-1, 24).copy()).cuda()
        doff = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        dids = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for mode in (1, 2, 128, 1 << 8, 1 << 31, SIZES | FILL, SIZES | FILL | TRI, NOACC | 1, TRI | 2):
            assert L.rtbvh_region_async(h, vp(dr), 4, vp(doff), vp(dids), 64, mode, None) == INVALID_ARG, mode
            assert L.rtbvh_region_host(h, vp(regions), 4, vp(off), vp(ids), 64, mode) == INVALID_ARG, mode
        assert L.rtbvh_region_async(h, None, 4, vp(doff), vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_region_async(h, vp(dr), 4, None, vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_region_async(h, vp(dr), 4, vp(doff), None, 64, 0, None) == INVALID_ARG
        assert L.rtbvh_region_async(h, vp(dr), 4, vp(doff), None, 64, FILL, None) == INVALID_ARG
        assert L.rtbvh_region_async(h, vp(dr), 1 << 31, vp(doff), vp(dids), 64, 0, None) == INVALID_ARG
        assert L.rtbvh_region_host(h, vp(regions), 4, None, vp(ids), 64, 0) == INVALID_ARG
        assert L.rtbvh_region_host(h, vp(regions), 4, vp(off), None, 64, 0) == INVALID_ARG
        assert L.rtbvh_region_host(h, vp(regions), 1 << 31, vp(off), vp(ids), 64, 0) == INVALID_ARG
        assert L.rtbvh_region_counts(h, None) == INVALID_ARG
        ctx.synchronize()
        assert (doff.cpu().numpy() == -1).all() and (dids.cpu().numpy() == -1).all()   # nothing was written
        assert not off.any() and not ids.any()
        # NULL ids are fine with capacity 0 and under SIZES; n == 0 writes offsets[0] only where there is one
        assert L.rtbvh_region_async(h, vp(dr), 4, vp(doff), None, 0, 0, None) == OK
        assert L.rtbvh_region_async(h, vp(dr), 4, vp(doff), None, 64, SIZES, None) == OK
        assert L.rtbvh_region_async(h, None, 0, None, None, 0, 0, None) == OK
        ctx.synchronize()
        assert doff.cpu().numpy().tolist() == [0, 12, 24, 36, 48]   # (the SIZES call: Rect's 12 triangles each)
        doff.fill_(-1)
        torch.cuda.synchronize()
        assert L.rtbvh_region_async(h, None, 0, vp(doff), None, 0, 0, None) == OK
        ctx.synchronize()
        assert doff.cpu().numpy().tolist() == [0, -1, -1, -1, -1]
        with pytest.raises(rt.RtbvhError) as e:
            ctx.region_counts()                     # still no counting region query
        assert e.value.status == NOT_READY
        ctx.update_vertices(np.ascontiguousarray(fixture_scene("Rect").vertices[:, :3]))
        with pytest.raises(rt.RtbvhError) as e:     # a stale tree
            ctx.region(regions)
        assert e.value.status == NOT_READY
        assert L.rtbvh_region_async(h, vp(dr), 4, vp(doff), vp(dids), 64, 0, None) == NOT_READY
        ctx.refit()
        d = load_scene_fixture("Rect")              # and the context still answers
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(W, H)[0])
        assert_region_equal(ctx.region(regions), rr.brute_region(tris, regions, wr.rank_of(ctx.read_sorted()[1])))
        ctx.synchronize()
