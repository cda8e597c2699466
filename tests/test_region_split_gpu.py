"""Split region queries on the GPU (the split field of rtbvh_region_async / rtbvh_region_host): the same offsets and
ids as the brute force over all triangles (tests/region_ref.py) and as the plain query, bit for bit, whatever K, mode,
tree form, entry or pairing of SIZES and FILL; nothing written outside a segment or past `capacity`; and the counts
of rtbvh_region_counts / rtbvh_region_split_counts.  Scenes, regions, helpers and the brute-force lists are those of
tests/test_region_gpu.py (computed once, shared)."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from tests import deep_scenes as ds
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests import region_ref as rr
from tests import region_split_ref as rs
from tests import test_region_gpu as rg
from tests import within_ref as wr

pytestmark = pytest.mark.gpu
OK, NOT_READY, INVALID_ARG, OVERFLOW = rg.OK, rg.NOT_READY, rg.INVALID_ARG, rg.OVERFLOW
SIZES, FILL, COUNT, TRI, NOACC = rg.SIZES, rg.FILL, rg.COUNT, rg.TRI, rg.NOACC
MODES, MODE_IDS, ACCEPTS, ACCEPT_IDS = rg.MODES, rg.MODE_IDS, rg.ACCEPTS, rg.ACCEPT_IDS
PATTERN = rg.PATTERN
AUTO = rt.REGION_SPLIT_AUTO
FIELDS = {"K2": rt.region_split(2), "K64": rt.region_split(64), "K4096": rt.region_split(4096), "auto": AUTO}
BIG = 5 * 48          # sample_regions' classes 5 (most of the scene) and the five special regions: 53 regions,
                      # few enough for K = 4096 itself (293 regions clamp it to 2048)


def field_k(field, n):
    return rs.auto_k(n, (field >> rt.REGION_SPLIT_SHIFT) & 15)


def sub_lists(want, first):
    """The brute-force lists of regions[first:]."""
    off, ids = want
    return (off[first:] - off[first]).astype(np.uint64), ids[int(off[first]):]


class Case(rg.Case):
    def __init__(self, scene, cam, form):
        super().__init__(scene, cam, form)
        self._plain = {}

    def plain(self, mode):
        """The plain query's (offsets, ids), checked against the brute force once."""
        if mode not in self._plain:
            got = self.ctx.region(self.regions, mode=mode, capacity=self.total(mode & TRI))
            rg.assert_region_equal(got, self.want[mode & TRI], "the plain query")
            self._plain[mode] = got
        return self._plain[mode]


@pytest.fixture(scope="module", params=[(s, c, f) for s in rg.SCENES for c in rg.CAMERAS for f in rg.FORMS],
                ids=lambda p: "-".join(p))
def case(request):
    c = Case(*request.param)
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. parity: entries, pairings, K
@pytest.mark.parametrize("field", list(FIELDS.values()), ids=list(FIELDS))
@pytest.mark.parametrize("acc", ACCEPTS, ids=ACCEPT_IDS)
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_split_lists_are_the_plain_lists(case, m, acc, field):
    want, total = case.want[m], case.total(m)
    n = len(case.regions)
    plain = case.plain(m | acc)
    mode = m | acc | field
    got = case.ctx.region(case.regions, mode=mode, capacity=total)                         # host, one call
    rg.assert_region_equal(got, want, "one call")
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
    rg.assert_region_equal(case.ctx.region(case.regions, mode=mode), want, "host: SIZES then FILL")
    np.testing.assert_array_equal(case.ctx.region(case.regions, mode=mode, sizes_only=True), want[0])
    rg.assert_region_equal(case.ctx.region(case.regions, mode=mode | COUNT, capacity=total), want, "COUNT")
    c, sc = case.ctx.region_counts(), case.ctx.region_split_counts()
    assert c["regions"] == n and c["ids"] == total                                         # regions, not pieces
    assert sc["k"] == field_k(field, n) and 0 < sc["pieces"] <= n * sc["k"]
    dev = rg.Device(case.ctx, case.regions)                                                # device, one call
    off, words = dev.run(total, mode)
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(words, want[1])
    for sizes_mode, fill_mode, what in ((m | acc, mode, "plain SIZES, split FILL"), (mode, m | acc, "split SIZES, plain FILL"),
                                        (mode, mode, "split SIZES, split FILL")):
        dev.offsets.fill_(-1)
        off, _ = dev.run(0, sizes_mode | SIZES, null_ids=True)
        np.testing.assert_array_equal(off, want[0], err_msg=what)
        off, words = dev.run(total, fill_mode | FILL)
        np.testing.assert_array_equal(off, want[0], err_msg=what)
        np.testing.assert_array_equal(words, want[1], err_msg=what)
    big = case.regions[BIG:]                                                               # few regions: K unclamped
    rg.assert_region_equal(case.ctx.region(big, mode=mode | COUNT, capacity=total), sub_lists(want, BIG), "53 regions")
    assert case.ctx.region_split_counts()["k"] == field_k(field, len(big)) == (4096 if field == AUTO else 1 << (field >> 16))


# ---------------------------------------------------------------- 2. capacity and foreign offsets
@pytest.mark.parametrize("field", [FIELDS["K64"], AUTO], ids=["K64", "auto"])
@pytest.mark.parametrize("acc", ACCEPTS, ids=ACCEPT_IDS)
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_capacity_truncates_and_never_writes_behind(case, m, acc, field):
    want, total = case.want[m], case.total(m)
    n = len(case.regions)
    dev = rg.Device(case.ctx, case.regions)
    k = n + rr.SPECIAL["whole"]                                  # one accepted range (a RANGE piece): cut after one id
    assert int(want[0][k + 1] - want[0][k]) == case.T
    cnt = np.diff(want[0]).astype(np.int64)
    b = int(np.argmax(cnt[:6 * 48]))                             # the longest sampled list: many pieces, cut inside
    assert cnt[b] > 2
    cuts = [int(want[0][b]) + int(cnt[b]) // 2 + 1, int(want[0][b]) + int(cnt[b]) // 3, int(want[0][b]) + 1]
    for capacity in [total, total - 1, int(want[0][k]) + 1] + cuts + [1, 0]:
        off, words = dev.run(capacity, m | acc | field)
        np.testing.assert_array_equal(off, want[0], err_msg=f"capacity {capacity}")       # offsets[-1]: the true total
        np.testing.assert_array_equal(words, want[1][:capacity], err_msg=f"capacity {capacity}")
    off, _ = dev.run(0, m | acc | field, null_ids=True)          # capacity 0: ids may be NULL
    np.testing.assert_array_equal(off, want[0])
    half = total // 2                                            # the host entry: min(total, capacity) ids
    off, ids = case.ctx.region(case.regions, mode=m | acc | field, capacity=half)
    np.testing.assert_array_equal(off, want[0])
    np.testing.assert_array_equal(ids, want[1][:half])
    rg.assert_region_equal(case.ctx.region(case.regions, mode=m | acc | field, capacity=total + 5), want, "above the total")


@pytest.mark.parametrize("field", [FIELDS["K64"], AUTO], ids=["K64", "auto"])
@pytest.mark.parametrize("acc", ACCEPTS, ids=ACCEPT_IDS)
def test_fill_over_smaller_offsets_writes_prefixes(case, acc, field):
    """test_region_gpu's: FILL of the box lists over the offsets of the (shorter) TRIANGLE lists.  A piece that begins
    behind its region's segment writes nothing; one that straddles its end is cut there."""
    off_s = case.want[TRI][0]
    off_l, ids_l = case.want[0]
    cnt_s = np.diff(off_s).astype(np.int64)
    total = int(off_s[-1])
    want_words = np.full(total, PATTERN, np.uint32)
    for k in range(len(case.regions)):
        want_words[int(off_s[k]):int(off_s[k]) + cnt_s[k]] = ids_l[int(off_l[k]):int(off_l[k]) + cnt_s[k]]
    dev = rg.Device(case.ctx, case.regions)
    for capacity in (total, total // 2):
        off, words = dev.run(capacity, FILL | acc | field, offsets=off_s)
        np.testing.assert_array_equal(off, off_s)                # FILL reads them only
        np.testing.assert_array_equal(words, want_words[:capacity], err_msg=f"capacity {capacity}")
    shifted = (off_s + np.uint64(7)).astype(np.uint64)           # offsets that begin behind the capacity
    off, words = dev.run(5, FILL | acc | field, offsets=shifted)
    assert (words == PATTERN).all()
    flat = np.full(len(off_s), 3, np.uint64)                     # empty segments
    off, words = dev.run(16, FILL | acc | field, offsets=flat)
    assert (words == PATTERN).all()


# ---------------------------------------------------------------- 3. counts
@pytest.mark.parametrize("field", [FIELDS["K2"], FIELDS["K64"], AUTO], ids=["K2", "K64", "auto"])
@pytest.mark.parametrize("m", MODES, ids=MODE_IDS)
def test_step_identity_and_accepts(case, m, field):
    """Without accepts every entered node is tested once, by the expansion or by a piece, and every entered leaf once:
    a pass of the split query makes the plain pass's steps exactly.  A one-call query walks twice and expands once."""
    ctx, want, total = case.ctx, case.want[m], case.total(m)

    def counts(mode, **kw):
        ctx.region(case.regions, mode=mode | COUNT, **kw)
        return ctx.region_counts()

    p1, s1 = counts(m | NOACC, sizes_only=True), counts(m | NOACC | field, sizes_only=True)
    sc = ctx.region_split_counts()
    print("one pass, no accepts: plain", p1, "split", s1, sc)
    assert s1["internal_steps"] == p1["internal_steps"] and s1["leaf_steps"] == p1["leaf_steps"]
    assert 0 < sc["expansion_tests"] <= s1["internal_steps"] and s1["accepted_subtrees"] == 0
    p2, s2 = counts(m | NOACC, capacity=total), counts(m | NOACC | field, capacity=total)
    sc = ctx.region_split_counts()
    assert p2["internal_steps"] == 2 * p1["internal_steps"] and p2["leaf_steps"] == 2 * p1["leaf_steps"]
    assert s2["internal_steps"] + sc["expansion_tests"] == p2["internal_steps"] and s2["leaf_steps"] == p2["leaf_steps"]
    pa, sa = counts(m, sizes_only=True), counts(m | field, sizes_only=True)
    print("one pass, accepts: plain", pa, "split", sa)
    assert sa["internal_steps"] + sa["leaf_steps"] <= pa["internal_steps"] + pa["leaf_steps"]
    assert sa["accepted_subtrees"] > 0 and 0 < sa["accepted_ids"] <= total
    assert sa["regions"] == pa["regions"] == len(case.regions) and sa["ids"] == pa["ids"] == total
    assert counts(m | field, capacity=total)["accepted_ids"] == sa["accepted_ids"]         # (counted once)


def test_a_large_region_is_cut_into_pieces():
    """A single region holding much of Test at K = 64: more than one piece, and the longest piece walk is strictly
    shorter than the plain walk."""
    s = rg.fixture_scene("Test")
    wvp, wv = rg.camera("reference")
    with rg.built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = wr.rank_of(ctx.read_sorted()[1])
        regions = rr.sample_regions(tris, 5)
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            cnt = np.diff(want[0]).astype(np.int64)
            cls5 = np.arange(5 * 48, 6 * 48)
            k = int(cls5[np.argmax(np.where(cnt[cls5] < len(tris), cnt[cls5], -1))])   # much of the scene, not all
            assert len(tris) // 4 < cnt[k] < len(tris)
            one = regions[k:k + 1]
            for acc in ACCEPTS:
                off = ctx.region(one, mode=m | acc | COUNT, sizes_only=True)
                p = ctx.region_counts()
                assert off.tolist() == [0, cnt[k]]
                off = ctx.region(one, mode=m | acc | COUNT | FIELDS["K64"], sizes_only=True)
                c, sc = ctx.region_counts(), ctx.region_split_counts()
                print("plain", p, "split", c, sc)
                assert off.tolist() == [0, cnt[k]]
                assert sc["k"] == 64 and 1 < sc["pieces"] <= 64
                assert 0 < sc["longest_piece_steps"] < p["internal_steps"] + p["leaf_steps"]
                rg.assert_region_equal(ctx.region(one, mode=m | acc | FIELDS["K64"]), sub_lists((want[0][:k + 2], want[1][:int(want[0][k + 1])]), k))


def test_auto_k_is_the_documented_formula():
    s = rg.fixture_scene("Rect")
    wvp, wv = rg.camera("reference")
    with rg.built(s, wvp, wv) as ctx:
        never = np.zeros((1 << 19) + 1, rt.REGION_DTYPE)
        never["plane"][:, 0] = (0, 0, 0, 1)
        for n, k in ((1, 4096), (256, 4096), (293, 2048), (1 << 19, 2), ((1 << 19) + 1, 1)):
            assert rs.auto_k(n) == k
            off = ctx.region(never[:n], mode=AUTO | COUNT, sizes_only=True)
            assert not off.any()
            sc = ctx.region_split_counts()
            assert sc == dict(k=k, pieces=0, expansion_tests=0, longest_piece_steps=0), n
            assert ctx.region_counts()["regions"] == n
        ctx.region(never[:1 << 15], mode=rt.region_split(64) | COUNT, sizes_only=True)   # an explicit field is an upper limit
        assert ctx.region_split_counts()["k"] == 32
        ctx.region(never[:5], mode=rt.region_split(64) | COUNT, sizes_only=True)
        assert ctx.region_split_counts()["k"] == 64


# ---------------------------------------------------------------- 4. small and special scenes
@pytest.mark.parametrize("form", list(rg.FORMS))
def test_the_root_taken_whole_is_one_range_and_no_step(form):
    s = rg.fixture_scene("Test")
    wvp, wv = rg.camera("reference")
    with rg.built(s, wvp, wv, flags=rg.FORMS[form]) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        order = ctx.read_sorted()[1]
        regions = rr.sample_regions(tris, 5, n_each=1)
        S = rr.SPECIAL
        for m in MODES:
            for field in FIELDS.values():
                off, ids = ctx.region(regions[S["whole"]:][:1], mode=m | COUNT | field)
                np.testing.assert_array_equal(ids, order)
                c, sc = ctx.region_counts(), ctx.region_split_counts()
                assert c["internal_steps"] == 0 and c["leaf_steps"] == 0 and c["accepted_ids"] == len(tris)
                assert sc["pieces"] == 1 and sc["expansion_tests"] == 0 and sc["longest_piece_steps"] == 0
                for name in ("never", "nan", "inf"):                                     # empty lists, no piece
                    off = ctx.region(regions[len(regions) + S[name]:][:1], mode=m | COUNT | field, sizes_only=True)
                    assert off.tolist() == [0, 0]
                    assert ctx.region_split_counts()["pieces"] == 0 and ctx.region_counts()["leaf_steps"] == 0


@pytest.mark.parametrize("ntris", [1, 2])
@pytest.mark.parametrize("cam", rg.CAMERAS)
def test_one_and_two_triangle_scenes(ntris, cam):
    s = rr.tiny_scene(ntris)
    wvp, wv = rg.camera(cam)
    with rg.built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = wr.rank_of(ctx.read_sorted()[1])
        regions = rr.sample_regions(tris, ntris, n_each=16)
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            for acc in ACCEPTS:
                for field in FIELDS.values():
                    rg.assert_region_equal(ctx.region(regions, mode=m | acc | field), want)
                    rg.assert_region_equal(ctx.region(regions, mode=m | acc | field | COUNT, capacity=int(want[0][-1])), want, "one call")
                    assert ctx.region_counts()["ids"] == int(want[0][-1])
                    assert ctx.region_split_counts()["pieces"] <= ntris * len(regions)


@pytest.mark.parametrize("form", list(rg.FORMS))
def test_nan_triangle_scene(form):
    s = rr.nan_triangle_scene()
    wvp, wv = rg.camera("identity")
    with rg.built(s, wvp, wv, flags=rg.FORMS[form]) as ctx:
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
                for field in FIELDS.values():
                    rg.assert_region_equal(ctx.region(regions, mode=m | acc | COUNT | field), want)
                    c = ctx.region_counts()
                    assert c["accepted_subtrees"] == 0 and c["accepted_ids"] == 0 and c["leaf_steps"] > 0


@pytest.mark.parametrize("form", list(rg.FORMS))
def test_guard_follows_refit(form):
    """The NaN word across update_vertices + refit to NaN positions and back: the expansion and the piece walks take
    nothing whole while a leaf box holds a NaN."""
    s = rg.fixture_scene("Test")
    wvp, wv = rg.camera("reference")
    P0 = np.ascontiguousarray(s.vertices[:, :3], np.float32)
    P1 = P0.copy()
    P1[s.indices[:3]] = np.nan
    v1 = s.vertices.copy()
    v1[:, :3] = P1
    tris0 = rw.clip_triangles(s.vertices, s.indices, wvp)
    with np.errstate(all="ignore"):
        tris1 = rw.clip_triangles(v1, s.indices, wvp)
    regions = rr.sample_regions(tris0, 5, n_each=24)

    def check(ctx, tris, accepts, what):
        rank = wr.rank_of(ctx.read_sorted()[1])
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            for field in (FIELDS["K64"], AUTO):
                rg.assert_region_equal(ctx.region(regions, mode=m | COUNT | field), want, what)
                c = ctx.region_counts()
                assert (c["accepted_subtrees"] > 0) == accepts, (what, c)

    with rg.built(s, wvp, wv, flags=rg.FORMS[form]) as ctx:
        check(ctx, tris0, True, "built")
        ctx.update_vertices(P1)
        ctx.refit()
        check(ctx, tris1, False, "refit to NaN positions")
        ctx.update_vertices(P0)
        ctx.refit()
        check(ctx, tris0, True, "refit back")


# ---------------------------------------------------------------- 5. the fan, the stack limit
@pytest.mark.parametrize("form", list(rg.FORMS))
def test_fan_slabs(form):
    s, _, nodes, wvp, wv = ds.fan()
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    regions = rg.fan_slabs()
    with rg.built(s, wvp, wv, flags=rg.FORMS[form]) as ctx:
        rank = wr.rank_of(ctx.read_sorted()[1])
        for m in MODES:
            want = rr.brute_region(tris, regions, rank, m == TRI)
            for acc in ACCEPTS:
                for field in FIELDS.values():                     # the expansion ends on the 36-level chain
                    rg.assert_region_equal(ctx.region(regions, mode=m | acc | field), want)
                    rg.assert_region_equal(ctx.region(regions, mode=m | acc | field, capacity=int(want[0][-1])), want, "one call")
    # stack_limit = 20: a piece starts with an empty stack, so a split query may lose fewer subtrees than the plain
    # one, or none; what it lists is a subsequence, the two passes agree, and the overflow is reported iff ids are lost
    L = rt.lib()
    with rg.built(s, wvp, wv, flags=rg.FORMS[form], stack_limit=20) as ctx:
        rank = wr.rank_of(ctx.read_sorted()[1])
        want = rr.brute_region(tris, regions, rank)
        cap = int(want[0][-1])
        dev = rg.Device(ctx, regions)
        lost = {}
        for name, field in [("plain", 0)] + list(FIELDS.items()):
            import torch
            buf = torch.full((cap + rg.GUARD,), PATTERN, dtype=torch.int32, device="cuda")
            dev.offsets.fill_(-1)
            torch.cuda.synchronize()
            assert L.rtbvh_region_async(ctx._h, rg.vp(dev.regions), dev.n, rg.vp(dev.offsets), rg.vp(buf), cap, field, None) == OK
            st = L.rtbvh_synchronize(ctx._h)
            assert L.rtbvh_synchronize(ctx._h) == OK              # once per new overflow
            off = dev.offsets.cpu().numpy().view(np.uint64)
            words = buf.cpu().numpy().view(np.uint32)
            total = int(off[-1])
            assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all() and 0 < total <= cap
            assert st == (OVERFLOW if total < cap else OK), name  # reported iff something was lost
            assert (words[total:] == PATTERN).all() and (words[:total] < len(tris)).all()   # the passes agree
            for k in range(len(regions)):
                g = words[int(off[k]):int(off[k + 1])]
                t = want[1][int(want[0][k]):int(want[0][k + 1])]
                assert rs.is_subsequence(g.tolist(), t.tolist()), (name, k)
            lost[name] = cap - total
        print("ids lost under stack_limit = 20:", lost)
        assert lost["plain"] > 0 and all(v <= lost["plain"] for v in lost.values())


# ---------------------------------------------------------------- 6. streams
def test_first_two_split_queries_of_a_tree_on_two_streams():
    """The first split query grows the context's piece buffers and writes the leaf-NaN word on its stream; a second
    one on another stream right behind it is ordered behind both."""
    import torch
    s = rg.fixture_scene("Test")
    wvp, wv = rg.camera("reference")
    with rg.built(s, wvp, wv) as ctx:
        tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rank = wr.rank_of(ctx.read_sorted()[1])
        regions = rr.sample_regions(tris, 5)
        want = {m: rr.brute_region(tris, regions, rank, m == TRI) for m in MODES}
        r1 = torch.from_numpy(regions.view(np.float32).reshape(-1, 24).copy()).cuda()
        r2 = r1[BIG:].contiguous()                               # fewer regions: a larger K, the buffers grow again
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for again in range(2):
            s1.wait_stream(torch.cuda.current_stream())
            s2.wait_stream(torch.cuda.current_stream())
            total = int(want[0][0][-1])
            o1, i1 = ctx.region(r1, mode=COUNT | FIELDS["K64"], capacity=total + 7, stream=s1)
            o2, i2 = ctx.region(r2, mode=TRI | AUTO, stream=s2)  # capacity=None: sized from the total
            s1.synchronize()
            s2.synchronize()
            np.testing.assert_array_equal(o1.cpu().numpy().view(np.uint64), want[0][0])
            np.testing.assert_array_equal(i1[:total].cpu().numpy().view(np.uint32), want[0][1])
            sub = sub_lists(want[TRI], BIG)
            np.testing.assert_array_equal(o2.cpu().numpy().view(np.uint64), sub[0])
            np.testing.assert_array_equal(i2.cpu().numpy().view(np.uint32), sub[1])
            assert ctx.region_counts()["accepted_subtrees"] > 0 and ctx.region_split_counts()["k"] == 64
            ctx.synchronize()
            ctx.refit()                                          # a new tree epoch: the word is written again


# ---------------------------------------------------------------- 7. errors
def test_errors():
    import torch
    big = np.float32(3e38)
    regions = rt.box_region(np.full((4, 3), -big, np.float32), np.full((4, 3), big, np.float32))
    off = np.zeros(5, np.uint64)
    ids = np.zeros(64, np.uint32)
    out = np.zeros(4, np.uint64)
    L = rt.lib()
    K64 = FIELDS["K64"]
    with rt.Context(device=0) as ctx:
        ctx.set_scene(rg.fixture_scene("Rect"))
        ctx.set_camera(*rt.camera_reference(rg.W, rg.H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.region(regions, mode=AUTO)
        assert e.value.status == NOT_READY
        o, p = ctx.region(regions[:0], mode=AUTO)    # n == 0 is OK even before a build
        assert o.tolist() == [0] and p.shape == (0,)
        ctx.build()
        h = ctx._h
        assert L.rtbvh_region_split_counts(h, rg.vp(out)) == NOT_READY
        assert L.rtbvh_region_split_counts(h, None) == INVALID_ARG
        assert L.rtbvh_region_split_counts(None, rg.vp(out)) == INVALID_ARG
        dr = torch.from_numpy(regions.view(np.float32).reshape(-1, 24).copy()).cuda()
        doff = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        dids = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bad = [13 << 16, 14 << 16, 13 << 16 | COUNT, 14 << 16 | TRI, 1 << 20, 1 << 15]
        bad += [f | b for f in (K64, AUTO) for b in (1, 2, 1 << 7, 1 << 8, 1 << 31, SIZES | FILL, SIZES | FILL | TRI)]
        for mode in bad:
            assert L.rtbvh_region_async(h, rg.vp(dr), 4, rg.vp(doff), rg.vp(dids), 64, mode, None) == INVALID_ARG, hex(mode)
            assert L.rtbvh_region_host(h, rg.vp(regions), 4, rg.vp(off), rg.vp(ids), 64, mode) == INVALID_ARG, hex(mode)
        assert L.rtbvh_region_async(h, None, 0, None, None, 0, 13 << 16, None) == INVALID_ARG      # n == 0 too
        assert L.rtbvh_region_async(h, None, 4, rg.vp(doff), rg.vp(dids), 64, K64, None) == INVALID_ARG
        assert L.rtbvh_region_async(h, rg.vp(dr), 4, None, rg.vp(dids), 64, K64, None) == INVALID_ARG
        assert L.rtbvh_region_async(h, rg.vp(dr), 4, rg.vp(doff), None, 64, K64, None) == INVALID_ARG
        assert L.rtbvh_region_async(h, rg.vp(dr), 4, rg.vp(doff), None, 64, K64 | FILL, None) == INVALID_ARG
        assert L.rtbvh_region_async(h, rg.vp(dr), 1 << 31, rg.vp(doff), rg.vp(dids), 64, K64, None) == INVALID_ARG
        ctx.synchronize()
        assert (doff.cpu().numpy() == -1).all() and (dids.cpu().numpy() == -1).all()   # nothing was written
        assert not off.any() and not ids.any()
        assert L.rtbvh_region_split_counts(h, rg.vp(out)) == NOT_READY
        ctx.region(regions, mode=COUNT)              # a counting query without a field does not make them ready
        assert L.rtbvh_region_split_counts(h, rg.vp(out)) == NOT_READY
        ctx.region(regions, mode=K64)                # nor a split query that does not count
        assert L.rtbvh_region_split_counts(h, rg.vp(out)) == NOT_READY
        assert L.rtbvh_region_async(h, rg.vp(dr), 4, rg.vp(doff), None, 64, K64 | SIZES | COUNT, None) == OK
        assert L.rtbvh_region_split_counts(h, rg.vp(out)) == OK
        assert out.tolist() == [64, 4, 0, 0]         # four roots taken whole
        assert doff.cpu().numpy().tolist() == [0, 12, 24, 36, 48]
        ctx.update_vertices(np.ascontiguousarray(rg.fixture_scene("Rect").vertices[:, :3]))
        with pytest.raises(rt.RtbvhError) as e:     # a stale tree
            ctx.region(regions, mode=AUTO)
        assert e.value.status == NOT_READY
        ctx.refit()
        d = rg.load_scene_fixture("Rect")
        tris = rw.clip_triangles(d["vertices"], d["indices"], rt.camera_reference(rg.W, rg.H)[0])
        rg.assert_region_equal(ctx.region(regions, mode=AUTO), rr.brute_region(tris, regions, wr.rank_of(ctx.read_sorted()[1])))
        ctx.synchronize()
