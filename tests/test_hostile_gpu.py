"""The build, the refit, the trace and every query kind on hostile geometry (tests/hostile_scenes.py): needles,
collinear triangles, duplicates, one-ulp slivers, denormal and overflowing coordinates, NaN and infinite vertices,
mixed into a wavy grid at real tree depth.  Every comparison is bit for bit, against the CPU oracle (build, refit,
trace, the reference-order ray walk) or the kind's brute force over all triangles, through the assertion helpers of
the kind's own test module.  tests/test_hostile_cpu.py shows without a GPU that these scenes tell a wrong kernel
from a right one.

The variants name the cause of a failure: `degenerate` (finite, a finite root box: the certified walks and the
*_SORT orders stay engaged), `huge` (+ 1e25 triangles), `nonfinite` (`degenerate` + NaN and inf), `all`."""
import functools

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import allhits_ref as ar
from tests import cross_ref as xr
from tests import hostile_scenes as hs
from tests import khits_ref as kh
from tests import knn_ref as kr
from tests import nearest_ref as nr
from tests import overlap_ref as ovr
from tests import ray_walk_ref as rw
from tests import signed_ref as sr
from tests import within_ref as wr
from tests.test_allhits_gpu import assert_allhits_equal
from tests.test_collide_gpu import MODE_IDS as COLLIDE_IDS
from tests.test_collide_gpu import MODES as COLLIDE_MODES
from tests.test_collide_gpu import assert_collide_equal
from tests.test_cross_gpu import assert_cross_equal
from tests.test_gpu_parity import TRACE_MODES
from tests.test_khits_gpu import assert_khits_equal
from tests.test_knn_gpu import assert_knn_equal
from tests.test_nearest_gpu import assert_nearest_equal
from tests.test_overlap_gpu import assert_overlap_equal
from tests.test_query_gpu import assert_genuine, assert_hits_equal
from tests.test_signed_gpu import assert_records_equal
from tests.test_within_gpu import assert_within_equal

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
FORMS = {"records": 0, "node boxes": rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD}
SMALL = [(v, c, 12) for v in hs.VARIANTS for c in hs.CAMERAS]
CASES = SMALL + [("all", c, 64) for c in hs.CAMERAS]
FRAMES = [(64, 48), (97, 53)]
TOPOLOGY = ("parent", "child_l", "child_r", "code", "index")


def case_id(p):
    return f"{p[0]}-{p[1]}-G{p[2]}"


# ---------------------------------------------------------------- the CPU side of a case, computed once
class Ref:
    """A variant under one camera: its BVH-space triangles, the oracle's tree and sort order, the inputs, and each
    kind's reference answers (computed when first asked for, shared by both tree forms)."""

    def __init__(self, variant, cam, G):
        self.h = hs.hostile(variant, G)
        self.variant, self.G, self.T = variant, G, self.h.T
        self.wvp, self.wv = hs.camera(cam)
        self.tris = self.h.tris(self.wvp)
        self.nodes = orc.build(hs.oracle_scene(self.h.scene), self.wvp)
        self.order = self.nodes["index"][:self.T] // 3
        self.rank = wr.rank_of(self.order)
        self.inp = hs.Inputs(self.tris, self.h.labels)
        self.finite_box = bool(np.isfinite(self.nodes[self.T]["bb_min"]).all() and
                               np.isfinite(self.nodes[self.T]["bb_max"]).all())

    @functools.cached_property
    def ans(self):
        return Answers(self.tris, self.h.indices, self.inp)

    @functools.cached_property
    def closest(self):
        return rw.walk(self.nodes, self.tris, self.inp.ray_o, self.inp.ray_d)

    @functools.cached_property
    def collide(self):
        return self.ans.collide(self.rank)


def by_rank(off, items, tri, rank):
    """The items of CSR lists, each list put into ascending rank[tri]."""
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    return items[np.lexsort((np.asarray(rank)[np.asarray(tri).astype(np.int64)], owner))]


class Answers:
    """Each kind's brute force over (tris, inputs), computed when first asked for.  The members of the list kinds do
    not depend on the tree, only their order does: they are kept in triangle order and put into a tree's sort order
    by `by_rank`, so a refitted tree of another order reuses them."""

    def __init__(self, tris, indices, inp):
        self.tris, self.indices, self.inp, self.T = tris, indices, inp, len(tris)
        self.ids = np.arange(self.T)

    @functools.cached_property
    def nearest(self):
        return nr.brute(self.tris, self.inp.points)

    @functools.cached_property
    def dist2(self):
        return kr.dist2_matrix(self.tris, self.inp.points)

    @functools.cached_property
    def bound(self):
        """A radius (squared) that lists about ten triangles a point: the median of the points' tenth distances."""
        d = np.where(np.isnan(self.dist2[0]), INF, self.dist2[0])
        return np.float32(np.median(np.sort(d, 1)[:, 9]))

    @functools.cached_property
    def _within(self):
        return wr.brute_within(self.tris, self.inp.points, self.bound, self.ids)

    def within(self, rank):
        off, pairs = self._within
        return off, by_rank(off, pairs, pairs["tri"], rank)

    @functools.cached_property
    def members(self):
        return kh.members(self.tris, self.inp.ray_o, self.inp.ray_d)

    def allhits(self, rank, with_mn=False):
        off, hits, mn = self.members
        out = (off, by_rank(off, hits, hits["tri"], rank))
        return out + (by_rank(off, mn, hits["tri"], rank),) if with_mn else out

    @functools.cached_property
    def _overlap(self):
        return {m: ovr.brute_overlap(self.tris, self.inp.qlo, self.inp.qhi, self.ids, bool(m)) for m in (0, rt.OVERLAP_TRIANGLE)}

    def overlap(self, m, rank):
        off, ids = self._overlap[m]
        return off, by_rank(off, ids, ids, rank)

    @functools.cached_property
    def signed_vote3(self):
        return sr.brute(self.tris, self.inp.points, vote3=True)

    @functools.cached_property
    def _pairs(self):
        from tests import collide_ref as cr
        return {0: cr.member_pairs(self.tris, self.indices, False), rt.COLLIDE_TRIANGLE: cr.member_pairs(self.tris, self.indices, True)}

    def collide(self, rank):
        from tests import collide_ref as cr
        return {m: cr.csr(self._pairs[m & rt.COLLIDE_TRIANGLE], rank, self.T, bool(m & rt.COLLIDE_SYMMETRIC))
                for m in COLLIDE_MODES}

    @functools.cached_property
    def _cross(self):
        return xr.brute_cross(self.tris, self.inp.queries, self.ids)

    def cross(self, rank):
        off, ids = self._cross
        return off, by_rank(off, ids, ids, rank)


@functools.lru_cache(maxsize=None)
def ref(variant, cam, G):
    return Ref(variant, cam, G)


def context(scene, wvp, wv, **kw):
    ctx = rt.Context(device=0, **kw)
    ctx.set_scene(scene)
    ctx.set_camera(wvp, wv)
    return ctx


@pytest.fixture(scope="module", params=[(c, f) for c in CASES for f in FORMS],
                ids=lambda p: case_id(p[0]) + "-" + p[1].replace(" ", "-"))
def built(request):
    """(Ref, a context built over the variant in one tree form).  The sort order is the oracle's, so the reference
    lists (ordered by it) are shared by both forms."""
    case, form = request.param
    r = ref(*case)
    ctx = context(r.h.scene, r.wvp, r.wv, flags=FORMS[form])
    ctx.build()
    np.testing.assert_array_equal(ctx.read_sorted()[1], r.order)
    yield r, ctx
    ctx.close()


def assert_nodes_equal(got, want, what=""):
    """Topology, codes and indices as integers; boxes as floats with NaN equal to NaN (where both inputs of a min are
    NaN the payload is not part of the contract)."""
    for f in TOPOLOGY:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")
    for f in ("bb_min", "bb_max"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")


# ---------------------------------------------------------------- 1. build
@pytest.mark.parametrize("morton", [rt.MORTON_CPUTESTS, rt.MORTON_HLSL], ids=["cputests", "hlsl"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_build_matches_oracle(case, morton):
    r = ref(*case)
    s = r.h.scene
    with context(s, r.wvp, r.wv, morton_mode=morton) as c:
        c.build()
        codes = c.read_morton()
        keys, ids = c.read_sorted()
        nodes = c.read_bvh()
    osc = hs.oracle_scene(s)
    ocodes = orc.morton_tris(osc, morton, r.wvp, (-700,) * 3, (700,) * 3)
    np.testing.assert_array_equal(codes, ocodes)
    perm = orc.split_sort(ocodes)
    np.testing.assert_array_equal(ids, perm)
    np.testing.assert_array_equal(keys, ocodes[perm])
    assert_nodes_equal(nodes, orc.build(osc, r.wvp, morton_mode=morton, sort_mode=0))
    if morton == rt.MORTON_CPUTESTS:
        assert_nodes_equal(nodes, r.nodes, "the default sort")
    nan = np.isnan(nodes["bb_min"]).any(1)
    assert int(nan.sum()) >= (4 if r.variant in hs.NONFINITE_VARIANTS else 0)   # (G = 64: 32 all-NaN leaves)


def same_words(a, b):
    """uint32 records equal word for word, a NaN standing for any NaN."""
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    with np.errstate(all="ignore"):
        return bool(((a == b) | (np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32)))).all())


@pytest.mark.parametrize("modes", [(0, 0), (1, 0), (0, 1)], ids=["cputests", "hlsl", "cputests-delta"])
@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_one_workgroup_build_equals_multi_kernel_build(case, modes):
    r = ref(*case)
    out = []
    for flags in (0, rt.FLAG_MULTI_KERNEL_BUILD):
        with context(r.h.scene, r.wvp, r.wv, flags=flags, morton_mode=modes[0], delta_mode=modes[1]) as c:
            c.build()
            out.append((c.read_bvh(), c.read_morton(), c.read_sorted(), c.read_wide()))
    a, b = out
    assert_nodes_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        np.testing.assert_array_equal(x, y)
    assert same_words(a[3], b[3])


# ---------------------------------------------------------------- 2. refit
def leaf_boxes(tris):
    return nr.leaf_data(tris)[3:]


def check_kinds(ctx, ans, nodes, what, full=True):
    """One call of every query kind against its reference (`ans`, an Answers), in the sort order of `nodes`."""
    tris, inp, T = ans.tris, ans.inp, ans.T
    rank = wr.rank_of(nodes["index"][:T] // 3)
    pts, o, d = inp.points, inp.ray_o, inp.ray_d
    rays = rt.make_rays(o, d)
    walked = rw.walk(nodes, tris, o, d)
    assert_nearest_equal(ctx.nearest(pts), ans.nearest, what + " nearest")
    assert_overlap_equal(ctx.overlap(inp.qlo, inp.qhi), ans.overlap(0, rank), what + " overlap")
    assert_hits_equal(ctx.query(rays), walked, what + " query")
    if not full:
        return
    assert_within_equal(ctx.within(pts, ans.bound), ans.within(rank), what + " within")
    assert_knn_equal(ctx.knn(pts, hs.KNN_K), kr.select_k(*ans.dist2, hs.KNN_K), what + " knn")
    assert_hits_equal(ctx.query(rays, rt.QUERY_CERTIFIED), walked, what + " certified query")
    assert_allhits_equal(ctx.allhits(rays), ans.allhits(rank), what + " allhits")
    assert_khits_equal(ctx.khits(rays, hs.KHITS_K), kh.select_k(ans.members, hs.KHITS_K), what + " khits")
    assert_overlap_equal(ctx.overlap(inp.qlo, inp.qhi, mode=rt.OVERLAP_TRIANGLE), ans.overlap(rt.OVERLAP_TRIANGLE, rank),
                         what + " overlap, triangles")
    assert_records_equal(ctx.signed(pts, mode=rt.SIGNED_VOTE3), ans.signed_vote3, what + " signed")
    want = ans.collide(rank)
    for m in (rt.COLLIDE_TRIANGLE, rt.COLLIDE_SYMMETRIC):
        assert_collide_equal(ctx.collide(m), want[m], what + " collide")
    assert_cross_equal(ctx.cross(rt.make_tris(inp.queries)), ans.cross(rank), what + " cross")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_refit_to_hostile_positions_and_back(case, form):
    """The clean base (every hostile slot holding a clean copy) built, moved to the hostile positions and refitted:
    the build's topology, the oracle's refit of the hostile leaf boxes, and every query kind's brute force.  Moved
    back and refitted: no NaN or inf is left in a node box, and the clean answers.  Rebuilt: a fresh context's tree.
    (G = 64, the multi-kernel refit: every kind on the hostile positions, whose references the query tests share;
    back on the clean ones the boxes, nearest, overlap and query -- a second set of brute forces over 9,248 triangles
    would take this test past a few seconds, and G = 12 runs every kind there in both forms.)"""
    r = ref(*case)
    h = r.h
    clean_tris = h.tris(r.wvp, clean=True)
    clean = Answers(clean_tris, h.indices, hs.Inputs(clean_tris, np.zeros(h.T, np.int64)))
    with context(h.clean, r.wvp, r.wv, flags=FORMS[form]) as ctx:
        ctx.build()
        tree0 = ctx.read_bvh()
        order0 = ctx.read_sorted()[1].copy()
        T = h.T
        par, cl, cr_ = (np.ascontiguousarray(tree0[f]) for f in ("parent", "child_l", "child_r"))
        for what, P, ans in (("hostile", h.positions, r.ans), ("clean", h.clean_positions, clean)):
            tris = ans.tris
            ctx.update_vertices(P)
            ctx.refit()
            np.testing.assert_array_equal(ctx.read_sorted()[1], order0)
            tree = ctx.read_bvh()
            for f in TOPOLOGY:
                np.testing.assert_array_equal(tree[f], tree0[f], err_msg=f"{what} {f}")
            lo, hi = leaf_boxes(tris[tree0["index"][:T] // 3])
            bmin, bmax = np.zeros((2 * T - 1, 3), np.float32), np.zeros((2 * T - 1, 3), np.float32)
            bmin[:T], bmax[:T] = lo, hi
            bmin, bmax, _ = orc.refit(T, par, cl, cr_, bmin, bmax)
            np.testing.assert_array_equal(tree["bb_min"], bmin, err_msg=what)
            np.testing.assert_array_equal(tree["bb_max"], bmax, err_msg=what)
            if what == "clean":
                assert np.isfinite(tree["bb_min"]).all() and np.isfinite(tree["bb_max"]).all()
                np.testing.assert_array_equal(tree["bb_min"], tree0["bb_min"])
                np.testing.assert_array_equal(tree["bb_max"], tree0["bb_max"])
            elif r.variant in hs.NONFINITE_VARIANTS:
                assert np.isnan(tree["bb_min"][:T]).any() and np.isinf(tree["bb_min"][T]).all()
            check_kinds(ctx, ans, tree, what, full=what == "hostile" or r.G == 12)
        ctx.build()
        with context(h.clean, r.wvp, r.wv, flags=FORMS[form]) as fresh:
            fresh.build()
            assert_nodes_equal(ctx.read_bvh(), fresh.read_bvh(), "rebuild")
            assert same_words(ctx.read_wide(), fresh.read_wide())


# ---------------------------------------------------------------- 3. trace
@functools.lru_cache(maxsize=None)
def oracle_frame(variant, cam, W, H):
    h = hs.hostile(variant)
    wvp, wv = hs.camera(cam, W, H)
    osc = hs.oracle_scene(h.scene)
    nodes = orc.build(osc, wvp)
    fb, inten, st = orc.trace(osc, nodes, wvp, wv, W, H, 1, want_intensity=True)
    return wvp, wv, nodes, fb, inten, st


@pytest.mark.parametrize("mode", list(TRACE_MODES))
@pytest.mark.parametrize("W,H", FRAMES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_trace_matches_oracle(case, W, H, mode):
    """One bounce, every trace mode: the oracle's framebuffer and intensity, no stack overflow.  On `degenerate` the
    certified mode certifies every ray (a fallback for every ray would make the comparison empty); on the variants
    with an infinite root box it re-traces every bounce ray and no primary ray, by design (include/rtbvh.h)."""
    variant, cam, _ = case
    wvp, wv, nodes, ofb, oint, ost = oracle_frame(variant, cam, W, H)
    assert ost["hits"] >= (W * H // 10 if cam == "reference" else 100) and ost["bounce"] > 0
    with context(hs.hostile(variant).scene, wvp, wv, flags=TRACE_MODES[mode] | rt.FLAG_COUNT_VISITS) as c:
        c.compute_bvh(W, H, 1)
        fb, inten, st = c.read_framebuffer(), c.read_intensity(), c.stats()
        assert_nodes_equal(c.read_bvh(), nodes)
    assert not np.isnan(ofb).any()
    np.testing.assert_array_equal(fb, ofb)
    np.testing.assert_array_equal(inten, oint)
    assert st["stack_overflows"] == 0
    assert sum(st["hits"]) == ost["hits"] and st["bounce_rays"] == ost["bounce"]
    if mode == "certified":
        redo = st["redo_rays"]
        print(f"{variant} {cam} {W}x{H}: certified trace re-traced {redo[0]} of {st['primary_rays']} primary and "
              f"{redo[1]} of {st['bounce_rays']} bounce rays ({st['redo_deferred']} deferred)")
        assert st["walk_state"] == 2 and st["cert_traces"] == 1
        if variant == "degenerate":               # a finite root box: every ray of the frame is certified
            assert list(redo) == [0, 0] and st["redo_deferred"] == 0
        if variant in hs.NONFINITE_VARIANTS:      # an infinite one: no QNode frame at the root, every bounce ray
            assert redo[0] == 0 and redo[1] == st["bounce_rays"] > 0      # is re-traced; the binned primary pass: none


# ---------------------------------------------------------------- 4. the query kinds
@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_lists_put_into_rank_order_are_the_brute_forces(case):
    """No GPU: Answers keeps the list kinds' members in triangle order and sorts them by a tree's rank; that is
    each kind's own brute force called with that rank."""
    from tests.test_collide_gpu import brute as collide_brute
    r = ref(*case)
    a, inp, rank = r.ans, r.inp, r.rank
    assert_within_equal(a.within(rank), wr.brute_within(r.tris, inp.points, a.bound, rank))
    assert_allhits_equal(a.allhits(rank), ar.brute_allhits(r.tris, inp.ray_o, inp.ray_d, INF, rank))
    for m in (0, rt.OVERLAP_TRIANGLE):
        assert_overlap_equal(a.overlap(m, rank), ovr.brute_overlap(r.tris, inp.qlo, inp.qhi, rank, bool(m)))
    assert_cross_equal(a.cross(rank), xr.brute_cross(r.tris, inp.queries, rank))
    want = collide_brute(r.tris, r.h.indices, rank)
    for m in COLLIDE_MODES:
        assert_collide_equal(a.collide(rank)[m], want[m])


def test_nearest(built):
    r, ctx = built
    pts, want = r.inp.points, r.ans.nearest
    assert want["found"].all() and (want["ties"] > 1).sum() >= 32
    assert_nearest_equal(ctx.nearest(pts), want)
    assert_nearest_equal(ctx.nearest(pts, mode=rt.NEAREST_SORT | rt.NEAREST_COUNT), want, "SORT | COUNT")
    assert ctx.nearest_counts()["found"] == len(pts)
    # the bounds of test_nearest_gpu.test_max_dist2_around_each_answer
    d = want["dist2"]
    k = np.arange(len(d)) % 4
    bound = np.where(k == 0, np.float32(.5) * d, np.where(k == 1, d, np.where(k == 2, np.nextafter(d, np.float32(0)),
                                                                             np.float32(4) * d))).astype(np.float32)
    bounded = nr.brute(r.tris, pts, bound)
    pos = (d > 0) & np.isfinite(d)      # (a point 1e25 away: dist2 = +inf, which half of it and +inf still admit)
    assert not bounded["found"][pos & ((k == 0) | (k == 2))].any() and bounded["found"][(k == 1) | (k == 3)].all()
    assert_nearest_equal(ctx.nearest(pts, bound), bounded, "bounded")
    assert_nearest_equal(ctx.nearest(pts, bound, mode=rt.NEAREST_SORT), bounded, "bounded, SORT")
    assert_nearest_equal(ctx.nearest(pts, INF), want, "bound +inf")


def test_within(built):
    r, ctx = built
    pts = r.inp.points
    bound = r.ans.bound
    want = r.ans.within(r.rank)
    per = int(want[0][-1]) / len(pts)
    assert 7 <= per <= 13           # about ten triangles a point (8.5 to 10.5 over the cases)
    assert_within_equal(ctx.within(pts, bound), want)
    assert_within_equal(ctx.within(pts, bound, mode=rt.WITHIN_SORT | rt.WITHIN_COUNT, capacity=int(want[0][-1])),
                        want, "SORT | COUNT")
    assert ctx.within_counts()["pairs"] == int(want[0][-1])
    sub = np.ascontiguousarray(pts[::8])                     # +inf: every triangle whose dist2 is no NaN
    every = wr.brute_within(r.tris, sub, INF, r.rank)
    lists = np.diff(every[0]).astype(np.int64)
    nan_tris = int(np.isnan(r.ans.dist2[0][::8]).all(0).sum())
    assert (lists <= r.T).all() and lists.max() == r.T - nan_tris
    assert_within_equal(ctx.within(sub, INF), every, "+inf")
    assert_within_equal(ctx.within(sub, INF, mode=rt.WITHIN_SORT), every, "+inf, SORT")


@pytest.mark.parametrize("k", [1, 8, 32])
def test_knn(built, k):
    r, ctx = built
    pts = r.inp.points
    d, finite = r.ans.dist2
    want = kr.select_k(d, finite, k)
    assert (want[0] != kr.NONE).all()
    assert_knn_equal(ctx.knn(pts, k), want)
    assert_knn_equal(ctx.knn(pts, k, mode=rt.KNN_SORT | rt.KNN_COUNT), want, "SORT | COUNT")
    dj = want[1][:, k - 1]
    bound = np.where(np.arange(len(dj)) % 2 == 0, dj, np.nextafter(dj, np.float32(0))).astype(np.float32)
    assert_knn_equal(ctx.knn(pts, k, bound), kr.select_k(d, finite, k, bound), "bounded")
    if k == 1:   # the header: with k = 1 the pair is the closest-point query's
        near = ctx.nearest(pts)
        got = ctx.knn(pts, 1)
        np.testing.assert_array_equal(got["tri"][:, 0], near["tri"])
        np.testing.assert_array_equal(nr.bits(got["dist2"][:, 0]), nr.bits(near["dist2"]))
        np.testing.assert_array_equal(got["tri"][:, 0], r.ans.nearest["tri"])


@pytest.mark.parametrize("limited", [False, True], ids=["inf", "t_max"])
def test_query(built, limited):
    """Closest and any hit; plain, QUERY_CERTIFIED, QUERY_SORT; with and without t_max: the reference-order walk of
    the oracle's tree (the build test shows the context's tree is that tree)."""
    r, ctx = built
    o, d = r.inp.ray_o, r.inp.ray_d
    want = r.closest
    assert want["hit"].sum() >= 50 and not want["hit"].all()    # (G = 64, identity: most triangles have |det| < 0.01)
    t_max = np.full(len(o), INF, np.float32)
    if limited:   # around each ray's own closest t: 0.5 t, t exactly, the float below t (misses: 10)
        t = want["t"]
        k = np.arange(len(t)) % 3
        t_max = np.where(want["hit"], np.where(k == 0, np.float32(.5) * t, np.where(k == 1, t, np.nextafter(t, np.float32(0)))),
                         np.float32(10)).astype(np.float32)
        want = rw.walk(r.nodes, r.tris, o, d, t_max=t_max)
        assert (r.closest["hit"] & ~want["hit"]).any()
    rays = rt.make_rays(o, d, t_max)
    CERT, SORT, COUNT, ANY = rt.QUERY_CERTIFIED, rt.QUERY_SORT, rt.QUERY_COUNT, rt.QUERY_ANY
    for mode in (0, SORT, CERT, CERT | SORT | COUNT):
        assert_hits_equal(ctx.query(rays, mode), want, f"mode {mode}")
    wc = ctx.query_walk_counts()
    assert sum(wc.values()) == len(o)
    print(f"{r.variant} G={r.G}: certified query walk counts {wc}")
    if r.finite_box:      # a finite QNode frame at the root: the certified walk must take rays
        assert wc["certified"] > len(o) // 2 and wc["fallback"] == 0
    else:                 # none at the root: every covered ray is re-traced in the reference order, by design
        assert wc["certified"] == 0 and wc["fallback"] == 0 and wc["redone"] > len(o) // 2
    for mode in (ANY, ANY | SORT, ANY | CERT, ANY | CERT | SORT | COUNT):
        got = ctx.query(rays, mode)
        np.testing.assert_array_equal(got["t"] != -1, want["hit"], err_msg=f"any-hit, mode {mode}")
        assert_genuine(got, r.tris, o, d, t_max)
    assert ctx.query_counts()["hits"] == int(want["hit"].sum())


def test_allhits(built):
    r, ctx = built
    o, d = r.inp.ray_o, r.inp.ray_d
    off, hits, mn = r.ans.members                                  # (in triangle order: the lists' contents)
    want = r.ans.allhits(r.rank)
    assert int(want[0][-1]) == len(hits) >= 50 and (np.diff(want[0].astype(np.int64)) >= 2).sum() >= 5
    rays = rt.make_rays(o, d)
    assert_allhits_equal(ctx.allhits(rays), want)
    assert_allhits_equal(ctx.allhits(rays, mode=rt.ALLHITS_SORT | rt.ALLHITS_COUNT, capacity=len(hits)), want, "SORT | COUNT")
    assert ctx.allhits_counts()["hits"] == len(hits)
    by_t = (want[0], ar.order_by_t(*want))
    assert_allhits_equal(ctx.allhits(rays, mode=rt.ALLHITS_BY_T), by_t, "BY_T")
    assert_allhits_equal(ctx.allhits(rays, mode=rt.ALLHITS_BY_T | rt.ALLHITS_SORT, capacity=len(hits)), by_t, "BY_T | SORT")
    # every third ray: the t of its first member exactly or the float below it, in turn (no member: 10)
    woff, whits, wmn = r.ans.allhits(r.rank, with_mn=True)
    cnt = np.diff(woff.astype(np.int64))
    tm = np.full(len(o), INF, np.float32)
    for k in range(0, len(o), 3):
        t = whits["t"][int(woff[k])] if cnt[k] else np.float32(10)
        tm[k] = t if k % 2 == 0 or not cnt[k] else np.nextafter(t, np.float32(0))
    cut = ar.cut(woff, whits, wmn, tm)
    assert int(cut[0][-1]) < len(hits)
    assert_allhits_equal(ctx.allhits(rt.make_rays(o, d, tm)), cut, "mixed t_max")


@pytest.mark.parametrize("k", [1, 4, 16])
def test_khits(built, k):
    r, ctx = built
    o, d = r.inp.ray_o, r.inp.ray_d
    want = kh.select_k(r.ans.members, k)
    assert kh.found(want)[:, 0].sum() >= 50
    rays = rt.make_rays(o, d)
    assert_khits_equal(ctx.khits(rays, k), want)
    assert_khits_equal(ctx.khits(rays, k, mode=rt.KHITS_SORT | rt.KHITS_COUNT), want, "SORT | COUNT")
    assert ctx.khits_counts()["found"] == int(kh.found(want).sum())
    tm = np.where(np.arange(len(o)) % 2 == 0, INF, np.float32(2.5)).astype(np.float32)
    assert_khits_equal(ctx.khits(rt.make_rays(o, d, tm), k), kh.select_k(r.ans.members, k, tm), "mixed t_max")
    np.testing.assert_array_equal(kh.found(want)[:, 0], r.closest["hit"])


@pytest.mark.parametrize("m", [0, rt.OVERLAP_TRIANGLE], ids=["boxes", "triangles"])
def test_overlap(built, m):
    r, ctx = built
    qlo, qhi = r.inp.qlo, r.inp.qhi
    want = r.ans.overlap(m, r.rank)
    total = int(want[0][-1])
    assert 0 < total < len(qlo) * r.T
    assert_overlap_equal(ctx.overlap(qlo, qhi, mode=m), want)
    assert_overlap_equal(ctx.overlap(rt.make_boxes(qlo, qhi), mode=m | rt.OVERLAP_SORT | rt.OVERLAP_COUNT, capacity=total),
                         want, "SORT | COUNT")
    assert ctx.overlap_counts()["ids"] == total


def test_signed(built):
    r, ctx = built
    pts = r.inp.points
    for mode, kw in ((0, {}), (rt.SIGNED_VOTE3, {"vote3": True}), (rt.SIGNED_INSIDE_ONLY, {"inside_only": True}),
                     (rt.SIGNED_VOTE3 | rt.SIGNED_SORT | rt.SIGNED_COUNT, {"vote3": True})):
        want = sr.brute(r.tris, pts, **kw)
        if not kw.get("inside_only"):
            for f in ("tri", "dist2"):
                np.testing.assert_array_equal(want[f], r.ans.nearest[f])
        assert_records_equal(ctx.signed(pts, mode=mode), want, f"mode {mode}")
    assert 0 < ctx.signed_counts()["inside"] == int((want["flags"] & 1).sum()) < len(pts)


@pytest.mark.parametrize("m", COLLIDE_MODES, ids=COLLIDE_IDS)
def test_collide(built, m):
    """All four modes.  The repeated-index triangles exercise the common-vertex rule (N): their triples (i, i, j)
    share an index with every base triangle around i or j."""
    r, ctx = built
    want = r.collide[m]
    total = int(want[0][-1])
    assert total > 0
    assert_collide_equal(ctx.collide(m), want)
    assert_collide_equal(ctx.collide(m | rt.COLLIDE_COUNT, capacity=total), want, "COUNT, one call")
    assert ctx.collide_counts()["entries"] == total
    hostile_rows = np.diff(want[0]).astype(np.int64)[r.h.labels == hs.cls("repeated-index")]
    assert hostile_rows.sum() > 0


def test_cross_and_cross_first(built):
    r, ctx = built
    q = r.inp.queries
    want = r.ans.cross(r.rank)
    total = int(want[0][-1])
    assert 0 < total < len(q) * r.T
    t = rt.make_tris(q)
    assert_cross_equal(ctx.cross(t), want)
    assert_cross_equal(ctx.cross(t, rt.CROSS_SORT | rt.CROSS_COUNT, capacity=total), want, "SORT | COUNT")
    assert ctx.cross_counts()["ids"] == total
    head = xr.first_of(*want)
    np.testing.assert_array_equal(ctx.cross_first(t), head)
    np.testing.assert_array_equal(ctx.cross_first(t, rt.CROSS_SORT), head)
    bad = ~xr.valid_queries(q)                                # a non-finite query: no walk
    assert (np.diff(want[0]).astype(np.int64)[bad] == 0).all() and (head[bad] == xr.NONE).all()


def test_cross_of_the_scenes_own_triangles_is_the_symmetric_collide_list(built):
    """The header's identity: the scene's own triangles as queries, the entries that share a vertex index dropped,
    are the COLLIDE_TRIANGLE | COLLIDE_SYMMETRIC lists -- row by row for the triangles that are valid queries.  A
    triangle with a non-finite vertex is no query (an empty list), while as a scene triangle its finite edges still
    cross others: its collide row is what the rows of its partners say."""
    r, ctx = built
    off, ids = xr.without_neighbours(*ctx.cross(rt.make_tris(r.tris)), r.h.indices)
    c_off, c_ids = ctx.collide(rt.COLLIDE_TRIANGLE | rt.COLLIDE_SYMMETRIC)
    assert_collide_equal((c_off, c_ids), r.collide[rt.COLLIDE_TRIANGLE | rt.COLLIDE_SYMMETRIC])
    valid = xr.valid_queries(r.tris)
    if valid.all():
        assert off.tobytes() == c_off.tobytes() and ids.tobytes() == c_ids.tobytes()
        return
    a, b = ar.segments(off, ids), ar.segments(c_off, c_ids)
    for k in np.nonzero(valid)[0]:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"triangle {k}")
    mirrored = [set() for _ in range(r.T)]
    for k in np.nonzero(valid)[0]:
        for x in b[k].tolist():
            mirrored[x].add(k)
    for k in np.nonzero(~valid)[0]:
        assert len(a[k]) == 0
        assert set(b[k].tolist()) & set(np.nonzero(valid)[0].tolist()) == mirrored[k], f"triangle {k}"
