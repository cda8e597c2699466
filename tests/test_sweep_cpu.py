"""Sphere-sweep queries without a GPU: the ABI's names, constants and layouts, make_sweeps and Context.sweep's argument
checks (which run before the library is touched), the host entries' protocol answers that need no device, the
restatement (tests/sweep_ref.py) against a float64 first-contact time, that the keys' clamp and the id tie-break are
exercised, and -- on the oracle's trees -- the lemma the GPU walk leans on: a nearer-first walk that
grows every box by r and enters it iff it passes the slab test with the best tk as the bound returns the brute force."""
import ctypes
import os
import re

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib
from tests import allhits_ref as ar
from tests import hostile_scenes as hs
from tests import nearest_ref as nr
from tests import ray_walk_ref as rw
from tests import sweep_ref as sr
from tests.conftest import REPO, load_scene_fixture

SCENES = ["Test", "Rect", "Image_Test"]
INF = sr.INF
NAMES = ("rtbvh_sweep_async", "rtbvh_sweep_host", "rtbvh_sweep_counts")


# ---------------------------------------------------------------- 1. the ABI
def test_exports_constants_and_layouts():
    L = rt.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert (rt.SWEEP_ANY, rt.SWEEP_SORT, rt.SWEEP_COUNT) == (1 << 0, 1 << 1, 1 << 2)
    assert rt.SWEEP_DTYPE.itemsize == 32 and rt.SWEEP_HIT_DTYPE.itemsize == 32
    assert rt.SWEEP_DTYPE.names == ("origin", "t_max", "direction", "radius")
    assert [rt.SWEEP_DTYPE.fields[k][1] for k in rt.SWEEP_DTYPE.names] == [0, 12, 16, 28]      # rtbvh_ray's layout
    assert [rt.RAY_DTYPE.fields[k][1] for k in rt.RAY_DTYPE.names] == [0, 12, 16, 28]
    assert rt.SWEEP_HIT_DTYPE.names == ("t", "point", "tri", "feature", "reserved")
    assert [rt.SWEEP_HIT_DTYPE.fields[k][1] for k in rt.SWEEP_HIT_DTYPE.names] == [0, 4, 16, 20, 24]
    assert rt.SWEEP_HIT_DTYPE == sr.SWEEP_HIT_DTYPE
    header = open(os.path.join(REPO, "include", "rtbvh.h")).read()
    for name, bit in (("ANY", 0), ("SORT", 1), ("COUNT", 2)):
        assert re.search(rf"RTBVH_SWEEP_{name} = 1u << {bit}\b", header), name
    for name in NAMES:
        assert re.search(rf"^rtbvh_status {name}\s*\(rtbvh_ctx\*", header, re.M), name
    assert re.search(r"rtbvh_sweep_async and rtbvh_sweep_host, and the rtbvh_read_\*", header)   # NOT_READY after an update
    assert re.search(r"^ \*  - Sweeps\.", header, re.M)                      # the degenerate-triangle section's bullet
    assert hasattr(rt.Context, "sweep") and hasattr(rt.Context, "sweep_counts")
    assert L.rtbvh_abi_version() == 8 and L.rtbvh_stats_size() == ctypes.sizeof(_lib.Stats)   # additive


def test_make_sweeps_round_trip():
    import torch
    rng = np.random.default_rng(2)
    o, d = rng.standard_normal((5, 3)).astype(np.float32), rng.standard_normal((5, 3)).astype(np.float32)
    r = rng.random(5, dtype=np.float32)
    s = rt.make_sweeps(o, d, r)
    assert s.dtype == rt.SWEEP_DTYPE and s.shape == (5,)
    np.testing.assert_array_equal(s["origin"], o)
    np.testing.assert_array_equal(s["direction"], d)
    np.testing.assert_array_equal(s["radius"], r)
    assert (s["t_max"] == INF).all()
    s1 = rt.make_sweeps(o, d, 0.25, 3.0)                                   # one radius, one t_max
    assert (s1["radius"] == np.float32(0.25)).all() and (s1["t_max"] == 3).all()
    t = rt.make_sweeps(torch.from_numpy(o), torch.from_numpy(d), torch.from_numpy(r), 3.0)
    assert tuple(t.shape) == (5, 8) and t.dtype == torch.float32
    s3 = rt.make_sweeps(o, d, r, 3.0)
    np.testing.assert_array_equal(t.numpy().view(np.uint32), s3.view(np.uint32).reshape(5, 8))   # the same bytes
    assert rt.check_sweeps(s3)[1] is not None and rt.check_sweeps(t.numpy())[1].dtype == rt.SWEEP_DTYPE
    with pytest.raises(ValueError):
        rt.make_sweeps(o, d[:4], r[:4])
    assert sr.misses(2).tobytes() == np.array([(-1, (0, 0, 0), 0xFFFFFFFF, 0, (0, 0))] * 2, rt.SWEEP_HIT_DTYPE).tobytes()


def test_bad_arguments_are_rejected_before_the_library_is_called():
    import torch
    ctx = rt.Context.__new__(rt.Context)   # no handle: any library call would fail differently
    ctx._h = None
    f32 = np.float32
    bad = [np.zeros((4, 7), f32), np.zeros((4, 4), f32), np.zeros(8, f32), np.zeros((4, 8), np.float64),
           np.zeros((8, 8), f32)[::2], np.zeros((4, 16), f32)[:, :8], np.zeros((2, 2), rt.SWEEP_DTYPE),
           np.zeros(8, rt.SWEEP_DTYPE)[::2], np.zeros(4, rt.RAY_DTYPE), [[0] * 8], None,
           torch.zeros((4, 8)), torch.zeros((4, 8), dtype=torch.float64), torch.zeros((4, 7))]
    for b in bad:
        with pytest.raises(ValueError):
            ctx.sweep(b)
    L = rt.lib()
    s = rt.make_sweeps(np.zeros((4, 3), f32), np.ones((4, 3), f32), 0.5)
    out = np.zeros(4, rt.SWEEP_HIT_DTYPE)
    cnt = np.zeros(4, np.uint64)
    p, o = ctypes.c_void_p(s.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert L.rtbvh_sweep_async(None, p, 4, o, 0, None) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_sweep_host(None, p, 4, o, 0) == _lib.ERR_INVALID_ARG
    assert L.rtbvh_sweep_counts(None, ctypes.c_void_p(cnt.ctypes.data)) == _lib.ERR_INVALID_ARG
    assert not out.view(np.uint32).any() and not cnt.any()


def test_the_precedence_of_the_host_entries_without_a_tree():
    """DESIGN.md 5p's order on a context that was never given a scene: mode bits, 2^31, n == 0, NULL arrays, no tree.
    A context needs a device to exist: where there is none, creating it fails with that status and the NULL-context
    checks above are all a host can ask (tests/test_sweep_gpu.py repeats these on a built context)."""
    try:
        ctx = rt.Context(device=0)
    except rt.RtbvhError as e:
        assert e.status == _lib.ERR_NO_DEVICE
        return
    with ctx:
        L = rt.lib()
        s = rt.make_sweeps(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32), 0.5)
        out = np.zeros(4, rt.SWEEP_HIT_DTYPE)
        p, o = ctypes.c_void_p(s.ctypes.data), ctypes.c_void_p(out.ctypes.data)
        for entry in (lambda *a: L.rtbvh_sweep_host(ctx._h, *a), lambda *a: L.rtbvh_sweep_async(ctx._h, *a, None)):
            assert entry(p, 0, o, 0) == _lib.OK                          # n == 0: nothing, even before a build
            assert entry(None, 0, None, 0) == _lib.OK
            assert entry(p, 4, o, 0) == _lib.ERR_NOT_READY
            for mode in (8, 16, 1 << 8, 1 << 31):
                assert entry(p, 4, o, mode) == _lib.ERR_INVALID_ARG, mode
                assert entry(None, 0, None, mode) == _lib.ERR_INVALID_ARG, mode   # the mode comes before n == 0
            assert entry(None, 4, o, 0) == _lib.ERR_INVALID_ARG          # NULL before NOT_READY
            assert entry(p, 4, None, 0) == _lib.ERR_INVALID_ARG
            assert entry(None, 1 << 31, None, 0) == _lib.ERR_INVALID_ARG  # 2^31 before the NULLs
        assert not out.view(np.uint32).any()
        with pytest.raises(rt.RtbvhError) as e:
            ctx.sweep_counts()
        assert e.value.status == _lib.ERR_NOT_READY


# ---------------------------------------------------------------- 2. the restatement against float64
N64 = 1500
T_MAX64 = np.float32(2)


def geometry_inputs():
    """N64 fixed-seed pairs: one random triangle with coordinates in [-1, 1] each, radii 0.01 .. 0.6, a centre in
    [-2, 2]^3 moving towards a point near the triangle (so that most sweeps touch it), a tenth of them started within
    reach of it."""
    rng = np.random.default_rng(20240611)
    tris = rng.uniform(-1, 1, (N64, 3, 3)).astype(np.float32)
    r = rng.uniform(0.01, 0.6, N64).astype(np.float32)
    w = rng.dirichlet((1, 1, 1), N64)
    aim = (tris.astype(np.float64) * w[:, :, None]).sum(1) + rng.normal(0, 0.25, (N64, 3))
    c = rng.uniform(-2, 2, (N64, 3))
    near = rng.random(N64) < 0.1
    c[near] = aim[near] + rng.normal(0, 0.2, (int(near.sum()), 3))
    d = (aim - c) * rng.uniform(0.3, 1.5, (N64, 1))
    return tris, c.astype(np.float32), d.astype(np.float32), r


def dist64(tris, p):
    """The float64 distance of the points p[k] to triangle k over the recovered vertices V0, V1 = fl(a + e1),
    V2 = fl(a + e2): nearest_ref's formulas in double precision, no box clamp."""
    a, e1, e2, _, _ = nr.leaf_data(tris)
    v0, v1, v2 = (x.astype(np.float64) for x in (a, (a + e1).astype(np.float32), (a + e2).astype(np.float32)))
    big = np.full_like(v0, np.inf)
    return np.sqrt(nr.tri_dist2(p, v0, v1 - v0, v2 - v0, -big, big)[0])


def first_contact64(tris, c, d, r, t_max, scan=2001, halvings=60):
    """(hit, t, margin): the float64 first-contact time of each pair by a dense scan of g(t) = dist(c + t d) - r over
    [0, t_max] then `halvings` bisections, and the margin min |g| decides by: g is convex in t (the distance of a
    point on a line to a convex set), so its minimum over [0, t_max] is refined by a ternary search."""
    c, d, r = c.astype(np.float64), d.astype(np.float64), r.astype(np.float64)
    g = lambda t: dist64(tris, c + t[:, None] * d) - r   # noqa: E731
    ts = np.linspace(0, float(t_max), scan)
    G = np.stack([g(np.full(len(c), t)) for t in ts], 1)
    neg = G <= 0
    hit = neg.any(1)
    k = np.argmax(neg, 1)
    lo, hi = ts[np.maximum(k - 1, 0)], ts[k]
    for _ in range(halvings):
        mid = (lo + hi) / 2
        inside = g(mid) <= 0
        hi, lo = np.where(inside, mid, hi), np.where(inside, lo, mid)
    t = np.where(k == 0, 0.0, hi)
    a, b = np.zeros(len(c)), np.full(len(c), float(t_max))
    for _ in range(100):
        m1, m2 = a + (b - a) / 3, b - (b - a) / 3
        left = g(m1) < g(m2)
        b, a = np.where(left, m2, b), np.where(left, a, m1)
    gmin = np.minimum(np.minimum(g(a), G.min(1)), g(b))
    return hit | (gmin <= 0), t, gmin


def test_restatement_against_a_float64_first_contact():
    """Hit / miss agrees with float64 for every pair whose path does not pass within 1e-4 r of touching or clearing
    (those may be at most 2% of the cases), every feature code occurs, and t and the contact distance are accurate.
    Measured on these inputs with the restatement alone: 0 disagreements of 1,500 with none left out, 1,079 hits;
    the largest |t32 - t64| 2.53e-05, the largest |dist64(centre at t32) - r| / r 1.54e-03 (radii down to 0.01 beside
    coordinates up to 2), the reported point at most 5.13e-07 off the triangle -- the asserted bounds are twice that:
    the GPU must equal the restatement's bits, so the margin guards only against edits of the input set."""
    tris, c, d, r = geometry_inputs()
    leaves = nr.leaf_data(tris)
    tm = np.full(N64, T_MAX64, np.float32)
    _, t, pt, feature, _ = sr.pair_tests(leaves, np.arange(N64), c, d, r, tm)   # (T) alone: no box, no tree
    hit32 = feature != 0
    hit64, t64, gmin = first_contact64(tris, c, d, r, T_MAX64)
    grazing = np.abs(gmin) <= 1e-4 * r.astype(np.float64)
    assert grazing.sum() <= 0.02 * N64
    sure = ~grazing
    disagree = int((hit32 != hit64)[sure].sum())
    both = sure & hit32 & hit64
    dt = np.abs(t.astype(np.float64) - t64)[both].max()
    moving = both & (feature != 1)
    centre = c.astype(np.float64) + t.astype(np.float64)[:, None] * d.astype(np.float64)
    touch = (np.abs(dist64(tris, centre) - r) / r)[moving].max()
    # the reported point lies on the triangle, r from the centre
    on = dist64(tris, pt.astype(np.float64))[both].max()
    reach = (np.abs(np.sqrt(((centre - pt) ** 2).sum(1)) - r) / r)[moving].max()
    print(f"sweeps vs float64: {disagree} disagreements of {N64}, {int(grazing.sum())} left out, {int(both.sum())} hits; "
          f"features {np.bincount(feature, minlength=9).tolist()}; max |t32 - t64| {dt:.3g}, "
          f"max |dist - r| / r {touch:.3g}, point off the triangle {on:.3g}, |centre - point| off r {reach:.3g}")
    assert disagree == 0
    assert set(range(1, 9)) <= set(feature.tolist())
    assert dt <= 2 * 2.53e-05
    assert touch <= 2 * 1.54e-03
    assert on <= 2 * 5.13e-07 and reach <= 2 * 1.54e-03
    assert (t[feature == 1] == 0).all() and (t[hit32] >= 0).all() and (t[hit32] <= T_MAX64).all()
    assert (t[~hit32] == -1).all() and not pt[~hit32].any()


def test_sweeps_that_are_not_walked():
    tris = np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    c, d = np.tile(np.float32([0.2, 0.2, 1]), (10, 1)), np.tile(np.float32([0, 0, -1]), (10, 1))
    r, tm = np.full(10, 0.25, np.float32), np.full(10, INF, np.float32)
    nan = np.float32(np.nan)
    c[1, 0], d[2, 1], d[3] = nan, INF, 0
    r[4], r[5], r[6] = -1, nan, INF
    tm[7], tm[8] = nan, -1
    r[9], tm[9] = -0.0, 5            # -0 counts as +0
    got = sr.brute(tris, c, d, r, tm)
    assert (got["tri"] != sr.NONE).tolist() == [True] + [False] * 8 + [True]
    np.testing.assert_array_equal(sr.hit_words(got[1:9]), sr.hit_words(sr.misses(8)))
    assert got["t"][0] == np.float32(0.75) and got["feature"][0] == 2 and got["t"][9] == 1 and got["feature"][9] == 2
    assert sr.brute(tris, c[:1], d[:1], r[:1], np.float32(0.7))["tri"][0] == sr.NONE     # t_max cuts
    assert sr.brute(tris, c[:1], d[:1], r[:1], np.float32(0.75))["tri"][0] == 0          # ... inclusively
    assert sr.brute(tris, c[:1], d[:1], np.float32(1), np.float32(0))["feature"][0] == 1   # t_max = 0: the overlap


def test_degenerate_triangles_answer_through_edges_and_vertices():
    """A needle and a point (the header's section on degenerate scene triangles): no face, still touched."""
    needle = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    point = np.float32([[5, 5, 5]] * 3)
    nanv = np.full((3, 3), np.nan, np.float32)
    tris = np.stack([needle, point, nanv])
    c = np.float32([[0.5, 0, 3], [5, 5, 9], [-1, 0, 3], [0.5, 0, 3]])
    d = np.float32([[0, 0, -1], [0, 0, -1], [0, 0, -1], [1, 0, 0]])
    got = sr.brute(tris, c, d, np.float32(0.5))
    assert got["tri"].tolist() == [0, 1, sr.NONE, sr.NONE]
    assert 3 <= got["feature"][0] <= 5 and 6 <= got["feature"][1] <= 8
    assert got["t"][0] == 2.5 and got["t"][1] == 3.5
    assert not (sr.members(tris, c, d, np.float32(0.5))["tri"] == 2).any()   # all-NaN: never a member


# ---------------------------------------------------------------- 3. the keys are exercised
def scene_sweeps(tris, seed=21):
    """64 sweeps of a scene: allhits_ref's rays (axis-parallel and in-plane ones among them), radii cycled over 0,
    small and large, and finite t_max for every third."""
    o, d = ar.sample_rays(tris, 24, 8, 8, 8, seed=seed)
    lo, hi = nr.root_box(tris)
    diag = np.float32(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    r = np.float32([0, 1e-3, 5e-2, 0.1 * diag])[np.arange(len(o)) % 4]
    return o, d, r, diag


def finite_t_max(mem, n, seed=3):
    """Every third sweep that has members: the t of one of its members exactly, or the float below it, in turn."""
    rng = np.random.default_rng(seed)
    tm = np.full(n, INF, np.float32)
    for k in range(0, n, 3):
        ts = mem["t"][mem["i"] == k]
        if len(ts) == 0:
            tm[k] = 10
            continue
        t = ts[int(rng.integers(0, len(ts)))]
        tm[k] = t if k % 2 == 0 else np.nextafter(t, np.float32(-1))
    return tm


@pytest.mark.parametrize("scene", SCENES)
def test_members_below_their_grown_leaf_boxs_entry_exist(scene):
    """Members with t < mn, where the key is the box's entry and not t.  Measured with the restatement alone, 704
    sweeps a scene at radii 0, 1e-3, 5e-2 and twice the root diagonal (tests/test_sweep_gpu.py's): Test 111 of
    340,502 members, Rect 76 of 2,933, Image_Test 700 of 537,028."""
    dd = load_scene_fixture(scene)
    tris = rw.clip_triangles(dd["vertices"], dd["indices"], np.eye(4, dtype=np.float32))
    o, d = ar.sample_rays(tris, 400, 48, 200, 40)
    diag = np.float32(np.sqrt(((np.subtract(*nr.root_box(tris)[::-1])).astype(np.float64) ** 2).sum()))
    r = np.float32([0, 1e-3, 5e-2, 2 * diag])[np.arange(len(o)) % 4]
    mem = sr.members(tris, o, d, r)
    below = int((mem["t"] < mem["mn"]).sum())
    print(f"{scene}: {below} of {len(mem['t'])} members have t < mn")
    assert below > 0
    tk = sr.key_t(mem["t"], mem["mn"])
    assert (tk >= mem["t"]).all() and (tk >= mem["mn"]).all() and (tk >= 0).all() and not np.signbit(tk).any()
    # the largest radius makes every triangle a member at tk = 0: the answer is the smallest member id
    ans = sr.select(mem)
    big = (np.arange(len(o)) % 4 == 3) & sr.walked(o, d, r, np.full(len(o), INF, np.float32))   # (the edge rays' NaNs)
    assert big.sum() >= 170
    assert (ans["feature"][big] == 1).all() and (ans["t"][big] == 0).all()
    assert (ans["tri"][big] == 0).sum() >= 170                     # (an origin far outside can be out of reach of 0)
    for i in np.nonzero(big)[0]:
        assert ans["tri"][i] == mem["tri"][(mem["i"] == i) & (mem["feature"] == 1)].min()


def test_coplanar_duplicates_are_decided_by_the_id():
    """stack_scene(40): every eighth triangle repeats the one before it exactly, so both have the same t, mn and tk
    for every sweep, and where such a pair is the first contact the smaller id wins."""
    s = ar.stack_scene(40)
    tris = rw.clip_triangles(s.vertices, s.indices, np.eye(4, dtype=np.float32))
    o, d = ar.stack_rays()
    o2 = o.copy()
    o2[:, 2] = 0.1 * 40 + 0.5                                     # from above too: the last plane pair is a duplicate
    o, d = np.concatenate([o, o2]), np.concatenate([d, -d])
    r = np.float32([0, 0.02, 0.2, 0.3])[np.arange(len(o)) % 4]
    mem = sr.members(tris, o, d, r)
    ans = sr.select(mem)
    assert (ans["tri"] != sr.NONE).all()
    key = sr.keys(mem["t"], mem["mn"], np.zeros(len(mem["t"]), np.uint64)) >> np.uint64(32)
    ties = 0
    for i in range(len(o)):
        m = mem["i"] == i
        first = key[m] == key[m].min()
        if first.sum() > 1:
            ties += 1
            assert ans["tri"][i] == mem["tri"][m][first].min()
    print(f"stack_scene(40): {ties} of {len(o)} sweeps whose smallest tk is shared")
    assert ties >= 64


# ---------------------------------------------------------------- 4. the lemma, on the oracle's trees
@pytest.mark.parametrize("scene", SCENES)
def test_a_nearer_first_walk_pruned_on_the_best_key_is_the_brute_force(scene):
    dd = load_scene_fixture(scene)
    wvp = rt.camera_reference(64, 48)[0]
    osc = orc.Scene(dd["vertices"], dd["indices"], dd["mat_indices"], dd["material_blob"])
    nodes = orc.build(osc, wvp)
    tris = rw.clip_triangles(dd["vertices"], dd["indices"], wvp)
    T = len(tris)
    leaves = nr.leaf_data(tris)
    leaf_tri = (nodes["index"][:T] // 3).astype(np.int64)               # the oracle's leaves are in sort order
    np.testing.assert_array_equal(nodes["bb_min"][:T], leaves[3][leaf_tri])   # the leaf boxes are the records'
    np.testing.assert_array_equal(nodes["bb_max"][:T], leaves[4][leaf_tri])
    o, d, r, diag = scene_sweeps(tris)
    assert len(o) == 64 and (np.abs(d) == 1).any() and (d == 0).any()
    mem_inf = sr.members(tris, o, d, r)
    pruned = unpruned = clamped = 0
    for tm in (np.full(64, INF, np.float32), finite_t_max(mem_inf, 64)):
        want = sr.brute(tris, o, d, r, tm)
        assert (want["tri"] != sr.NONE).sum() >= 16 and (want["tri"] == sr.NONE).any()
        walked = sr.walked(o, d, r, tm)
        for i in range(64):
            if not walked[i]:                                       # (a t_max below 0: the float below a t of 0)
                assert want["tri"][i] == sr.NONE
                continue
            rep = lambda x, m: np.repeat(np.asarray(x)[None], m, 0)   # noqa: E731
            base, mn = sr.node_tests(nodes, o[i], d[i], r[i])
            ok, t, pt, f, mn_leaf = sr.pair_tests(leaves, leaf_tri, rep(o[i], T), rep(d[i], T), rep(r[i], T), rep(tm[i], T))
            np.testing.assert_array_equal(rw.bits(mn_leaf), rw.bits(mn[:T]))
            clamped += int((ok & (t < mn_leaf)).sum())
            tk = sr.key_t(t, mn_leaf)
            args = (nodes, base.tolist(), mn.tolist(), (f != 0).tolist(), tk.tolist(), leaf_tri.tolist(), float(tm[i]))
            got, leaves_seen = sr.walk(*args)
            pruned += leaves_seen
            unpruned += sr.walk(*args, prune=False)[1]
            if want["tri"][i] == sr.NONE:
                assert got is None, i
                continue
            j = got[2]
            rec = sr.misses(1)
            rec["t"], rec["point"], rec["tri"], rec["feature"] = t[j], pt[j], leaf_tri[j], f[j]
            np.testing.assert_array_equal(sr.hit_words(rec), sr.hit_words(want[i:i + 1]), err_msg=str(i))
    print(f"{scene}: leaves visited {pruned} pruned, {unpruned} with the bound fixed at t_max; {clamped} members "
          f"with t < mn")
    assert 0 < pruned < unpruned   # ... and the walk did prune


def test_in_plane_sweeps_need_the_child_test_without_the_infinite_axes():
    """Image_Test under the identity: walls and floor in axis planes, so their triangles' leaf boxes are flat, and the
    tests' in-plane sweeps start level with a mesh vertex and have no component along that axis (1 / d infinite).  At
    r = 0 such a leaf box passes (B) -- 0 * inf = NaN drops the axis -- while the boxes around it fail it: a walk that
    tested the children by (B) as written would lose members the sphere touches through their edges (the all-hits
    queries' one exception, DESIGN.md 5f, which a ray's triangle test never accepts).  The walk of the header, which
    leaves those axes out of a child's test, equals the brute force."""
    dd = load_scene_fixture("Image_Test")
    wvp = np.eye(4, dtype=np.float32)
    nodes = orc.build(orc.Scene(dd["vertices"], dd["indices"], dd["mat_indices"], dd["material_blob"]), wvp)
    tris = rw.clip_triangles(dd["vertices"], dd["indices"], wvp)
    T = len(tris)
    leaves = nr.leaf_data(tris)
    leaf_tri = (nodes["index"][:T] // 3).astype(np.int64)
    o, d = ar.sample_rays(tris, 0, 0, 0, 40)
    o, d = o[16:], d[16:]                                        # (past the 16 edge rays: the 40 in-plane ones)
    assert len(o) == 40 and ((d == 0).sum(1) == 1).all()
    r = np.float32([0, 0, 0, 1e-3])[np.arange(40) % 4]
    want = sr.brute(tris, o, d, r)
    lost = 0
    rep = lambda x, m: np.repeat(np.asarray(x)[None], m, 0)   # noqa: E731
    for i in range(40):
        ok, t, pt, f, mn_leaf = sr.pair_tests(leaves, leaf_tri, rep(o[i], T), rep(d[i], T), rep(r[i], T), rep(INF, T))
        tk = sr.key_t(t, mn_leaf)
        for relaxed in (True, False):
            base, mn = sr.node_tests(nodes, o[i], d[i], r[i], relaxed)
            got, _ = sr.walk(nodes, base.tolist(), mn.tolist(), (f != 0).tolist(), tk.tolist(), leaf_tri.tolist(),
                             float("inf"))
            tri = sr.NONE if got is None else got[1]
            if relaxed:
                assert tri == want["tri"][i], i
            else:
                lost += int(tri != want["tri"][i])
    print(f"Image_Test, in-plane sweeps: {int((want['tri'] != sr.NONE).sum())} of 40 hit; a walk with (B) as written "
          f"at the children answers {lost} of them differently")
    assert lost > 0


@pytest.mark.parametrize("variant,cam", [("degenerate", "reference"), ("all", "identity")])
def test_the_walk_on_hostile_scenes_is_the_brute_force(variant, cam):
    """Points, needles, denormal, huge and non-finite triangles under the hostile scenes' own rays as sweep paths:
    axis-parallel sweeps from mesh vertices (two infinite 1 / d), and sweeps along the edges of denormal triangles,
    whose 1 / d is infinite on all three axes -- no axis is left for a child's test, and every child is entered."""
    h = hs.hostile(variant, 12)
    wvp, _ = hs.camera(cam)
    tris = h.tris(wvp)
    inp = hs.Inputs(tris, h.labels)
    o, d = inp.ray_o, inp.ray_d
    fin = tris[hs.finite_part(tris, h.labels)]
    lo, hi = nr.root_box(fin)
    diag = np.float32(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum()))
    r = (np.float32([0, 1e-3, 2e-2, 0.3]) * diag)[np.arange(len(o)) % 4]
    want = sr.brute(tris, o, d, r)
    nodes = orc.build(hs.oracle_scene(h.scene), wvp)
    T = len(tris)
    leaves = nr.leaf_data(tris)
    leaf_tri = (nodes["index"][:T] // 3).astype(np.int64)
    rep = lambda x, m: np.repeat(np.asarray(x)[None], m, 0)   # noqa: E731
    walked = sr.walked(o, d, r, np.full(len(o), INF, np.float32))
    no_axis = 0
    for i in np.nonzero(walked)[0]:
        with np.errstate(all="ignore"):
            no_axis += int(np.isinf(np.float32(1) / d[i]).all())
        _, t, _, f, mn_leaf = sr.pair_tests(leaves, leaf_tri, rep(o[i], T), rep(d[i], T), rep(r[i], T), rep(INF, T))
        base, mn = sr.node_tests(nodes, o[i], d[i], r[i])
        got, _ = sr.walk(nodes, base.tolist(), mn.tolist(), (f != 0).tolist(), sr.key_t(t, mn_leaf).tolist(),
                         leaf_tri.tolist(), float("inf"))
        assert (sr.NONE if got is None else got[1]) == want["tri"][i], i
    assert not (want["tri"][~walked] != sr.NONE).any()
    assert no_axis >= 4 and (want["tri"] != sr.NONE).sum() >= 100
