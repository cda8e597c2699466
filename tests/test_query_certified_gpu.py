"""Certified ray queries on the GPU (QUERY_CERTIFIED: the 4-wide certified walk, k_query_wide, and the
reference-order re-trace of the rays it cannot vouch for) against the numpy restatement of findCollision
(tests/ray_walk_ref.py, pinned to the oracle by tests/test_query_cpu.py).  Every comparison is bit-exact: t, u and v
are compared as uint32 views.  tests/test_query_certified_cpu.py checks the inputs' preconditions without a GPU."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import cert_scenes as cs
from tests import deep_scenes as ds
from tests import query_cert_ref as qc
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_query_gpu import (Case, assert_genuine, assert_hits_equal, edge_rays, random_rays, root_box,
                                  tiny_scene)

pytestmark = pytest.mark.gpu
W, H = 64, 48
SCENES = ["Test", "Rect", "Image_Test"]
CERT = rt.QUERY_CERTIFIED
BIG = 100_003
REFILL = 524_288 + 65   # more rays than the persistent grid has lanes (2048 x 256)


def walk_counts(ctx, rays):
    wc = ctx.query_walk_counts()
    assert sum(wc.values()) == rays, wc
    return wc


@pytest.fixture(scope="module", params=SCENES)
def case(request):
    """A reference scene (one-workgroup build, no QNodes: derived on the first certified query), its 4096 + 16 rays
    and their restated answers."""
    c = Case(request.param)
    yield c
    c.ctx.close()


# ---------------------------------------------------------------- 1. restatement parity
def test_closest_hit_matches_restatement(case):
    rays = rt.make_rays(case.o, case.d)
    assert_hits_equal(case.ctx.query(rays, CERT), case.want)
    got = case.ctx.query(rays, CERT | rt.QUERY_SORT | rt.QUERY_COUNT)
    assert_hits_equal(got, case.want, "SORT | COUNT")
    counts = case.ctx.query_counts()
    assert counts["rays"] == len(case.o) and counts["hits"] == int(case.want["hit"].sum())
    wc = walk_counts(case.ctx, len(case.o))
    assert wc["uncovered"] == int(qc.uncovered_mask(case.o, case.d).sum()) == 16   # the edge rays
    assert wc["fallback"] == 0 and wc["certified"] > 4000
    # a plain counting query reports its rays as fallback
    case.ctx.query(rays, rt.QUERY_COUNT)
    assert case.ctx.query_walk_counts() == {"certified": 0, "redone": 0, "uncovered": 0, "fallback": len(case.o)}


def test_t_max_matches_restatement(case):
    rays = rt.make_rays(case.o, case.d, case.t_max)
    assert_hits_equal(case.ctx.query(rays, CERT), case.want_tmax, "t_max")
    assert_hits_equal(case.ctx.query(rays, CERT | rt.QUERY_SORT | rt.QUERY_COUNT), case.want_tmax, "t_max SORT | COUNT")
    assert case.ctx.query_counts()["hits"] == int(case.want_tmax["hit"].sum())
    walk_counts(case.ctx, len(case.o))
    # t_max values for which no triangle is accepted, and the first float for which one might be
    vals = np.array([np.nan, -1, 0, 0.01, np.nextafter(np.float32(0.01), np.float32(1))], np.float32)
    tm = vals[np.arange(len(case.o)) % 5]
    want = rw.walk(case.nodes, case.tris, case.o, case.d, t_max=tm)
    assert not want["hit"][np.arange(len(case.o)) % 5 != 4].any()
    got = case.ctx.query(rt.make_rays(case.o, case.d, tm), CERT)
    assert_hits_equal(got, want, "tiny t_max")
    np.testing.assert_array_equal(got.view(np.uint32), case.ctx.query(rt.make_rays(case.o, case.d, tm)).view(np.uint32))


@pytest.mark.parametrize("limited", [False, True], ids=["inf", "t_max"])
def test_any_hit_mask_and_triangles(case, limited):
    t_max = case.t_max if limited else np.full(len(case.o), np.inf, np.float32)
    want = case.want_tmax if limited else case.want
    rays = rt.make_rays(case.o, case.d, t_max)
    for mode in (rt.QUERY_ANY, rt.QUERY_ANY | rt.QUERY_SORT | rt.QUERY_COUNT):
        got = case.ctx.query(rays, CERT | mode)
        np.testing.assert_array_equal(got["t"] != -1, want["hit"])
        assert_genuine(got, case.tris, case.o, case.d, t_max)
    counts = case.ctx.query_counts()
    assert counts["rays"] == len(case.o) and counts["hits"] == int(want["hit"].sum())
    walk_counts(case.ctx, len(case.o))


# ---------------------------------------------------------------- 2. the re-trace path is taken
@pytest.mark.parametrize("variant", ["small", "large"])
def test_hall_rays_without_a_certificate_are_retraced(variant):
    """The halls' flat walls: for some rays the reference's own hit fails the certificate (the count is pinned by
    tests/test_query_certified_cpu.py), so the walk must hand at least these to the re-trace.  small: the
    one-workgroup build; large: the multi-kernel build, crossing nodes."""
    s, _, nodes, wvp, wv = cs.hall(variant, "A")
    tris, o, d, want, bad = qc.hall_case(variant)
    assert int(bad.sum()) == qc.HALL_EXPECT[variant][1] > 0
    with rt.Context(device=0) as ctx:
        ctx.set_scene(s)
        ctx.set_camera(wvp, wv)
        ctx.build()
        got = ctx.query(rt.make_rays(o, d), CERT | rt.QUERY_COUNT)
        assert_hits_equal(got, want)
        wc = walk_counts(ctx, len(o))
        assert wc["redone"] >= int(bad.sum()) and wc["uncovered"] == 0 and wc["fallback"] == 0
        assert ctx.query_counts()["hits"] == int(want["hit"].sum())
        anyh = ctx.query(rt.make_rays(o, d), CERT | rt.QUERY_ANY)
        np.testing.assert_array_equal(anyh["t"] != -1, want["hit"])
        assert_genuine(anyh, tris, o, d)
        ctx.synchronize()


# ---------------------------------------------------------------- 3. uncovered rays
def test_uncovered_rays_take_the_reference_order(case):
    xo, xd = qc.extra_uncovered_rays(case.nodes)
    eo, ed = edge_rays(case.nodes)
    o, d = np.concatenate([xo, eo]), np.concatenate([xd, ed])
    want = rw.walk(case.nodes, case.tris, o, d)
    got = case.ctx.query(rt.make_rays(o, d), CERT | rt.QUERY_COUNT)
    assert_hits_equal(got, want)
    wc = walk_counts(case.ctx, len(o))
    assert wc["uncovered"] == int(qc.uncovered_mask(o, d).sum()) == 32 + 16
    # the shortened rays (|d| = 0.5) are covered, and their t is in units of |d|
    assert wc["certified"] + wc["redone"] == 16
    assert want["hit"][32:48].any()


@pytest.mark.parametrize("ntris", [1, 2, 3])
def test_tiny_scenes_with_non_unit_rays(ntris):
    """T = 1 (the root is a leaf) and QNodes with missing grandchildren; directions that are not unit: most are long
    (uncovered), some short (covered)."""
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
        d[::2] /= (np.float32(2) * np.sqrt((d[::2] * d[::2]).sum(1, keepdims=True)))   # every other one: |d| = 0.5
        want = rw.walk(nodes, tris, o, d)
        assert want["hit"].any() and not want["hit"].all()
        assert_hits_equal(ctx.query(rt.make_rays(o, d), CERT | rt.QUERY_COUNT), want)
        wc = walk_counts(ctx, 500)
        assert wc["uncovered"] == int(qc.uncovered_mask(o, d).sum()) and 0 < wc["uncovered"] < 500
        got = ctx.query(rt.make_rays(o, d), CERT | rt.QUERY_ANY)
        np.testing.assert_array_equal(got["t"] != -1, want["hit"])
        assert_genuine(got, tris, o, d)


# ---------------------------------------------------------------- 4. deep stacks
def test_fan_rays_leave_the_lds_part_of_the_stack():
    s, _, nodes, wvp, wv = ds.fan()
    tris, o, d, want = qc.fan_case()
    assert (want["max_stack"] == 35).all() and want["hit"].all()
    with rt.Context(device=0) as ctx:
        ctx.set_scene(s)
        ctx.set_camera(wvp, wv)
        ctx.build()
        assert_hits_equal(ctx.query(rt.make_rays(o, d), CERT | rt.QUERY_COUNT), want)
        wc = walk_counts(ctx, len(o))
        assert wc["uncovered"] == int(qc.uncovered_mask(o, d).sum()) == 3 and wc["fallback"] == 0
        ctx.synchronize()   # (no overflow reported: the walk's own overflows would be re-traced, not reported)


# ---------------------------------------------------------------- 5. refill and sizes
@pytest.fixture(scope="module")
def big():
    c = Case("Test")
    o, d = random_rays(c.nodes, BIG, seed=11)
    want = rw.walk(c.nodes, c.tris, o, d)
    yield c, o, d, want
    c.ctx.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(big, n):
    import torch
    c, o, d, want = big
    got = c.ctx.query(rt.make_rays(o[:n], d[:n]), CERT)
    assert got.shape == (n,)
    assert_hits_equal(got, {k: v[:n] for k, v in want.items()})
    dev = c.ctx.query(torch.from_numpy(rt.make_rays(o[:n], d[:n]).view(np.float32).reshape(-1, 8)).cuda(), CERT)
    assert tuple(dev.shape) == (n, 4)
    np.testing.assert_array_equal(dev.cpu().numpy().view(np.uint32), got.view(np.uint32).reshape(-1, 4))


def test_100003_rays(big):
    c, o, d, want = big
    assert_hits_equal(c.ctx.query(rt.make_rays(o, d), CERT), want)
    assert_hits_equal(c.ctx.query(rt.make_rays(o, d), CERT | rt.QUERY_SORT | rt.QUERY_COUNT), want, "SORT | COUNT")
    assert walk_counts(c.ctx, BIG)["fallback"] == 0


def test_more_rays_than_lanes_refill():
    c = Case("Rect")
    try:
        ro, rd = random_rays(c.nodes, REFILL - 4096, seed=13)
        o, d = np.concatenate([c.o[:4096], ro]), np.concatenate([c.d[:4096], rd])
        rays = rt.make_rays(o, d)
        plain = c.ctx.query(rays)
        assert_hits_equal(plain[:4096], {k: v[:4096] for k, v in c.want.items()}, "plain, first 4096")
        got = c.ctx.query(rays, CERT | rt.QUERY_COUNT)
        np.testing.assert_array_equal(got.view(np.uint32), plain.view(np.uint32))
        assert c.ctx.query_counts()["hits"] == int((plain["t"] != -1).sum())
        # (of half a million random unit directions a few have a component below 2^-20)
        assert walk_counts(c.ctx, REFILL)["uncovered"] == int(qc.uncovered_mask(o, d).sum()) < 16
    finally:
        c.ctx.close()


# ---------------------------------------------------------------- 6. fallbacks
@pytest.mark.parametrize("kwargs", [dict(stack_limit=32), dict(delta_mode=rt.DELTA_CPUTESTS)], ids=["limit", "cputests"])
def test_fallback_takes_the_plain_kernel(kwargs):
    d = load_scene_fixture("Rect")
    with rt.Context(device=0, **kwargs) as ctx:
        ctx.set_scene(rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]))
        ctx.set_camera(*rt.camera_reference(W, H))
        ctx.build()
        nodes = ctx.read_bvh()
        ro, rd = random_rays(nodes, 4096)
        eo, ed = edge_rays(nodes)
        rays = rt.make_rays(np.concatenate([ro, eo]), np.concatenate([rd, ed]))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.query_walk_counts()
        assert e.value.status == rt._lib.ERR_NOT_READY
        plain = ctx.query(rays)
        assert (plain["t"] != -1).any()
        for mode in (0, rt.QUERY_ANY, rt.QUERY_SORT):
            got = ctx.query(rays, CERT | rt.QUERY_COUNT | mode)
            if mode == rt.QUERY_ANY:
                np.testing.assert_array_equal(got["t"] != -1, plain["t"] != -1)
            else:
                np.testing.assert_array_equal(got.view(np.uint32), plain.view(np.uint32))
            assert ctx.query_walk_counts() == {"certified": 0, "redone": 0, "uncovered": 0, "fallback": len(rays)}
        ctx.synchronize()


def test_walk_counts_before_a_build_are_not_ready():
    d = load_scene_fixture("Rect")
    with rt.Context(device=0) as ctx:
        ctx.set_scene(rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]))
        ctx.set_camera(*rt.camera_reference(W, H))
        with pytest.raises(rt.RtbvhError) as e:
            ctx.query_walk_counts()
        assert e.value.status == rt._lib.ERR_NOT_READY
        with pytest.raises(rt.RtbvhError) as e:
            ctx.query(rt.make_rays(np.zeros((4, 3)), np.ones((4, 3))), CERT)
        assert e.value.status == rt._lib.ERR_NOT_READY


def test_unknown_bits_are_still_rejected(case):
    rays = rt.make_rays(case.o[:4], case.d[:4])
    for mode in (CERT | 8, CERT | 16, CERT | 128, CERT | 512, CERT << 1):
        with pytest.raises(rt.RtbvhError) as e:
            case.ctx.query(rays, mode)
        assert e.value.status == rt._lib.ERR_INVALID_ARG
    assert case.ctx.query(rays, CERT).shape == (4,)


# ---------------------------------------------------------------- 7. context state
def test_certified_query_leaves_the_trace_alone():
    """An AUTO_WALK context past 65,536 triangles (a certified-only build: node boxes, no records): the certified query
    and its re-trace read the forms the build wrote, and the trace still matches the oracle."""
    s = rt.synthetic(70_000, seed=0x5EED0004)
    wvp, wv = rt.camera_reference(W, H)
    with rt.Context(device=0, flags=rt.FLAG_AUTO_WALK) as auto, rt.Context(device=0) as plain:
        for c in (auto, plain):
            c.set_scene(s)
            c.set_camera(wvp, wv)
            c.build()
        nodes = plain.read_bvh()
        o, d = random_rays(nodes, 20_000, seed=3)
        eo, ed = edge_rays(nodes)
        rays = rt.make_rays(np.concatenate([o, eo]), np.concatenate([d, ed]))
        p = plain.query(rays)
        for c in (auto, plain):
            np.testing.assert_array_equal(c.query(rays, CERT | rt.QUERY_COUNT).view(np.uint32), p.view(np.uint32))
            wc = walk_counts(c, len(rays))
            assert wc["uncovered"] == 16 and wc["fallback"] == 0
        np.testing.assert_array_equal(auto.query(rays).view(np.uint32), p.view(np.uint32))
        auto.trace(W, H, 1)
        fb = auto.read_framebuffer()
        assert auto.stats()["walk_state"] == 2
        osc = orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob)
        ofb = orc.trace(osc, orc.build(osc, wvp), wvp, wv, W, H, 1, row_begin=0, row_end=16)[0]
        np.testing.assert_array_equal(fb[0:16].view(np.uint32), ofb.view(np.uint32))


def test_two_streams_and_device_tensors(case):
    import torch
    n = len(case.o)
    r1 = torch.from_numpy(rt.make_rays(case.o, case.d).view(np.float32).reshape(n, 8)).cuda()
    r2 = torch.from_numpy(rt.make_rays(case.o, case.d, case.t_max).view(np.float32).reshape(n, 8)).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    h1 = case.ctx.query(r1, CERT | rt.QUERY_COUNT, stream=s1)   # back to back, one context, two streams
    h2 = case.ctx.query(r2, rt.QUERY_SORT, stream=s2)           # (a plain query: the count block stays h1's)
    h3 = case.ctx.query(r2, CERT | rt.QUERY_SORT, stream=s1)
    s1.synchronize()
    s2.synchronize()
    assert h1.is_cuda and h1.dtype == torch.float32 and tuple(h1.shape) == (n, 4)
    for h, want in ((h1, case.want), (h2, case.want_tmax), (h3, case.want_tmax)):
        assert_hits_equal(h.cpu().numpy().view(rt.HIT_DTYPE).reshape(-1), want)
    assert case.ctx.query_counts()["hits"] == int(case.want["hit"].sum())
    assert walk_counts(case.ctx, n)["uncovered"] == 16
    with torch.cuda.stream(s1):
        h4 = case.ctx.query(r2, CERT, out=torch.empty((n, 4), dtype=torch.float32, device="cuda"))
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
        before = case.ctx.query(rays, CERT, stream=s1)   # outstanding while the build is enqueued
        case.ctx.set_camera(wvp2, wv2)
        case.ctx.build(sync=False)
        moved = case.ctx.query(rays, CERT, stream=s1)    # (the new tree's QNodes are derived again)
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
