"""Deep trees on the GPU (scenes: tests/deep_scenes.py; what they reach, by the oracle alone:
tests/test_deep_scenes_cpu.py).

The fan: thousands of rays of the primary pass and of every bounce pass need 24 to 35 stack entries.  The
one-ray-per-lane walks (k_primary, k_bounce, k_query, k_primary_redo / k_bounce_redo, the binary k_bounce_trav)
keep entries [0, 16) in LDS and the rest in scratch, the 4-wide bounce walk entries [0, 13) as a node id and a
bf16 distance in LDS and the rest as full pairs in scratch (trace.hip LANE_LSB, SB, SW); no other scene of the
suite but the 10M-triangle ones needs more than 12 entries.  Every comparison is bit for bit against the CPU
oracle's whole frame or against the numpy restatement of its walk (tests/ray_walk_ref.py).

The crossing scene: one group of 64 refit workgroups lists 1,261 crossing nodes, more than the GCAP = 1024
k_refit_group climbs in LDS, so it runs the global protocol for all of them (build.hip `m > GCAP`); a random tree
lists about 600 at most."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import cert_scenes as cs
from tests import deep_scenes as ds
from tests import ray_walk_ref as rw
from tests.test_gpu_parity import TRACE_MODES, _assert_nodes_equal, check_qnodes
from tests.test_query_cpu import primary_rays
from tests.test_query_gpu import assert_genuine, assert_hits_equal

pytestmark = pytest.mark.gpu

W, H, BOUNCES = ds.W, ds.H, 3
REFERENCE_ORDER = ("reference", "reference+sort", "packet", "refill+sort")   # the oracle's own steps
# probe (b): the modes of tests/test_gpu_parity.py test_stack_limit_reports_overflow and the two other 4-wide ones
PROBED = ("reference", "nearest", "packet", "nearest+packet", "nearest+packet+refill", "nearest+packet+wide",
          "refill+sort", "wide+sort", "binned+wide+refill")
# The binned primary pass keeps no stack, so an overflow of these can only be a bounce walk's: k_bounce in the
# reference and the nearest-first order, the binary k_bounce_trav in both, the 4-wide k_bounce_trav
BOUNCE_ONLY = {"binned": rt.FLAG_BINNED_PRIMARY,
               "binned+nearest": rt.FLAG_BINNED_PRIMARY | rt.FLAG_NEAREST_FIRST,
               "binned+refill": rt.FLAG_BINNED_PRIMARY | rt.FLAG_REFILL_BOUNCE,
               "binned+nearest+refill": rt.FLAG_BINNED_PRIMARY | rt.FLAG_NEAREST_FIRST | rt.FLAG_REFILL_BOUNCE,
               "binned+wide+refill": TRACE_MODES["binned+wide+refill"]}
LIMIT = 20   # above both LDS parts (16 and 13), below what the fan's rays need


def _fan_context(flags=0, stack_limit=0):
    s, _, _, wvp, wv = ds.fan()
    c = rt.Context(device=0, flags=flags, stack_limit=stack_limit)
    c.set_scene(s)
    c.set_camera(wvp, wv)
    return c


def _check_frame(c, want, mode=""):
    np.testing.assert_array_equal(c.read_framebuffer(), want["fb"], err_msg=mode)
    np.testing.assert_array_equal(c.read_intensity(), want["inten"], err_msg=mode)
    st, ost = c.stats(), want["stats"]
    assert sum(st["hits"]) == ost["hits"], mode
    assert st["bounce_rays"] == ost["bounce"], mode
    assert st["stack_overflows"] == 0, mode
    return st


# ---------------------------------------------------------------- a. every trace mode
@pytest.mark.parametrize("build", ["one workgroup", "multi-kernel"])
@pytest.mark.parametrize("mode", list(TRACE_MODES))
def test_fan_frame_matches_oracle(mode, build):
    """A 3-bounce frame of the fan in every shipped walk combination, on the tree of the one-workgroup build and
    of the multi-kernel build (a CERTIFIED context's then has node boxes and no records): framebuffer and
    intensity equal the oracle's whole frame, sum(hits) and bounce_rays equal its counts, nothing overflows, and
    the reference-order modes make the oracle's internal and leaf visits."""
    want = ds.fan_oracle(BOUNCES)
    assert want["stats"]["max_stack"] >= 30 and want["stats"]["stack_overflows"] == 0
    flags = TRACE_MODES[mode] | rt.FLAG_COUNT_VISITS | (rt.FLAG_MULTI_KERNEL_BUILD if build == "multi-kernel" else 0)
    with _fan_context(flags) as c:
        c.compute_bvh(W, H, BOUNCES)
        st = _check_frame(c, want, mode)
        if mode in REFERENCE_ORDER:
            assert sum(st["internal_visits"]) == want["stats"]["internal_visits"]
            assert sum(st["leaf_visits"]) == want["stats"]["leaf_visits"]
        _assert_nodes_equal(c.read_bvh(), ds.fan()[2], ds.fan()[0].num_tris)


# ---------------------------------------------------------------- b. proof that the deep segment ran
def _trace_limited(c, bounces):
    """Traces in a context with a stack limit; returns (raised ERR_STACK_OVERFLOW, stats' stack_overflows)."""
    raised = False
    try:
        c.trace(W, H, bounces)
    except rt.RtbvhError as e:
        assert e.status == rt._lib.ERR_STACK_OVERFLOW
        assert "stack" in str(e)
        raised = True
    n = c.stats()["stack_overflows"]
    c.synchronize()   # reported once
    return raised, n


@pytest.mark.parametrize("mode", PROBED)
def test_fan_rays_leave_the_lds_part_of_the_stack(mode):
    """With stack_limit = 20 -- past the entries the walks keep in LDS, 16 and 13 -- the frame's trace raises
    RTBVH_ERR_STACK_OVERFLOW and counts overflows: rays of this mode's walks pushed entry 19, so entries [16, 19)
    (the 4-wide walk: [13, 18)) went to scratch and came back.  Without a limit nothing overflows and the frame
    is the oracle's.  The reference order also overflows with the reference's own 32 entries
    (tests/test_deep_scenes_cpu.py predicts it), which it does not on Test.obj (tests/test_gpu_parity.py
    test_stack_limit_reports_overflow).

    Every mode of the list fired on an MI355X.  In the modes whose primary walk keeps a stack the overflow may be
    the primary walk's alone; test_fan_bounce_walks_leave_the_lds_part_of_the_stack separates the bounce walks.
    RTBVH_FLAG_CERTIFIED cannot be probed: a context with a stack limit falls back to the reference order
    (api.hip plan_trace).  Its 4-wide bounce walk is the instance of "binned+wide+refill"'s with CERT set, and
    test_fan_frame_matches_oracle compares its frame."""
    with _fan_context(TRACE_MODES[mode], LIMIT) as c:
        c.build()
        raised, n = _trace_limited(c, BOUNCES)
        assert raised and n > 0
    if mode == "reference":
        with _fan_context(0, 32) as c:
            c.build()
            raised, n = _trace_limited(c, BOUNCES)
            assert raised and n > 0
    with _fan_context(TRACE_MODES[mode] | rt.FLAG_COUNT_VISITS, 0) as c:
        c.build()
        c.trace(W, H, BOUNCES)
        _check_frame(c, ds.fan_oracle(BOUNCES), mode)


@pytest.mark.parametrize("mode", list(BOUNCE_ONLY))
def test_fan_bounce_walks_leave_the_lds_part_of_the_stack(mode):
    """The same probe where only a bounce walk can answer it: behind the binned primary pass, which keeps no
    stack (a trace of 0 bounces reports no overflow at stack_limit = 20), the 3-bounce frame overflows -- in the
    one-ray-per-lane bounce kernel and in the persistent binary walk, each in the reference and the nearest-first
    order, and in the 4-wide walk (tests/test_deep_scenes_cpu.py: every pass has a thousand rays and more at stack
    index 24 and above in both binary orders).  Without a limit the frames are the oracle's.  All five fired on
    an MI355X."""
    with _fan_context(BOUNCE_ONLY[mode], LIMIT) as c:
        c.build()
        assert _trace_limited(c, 0) == (False, 0)
        raised, n = _trace_limited(c, BOUNCES)
        assert raised and n > 0
    with _fan_context(BOUNCE_ONLY[mode] | rt.FLAG_COUNT_VISITS, 0) as c:
        c.build()
        c.trace(W, H, BOUNCES)
        _check_frame(c, ds.fan_oracle(BOUNCES), mode)


# ---------------------------------------------------------------- c. ray queries
class _Rays:
    """The fan's query rays and their restated answers (computed once): the primary rays, the rays entering the
    first bounce pass, 4,096 random rays in the root box (the fan is a speck of it: mostly misses) and 4,096
    through the window, up and down."""

    def __init__(self):
        s, os_, nodes, wvp, wv = ds.fan()
        self.nodes = nodes
        self.tris = rw.clip_triangles(s.vertices, s.indices, wvp)
        rng = np.random.default_rng(17)
        root = nodes[s.num_tris]
        lo, hi = root["bb_min"].astype(np.float32), root["bb_max"].astype(np.float32)
        ro = (lo + rng.random((4096, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
        rd = rng.standard_normal((4096, 3)).astype(np.float32)
        rd /= np.sqrt((rd * rd).sum(1, keepdims=True))
        wo = np.stack([rng.uniform(ds.P[0] - ds.R, ds.P[0] + ds.R, 4096), rng.uniform(ds.P[1] - ds.R, ds.P[1] + ds.R, 4096),
                       rng.uniform(ds.FRONT_Z, ds.MIRROR_Z, 4096)], 1).astype(np.float32)
        wd = np.stack([rng.uniform(-0.01, 0.01, 4096), rng.uniform(-0.01, 0.01, 4096), rng.choice([-1.0, 1.0], 4096)], 1)
        wd = (wd / np.sqrt((wd * wd).sum(1, keepdims=True))).astype(np.float32)
        po, pd = primary_rays(W, H)
        _, eo, ed = cs.entering_rays(os_, nodes, wvp, wv, W, H, 0)
        self.o = np.concatenate([po, eo, ro, wo]).astype(np.float32)
        self.d = np.concatenate([pd, ed, rd, wd]).astype(np.float32)
        self.want = rw.walk(nodes, self.tris, self.o, self.d)
        t = self.want["t"]
        k = np.arange(len(t)) % 3   # (tests/test_query_gpu.py Case: 0.5 t, t exactly, the float below t; misses 10)
        self.t_max = np.where(self.want["hit"], np.where(k == 0, np.float32(.5) * t, np.where(
            k == 1, t, np.nextafter(t, np.float32(0)))), np.float32(10)).astype(np.float32)
        self.want_tmax = rw.walk(nodes, self.tris, self.o, self.d, t_max=self.t_max)


@pytest.fixture(scope="module")
def fan_rays():
    return _Rays()


@pytest.mark.parametrize("tree", ["records", "node boxes"])
def test_fan_queries_match_restatement(fan_rays, tree):
    """k_query on the fan, on node records and on a certified multi-kernel build's node boxes: closest hits (t, u,
    v, tri bit for bit), QUERY_COUNT's totals, QUERY_SORT, t_max around each ray's own hit, and the any-hit mask
    with genuine triangles, all against the restatement -- whose walks of these rays reach stack index 35."""
    r = fan_rays
    ms = r.want["max_stack"]
    assert (ms >= 24).sum() >= 10_000 and (ms < 8).sum() >= 10_000
    assert (ms[-4096:] >= 24).sum() >= 500 and (r.want_tmax["max_stack"] >= 24).sum() >= 1_000
    flags = rt.FLAG_CERTIFIED | rt.FLAG_MULTI_KERNEL_BUILD if tree == "node boxes" else 0
    with _fan_context(flags) as c:
        c.build()
        rays = rt.make_rays(r.o, r.d)
        assert_hits_equal(c.query(rays), r.want)
        assert_hits_equal(c.query(rays, rt.QUERY_COUNT), r.want, "COUNT")
        counts = {"rays": len(r.o), "hits": int(r.want["hit"].sum()), "internal_visits": int(r.want["internal"].sum()),
                  "leaf_visits": int(r.want["leaf"].sum())}
        assert c.query_counts() == counts
        assert_hits_equal(c.query(rays, rt.QUERY_SORT), r.want, "SORT")
        assert_hits_equal(c.query(rays, rt.QUERY_SORT | rt.QUERY_COUNT), r.want, "SORT | COUNT")
        assert c.query_counts() == counts
        # t_max
        limited = rt.make_rays(r.o, r.d, r.t_max)
        got = c.query(limited)
        assert_hits_equal(got, r.want_tmax, "t_max")
        lost = r.want["hit"] & ~r.want_tmax["hit"]
        assert lost.any()
        assert (got["t"][r.want["hit"]] <= r.t_max[r.want["hit"]]).all()
        at = r.want["hit"] & (np.arange(len(r.o)) % 3 == 1)
        assert (rw.bits(got["t"][at]) == rw.bits(r.want["t"][at])).mean() > .9
        # any-hit
        for rr, want, tm in ((rays, r.want, None), (limited, r.want_tmax, r.t_max)):
            got = c.query(rr, rt.QUERY_ANY)
            np.testing.assert_array_equal(got["t"] != -1, want["hit"])
            assert_genuine(got, r.tris, r.o, r.d, tm)
        c.query(rays, rt.QUERY_ANY | rt.QUERY_COUNT)
        assert c.query_counts()["hits"] == counts["hits"]


def test_fan_queries_overflow_at_the_limit(fan_rays):
    """stack_limit = 20: the synchronous host entry raises RTBVH_ERR_STACK_OVERFLOW (k_query pushed entry 19,
    past its 16 in LDS), every hit it reports is genuine, and the rays that stay below the limit keep their
    answers."""
    r = fan_rays
    with _fan_context(0, LIMIT) as c:
        c.build()
        out = np.zeros(len(r.o), rt.HIT_DTYPE)
        with pytest.raises(rt.RtbvhError) as e:
            c.query(rt.make_rays(r.o, r.d), out=out)
        assert e.value.status == rt._lib.ERR_STACK_OVERFLOW
        assert (out["t"] != -1).any()
        assert_genuine(out, r.tris, r.o, r.d)
        below = r.want["max_stack"] < LIMIT   # (a ray overflows when it would push index LIMIT: walk_node)
        assert_hits_equal(out[below], {k: v[below] for k, v in r.want.items()}, "below the limit")


# ---------------------------------------------------------------- d. frames in flight and band traces
@pytest.mark.parametrize("mode", ["nearest+packet+wide", "certified"])
def test_fan_bands_and_frames_in_flight(mode):
    """Each of 3 ranks' bands of the 3-bounce frame (the weighted deal), traced alone on the context stream and
    as two frames in flight on caller streams (the launch without early shading, on the 512-block grid; the
    slots' own stacks and lists): the in-flight buffers equal the one traced alone, nothing overflows, and the
    bands put back in their rows give the oracle's frame."""
    import torch

    from raytracebvh_amd.tiles import band_row_ids
    nranks, share = 3, 11
    want = ds.fan_oracle(BOUNCES)
    streams = [torch.cuda.Stream() for _ in range(2)]
    with _fan_context(TRACE_MODES[mode] | rt.FLAG_COUNT_VISITS) as c:   # (the hit counts need COUNT_VISITS)
        c.compute_bvh(W, H, BOUNCES)
        _check_frame(c, want, mode)
        c.set_band_deal(share)
        frame = np.zeros_like(want["fb"])
        hits = bounce = 0
        for r in range(nranks):
            rows = rt.lib().rtbvh_deal_rows(H, r, nranks, share)
            alone = torch.full((rows, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
            bufs = [torch.full((rows, W, 4), -1.0, dtype=torch.float32, device="cuda:0") for _ in range(2)]
            torch.cuda.synchronize()   # (the fills run on torch's stream)
            c.trace_band_async(W, H, BOUNCES, r, nranks, alone.data_ptr())
            c.synchronize()
            st = c.stats()
            assert st["stack_overflows"] == 0
            for i, b in enumerate(bufs):
                c.trace_band_async(W, H, BOUNCES, r, nranks, b.data_ptr(), stream_ptr=streams[i].cuda_stream)
            c.synchronize()
            torch.cuda.synchronize()
            for i, b in enumerate(bufs):
                assert torch.equal(b, alone), (r, i)
            slot = c.stats()
            assert slot["stack_overflows"] == 0
            assert slot["bounce_rays"] == st["bounce_rays"] and sum(slot["hits"]) == sum(st["hits"])
            hits += sum(st["hits"])
            bounce += st["bounce_rays"]
            frame[band_row_ids(H, r, nranks, share)] = alone.cpu().numpy()
        np.testing.assert_array_equal(frame, want["fb"])
        assert hits == want["stats"]["hits"] and bounce == want["stats"]["bounce"]


# ---------------------------------------------------------------- e. the grouped refit's fallback
FW, FH = 64, 48
BINNED_FAST = TRACE_MODES["binned+wide+refill"]


@pytest.fixture(scope="module")
def crossing_frame():
    _, os_, nodes, wvp, wv = ds.crossing()
    fb, inten, st = orc.trace(os_, nodes, wvp, wv, FW, FH, 1, want_intensity=True)
    return dict(fb=fb, inten=inten, stats=st)


def _check_tree(c, nodes):
    got = c.read_bvh()
    _assert_nodes_equal(got, nodes, (len(nodes) + 1) // 2)


@pytest.mark.parametrize("walk", ["reference", "certified"])
def test_crossing_scene_builds_the_oracles_tree(walk, crossing_frame):
    """k_refit_group's `m > GCAP` branch (tests/test_deep_scenes_cpu.py: one group lists 1,261 crossing nodes): the
    multi-kernel build of the crossing scene in a plain context (node records) and in a certified one (node
    boxes, the crossing nodes' QNodes written late) gives the oracle's tree, field by field, and the oracle's
    frame; so it does a second time in the same context after a 1,000-triangle build -- the crossing-node lists,
    their counts and the tickets start clean."""
    s, _, nodes, wvp, wv = ds.crossing()
    small = rt.synthetic(1000, seed=0x5EED0021)
    small_nodes = orc.build(cs.oscene_of(small), wvp)
    assert ds.crossing_per_group(nodes).max() > ds.GCAP
    with rt.Context(device=0, flags=TRACE_MODES[walk] | rt.FLAG_COUNT_VISITS) as c:
        for scene, tree in ((s, nodes), (small, small_nodes), (s, nodes)):
            c.set_scene(scene)
            c.set_camera(wvp, wv)
            c.build()
            _check_tree(c, tree)
            if scene is s:
                c.trace(FW, FH, 1)
                _check_frame(c, crossing_frame, walk)
                _check_tree(c, tree)   # (the trace derived what it needed and left the tree alone)


@pytest.mark.parametrize("walk", ["certified", "binned+wide+refill"])
def test_crossing_scene_through_compute_bvh(walk, crossing_frame):
    """rtbvh_compute_bvh with the binned primary pass leaves the crossing nodes to the frame: k_refit_group runs
    behind the build and k_pb_count_late quantizes the nodes it listed beside the pass's count.  Twice, with a
    small scene's frame between: the oracle's tree, and in the certified walks the oracle's frame."""
    s, _, nodes, wvp, wv = ds.crossing()
    small = rt.synthetic(1000, seed=0x5EED0021)
    with rt.Context(device=0, flags=TRACE_MODES[walk] | rt.FLAG_COUNT_VISITS) as c:
        for scene in (s, small, s):
            c.set_scene(scene)
            c.set_camera(wvp, wv)
            c.compute_bvh(FW, FH, 1)
            if scene is s:
                _check_tree(c, nodes)
                assert c.stats()["stack_overflows"] == 0
                if walk == "certified":
                    _check_frame(c, crossing_frame, walk)


def test_crossing_scene_qnodes_contain_the_exact_boxes():
    """tests/test_gpu_parity.py test_qnodes_contain_the_exact_boxes' checks on the certified context's QNodes of
    the crossing scene, the crossing nodes' (written late, from the boxes the global protocol completed) among
    them."""
    s, _, _, wvp, wv = ds.crossing()
    check_qnodes(s, (wvp, wv), flags=rt.FLAG_CERTIFIED)
