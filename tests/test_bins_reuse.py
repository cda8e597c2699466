"""The binned primary pass's bin sets as a product of (built tree, frame shape): filled once, read by every later
binned trace of the same key on any stream (api.hip PbKey / find_bins), refilled after a build, a shape, rank or
deal change.  Every frame is compared bit for bit with a fresh context's frame of the same inputs -- a fresh
context's first trace has no set to reuse -- or with the reference-order frame."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from tests.conftest import load_scene_fixture

pytestmark = pytest.mark.gpu

FAST = rt.FLAG_NEAREST_FIRST | rt.FLAG_PACKET_PRIMARY | rt.FLAG_REFILL_BOUNCE | rt.FLAG_WIDE_BVH
BINNED = FAST | rt.FLAG_BINNED_PRIMARY          # the unchecked binned pass
MODES = [pytest.param(rt.FLAG_CERTIFIED, id="certified"), pytest.param(BINNED, id="binned")]
SMALL, LARGE = (100, 70), (200, 136)            # neither a multiple of the 32-pixel tile; 4 x 3 and 7 x 5 tiles
SEED = 0x5EED0021

_scenes, _frames = {}, {}


def scene(seed=SEED, ntris=20_000):
    if (seed, ntris) not in _scenes:
        _scenes[seed, ntris] = rt.synthetic(ntris, seed=seed, half_extent=(30, 30, 20))
    return _scenes[seed, ntris]


def camera(W, H, orbit=0):
    eye = np.array(rt.EYE_REFERENCE, np.float32)
    for _ in range(orbit):
        eye = rt.camera_orbit(eye, rt.KEY_LEFT)
    return rt.camera_look(eye, W, H)


def setup(c, W, H, seed=SEED, orbit=0, ntris=20_000):
    """The scene, the camera of a W x H frame, the build."""
    c.set_scene(scene(seed, ntris))
    c.set_camera(*camera(W, H, orbit))
    c.build()


def fresh(flags, W, H, seed=SEED, orbit=0, rank=0, nranks=1, share=16, ntris=20_000, bounces=1, cam=None):
    """The frame (or the rank's bands) of a context that traces once: computed once per key, never written."""
    import torch
    cam = cam or (W, H)
    key = (flags, W, H, seed, orbit, rank, nranks, share, ntris, bounces, cam)
    if key not in _frames:
        with rt.Context(device=0, flags=flags) as c:
            setup(c, *cam, seed, orbit, ntris)
            c.set_band_deal(share)
            if nranks == 1:
                c.trace(W, H, bounces)
                out = c.read_framebuffer()
            else:
                out = band(c, W, H, rank, nranks, share, bounces)
            assert c.bin_builds() == 1
        out.setflags(write=False)
        _frames[key] = out
        torch.cuda.synchronize()
    return _frames[key]


def band(c, W, H, rank, nranks, share, bounces=1, stream=None):
    import torch
    rows = rt.lib().rtbvh_deal_rows(H, rank, nranks, share)
    buf = torch.full((rows, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()   # the fill runs on torch's stream
    c.trace_band_async(W, H, bounces, rank, nranks, buf.data_ptr(), stream_ptr=stream.cuda_stream if stream else None)
    c.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("flags", MODES)
def test_three_traces_of_one_build_fill_once(flags, monkeypatch):
    W, H = SMALL
    want = fresh(flags, W, H)
    with rt.Context(device=0, flags=flags) as c:
        setup(c, W, H)
        for i in range(3):
            c.trace(W, H, 1)
            np.testing.assert_array_equal(c.read_framebuffer(), want, err_msg=f"trace {i}")
        assert c.bin_builds() == 1 and c.bin_sets() == 1
    monkeypatch.setenv("RTBVH_BINS_REUSE", "0")   # read by rtbvh_create: a fill per trace
    with rt.Context(device=0, flags=flags) as c:
        setup(c, W, H)
        for i in range(3):
            c.trace(W, H, 1)
            np.testing.assert_array_equal(c.read_framebuffer(), want, err_msg=f"no reuse, trace {i}")
        assert c.bin_builds() == 3


@pytest.mark.parametrize("flags", MODES)
def test_shape_change_refills(flags):
    """One tree (built under the larger frame's camera), the frame size alone changing: the set is refilled on
    every change and only then."""
    with rt.Context(device=0, flags=flags) as c:
        setup(c, *LARGE)
        for k, ((W, H), miss) in enumerate(((SMALL, 1), (LARGE, 1), (SMALL, 1), (SMALL, 0))):
            before = c.bin_builds()
            c.trace(W, H, 1)
            np.testing.assert_array_equal(c.read_framebuffer(), fresh(flags, W, H, cam=LARGE), err_msg=f"step {k}")
            assert c.bin_builds() - before == miss, k
        assert c.bin_sets() == 1


@pytest.mark.parametrize("flags", MODES)
def test_a_new_build_invalidates(flags):
    W, H = SMALL
    with rt.Context(device=0, flags=flags) as c:
        setup(c, W, H)
        c.trace(W, H, 1)
        np.testing.assert_array_equal(c.read_framebuffer(), fresh(flags, W, H))
        c.set_scene(scene(SEED + 1))
        c.build()
        c.trace(W, H, 1)
        np.testing.assert_array_equal(c.read_framebuffer(), fresh(flags, W, H, seed=SEED + 1))
        assert c.bin_builds() == 2
        c.set_camera(*camera(W, H, orbit=3))
        c.build()
        c.trace(W, H, 1)
        np.testing.assert_array_equal(c.read_framebuffer(), fresh(flags, W, H, seed=SEED + 1, orbit=3))
        c.trace(W, H, 1)
        np.testing.assert_array_equal(c.read_framebuffer(), fresh(flags, W, H, seed=SEED + 1, orbit=3))
        assert c.bin_builds() == 3
        assert not np.array_equal(fresh(flags, W, H, seed=SEED + 1, orbit=3), fresh(flags, W, H, seed=SEED + 1))


@pytest.mark.parametrize("flags", MODES)
def test_bands_under_two_deals_and_alternating_ranks(flags):
    W, H = LARGE   # 17 bands of 8 rows
    with rt.Context(device=0, flags=flags) as c:
        setup(c, W, H)
        for share in (16, 13):
            c.set_band_deal(share)
            for r in range(3):
                np.testing.assert_array_equal(band(c, W, H, r, 3, share), fresh(flags, W, H, rank=r, nranks=3, share=share),
                                              err_msg=f"share {share} rank {r}")
        assert c.bin_builds() == 6
        for r in (0, 1, 0, 1, 1):
            np.testing.assert_array_equal(band(c, W, H, r, 3, 13), fresh(flags, W, H, rank=r, nranks=3, share=13),
                                          err_msg=f"alternating, rank {r}")
        assert c.bin_builds() == 10   # (one stream, one set: every change of rank refills it; the repeat does not)


@pytest.mark.parametrize("flags", MODES)
def test_four_streams_share_one_set(flags):
    """bench.py's run(): frame i on stream i % 4, stream 0 the context's; no host synchronisation between the first
    frame (which fills the set) and the frames of the other streams (which wait for the fill on the device)."""
    import torch
    W, H = LARGE
    want = fresh(flags, W, H, bounces=2)
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0") for _ in range(8)]
    with rt.Context(device=0, flags=flags, stream=streams[0].cuda_stream) as c:
        setup(c, W, H)
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            c.trace_band_async(W, H, 2, 0, 1, b.data_ptr(), stream_ptr=streams[i % 4].cuda_stream)
        c.synchronize()
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            np.testing.assert_array_equal(b.cpu().numpy(), want, err_msg=f"frame {i}")
        assert c.bin_builds() == 1 and c.bin_sets() == 1


@pytest.mark.parametrize("flags", MODES)
def test_build_while_frames_are_in_flight(flags):
    import torch
    W, H = LARGE
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = [torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0") for _ in range(8)]
    with rt.Context(device=0, flags=flags, stream=streams[0].cuda_stream) as c:
        setup(c, W, H)
        torch.cuda.synchronize()
        for i in range(4):
            c.trace_band_async(W, H, 2, 0, 1, bufs[i].data_ptr(), stream_ptr=streams[i].cuda_stream)
        c.set_camera(*camera(W, H, orbit=2))
        c.build(sync=False)   # (waits for the four frames on the device)
        for i in (3, 2, 1, 0):   # a caller stream's slot fills the new tree's set this time
            c.trace_band_async(W, H, 2, 0, 1, bufs[4 + i].data_ptr(), stream_ptr=streams[i].cuda_stream)
        c.synchronize()
        torch.cuda.synchronize()
        for i in range(4):
            np.testing.assert_array_equal(bufs[i].cpu().numpy(), fresh(flags, W, H, bounces=2), err_msg=f"old tree {i}")
            np.testing.assert_array_equal(bufs[4 + i].cpu().numpy(), fresh(flags, W, H, orbit=2, bounces=2),
                                          err_msg=f"new tree {i}")
        assert c.bin_builds() == 2


@pytest.mark.parametrize("flags", MODES)
def test_overflowed_bins_are_reused_with_their_walk(flags):
    """Leaves whose boxes cover most of the frame overflow the bins (3 entries per leaf + 16 per tile): the
    overflowed tiles are traced by a per-lane walk behind the binned kernel, which finds them in the set's tile
    offsets -- on the reusing trace too."""
    rng = np.random.default_rng(11)
    n = 3000
    c0 = rng.uniform(-40, 40, (n, 1, 3)).astype(np.float32)
    tri = (c0 + rng.uniform(-60, 60, (n, 3, 3)).astype(np.float32)).reshape(-1, 3)
    verts = np.zeros((3 * n, 8), np.float32)
    verts[:, :3] = tri
    verts[:, 5] = 1.0
    d = load_scene_fixture("Test")
    s = rt.Scene(verts, np.arange(3 * n, dtype=np.uint32), np.zeros(n, np.uint32), d["material_blob"])
    W, H = 800, 600
    with rt.Context(device=0) as ref:
        ref.set_scene(s)
        ref.set_camera(*rt.camera_reference(W, H))
        ref.build()
        ref.trace(W, H, 1)
        want = ref.read_framebuffer()
    with rt.Context(device=0, flags=flags | rt.FLAG_COUNT_VISITS) as c:
        c.set_scene(s)
        c.set_camera(*rt.camera_reference(W, H))
        c.build()
        for i in range(2):
            c.trace(W, H, 1)
            np.testing.assert_array_equal(c.read_framebuffer(), want, err_msg=f"trace {i}")
            assert c.stats()["internal_visits"][0] > 0   # a walk traced the overflowed tiles
        assert c.bin_builds() == 1


@pytest.mark.parametrize("flags", MODES)
def test_counts_of_a_reusing_trace(flags):
    """RTBVH_FLAG_COUNT_VISITS: the entries binned, the rays and the hits of a reusing trace are the filling
    trace's.  (The entries past the block test and the leaf visits they lead to depend on the order in which the
    waves claim a tile's bins, and a bounce ray's visits on whether the walk or the re-trace kernel takes a deferred
    ray -- from run to run of one and the same trace as well, so they say nothing about the bins: not compared.)"""
    W, H = LARGE
    with rt.Context(device=0, flags=flags | rt.FLAG_COUNT_VISITS) as c:
        setup(c, W, H)
        got = []
        for _ in range(3):
            c.trace(W, H, 2)
            got.append(c.stats())
        assert c.bin_builds() == 1
    assert got[0]["bin_entries"][0] > 0 and got[0]["hits"][0] > 0 and got[0]["hits"][1] > 0
    for st in got[1:]:
        assert st["bin_entries"][0] == got[0]["bin_entries"][0]
        for key in ("primary_rays", "bounce_rays", "hits", "textured_hits"):
            assert np.array_equal(np.asarray(st[key]), np.asarray(got[0][key])), key


def test_graph_frames_then_a_plain_trace():
    """RTBVH_FLAG_GRAPH | RTBVH_FLAG_AUTO_WALK past AUTO_WALK_MAX_TRIS (65,536 triangles: the certified walks, so
    the binned pass): the captured frame holds its own bin passes and marks no set valid, a plain trace behind it
    fills the set for the replayed tree and does not re-capture, and the next replay invalidates it again."""
    W, H = LARGE
    n = 70_000
    flags = rt.FLAG_GRAPH | rt.FLAG_AUTO_WALK
    with rt.Context(device=0) as ref:
        setup(ref, W, H, ntris=n)
        ref.trace(W, H, 1)
        want = ref.read_framebuffer()
    with rt.Context(device=0, flags=flags) as g:
        g.set_scene(scene(ntris=n))
        g.set_camera(*camera(W, H))
        for _ in range(2):
            g.compute_bvh(W, H, 1)
            np.testing.assert_array_equal(g.read_framebuffer(), want)
        assert g.stats()["graph_captures"] == 1 and g.stats()["walk_state"] == 2
        fills = g.bin_builds()
        for k in range(2):
            g.trace(W, H, 1)
            np.testing.assert_array_equal(g.read_framebuffer(), want, err_msg=f"plain trace {k}")
        assert g.bin_builds() == fills + 1 and g.stats()["graph_captures"] == 1
        g.compute_bvh(W, H, 1)   # a replay: it rewrites the tree and the context stream's set
        np.testing.assert_array_equal(g.read_framebuffer(), want)
        g.trace(W, H, 1)
        np.testing.assert_array_equal(g.read_framebuffer(), want)
        assert g.bin_builds() == fills + 2 and g.stats()["graph_captures"] == 1
