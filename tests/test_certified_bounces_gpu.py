"""The certified walks (RTBVH_FLAG_CERTIFIED, RTBVH_FLAG_AUTO_WALK above its size) over frames of several
bounce passes with deferred rays in every pass: the halls of mirrors of tests/cert_scenes.py
(tests/test_cert_scenes_cpu.py shows, by the oracle alone, that every pass defers rays and walks rays).

What a one-pass frame cannot show: the defer list is reused by the passes of a frame and by the frames of a
context (zeroed once; "clean" because every reader clears what it takes), each pass has its own counters,
and three readers take deferred rays (the deferral workers, the drained waves, k_bounce_redo's leftover
branch).  Every comparison is bit for bit against the CPU oracle's whole frame; every test runs once."""
import os
import subprocess
import sys

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import cert_scenes as cs

pytestmark = pytest.mark.gpu

W, H = cs.W, cs.H
CERT = rt.FLAG_CERTIFIED | rt.FLAG_COUNT_VISITS
WALK_FLAGS = rt.FLAG_NEAREST_FIRST | rt.FLAG_PACKET_PRIMARY | rt.FLAG_REFILL_BOUNCE | rt.FLAG_WIDE_BVH
BINNED_FAST = WALK_FLAGS | rt.FLAG_BINNED_PRIMARY
VARIANT_LIB = os.path.join(rt._lib.HERE, "librtbvh_defer_redo.so")


def _check_stats(st, want):
    """hits, bounce_rays and textured_hits count a ray shaded twice twice, so their equality with the oracle's
    is the double-shading detector (and a ray left unshaded shows in them and in the frame)."""
    ost = want["stats"]
    assert sum(st["hits"]) == ost["hits"]
    assert st["bounce_rays"] == ost["bounce"]
    assert st["textured_hits"] == ost["textured_hits"]
    assert st["stack_overflows"] == 0
    assert st["redo_deferred"] == want["deferred"]
    assert st["redo_rays"][1] >= st["redo_deferred"]
    assert st["redo_total"] == st["redo_rays"][0] + st["redo_rays"][1]


def _check_frame(c, want):
    np.testing.assert_array_equal(c.read_framebuffer(), want["fb"])
    np.testing.assert_array_equal(c.read_intensity(), want["inten"])
    _check_stats(c.stats(), want)


@pytest.mark.parametrize("variant,walk,bounces", [("small", "certified", 3), ("large", "certified", 3),
                                                  ("large", "auto", 3), ("few", "certified", 3), ("few", "auto", 3),
                                                  ("small", "certified", 14)])
def test_three_pass_frame(variant, walk, bounces):
    """A frame of 3 passes (and one of 14, the ABI's maximum) whose every pass has deferred rays, flagged rays
    and early-shaded rays feeding the next queue: framebuffer and intensity equal the oracle's whole frame.
    sum(hits), bounce_rays and textured_hits equal the oracle's: a ray shaded twice counts twice in these, so
    they are the double-shading detector.  redo_deferred is the oracle's count of the rays the walk's claim-time
    test defers, summed over the passes (each pass has its own counter).  (RTBVH_FLAG_AUTO_WALK takes the
    reference order on the small scene: not run there.)"""
    s, _, _, wvp, wv = cs.hall(variant, "A")
    want = cs.hall_oracle(variant, "A", bounces)
    assert want["deferred"] > 0 and want["stats"]["bounce"] > want["deferred"]
    flags = rt.FLAG_AUTO_WALK if walk == "auto" else rt.FLAG_CERTIFIED
    with rt.Context(device=0, flags=flags | rt.FLAG_COUNT_VISITS) as c:
        c.set_scene(s)
        c.set_camera(wvp, wv)
        c.compute_bvh(W, H, bounces)
        _check_frame(c, want)
        if walk == "auto":
            assert c.stats()["walk_state"] == 2


def test_frames_a_b_a_keep_the_defer_list_clean():
    """One certified context, cameras A, B, A, B: each frame and each redo_deferred is its own camera's (the two
    cameras defer different pixels and different counts), so no entry of the defer list and no per-pass counter
    survives a frame.  Then fewer passes followed by more on the last tree, a larger frame (which reallocates the
    defer and re-trace lists), and the first size again."""
    s = cs.hall("large", "A")[0]
    want = {cam: cs.hall_oracle("large", cam, 3) for cam in "AB"}
    assert want["A"]["deferred"] != want["B"]["deferred"]
    with rt.Context(device=0, flags=CERT) as c:
        c.set_scene(s)
        for cam in "ABAB":
            c.set_camera(*cs.camera(cam))
            c.compute_bvh(W, H, 3)
            _check_frame(c, want[cam])
        c.trace(W, H, 1)
        _check_frame(c, cs.hall_oracle("large", "B", 1))
        c.trace(W, H, 3)
        _check_frame(c, want["B"])
        c.trace(2 * W, 2 * H, 3)
        _check_frame(c, cs.hall_oracle("large", "B", 3, 2 * W, 2 * H))
        c.trace(W, H, 3)
        _check_frame(c, want["B"])


def test_graph_replays():
    """RTBVH_FLAG_CERTIFIED | RTBVH_FLAG_GRAPH: the first compute_bvh captures, the next two replay the graph at
    camera B and back at A (the early-shading instance inside a captured graph, the list and the counters
    zeroed by the replayed launches): one capture, each frame and redo_deferred its camera's."""
    s = cs.hall("large", "A")[0]
    with rt.Context(device=0, flags=CERT | rt.FLAG_GRAPH) as g:
        g.set_scene(s)
        for cam in "ABA":
            g.set_camera(*cs.camera(cam))
            g.compute_bvh(W, H, 3)
            _check_frame(g, cs.hall_oracle("large", cam, 3))
        assert g.stats()["graph_captures"] == 1


@pytest.mark.parametrize("nranks,share", [(1, 16), (3, 11)])
def test_slots_and_bands(nranks, share):
    """Each rank's bands of a 3-pass frame, traced alone on the context stream (the walk's early-shading instance)
    and as three frames in flight on caller streams (the plain instance, the slots' own defer lists): every
    in-flight buffer equals the one traced alone, a slot's redo_deferred equals the alone trace's, the ranks'
    counts add up to the frame's, and the bands put back in their rows give the oracle's frame."""
    import torch

    from raytracebvh_amd.tiles import band_row_ids
    s, _, _, wvp, wv = cs.hall("large", "A")
    want = cs.hall_oracle("large", "A", 3)
    streams = [torch.cuda.Stream() for _ in range(3)]
    with rt.Context(device=0, flags=CERT) as c:
        c.set_scene(s)
        c.set_camera(wvp, wv)
        c.compute_bvh(W, H, 3)
        _check_frame(c, want)
        c.set_band_deal(share)
        frame = np.zeros_like(want["fb"])
        deferred = []
        for r in range(nranks):
            rows = rt.lib().rtbvh_deal_rows(H, r, nranks, share)
            alone = torch.full((rows, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
            bufs = [torch.full((rows, W, 4), -1.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
            torch.cuda.synchronize()   # (the fills run on torch's stream)
            c.trace_band_async(W, H, 3, r, nranks, alone.data_ptr())
            c.synchronize()
            st = c.stats()
            deferred.append(st["redo_deferred"])
            assert st["stack_overflows"] == 0 and st["redo_rays"][1] >= st["redo_deferred"]
            for i, b in enumerate(bufs):
                c.trace_band_async(W, H, 3, r, nranks, b.data_ptr(), stream_ptr=streams[i].cuda_stream)
            c.synchronize()
            torch.cuda.synchronize()
            for i, b in enumerate(bufs):
                assert torch.equal(b, alone), (r, i)
            slot = c.stats()
            assert slot["redo_deferred"] == deferred[-1]
            assert slot["bounce_rays"] == st["bounce_rays"] and sum(slot["hits"]) == sum(st["hits"])
            frame[band_row_ids(H, r, nranks, share)] = alone.cpu().numpy()
        np.testing.assert_array_equal(frame, want["fb"])
        assert all(n > 0 for n in deferred) and sum(deferred) == want["deferred"]


@pytest.mark.parametrize("knobs", [{"RTBVH_EARLY_SHADE": "0"}, {"RTBVH_KEEP_RECORDS": "1"},
                                   {"RTBVH_EARLY_SHADE": "0", "RTBVH_KEEP_RECORDS": "1"}],
                         ids=["no early shading", "keep records", "both"])
def test_knobs_render_the_default_frame(knobs, monkeypatch):
    """The A/B knobs rtbvh_create reads (shading in a launch of its own after the walk; a certified-only build
    that also writes the node records): frame, intensity, hits, bounce_rays and redo_deferred are the default
    context's (and the oracle's)."""
    s, _, _, wvp, wv = cs.hall("large", "A")
    want = cs.hall_oracle("large", "A", 3)

    def frame():
        with rt.Context(device=0, flags=CERT) as c:
            c.set_scene(s)
            c.set_camera(wvp, wv)
            c.compute_bvh(W, H, 3)
            return c.read_framebuffer(), c.read_intensity(), c.stats()
    for k in ("RTBVH_EARLY_SHADE", "RTBVH_KEEP_RECORDS"):
        monkeypatch.delenv(k, raising=False)
    dfb, dint, dst = frame()
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)   # (before the context is created)
    fb, inten, st = frame()
    np.testing.assert_array_equal(fb, dfb)
    np.testing.assert_array_equal(inten, dint)
    for k in ("hits", "bounce_rays", "redo_deferred", "textured_hits"):
        assert st[k] == dst[k], k
    np.testing.assert_array_equal(dfb, want["fb"])
    _check_stats(st, want)


def test_every_deferred_ray_through_the_retrace_kernel(tmp_path):
    """The A/B library librtbvh_defer_redo.so (-DRTBVH_DEFER_INWALK=0 -DRTBVH_DEFER_WORKERS=0; build() makes it)
    has no wave that walks deferred rays inside k_bounce_trav: every deferred ray of every pass reaches
    k_bounce_redo's leftover branch (i < nd), which the product library reaches only by timing.  A fresh child
    process loads it (RTBVH_LIB) and traces the large and the few hall, 3 passes, on the context stream and on a
    caller stream: frames and stats equal the oracle's."""
    assert os.path.exists(VARIANT_LIB), f"{VARIANT_LIB} is not built (__graft_entry__.build() makes it)"
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cert_variant_child.py")
    out = str(tmp_path / "variant.npz")
    p = subprocess.run([sys.executable, helper, out], env={**os.environ, "RTBVH_LIB": VARIANT_LIB}, timeout=120,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    z = np.load(out)
    assert str(z["lib_path"]) == VARIANT_LIB
    for variant in ("large", "few"):
        want = cs.hall_oracle(variant, "A", 3)
        for where in ("ctx", "slot"):   # the context stream, a caller stream
            np.testing.assert_array_equal(z[f"{variant}_{where}_fb"], want["fb"], err_msg=f"{variant} {where}")
            _check_stats({k: z[f"{variant}_{where}_{k}"].tolist() for k in cs.STATS_CHECKED}, want)
        np.testing.assert_array_equal(z[f"{variant}_ctx_inten"], want["inten"])


@pytest.mark.parametrize("fw,fh", [(32768, 16), (32776, 16), (16, 32768), (16, 32776)])
def test_frames_past_the_binned_pass_size(fw, fh):
    """The binned primary pass's footprints are exact up to 32768 pixels a side (rtbvh_device.h leaf_footprint); a
    wider or taller frame leaves it (api.hip enqueue_walks): a certified trace takes the reference-order lane
    walk, any other the 4-wide packet walk, which needs the leaf pseudo-records derived.  Frames at the last
    size that bins and at the first past it, wide and tall, over a strip of triangles under every column (row),
    the first and last 8 included: each walk's frame equals the reference order's, which equals the oracle's on
    sampled rows."""
    tall = fh > fw
    s = cs.strip_scene(tall)
    wvp, wv = cs.camera("A")
    with rt.Context(device=0) as ref:
        ref.set_scene(s)
        ref.set_camera(wvp, wv)
        ref.compute_bvh(fw, fh, 1)
        want = ref.read_framebuffer()
        nodes = ref.read_bvh()
    os_ = cs.oscene_of(s)
    if tall:   # the rows that hold the strip's ends
        for r0, r1 in ((0, 8), (fh - 8, fh)):
            ofb, _, ost = orc.trace(os_, nodes, wvp, wv, fw, fh, 1, r0, r1, 1)
            np.testing.assert_array_equal(want[r0:r1], ofb)
            assert ost["hits"] == 8 * fw
    else:
        ofb, _, ost = orc.trace(os_, nodes, wvp, wv, fw, fh, 1, 3, fh, 8)
        np.testing.assert_array_equal(want[3:fh:8], ofb)
        assert ost["hits"] == 2 * fw
    hit = want[..., 0] != 0.5   # (a primary miss leaves the clear colour; a hit's 0.32 is blended towards it)
    ends = (hit[:8], hit[-8:]) if tall else (hit[:, :8], hit[:, -8:])
    assert ends[0].all() and ends[1].all()
    for flags in (rt.FLAG_CERTIFIED, BINNED_FAST, rt.FLAG_BINNED_PRIMARY):
        with rt.Context(device=0, flags=flags) as c:
            c.set_scene(s)
            c.set_camera(wvp, wv)
            c.compute_bvh(fw, fh, 1)
            np.testing.assert_array_equal(c.read_framebuffer(), want, err_msg=hex(flags))
            if flags == BINNED_FAST:
                assert c.stats()["walk_flags"] == BINNED_FAST
