"""Certified ray queries (QUERY_CERTIFIED) without a GPU: the constants and the export, the preconditions of
tests/test_query_certified_gpu.py's inputs (so that its assertions cannot pass vacuously), and the t_max
initial-key encoding restated in numpy against the reference-order restatement."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import deep_scenes as ds
from tests import query_cert_ref as qc
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_query_gpu import edge_rays, random_rays

W, H = 64, 48


# ---------------------------------------------------------------- exports and constants
def test_constant_and_export():
    assert rt.QUERY_CERTIFIED == 256 == 1 << 8
    # bits 3..7 stay unknown: the composed modes use bits 0, 1, 2 and 8 only
    assert (rt.QUERY_CERTIFIED | rt.QUERY_ANY | rt.QUERY_SORT | rt.QUERY_COUNT) == 0x107
    assert "rtbvh_query_walk_counts" in rt._lib.EXPORTS
    L = rt.lib()
    out = (ctypes.c_uint64 * 4)()
    assert L.rtbvh_query_walk_counts(None, out) == rt._lib.ERR_INVALID_ARG   # (no context without a GPU)
    assert hasattr(rt.Context, "query_walk_counts")


# ---------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("variant", ["small", "large"])
def test_hall_rays_have_hits_the_certificate_rejects(variant):
    """For some rays the reference's own answer fails the certificate (Moller-Trumbore rounds t below the flat wall
    box's entry): a certified query must re-trace at least these."""
    tris, o, d, want, bad = qc.hall_case(variant)
    hits, fails = qc.HALL_EXPECT[variant]
    assert len(o) == qc.HALL_RAYS[variant]
    assert int(want["hit"].sum()) == hits
    assert int(bad.sum()) == fails > 0
    assert not qc.uncovered_mask(o, d).any()   # (unit directions inside the box: the walk takes them all)


def test_fan_rays_are_deep():
    tris, o, d, want = qc.fan_case()
    assert len(o) == 2048 and want["hit"].all()
    assert (want["max_stack"] == 35).all()   # past the 4-wide walk's 13 LDS entries and the binary walks' 16
    assert int(qc.uncovered_mask(o, d).sum()) == 3
    assert ds.fan()[0].num_tris == 97


@pytest.mark.parametrize("name", ["Test", "Rect", "Image_Test"])
def test_uncovered_counts_of_the_edge_rays(name):
    d = load_scene_fixture(name)
    oscene = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    nodes = orc.build(oscene, rt.camera_reference(W, H)[0])
    eo, ed = edge_rays(nodes)
    # axis-parallel (1 / 0), |d| >= 1.5, NaN and zero directions, a NaN origin: every edge ray is uncovered
    assert qc.uncovered_mask(eo, ed).all() and len(eo) == 16
    dd = (ed.astype(np.float64) ** 2).sum(1)
    assert all(np.isnan(x) or x == 0 or x == 1 or x >= 1.5 ** 2 for x in dd)
    ro, rd = random_rays(nodes, 4096)
    assert not qc.uncovered_mask(ro, rd).any()
    xo, xd = qc.extra_uncovered_rays(nodes)
    unc = qc.uncovered_mask(xo, xd)
    assert unc[:32].all() and not unc[32:].any()
    # far from the thresholds 2^20, 2^90 and MT_DD
    assert np.allclose((xd[32:].astype(np.float64) ** 2).sum(1), 0.25, rtol=1e-5)


# ---------------------------------------------------------------- the initial-key encoding of t_max
def test_initial_key_encoding_matches_reference_with_t_max():
    """Start the key at (t_max, 0xFFFFFFFF) and take the (t, leaf) minimum: for every ray whose reference answer
    passes the certificate this is the reference's answer -- t exactly at t_max still wins, a triangle beyond
    t_max never does, and a key that keeps the sentinel is a miss."""
    d = load_scene_fixture("Rect")
    oscene = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    wvp = rt.camera_reference(W, H)[0]
    nodes = orc.build(oscene, wvp)
    tris = rw.clip_triangles(d["vertices"], d["indices"], wvp)
    ro, rd = random_rays(nodes, 4096)
    eo, ed = edge_rays(nodes)
    o, dd = np.concatenate([ro, eo]), np.concatenate([rd, ed])
    free = rw.walk(nodes, tris, o, dd)
    t = free["t"]
    k = np.arange(len(t)) % 3
    t_max = np.where(free["hit"], np.where(k == 0, np.float32(.5) * t, np.where(k == 1, t, np.nextafter(t, np.float32(0)))),
                     np.float32(10)).astype(np.float32)
    for tm in (np.full(len(o), np.inf, np.float32), t_max):
        want = rw.walk(nodes, tris, o, dd, t_max=tm)
        key, tri = qc.brute_force_keys(nodes, tris, o, dd, tm)
        hit = (key & qc.SENTINEL) != qc.SENTINEL
        bt = np.where(hit, qc.key_t(key), np.float32(-1))
        # the reference's answer vouched for by its own box; a miss is vouched for when no triangle is in range
        ok = want["hit"] & ~qc.cert_failures(tris, want, o, dd)
        assert ok.sum() > 500   # (Rect: 2908 of the rays hit, about a third of them lose the hit to t_max)
        np.testing.assert_array_equal(hit[ok], True)
        np.testing.assert_array_equal(rw.bits(bt[ok]), rw.bits(want["t"][ok]))
        np.testing.assert_array_equal(tri[ok], want["tri"][ok])
        assert (bt[hit] <= tm[hit]).all()
        # and the other way round, as the kernel uses it: a winner whose own box passes is the reference's answer
        w = np.nonzero(hit)[0]
        cert = np.zeros(len(o), bool)
        cert[w] = qc.leaf_box_passes(tris, tri[w].astype(np.int64), o[w], dd[w], bt[w])
        np.testing.assert_array_equal(want["hit"][cert], True)
        np.testing.assert_array_equal(rw.bits(bt[cert]), rw.bits(want["t"][cert]))
        np.testing.assert_array_equal(tri[cert], want["tri"][cert])
    # t_max == t exactly kept the hit wherever the reference kept it
    at = free["hit"] & (k == 1)
    assert (want["hit"][at]).mean() > .9
    # no triangle can be accepted for !(t_max > EPSILON): the reference misses -- the kernel answers these rays
    # without a walk (as unsigned integers the key orders non-negative t_max only: NaN and negative values must
    # not reach it) -- and so does the key where it applies
    for bad in (np.nan, -1.0, 0.0, 0.01):
        tm = np.full(len(o), bad, np.float32)
        assert not rw.walk(nodes, tris, o, dd, t_max=tm)["hit"].any()
        if bad >= 0:
            key, _ = qc.brute_force_keys(nodes, tris, o, dd, tm)
            assert ((key & qc.SENTINEL) == qc.SENTINEL).all()
