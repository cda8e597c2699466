"""Ray queries, the part that needs no GPU: the numpy restatement of findCollision that the GPU tests
compare against (tests/ray_walk_ref.py) pinned to the CPU oracle's own counters, and the host-side surface
(exports, record sizes, argument validation)."""
import ctypes

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from raytracebvh_amd import _lib as L
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture

W, H = 64, 48
BACKGROUND = np.array([.5, .5, .5, 1.], np.float32)


def primary_rays(w, h):
    """RayTraceLaunch.hlsl:23-30: pixel (x, y) is the ray from ((x - W/2) / 4, (y - H/2) / 4, 0) along +z."""
    y, x = np.mgrid[0:h, 0:w]
    o = np.stack([(x.astype(np.float32) - np.float32(w >> 1)) / np.float32(4),
                  (y.astype(np.float32) - np.float32(h >> 1)) / np.float32(4), np.zeros((h, w), np.float32)], -1)
    d = np.zeros((h * w, 3), np.float32)
    d[:, 2] = 1
    return o.reshape(-1, 3), d


@pytest.fixture(scope="module", params=["Test", "Rect", "Image_Test"])
def pinned(request):
    d = load_scene_fixture(request.param)
    s = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    wvp, wv = orc.camera_reference(W, H)
    nodes = orc.build(s, wvp)
    fb0, _, st0, refl, _ = orc.trace(s, nodes, wvp, wv, W, H, 0, want_records=True)
    _, _, st1 = orc.trace(s, nodes, wvp, wv, W, H, 1)
    return {"nodes": nodes, "tris": rw.clip_triangles(d["vertices"], d["indices"], wvp), "fb0": fb0, "st0": st0,
            "st1": st1, "refl": refl.reshape(-1, 14)}


def test_restatement_primary_rays_match_oracle(pinned):
    o, d = primary_rays(W, H)
    r = rw.walk(pinned["nodes"], pinned["tris"], o, d)
    st = pinned["st0"]
    assert int(r["hit"].sum()) == st["hits"]
    assert int(r["internal"].sum()) == st["internal_visits"]
    assert int(r["leaf"].sum()) == st["leaf_visits"]
    np.testing.assert_array_equal(r["hit"].reshape(H, W), (pinned["fb0"] != BACKGROUND).any(-1))
    assert (r["tri"][~r["hit"]] == 0xFFFFFFFF).all() and (r["t"][~r["hit"]] == -1).all()
    assert int(r["max_stack"].max()) == st["max_stack"]


def test_restatement_nearest_order_returns_the_reference_hits(pinned):
    """order="nearest" (trace.hip's binary nearest-first rule) answers as the reference order on the OBJ scenes."""
    rec = pinned["refl"]
    live = rec[:, 0] > 0
    for o, d in (primary_rays(W, H), (rec[live, 1:4], rec[live, 4:7])):
        r = rw.walk(pinned["nodes"], pinned["tris"], o, d)
        q = rw.walk(pinned["nodes"], pinned["tris"], o, d, order="nearest")
        for f in ("t", "u", "v"):
            np.testing.assert_array_equal(rw.bits(q[f]), rw.bits(r[f]), err_msg=f)
        np.testing.assert_array_equal(q["tri"], r["tri"])
        assert int(q["internal"].sum()) <= int(r["internal"].sum())


def test_restatement_reflect_records_match_oracle(pinned):
    rec = pinned["refl"]
    live = rec[:, 0] > 0
    r = rw.walk(pinned["nodes"], pinned["tris"], rec[live, 1:4], rec[live, 4:7])
    st0, st1 = pinned["st0"], pinned["st1"]
    assert int(live.sum()) == st1["bounce"]
    assert int(r["hit"].sum()) == st1["hits"] - st0["hits"]
    assert int(r["internal"].sum()) == st1["internal_visits"] - st0["internal_visits"]
    assert int(r["leaf"].sum()) == st1["leaf_visits"] - st0["leaf_visits"]
    # any-hit answers the same question, and its triangle is a genuine hit
    a = rw.walk(pinned["nodes"], pinned["tris"], rec[live, 1:4], rec[live, 4:7], any_hit=True)
    np.testing.assert_array_equal(a["hit"], r["hit"])
    h = a["hit"]
    t, u, v = rw.tri_test(pinned["tris"], a["tri"][h].astype(np.int64), rec[live, 1:4][h], rec[live, 4:7][h])
    np.testing.assert_array_equal(rw.bits(t), rw.bits(a["t"][h]))
    np.testing.assert_array_equal(rw.bits(u), rw.bits(a["u"][h]))
    np.testing.assert_array_equal(rw.bits(v), rw.bits(a["v"][h]))


def test_restatement_t_max(pinned):
    """t_max at the closest t keeps the hit; just below it the ray takes a farther triangle or misses."""
    o, d = primary_rays(W, H)
    r = rw.walk(pinned["nodes"], pinned["tris"], o, d)
    h = r["hit"]
    at = rw.walk(pinned["nodes"], pinned["tris"], o[h], d[h], t_max=r["t"][h])
    np.testing.assert_array_equal(rw.bits(at["t"]), rw.bits(r["t"][h]))
    np.testing.assert_array_equal(at["tri"], r["tri"][h])
    below = rw.walk(pinned["nodes"], pinned["tris"], o[h], d[h], t_max=np.nextafter(r["t"][h], np.float32(0)))
    assert (~below["hit"] | (below["t"] < r["t"][h])).all()
    assert not (below["hit"] & (below["tri"] == r["tri"][h])).any()


def test_library_exports_and_record_sizes():
    lib = rt.lib()
    for name in ("rtbvh_query_async", "rtbvh_query_host", "rtbvh_query_counts"):
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    assert ctypes.sizeof(L.Ray) == 32 and ctypes.sizeof(L.Hit) == 16
    assert rt.RAY_DTYPE.itemsize == ctypes.sizeof(L.Ray) and rt.HIT_DTYPE.itemsize == ctypes.sizeof(L.Hit)
    for f in ("origin", "t_max", "direction", "reserved"):
        assert rt.RAY_DTYPE.fields[f][1] == getattr(L.Ray, f).offset
    for f in ("t", "u", "v", "tri"):
        assert rt.HIT_DTYPE.fields[f][1] == getattr(L.Hit, f).offset
    assert (rt.QUERY_CLOSEST, rt.QUERY_ANY, rt.QUERY_SORT, rt.QUERY_COUNT) == (0, 1, 2, 4)
    assert lib.rtbvh_abi_version() == 8


def test_make_rays_numpy():
    o = np.arange(6, dtype=np.float64).reshape(2, 3)
    d = np.ones((2, 3))
    rays = rt.make_rays(o, d)
    assert rays.dtype == rt.RAY_DTYPE and rays.shape == (2,)
    np.testing.assert_array_equal(rays["origin"], o.astype(np.float32))
    assert np.isinf(rays["t_max"]).all() and (rays["reserved"] == 0).all()
    rays = rt.make_rays(o, d, t_max=[1.5, 2.5])
    np.testing.assert_array_equal(rays["t_max"], np.array([1.5, 2.5], np.float32))
    flat = rays.view(np.float32).reshape(2, 8)
    np.testing.assert_array_equal(flat[:, 4:7], 1)
    with pytest.raises(ValueError):
        rt.make_rays(o, np.ones((3, 3)))


@pytest.mark.parametrize("bad", [
    np.zeros((4, 7), np.float32),                 # wrong shape
    np.zeros((4, 8), np.float64),                 # wrong dtype
    np.zeros(32, np.float32),                     # not (N, 8)
    np.zeros((4, 16), np.float32)[:, ::2],        # not contiguous
    np.zeros((2, 2), L.RAY_DTYPE),                # RAY_DTYPE, not one-dimensional
    np.zeros(8, L.RAY_DTYPE)[::2],                # RAY_DTYPE, not contiguous
    [[0.0] * 8],                                  # not an array
], ids=["shape", "dtype", "ndim", "strided", "ray-2d", "ray-strided", "list"])
def test_query_rejects_bad_rays_before_the_library(bad):
    ctx = rt.Context.__new__(rt.Context)   # no rtbvh_ctx behind it: the check must come first
    with pytest.raises(ValueError):
        ctx.query(bad)
    with pytest.raises(ValueError):
        rt.check_query_rays(bad)


def test_query_rejects_host_tensors():
    import torch
    ctx = rt.Context.__new__(rt.Context)
    with pytest.raises(ValueError):
        ctx.query(torch.zeros((4, 8), dtype=torch.float32))   # a CPU tensor: the wrong device
    with pytest.raises(ValueError):
        rt.check_query_rays(torch.zeros((4, 8), dtype=torch.float64))
    with pytest.raises(ValueError):
        rt.check_query_rays(torch.zeros((8, 4), dtype=torch.float32))


def test_check_query_rays_accepts_both_numpy_forms():
    kind, r = rt.check_query_rays(np.zeros((5, 8), np.float32))
    assert kind == "numpy" and r.dtype == rt.RAY_DTYPE and r.shape == (5,)
    kind, r = rt.check_query_rays(np.zeros(3, rt.RAY_DTYPE))
    assert kind == "numpy" and r.shape == (3,)
