"""Animated geometry without a device: the new entry points' NULL-context answers, the Python wrapper's input
checks (raytracebvh_amd.check_vertex_array, which Context.update_vertices runs first) and the host tool's
--animate mode in its usage text."""
import os
import subprocess

import numpy as np
import pytest

import raytracebvh_amd as rt
from tests.test_tools import TOOL, _build_tool


def test_null_context_is_an_invalid_argument():
    L = rt.lib()
    p = np.zeros((4, 3), np.float32)
    assert L.rtbvh_update_vertices_async(None, p.ctypes.data, 3, None, 0, 0, 4, None) == rt._lib.ERR_INVALID_ARG
    assert L.rtbvh_update_vertices_host(None, p.ctypes.data, 3, None, 0, 0, 4) == rt._lib.ERR_INVALID_ARG
    assert L.rtbvh_update_vertices_host(None, None, 3, None, 0, 0, 0) == rt._lib.ERR_INVALID_ARG
    assert L.rtbvh_refit_async(None) == rt._lib.ERR_INVALID_ARG
    assert L.rtbvh_refit(None) == rt._lib.ERR_INVALID_ARG


def test_numpy_arrays_and_their_strides():
    p = np.arange(30, dtype=np.float32).reshape(10, 3)
    kind, a, stride = rt.check_vertex_array(p)
    assert kind == "numpy" and a is p and stride == 3
    v = np.zeros((10, 8), np.float32)   # an rtbvh_vertex array: positions at 0, normals at 3
    assert rt.check_vertex_array(v[:, :3])[2] == 8 and rt.check_vertex_array(v[:, 3:6], "normals")[2] == 8
    assert rt.check_vertex_array(np.zeros((10, 4), np.float32)[:, :3])[2] == 4
    assert rt.check_vertex_array(v[::2, :3])[2] == 16
    kind, a, stride = rt.check_vertex_array(p[:0])
    assert kind == "numpy" and a.shape == (0, 3) and stride == 3
    assert rt.check_vertex_array(v[:1, 3:6])[1].flags["C_CONTIGUOUS"]   # (one row: packed)


@pytest.mark.parametrize("bad", [
    np.zeros((10, 3), np.float64), np.zeros((10, 3), np.int32), np.zeros(30, np.float32), np.zeros((10, 2), np.float32),
    np.zeros((10, 4), np.float32), np.zeros((2, 5, 3), np.float32), np.zeros((3, 10), np.float32).T,
    np.zeros((10, 6), np.float32)[:, ::2], np.zeros((10, 3), np.float32)[::-1], [[0.0, 0.0, 0.0]], None,
], ids=["f64", "i32", "flat", "two-columns", "four-columns", "3d", "transposed", "column-stride", "reversed", "list",
        "none"])
def test_bad_arrays_are_rejected(bad):
    with pytest.raises(ValueError, match="update_vertices"):
        rt.check_vertex_array(bad)


def test_tensors_must_be_float32_and_on_the_gpu():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="GPU"):
        rt.check_vertex_array(torch.zeros((10, 3)))   # a CPU tensor: numpy arrays take the host path
    for bad in (torch.zeros((10, 3), dtype=torch.float64), torch.zeros((10, 4)), torch.zeros(30),
                torch.zeros((10, 3), dtype=torch.int32)):
        with pytest.raises(ValueError, match="float32"):
            rt.check_vertex_array(bad, "normals")


def test_context_methods_exist():
    for name in ("update_vertices", "refit"):
        assert callable(getattr(rt.Context, name))


def test_tool_help_lists_animate():
    _build_tool()
    r = subprocess.run([TOOL, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--animate" in r.stdout and "--refit" in r.stdout
    r = subprocess.run([TOOL, "--synthetic", "10", "--refit"], capture_output=True, text=True)
    assert r.returncode == 1 and "--animate" in r.stderr
