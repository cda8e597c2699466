"""bench.py's command line: a plain run reports the headline alone and honours --steps, --full keeps
the side measurements, and --dump-outputs writes the frame of the last timed step."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("rtbvh_bench_py", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(tmp_path):
    """A frame within DUMP_BUDGET is written whole; a larger one as the same seeded pixel sample every
    time, in float32, within the budget."""
    b = _bench_module()
    rng = np.random.default_rng(3)
    small = rng.random((9, 7, 4), dtype=np.float32)
    b.dump_outputs(str(tmp_path / "a"), small)
    got = np.load(tmp_path / "a" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    assert b.DUMP_BUDGET <= 64 * 10**6
    # one pixel more than the budget holds (height 1: a (1, n + 1, 4) frame)
    n = b.DUMP_BUDGET // 16
    big = np.arange(4 * (n + 1), dtype=np.float32).reshape(1, n + 1, 4)
    b.dump_outputs(str(tmp_path / "b"), big)
    b.dump_outputs(str(tmp_path / "c"), big)
    s1 = np.load(tmp_path / "b" / "frame.npy", mmap_mode="r")
    s2 = np.load(tmp_path / "c" / "frame.npy", mmap_mode="r")
    assert s1.dtype == np.float32 and s1.shape == (n, 4) and s1.nbytes <= b.DUMP_BUDGET
    assert np.array_equal(s1, s2)
    px = (s1[:, 0] / 4).astype(np.int64)          # the sampled pixels: rows of `big`, ascending, one left out
    assert (np.diff(px) >= 1).all() and np.array_equal(s1[:, 1], s1[:, 0] + 1)


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_certified_frame(tmp_path):
    """A plain run on C3 (Test.obj, 1920x1080): the result line holds the headline fields and none of the
    --full measurements, --steps is the number of timed steps, and the dumped frame is the certified
    mode's frame of the same scene and camera traced here (bit for bit)."""
    import raytracebvh_amd as rt

    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--workload", "c3", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "Mrays/s"
    assert d["value"] == pytest.approx(d["config"]["rays_per_step"] / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert d["traversal"]["mode"] == "certified" and d["full"] is False
    for key in ("cpu_baseline", "parity", "roofline", "build", "kernels", "c3_1080p", "frame_rebuild"):
        assert key not in d, key
    frame = np.load(tmp_path / "out" / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (1080, 1920, 4)
    scene = rt.load_npz(os.path.join(REPO, "tests", "golden", "scenes", "Test.npz"))
    with rt.Context(device=0, flags=rt.FLAG_CERTIFIED) as c:
        c.set_scene(scene)
        c.set_camera(*rt.camera_reference(1920, 1080))
        c.compute_bvh(1920, 1080, 1)
        want = c.read_framebuffer()
    assert np.array_equal(frame, want)
