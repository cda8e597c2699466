"""Child process of tests/test_certified_bounces_gpu.py::test_every_deferred_ray_through_the_retrace_kernel.

Usage: python cert_variant_child.py OUT.npz, with RTBVH_LIB naming the library to load (the A/B build
librtbvh_defer_redo.so: no wave walks deferred rays inside the bounce walk, k_bounce_redo takes them all).
Traces the large and the few hall of mirrors (tests/cert_scenes.py), 3 bounces, certified, once on the
context stream and once on a caller stream, and writes frames, intensities and stats to OUT.npz.
"""
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np   # noqa: E402
import torch   # noqa: E402

import raytracebvh_amd as rt   # noqa: E402
from tests import cert_scenes as cs   # noqa: E402


def main(out_path):
    W, H, bounces = cs.W, cs.H, 3
    out = {"lib_path": np.array(rt._lib.LIB_PATH)}
    stream = torch.cuda.Stream()
    for variant in ("large", "few"):
        s = cs.hall_of_mirrors(variant)
        with rt.Context(device=0, flags=rt.FLAG_CERTIFIED | rt.FLAG_COUNT_VISITS) as c:
            c.set_scene(s)
            c.set_camera(*cs.camera("A"))
            c.compute_bvh(W, H, bounces)
            out[f"{variant}_ctx_fb"] = c.read_framebuffer()
            out[f"{variant}_ctx_inten"] = c.read_intensity()
            st = c.stats()
            for k in cs.STATS_CHECKED:
                out[f"{variant}_ctx_{k}"] = np.array(st[k], np.uint64)
            buf = torch.full((H, W, 4), -1.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()   # (the fill runs on torch's stream)
            c.trace_band_async(W, H, bounces, 0, 1, buf.data_ptr(), stream_ptr=stream.cuda_stream)
            c.synchronize()
            torch.cuda.synchronize()
            out[f"{variant}_slot_fb"] = buf.cpu().numpy()
            st = c.stats()
            for k in cs.STATS_CHECKED:
                out[f"{variant}_slot_{k}"] = np.array(st[k], np.uint64)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
