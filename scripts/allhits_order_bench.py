"""The cost of RTBVH_ALLHITS_BY_T's ordering pass by list length: the measurement behind its thresholds.

    python scripts/allhits_order_bench.py [--out FILE] [--reps 5]
    RTBVH_LIB=<a build with -DRTBVH_ALLHITS_LANE_MAX=.. / -DRTBVH_ALLHITS_LDS_MAX=..> python scripts/allhits_order_bench.py

A stack of K parallel triangles (plane k at z = 0.1 k, dealt in a shuffled order) is pierced by N rays whose t_max
cuts every list to exactly m hits, for each m of `--lengths`.  Rays along +z meet the planes in nearly ascending t
(the sort order follows z): the insertion sort's best case; rays along -z from above meet them in descending t: its
worst case.  Per m and direction: mode 0 and mode 0 | BY_T, HIP events around the call, the median of `reps` after a
warm-up; the difference is the ordering pass (two launches and the rays' stored counts included).  Prints and, with
--out, writes JSON: microseconds of the pass per 1000 lists.  Not part of bench.py.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def stack(K):
    import raytracebvh_amd as rt
    t = np.zeros((K + 2, 3, 3), np.float32)
    t[:K, :, :2] = np.float32([[-1, -1], [17, -1], [-1, 17]])
    t[:K, :, 2] = (np.arange(K) * 0.1).astype(np.float32)[:, None]
    t[K] = [(-2, -2, -1), (-1.9, -2, -1), (-2, -1.9, -1)]
    t[K + 1] = [(18, 18, 0.1 * K + 1), (17.9, 18, 0.1 * K + 1), (18, 17.9, 0.1 * K + 1)]
    t[:K] = t[np.random.default_rng(K).permutation(K)]
    v = np.zeros((3 * (K + 2), 8), np.float32)
    v[:, :3] = t.reshape(-1, 3)
    v[:, 5] = -1
    return rt.Scene(v, np.arange(3 * (K + 2), dtype=np.uint32), np.zeros(K + 2, np.uint32),
                    np.zeros(1, rt.MATERIAL_DTYPE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--planes", type=int, default=8192)
    ap.add_argument("--lengths", default="2,4,8,12,16,24,32,48,64,128,512,1024,2048,4096,8192")
    args = ap.parse_args()
    lengths = [int(x) for x in args.lengths.split(",")]
    K = args.planes

    import torch

    import raytracebvh_amd as rt

    L = rt.lib()
    eye = np.eye(4, dtype=np.float32)
    res = {}
    with rt.Context(device=0) as ctx:
        ctx.set_scene(stack(K))
        ctx.set_camera(eye, eye)
        ctx.build()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        sh = ctypes.c_void_p(stream.cuda_stream)
        rng = np.random.default_rng(1)
        for m in lengths:
            n = int(min(65536, max(64, (1 << 25) // m)))
            xy = rng.uniform(1, 7, (n, 2))
            for name, z0, dz in (("ascending", -0.5, 1.0), ("descending", 0.1 * (K - 1) + 0.5, -1.0)):
                o = np.concatenate([xy, np.full((n, 1), z0)], 1).astype(np.float32)
                d = np.tile(np.float32([0, 0, dz]), (n, 1))
                rays = torch.from_numpy(rt.make_rays(o, d, np.float32(0.5 + 0.1 * (m - 1) + 0.05))
                                        .view(np.float32).reshape(n, 8)).cuda()
                offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
                hits = torch.empty((n * m, 4), dtype=torch.float32, device="cuda")

                def run(mode):
                    ms = []
                    for k in range(args.reps + 1):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        st = L.rtbvh_allhits_async(ctx._h, ctypes.c_void_p(rays.data_ptr()), n,
                                                   ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(hits.data_ptr()),
                                                   n * m, mode, sh)
                        assert st == 0, st
                        e1.record(stream)
                        e1.synchronize()
                        if k:
                            ms.append(e0.elapsed_time(e1))
                    return float(np.median(ms))

                plain = run(0)
                assert int(offsets[-1].item()) == n * m, (m, name, int(offsets[-1].item()))
                by_t = run(rt.ALLHITS_BY_T)
                t = hits[:, 0].reshape(n, m)
                assert bool((t[:, 1:] >= t[:, :-1]).all()), (m, name)
                res.setdefault(name, {})[str(m)] = {
                    "lists": n, "ms_mode0": round(plain, 4), "ms_by_t": round(by_t, 4),
                    "order_us_per_1000_lists": round((by_t - plain) * 1e6 / n, 2)}
                del rays, offsets, hits
        ctx.synchronize()
    result = {"workload": f"{K} stacked planes, lists cut to m hits by t_max; ascending: rays along +z, descending: -z",
              "library": os.environ.get("RTBVH_LIB", "librtbvh.so"), "device": torch.cuda.get_device_name(0),
              "reps": args.reps, "results": res}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
