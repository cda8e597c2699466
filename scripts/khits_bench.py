"""First-k ray query throughput on the C5 scene, beside what a caller had before for the same rays.

    python scripts/khits_bench.py [--out profiles/khits_bench.json] [--reps 5]

Builds C5 (10M synthetic triangles, 3840 x 2160) and takes the rays scripts/query_bench.py takes: the live reflection
rays of the reference-order frame's primary pass, in pixel order, t_max = +inf.  Times Context.khits on device
tensors with HIP events around the call, the median of `reps` repetitions after one warm-up, for k = 1, 2, 8 and 16,
each in the given order and with KHITS_SORT, and reads the steps per ray of one KHITS_COUNT query per k (the order
does not change a ray's walk).  The sorted and the unsorted lists must be the same bits, each k's list must start
with the smaller k's, and slot 0 must be a hit exactly where the closest-hit query hits.  In the same process:

  query_closest     rtbvh_query_async, QUERY_CLOSEST (the plain kernel), and with QUERY_SORT;
  query_certified   QUERY_CERTIFIED, and with QUERY_SORT;
  allhits_by_t      rtbvh_allhits_async in one call (sizes, scan, fill) with ALLHITS_BY_T and capacity = the exact
                    total, and with ALLHITS_SORT: the route to "the first k crossings" before this query, without the
                    host's cut of each list.  Timed before and after the first-k cases (the drift between the two
                    is the noise to hold a difference against); the ratios use the mean of the two medians.

Writes ms, Mrays/s, the steps, and each first-k case's time over the all-hits route's and over the closest-hit
query's as JSON.  No gate.  Not part of bench.py.  RTBVH_LIB=<an A/B build of the library> measures that build.
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

KS = (1, 2, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "khits_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    assert torch.cuda.is_available(), "khits_bench needs a GPU"
    W, H = args.width, args.height
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    with rt.Context(device=0, flags=rt.FLAG_REFRACT_RECORDS) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(*rt.camera_reference(W, H))
        ctx.build()
        ctx.trace(W, H, 0)   # the reflect records of the primary pass: the rays the bounce pass walks (query_bench)
        refl, _ = ctx.read_rays()
        rec = refl.reshape(-1, 14)
        live = rec[:, 0] > 0
        host = rt.make_rays(rec[live, 1:4], rec[live, 4:7])
        del refl, rec
        rays = torch.from_numpy(host.view(np.float32).reshape(-1, 8)).cuda()
        n = int(rays.shape[0])
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())

        def timed(f):
            ms = []
            for rep in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                if rep:   # (the first is the warm-up)
                    ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            return {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                    "ms_median": round(med, 4), "mrays_per_s": round(n / med / 1e3, 1)}

        res = {}
        # what a caller had before: the closest-hit queries ...
        qout = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        for name, mode in (("query_closest", rt.QUERY_CLOSEST), ("query_closest_sort", rt.QUERY_SORT),
                           ("query_certified", rt.QUERY_CERTIFIED),
                           ("query_certified_sort", rt.QUERY_CERTIFIED | rt.QUERY_SORT)):
            res[name] = timed(lambda: ctx.query(rays, mode, out=qout, stream=stream))
            ctx.query(rays, mode | rt.QUERY_COUNT, out=qout, stream=stream)
            qc = ctx.query_counts()
            res[name]["internal_steps_per_ray"] = round(qc["internal_visits"] / n, 3)
            res[name]["leaf_steps_per_ray"] = round(qc["leaf_visits"] / n, 3)
        ctx.query(rays, rt.QUERY_CLOSEST, out=qout, stream=stream)
        stream.synchronize()
        closest_hit = qout[:, 0] != -1
        # ... and every crossing, ordered by (t, tri), in one call
        offsets, _ = ctx.allhits(rays, mode=rt.ALLHITS_COUNT, capacity=0, stream=stream)
        stream.synchronize()
        ac = ctx.allhits_counts()
        total = int(offsets[n].item())
        assert ac["rays"] == n and ac["hits"] == total, ac
        res["allhits"] = {"hits": total, "hits_per_ray": round(total / n, 3),
                          "longest_list": int((offsets[1:] - offsets[:-1]).max().item()),
                          "internal_steps_per_ray_both_passes": round(ac["internal_steps"] / n, 3),
                          "leaf_steps_per_ray_both_passes": round(ac["leaf_steps"] / n, 3)}
        ahits = torch.empty((total, 4), dtype=torch.float32, device="cuda")   # (allocated once, outside the timing)
        L, sh = rt.lib(), ctypes.c_void_p(stream.cuda_stream)

        def allhits_by_t(sort):
            st = L.rtbvh_allhits_async(ctx._h, ctypes.c_void_p(rays.data_ptr()), n, ctypes.c_void_p(offsets.data_ptr()),
                                       ctypes.c_void_p(ahits.data_ptr()), total, rt.ALLHITS_BY_T | sort, sh)
            assert st == 0, st

        def allhits_route(tag):
            for label, sort in (("", 0), ("_sort", rt.ALLHITS_SORT)):
                res[f"allhits_by_t{label}_{tag}"] = timed(lambda: allhits_by_t(sort))

        allhits_route("before")
        # the first-k queries
        prev = None
        for k in KS:
            out = torch.empty((n, k, 4), dtype=torch.float32, device="cuda")
            case = {}
            first = None
            for label, mode in (("", 0), ("_sort", rt.KHITS_SORT)):
                case["khits" + label] = timed(lambda: ctx.khits(rays, k, mode=mode, out=out, stream=stream))
                if first is None:
                    first = out.clone()
                else:   # the same lists, bit for bit
                    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), k
            assert torch.equal(first[:, 0, 0] != -1, closest_hit), k      # slot 0: a hit iff the closest-hit query hits
            if prev is not None:   # the smaller k's list is this one's head
                assert torch.equal(first[:, :prev.shape[1]].view(torch.int32), prev.view(torch.int32)), k
            prev = first
            ctx.khits(rays, k, mode=rt.KHITS_COUNT, out=out, stream=stream)
            c = ctx.khits_counts()
            assert c["rays"] == n and c["found"] == int((first[:, :, 0] != -1).sum().item()), c
            case["found_per_ray"] = round(c["found"] / n, 3)
            case["internal_steps_per_ray"] = round(c["internal_steps"] / n, 3)
            case["leaf_steps_per_ray"] = round(c["leaf_steps"] / n, 3)
            res[f"k{k}"] = case
            del out
        del prev, first
        allhits_route("after")
        for label in ("", "_sort"):
            b, a = (res[f"allhits_by_t{label}_{tag}"]["ms_median"] for tag in ("before", "after"))
            route = (a + b) / 2
            res["allhits_by_t" + label] = {"ms_median_mean_of_before_and_after": round(route, 4),
                                           "after_over_before": round(a / b, 4),
                                           "time_over_closest": round(route / res["query_closest" + label]["ms_median"], 3)}
            for k in KS:
                t = res[f"k{k}"]["khits" + label]
                t["time_over_allhits_by_t"] = round(t["ms_median"] / route, 4)
                t["allhits_by_t_over_this"] = round(route / t["ms_median"], 3)
                t["time_over_closest"] = round(t["ms_median"] / res["query_closest" + label]["ms_median"], 3)
        ctx.synchronize()
    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50), {W}x{H}, the live reflection "
                    "rays of the reference-order frame as query rays (scripts/query_bench.py's), pixel order, "
                    "t_max = +inf, node records; k = 1, 2, 8, 16",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "rays": n,
        "reps": args.reps,
        "not_measured": "node-box trees (FLAG_AUTO_WALK builds), finite t_max, k other than 1, 2, 8 and 16, the host's "
                        "cut of each all-hits list to its first k",
        "results": res,
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
