"""All-hits ray query throughput on the C5 scene, beside the closest-hit and any-hit queries of the same rays.

    python scripts/allhits_bench.py [--out profiles/allhits_bench.json] [--reps 5]

Builds C5 (10M synthetic triangles, 3840 x 2160) and takes the rays scripts/query_bench.py takes: the live reflection
rays of the reference-order frame's primary pass, in pixel order, t_max = +inf.  If their lists would not fit
`--max-gb` of hits, every s-th ray is taken (recorded as ray_stride).  Times with HIP events around the call, the
median of `reps` repetitions after one warm-up:

  sizes   RTBVH_ALLHITS_SIZES alone;
  fill    RTBVH_ALLHITS_FILL alone, on the offsets of the sizes call;
  both    mode 0 with capacity = the exact total;
  by_t    mode 0 | RTBVH_ALLHITS_BY_T: its added cost over `both` is the ordering pass;

each also with ALLHITS_SORT (the offsets must be the same bytes and the hits have the same order-sensitive digest),
and closest-hit and any-hit rtbvh_query_async on the same rays in the same process as the yardstick.  One COUNT call
per form gives the node and leaf steps per ray.  Writes hits per ray, the list-length histogram, milliseconds, the
ratios to closest-hit and the steps as JSON.  No gate.  Not part of bench.py.  RTBVH_LIB=<an A/B build of the library>
measures that build.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "allhits_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--max-gb", type=float, default=24.0, help="the most hits to hold, in GB")
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    L = rt.lib()
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
        all_rays = torch.from_numpy(host.view(np.float32).reshape(-1, 8)).cuda()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        sh = ctypes.c_void_p(stream.cuda_stream)

        def ptr(t):
            return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

        state = {}

        def allhits(hits, mode):
            st = L.rtbvh_allhits_async(ctx._h, ptr(state["rays"]), state["n"], ptr(state["offsets"]), ptr(hits),
                                       0 if hits is None else hits.shape[0], mode, sh)
            assert st == 0, st

        def use(rays):
            state.update(rays=rays, n=int(rays.shape[0]),
                         offsets=torch.empty(int(rays.shape[0]) + 1, dtype=torch.int64, device="cuda"))

        use(all_rays)
        allhits(None, rt.ALLHITS_SIZES)
        stream.synchronize()
        total_all = int(state["offsets"][-1].item())
        stride = max(1, -(-total_all * 16 // int(args.max_gb * 1e9)))
        if stride > 1:
            use(all_rays[::stride].contiguous())
        rays, n, offsets = state["rays"], state["n"], state["offsets"]

        def timed(f):
            ms = []
            for k in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                if k:   # (the first is the warm-up)
                    ms.append(e0.elapsed_time(e1))
            return ms

        def entry(ms, items=None):
            med = float(np.median(ms))
            e = {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                 "ms_median": round(med, 4), "mrays_per_s": round(n / med / 1e3, 1)}
            if items is not None:
                e["mhits_per_s"] = round(items / med / 1e3, 1)
            return e

        def digest(hits, chunk=1 << 26):
            """An order-sensitive 64-bit sum of the hits' bytes."""
            w = hits.view(torch.int64).reshape(-1)
            acc = 0
            for b in range(0, w.numel(), chunk):
                x = w[b:b + chunk]
                k = torch.arange(b, b + x.numel(), device=x.device, dtype=torch.int64) * 2 + 1
                acc = (acc + int((x * k).sum().item())) & 0xFFFFFFFFFFFFFFFF
            return acc

        allhits(None, rt.ALLHITS_SIZES | rt.ALLHITS_COUNT)
        c_sizes = ctx.allhits_counts()
        total = int(offsets[n].item())
        assert c_sizes["rays"] == n and c_sizes["hits"] == total, c_sizes
        cnt = (offsets[1:] - offsets[:-1])
        edges = [0, 1, 2, 4, 8, 16, 17, 32, 64, 256, 2048, 2049]
        hist = {f">={e}": int((cnt >= e).sum().item()) for e in edges}
        res = {"hits": total, "hits_per_ray": round(total / n, 3), "longest_list": int(cnt.max().item()),
               "rays_with_at_least": hist,
               "sizes_internal_steps_per_ray": round(c_sizes["internal_steps"] / n, 3),
               "sizes_leaf_steps_per_ray": round(c_sizes["leaf_steps"] / n, 3)}
        hits = torch.empty((total, 4), dtype=torch.float32, device="cuda")
        first = None
        for label, sort in (("", 0), ("_sort", rt.ALLHITS_SORT)):
            runs = {"sizes": lambda: allhits(None, rt.ALLHITS_SIZES | sort),
                    "fill": lambda: allhits(hits, rt.ALLHITS_FILL | sort),      # (offsets: the sizes call's)
                    "both": lambda: allhits(hits, sort)}
            for name, f in runs.items():
                res[name + label] = entry(timed(f), total)
            got = (offsets.clone(), digest(hits))
            if first is None:
                first = got
            else:   # the same output, byte for byte
                assert torch.equal(got[0], first[0]) and got[1] == first[1]
            res["by_t" + label] = entry(timed(lambda: allhits(hits, rt.ALLHITS_BY_T | sort)), total)
            res["by_t" + label]["added_ms_over_both"] = round(
                res["by_t" + label]["ms_median"] - res["both" + label]["ms_median"], 4)
            keys = hits.view(torch.int32)
            key = (keys[:, 0].to(torch.int64) << 32) | (keys[:, 3].to(torch.int64) & 0xFFFFFFFF)
            inner = torch.ones(total, dtype=torch.bool, device="cuda")
            inner[offsets[1:n].clamp(max=max(total - 1, 0))] = False   # (a list's first hit follows another list)
            assert bool(((key[1:] > key[:-1]) | ~inner[1:]).all()), "BY_T: a list out of order"
            del keys, key, inner
            hits.zero_()
            torch.cuda.synchronize()
        allhits(hits, rt.ALLHITS_COUNT)
        c_both = ctx.allhits_counts()
        assert c_both["hits"] == total, c_both
        res["both_internal_steps_per_ray"] = round(c_both["internal_steps"] / n, 3)
        res["both_leaf_steps_per_ray"] = round(c_both["leaf_steps"] / n, 3)
        del hits
        # the yardstick: closest-hit and any-hit queries on the same rays
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        for name, mode in (("closest", rt.QUERY_CLOSEST), ("any", rt.QUERY_ANY), ("closest_sort", rt.QUERY_SORT)):
            res["query_" + name] = entry(timed(lambda: ctx.query(rays, mode, out=out, stream=stream)))
            res["query_" + name]["hits"] = int((out[:, 0] != -1).sum().item())
            ctx.query(rays, mode | rt.QUERY_COUNT, out=out, stream=stream)
            qc = ctx.query_counts()
            res["query_" + name]["internal_steps_per_ray"] = round(qc["internal_visits"] / n, 3)
            res["query_" + name]["leaf_steps_per_ray"] = round(qc["leaf_visits"] / n, 3)
        assert res["query_closest"]["hits"] == int((cnt > 0).sum().item())   # empty iff the closest-hit query misses
        for label in ("", "_sort"):
            for name in ("sizes", "fill", "both", "by_t"):
                res[name + label]["time_over_closest"] = round(
                    res[name + label]["ms_median"] / res["query_closest" + label]["ms_median"], 3)
        ctx.synchronize()
    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50), {W}x{H}, the live reflection "
                    "rays of the reference-order frame as query rays (scripts/query_bench.py's), pixel order, "
                    "t_max = +inf",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "rays": n,
        "ray_stride": stride,
        "hits_of_all_rays": total_all,
        "reps": args.reps,
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
