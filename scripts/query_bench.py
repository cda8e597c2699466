"""Ray-query throughput on the C5 scene against the trace's own walk of the same rays.

    python scripts/query_bench.py [--out profiles/query_bench.json] [--reps 5]

1. Traces one C5 frame (10M synthetic triangles, 3840 x 2160, one bounce) in the reference order with
   FLAG_REFRACT_RECORDS | FLAG_REFILL_BOUNCE | FLAG_TIMING: ms_stage[7] is the refill walk (k_bounce_trav) of
   the frame's live reflection rays.
2. Reads the reflect records of that frame's primary pass (the same frame with no bounce: the rays the
   bounce pass walked) and packs the live ones (intensity > 0) as query rays, in pixel order.
3. Times Context.query on those rays with HIP events: closest-hit, any-hit, and closest-hit with QUERY_SORT,
   then the same three with QUERY_CERTIFIED, `reps` repetitions after one warm-up; and reads the walk counts of
   `reps` certified counting queries, and times a batch the certified walk cannot take (the same rays with
   directions of length 2: every ray uncovered) in both modes.
4. Traces the frame once more as a certified one (FLAG_CERTIFIED | FLAG_REFILL_BOUNCE | FLAG_TIMING) in a second
   context: its ms_stage[7] is the certified 4-wide bounce walk of the same rays, the certified query's yardstick.

The query walks the very rays ms_stage[7] walked, in the same order, so that stage is the yardstick: the
query adds 48 B of ray and hit traffic per ray and drops the hit-record hand-off.  Writes Mrays/s per mode,
the stage, their ratio and the run-to-run spread (min to max) as JSON.  Not part of bench.py.
RTBVH_LIB=<an A/B build of the library> measures that build (raytracebvh_amd/csrc/Makefile); --plain-only times the
plain modes alone (a library from before QUERY_CERTIFIED) and writes no file unless --out is given.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    if args.out is None and not args.plain_only:
        args.out = os.path.join(REPO, "profiles", "query_bench.json")

    import torch

    import raytracebvh_amd as rt

    W, H = args.width, args.height
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    flags = rt.FLAG_REFRACT_RECORDS | rt.FLAG_REFILL_BOUNCE | rt.FLAG_TIMING
    with rt.Context(device=0, flags=flags) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(*rt.camera_reference(W, H))
        ctx.build()
        ctx.trace(W, H, 1)   # warm-up
        stage7 = []
        for _ in range(args.reps):   # the frame, one at a time: each one's own ms_stage[7]
            ctx.reset_stats()
            ctx.trace(W, H, 1)
            st = ctx.stats()
            stage7.append(st["ms_stage"][7])
        bounce_rays = st["bounce_rays"]
        # the records of a frame hold the rays after its last pass: the rays the bounce pass walked are the
        # reflect records of the same frame's primary pass alone
        ctx.trace(W, H, 0)
        refl, _ = ctx.read_rays()
        rec = refl.reshape(-1, 14)
        live = rec[:, 0] > 0
        n = int(live.sum())
        assert n == bounce_rays, (n, bounce_rays)   # the rays the stage walked
        host = rt.make_rays(rec[live, 1:4], rec[live, 4:7])
        del refl, rec
        rays = torch.from_numpy(host.view(np.float32).reshape(n, 8)).cuda()
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        modes = {"closest": rt.QUERY_CLOSEST, "any": rt.QUERY_ANY, "closest_sort": rt.QUERY_SORT}
        if not args.plain_only:
            modes.update({"closest_certified": rt.QUERY_CERTIFIED, "any_certified": rt.QUERY_CERTIFIED | rt.QUERY_ANY,
                          "closest_certified_sort": rt.QUERY_CERTIFIED | rt.QUERY_SORT})
        plain = None
        res = {}
        for name, mode in modes.items():
            ms = []
            for k in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.query(rays, mode, out=out, stream=stream)
                e1.record(stream)
                e1.synchronize()
                if k:   # (the first is the warm-up)
                    ms.append(e0.elapsed_time(e1))
            hits = int((out[:, 0] != -1).sum().item())
            if name == "closest":
                plain = out.clone()
            elif "closest" in name:   # the same hits, bit for bit
                assert torch.equal(out.view(torch.int32), plain.view(torch.int32)), name
            res[name] = {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                         "ms_median": round(float(np.median(ms)), 4),
                         "mrays_per_s": round(n / float(np.median(ms)) / 1e3, 1), "hits": hits}
        ctx.query(rays, rt.QUERY_COUNT, out=out, stream=stream)
        counts = ctx.query_counts()
        walk = []
        unc = {}
        if not args.plain_only:
            # the same rays with doubled directions (t halves, the hits stay): |d| = 2 is past the margin's bound, so
            # the certified query lists every ray at its claim and the plain kernel walks them all
            long_rays = rays.clone()
            long_rays[:, 4:7] *= 2
            for name, mode in (("closest", rt.QUERY_CLOSEST), ("closest_certified", rt.QUERY_CERTIFIED)):
                ms = []
                for k in range(args.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    ctx.query(long_rays, mode, out=out, stream=stream)
                    e1.record(stream)
                    e1.synchronize()
                    if k:
                        ms.append(e0.elapsed_time(e1))
                unc[name] = {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                             "ms_median": round(float(np.median(ms)), 4), "hits": int((out[:, 0] != -1).sum().item())}
            ctx.query(long_rays, rt.QUERY_CERTIFIED | rt.QUERY_COUNT, out=out, stream=stream)
            unc["walk_counts"] = ctx.query_walk_counts()
            del long_rays
        if not args.plain_only:
            for _ in range(args.reps):
                ctx.query(rays, rt.QUERY_CERTIFIED | rt.QUERY_COUNT, out=out, stream=stream)
                walk.append(ctx.query_walk_counts())
            cert_counts = ctx.query_counts()
        ctx.synchronize()
    cert7 = []
    if not args.plain_only:
        del rays, out
        cflags = rt.FLAG_CERTIFIED | rt.FLAG_REFILL_BOUNCE | rt.FLAG_TIMING
        with rt.Context(device=0, flags=cflags) as ctx:
            ctx.set_scene(scene)
            ctx.set_camera(*rt.camera_reference(W, H))
            ctx.build()
            ctx.trace(W, H, 1)   # warm-up
            for _ in range(args.reps):
                ctx.reset_stats()
                ctx.trace(W, H, 1)
                st = ctx.stats()
                cert7.append(st["ms_stage"][7])
            assert st["bounce_rays"] == n, (st["bounce_rays"], n)
    s7 = float(np.median(stage7))
    c = res["closest"]
    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50), {W}x{H}, the live "
                    "reflection rays of the reference-order frame as query rays, pixel order",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "rays": n,
        "reps": args.reps,
        "modes": res,
        "closest_counts": counts,
        "ms_stage7": {"ms": [round(v, 4) for v in stage7], "ms_min": round(min(stage7), 4),
                      "ms_max": round(max(stage7), 4), "ms_median": round(s7, 4),
                      "mrays_per_s": round(n / s7 / 1e3, 1)},
        "closest_over_stage7": round(c["ms_median"] / s7, 4),
        "closest_spread_ms": round(c["ms_max"] - c["ms_min"], 4),
        "closest_minus_stage7_ms": round(c["ms_median"] - s7, 4),
    }
    if not args.plain_only:
        cc, c7 = res["closest_certified"], float(np.median(cert7))
        result.update({
            "certified_counts": cert_counts,
            # how the rays of a certified counting query were answered, per field over the repetitions
            "certified_walk_counts": {k: {"min": min(w[k] for w in walk), "max": max(w[k] for w in walk)}
                                      for k in walk[0]},
            "ms_stage7_certified": {"ms": [round(v, 4) for v in cert7], "ms_min": round(min(cert7), 4),
                                    "ms_max": round(max(cert7), 4), "ms_median": round(c7, 4),
                                    "mrays_per_s": round(n / c7 / 1e3, 1)},
            "closest_over_closest_certified": round(c["ms_median"] / cc["ms_median"], 4),
            "any_over_any_certified": round(res["any"]["ms_median"] / res["any_certified"]["ms_median"], 4),
            "closest_certified_spread_ms": round(cc["ms_max"] - cc["ms_min"], 4),
            "closest_certified_over_stage7_certified": round(cc["ms_median"] / c7, 4),
            # every ray uncovered (directions of length 2): the certified query against the plain one
            "uncovered_batch": unc,
        })
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
