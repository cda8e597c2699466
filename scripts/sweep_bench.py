"""Sphere-sweep query throughput on the C5 scene, beside the route a caller had before: sphere tracing by nearest.

    python scripts/sweep_bench.py [--out profiles/sweep_bench.json] [--reps 5] [--quick]

Builds C5 (10M synthetic triangles, 3840 x 2160) and takes the rays scripts/query_bench.py takes -- the live
reflection rays of the reference-order frame's primary pass, in pixel order -- as sweep paths.  A radius is a distance
only where the BVH space is object space, so the rays are mapped back through the camera's affine map (origins as
points, directions as vectors, not renormalised: t is kept) and the tree is rebuilt under an identity camera.  Every
sweep gets t_max = the parameter at which it has moved two root diagonals.

Times Context.sweep on device tensors with HIP events around the call, the median of `reps` repetitions after one
warm-up, for r = 0, 1e-4, 1e-3 and 1e-2 of the root diagonal, each in the given order and with SWEEP_SORT (the same
bytes: asserted), SWEEP_ANY at r = 1e-3 (the same hit / miss: asserted), and reads the steps per sweep of one
SWEEP_COUNT query per case.  In the same process, for each radius above 0, the earlier route: sphere tracing through
Context.nearest on device tensors -- t += (dist - r) / |d| from t = 0 for the sweeps still undecided, compacted
every iteration, until dist - r <= 1e-4 r (touching), t > t_max (a miss) or 64 iterations -- timed by the wall clock
around the loop (it synchronises once an iteration, to know how many are left), with its iteration count, the share
left undecided and how its hit / miss compares with the sweep's.

Writes ms, Msweeps/s and the steps as JSON.  No gate.  Not part of bench.py.  RTBVH_LIB=<an A/B build of the library>
measures that build; --quick times r = 1e-3 alone (default, SORT, ANY) and skips the sphere tracing: the A/B of the
kernel's launch bound (profiles/sweep_ab.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FRACTIONS = (0.0, 1e-4, 1e-3, 1e-2)
TRACE_ITERATIONS, TRACE_TOLERANCE = 64, 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sweep_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    assert torch.cuda.is_available(), "sweep_bench needs a GPU"
    W, H = args.width, args.height
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    eye = np.eye(4, dtype=np.float32)
    with rt.Context(device=0, flags=rt.FLAG_REFRACT_RECORDS) as ctx:
        ctx.set_scene(scene)
        wvp, wv = rt.camera_reference(W, H)
        ctx.set_camera(wvp, wv)
        ctx.build()
        ctx.trace(W, H, 0)   # the reflect records of the primary pass: the rays the bounce pass walks (query_bench)
        refl, _ = ctx.read_rays()
        rec = refl.reshape(-1, 14)
        live = rec[:, 0] > 0
        # BVH space = positions times WVP, .xyz: p' = p A + b.  Back to object space.
        m = np.asarray(wvp, np.float64).reshape(4, 4)
        ainv = np.linalg.inv(m[:3, :3])
        o = ((rec[live, 1:4].astype(np.float64) - m[3, :3]) @ ainv).astype(np.float32)
        d = (rec[live, 4:7].astype(np.float64) @ ainv).astype(np.float32)
        del refl, rec
        ctx.set_camera(eye, eye)
        ctx.build()
        pos = scene.vertices[:, :3]
        diag = float(np.sqrt(((pos.max(0) - pos.min(0)).astype(np.float64) ** 2).sum()))
        n = len(o)
        t_max = (2 * diag / np.sqrt((d.astype(np.float64) ** 2).sum(1))).astype(np.float32)
        od, dd, tm = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(t_max).cuda()
        dlen = torch.linalg.vector_norm(dd, dim=1)
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
                    "ms_median": round(med, 4), "msweeps_per_s": round(n / med / 1e3, 1)}

        def steps(sweeps, mode):
            ctx.sweep(sweeps, mode=mode | rt.SWEEP_COUNT, stream=stream)
            c = ctx.sweep_counts()
            assert c["sweeps"] == n, c
            return {"hits_per_sweep": round(c["hits"] / n, 4), "internal_steps_per_sweep": round(c["internal_steps"] / n, 3),
                    "leaf_steps_per_sweep": round(c["leaf_steps"] / n, 3)}

        def sphere_trace(r):
            """The earlier route.  Returns the case's record and the hit mask."""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                t = torch.zeros(n, dtype=torch.float32, device="cuda")
                hit = torch.zeros(n, dtype=torch.bool, device="cuda")
                idx = torch.arange(n, device="cuda")
                iters = torch.zeros(n, dtype=torch.int32, device="cuda")
                calls, points = 0, 0
                for _ in range(TRACE_ITERATIONS):
                    if idx.numel() == 0:
                        break
                    p = torch.empty((idx.numel(), 4), dtype=torch.float32, device="cuda")
                    p[:, :3] = od[idx] + t[idx, None] * dd[idx]
                    p[:, 3] = float("inf")
                    res = ctx.nearest(p, stream=stream)
                    calls, points = calls + 1, points + idx.numel()
                    gap = torch.sqrt(res[:, 3]) - r
                    iters[idx] += 1
                    touch = gap <= TRACE_TOLERANCE * r
                    hit[idx[touch]] = True
                    t[idx] = t[idx] + gap / dlen[idx]
                    idx = idx[~touch & (t[idx] <= tm[idx])]
                left = idx.numel()
            stream.synchronize()
            sec = time.perf_counter() - t0
            return {"ms_wall": round(sec * 1e3, 2), "msweeps_per_s": round(n / sec / 1e6, 2), "nearest_calls": calls,
                    "points_queried": points, "mean_iterations_per_sweep": round(float(iters.float().mean().item()), 3),
                    "max_iterations": int(iters.max().item()), "undecided_after_64": left,
                    "undecided_share": round(left / n, 6), "hits_per_sweep": round(float(hit.float().mean().item()), 4)}, hit

        res = {}
        for frac in ((1e-3,) if args.quick else FRACTIONS):
            r = frac * diag
            sweeps = rt.make_sweeps(od, dd, r, tm)
            case = {"radius": r}
            first = None
            for label, mode in (("", 0), ("_sort", rt.SWEEP_SORT)):
                case["sweep" + label] = timed(lambda: ctx.sweep(sweeps, mode=mode, stream=stream))
                out = ctx.sweep(sweeps, mode=mode, stream=stream)
                stream.synchronize()
                if first is None:
                    first = out
                else:   # the same records, bit for bit
                    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), frac
            case.update(steps(sweeps, 0))
            if frac == 1e-3:
                case["sweep_any"] = timed(lambda: ctx.sweep(sweeps, mode=rt.SWEEP_ANY, stream=stream))
                out = ctx.sweep(sweeps, mode=rt.SWEEP_ANY, stream=stream)
                stream.synchronize()
                assert torch.equal(out[:, 0] != -1, first[:, 0] != -1)
                case["sweep_any"].update(steps(sweeps, rt.SWEEP_ANY))
            feat = first[:, 5].contiguous().view(torch.int32)
            case["features"] = {str(k): int((feat == k).sum().item()) for k in range(9)}
            if r > 0 and not args.quick:
                case["sphere_tracing_by_nearest"], hit = sphere_trace(r)
                shit = first[:, 0] != -1
                case["sphere_tracing_by_nearest"]["hit_where_sweep_misses"] = int((hit & ~shit).sum().item())
                case["sphere_tracing_by_nearest"]["miss_or_undecided_where_sweep_hits"] = int((~hit & shit).sum().item())
                case["sphere_tracing_by_nearest"]["time_over_sweep"] = round(
                    case["sphere_tracing_by_nearest"]["ms_wall"] / case["sweep"]["ms_median"], 2)
            res[f"r_{frac:g}_diag"] = case
        ctx.synchronize()
    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under an identity camera, the "
                    f"live reflection rays of the {W}x{H} reference-order frame (scripts/query_bench.py's) mapped to "
                    "object space as sweep paths, pixel order, t_max = two root diagonals of travel, node records",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "sweeps": n,
        "root_diagonal": diag,
        "reps": args.reps,
        "not_measured": "node-box trees (FLAG_AUTO_WALK builds), t_max = +inf, radii above 1e-2 of the diagonal, "
                        "non-uniform radii in one batch, sphere tracing at r = 0 (its stopping rule needs r > 0), "
                        "a sphere tracing that keeps its points on the device without the per-iteration count",
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
