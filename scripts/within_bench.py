"""Radius query throughput on the C5 scene.

    python scripts/within_bench.py [--out profiles/within_bench.json] [--reps 5] [--radii 4,10]
    python scripts/within_bench.py --probe --radii 4,8,12,16      # pairs per point of each radius only, no file

Builds C5 and the near-surface device points of scripts/nearest_bench.py (the primary rays' hit points displaced by
`--displace` of the root box's diagonal) and, for each radius r of `--radii` (in displacements: max_dist2 =
(r displacements)^2; 4 is nearest_bench's bounded case, the second was chosen after a first run so that the mean list
is about ten times longer), times with HIP events, the median of `reps` repetitions after one warm-up:

  sizes   RTBVH_WITHIN_SIZES alone;
  fill    RTBVH_WITHIN_FILL alone, on the offsets of the sizes call;
  both    mode 0 with capacity = the exact total;

each also with WITHIN_SORT (the offsets must be the same bytes and the pairs have the same order-sensitive digest), and
Context.nearest on the same points and bound in the same process: the only baseline there is -- existing code, a walk
whose bound shrinks.  One WITHIN_COUNT call per form gives the steps per point.  Writes Mpoints/s, Mpairs/s, pairs
per point, the steps and the ratios to nearest as JSON.  No gate.  Not part of bench.py.  RTBVH_LIB=<an A/B build of the library> measures that build.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "within_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--displace", type=float, default=1e-3)
    ap.add_argument("--radii", default="4,10", help="in displacements, comma-separated")
    ap.add_argument("--probe", action="store_true", help="pairs per point of each radius only")
    args = ap.parse_args()
    radii = [float(r) for r in args.radii.split(",")]

    import torch

    import raytracebvh_amd as rt

    L = rt.lib()
    W, H = args.width, args.height
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    wvp, wv = rt.camera_reference(W, H)
    m = torch.from_numpy(np.ascontiguousarray(wvp, np.float32).reshape(4, 4)).cuda()
    pos = torch.from_numpy(np.ascontiguousarray(scene.vertices[:, :3])).cuda()
    clip = pos @ m[:3, :3] + m[3, :3]
    lo, hi = clip.min(0).values, clip.max(0).values
    del pos, clip
    diag = float(torch.linalg.norm(hi - lo))
    disp = args.displace * diag
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(wvp, wv)
        ctx.build()
        # nearest_bench's near-surface points, from the same generator
        ys, xs = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        o = torch.stack([(xs.reshape(-1) - W // 2) / 4.0, (ys.reshape(-1) - H // 2) / 4.0,
                         torch.zeros(W * H, device="cuda")], 1).float()
        d = torch.zeros_like(o)
        d[:, 2] = 1
        hits = ctx.query(rt.make_rays(o, d))
        hit = hits[:, 0] != -1
        gen = torch.Generator(device="cuda").manual_seed(5)
        surf = o[hit] + hits[hit, 0:1] * d[hit]
        del ys, xs, o, d, hits
        n = int(surf.shape[0])
        u = torch.randn((n, 3), device="cuda", generator=gen)
        near = surf + disp * u / torch.linalg.norm(u, dim=1, keepdim=True)
        del surf, u
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        sh = ctypes.c_void_p(stream.cuda_stream)
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        near_out = torch.empty((n, 8), dtype=torch.float32, device="cuda")

        def ptr(t):
            return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

        def within(pts, pairs, mode):
            st = L.rtbvh_within_async(ctx._h, ptr(pts), n, ptr(offsets), ptr(pairs),
                                      0 if pairs is None else pairs.shape[0], mode, sh)
            assert st == 0, st

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

        def digest(pairs, chunk=1 << 26):
            """An order-sensitive 64-bit sum of the pairs' bytes (a list may be tens of GB: no second copy)."""
            w = pairs.view(torch.int64).reshape(-1)
            acc = 0
            for b in range(0, w.numel(), chunk):
                x = w[b:b + chunk]
                k = torch.arange(b, b + x.numel(), device=x.device, dtype=torch.int64) * 2 + 1
                acc = (acc + int((x * k).sum().item())) & 0xFFFFFFFFFFFFFFFF
            return acc

        res = {}
        for r in radii:
            pts = rt.make_points(near, (r * disp) ** 2)
            within(pts, None, rt.WITHIN_SIZES | rt.WITHIN_COUNT)
            c_sizes = ctx.within_counts()
            total = int(offsets[n].item())
            case = {"radius_in_displacements": r, "max_dist2": (r * disp) ** 2, "pairs": total,
                    "pairs_per_point": round(total / n, 3),
                    "sizes_internal_steps_per_point": round(c_sizes["internal_steps"] / n, 3),
                    "sizes_leaf_steps_per_point": round(c_sizes["leaf_steps"] / n, 3)}
            assert c_sizes["points"] == n and c_sizes["pairs"] == total, c_sizes
            res[f"r{r:g}"] = case
            if args.probe:
                continue
            pairs = torch.empty((total, 2), dtype=torch.float32, device="cuda")
            first = None
            for label, sort in (("", 0), ("_sort", rt.WITHIN_SORT)):
                runs = {"sizes": lambda: within(pts, None, rt.WITHIN_SIZES | sort),
                        "fill": lambda: within(pts, pairs, rt.WITHIN_FILL | sort),     # (offsets: the sizes call's)
                        "both": lambda: within(pts, pairs, sort)}
                for name, f in runs.items():
                    ms = timed(f)
                    med = float(np.median(ms))
                    case[name + label] = {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4),
                                          "ms_max": round(max(ms), 4), "ms_median": round(med, 4),
                                          "mpoints_per_s": round(n / med / 1e3, 1),
                                          "mpairs_per_s": round(total / med / 1e3, 1)}
                got = (offsets.clone(), digest(pairs))
                if first is None:
                    first = got
                else:   # the same output, byte for byte
                    assert torch.equal(got[0], first[0]) and got[1] == first[1], r
                pairs.zero_()
                torch.cuda.synchronize()
            del first, got
            within(pts, pairs, rt.WITHIN_COUNT)
            c_both = ctx.within_counts()
            assert c_both["pairs"] == total, c_both
            case["both_internal_steps_per_point"] = round(c_both["internal_steps"] / n, 3)
            case["both_leaf_steps_per_point"] = round(c_both["leaf_steps"] / n, 3)
            # the baseline: the closest-point query on the same points and bound
            for label, mode in (("", 0), ("_sort", rt.NEAREST_SORT)):
                ms = timed(lambda: ctx.nearest(pts, mode=mode, out=near_out, stream=stream))
                med = float(np.median(ms))
                case["nearest" + label] = {"ms": [round(v, 4) for v in ms], "ms_median": round(med, 4),
                                           "mpoints_per_s": round(n / med / 1e3, 1)}
            ctx.nearest(pts, mode=rt.NEAREST_COUNT, out=near_out, stream=stream)
            cn = ctx.nearest_counts()
            case["nearest"]["internal_steps_per_point"] = round(cn["internal_steps"] / n, 3)
            case["nearest"]["leaf_steps_per_point"] = round(cn["leaf_steps"] / n, 3)
            case["nearest"]["found_fraction"] = round(cn["found"] / n, 6)
            for label in ("", "_sort"):
                for name in ("sizes", "fill", "both"):
                    case[name + label]["time_over_nearest"] = round(
                        case[name + label]["ms_median"] / case["nearest" + label]["ms_median"], 3)
            del pairs
        ctx.synchronize()
    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under the {W}x{H} reference "
                    "camera, node records; points: the primary rays' hit points displaced by "
                    f"{args.displace} of the root box's diagonal (nearest_bench's near_surface); max_dist2 = "
                    "(r displacements)^2 for each r of radii_in_displacements",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "points": n,
        "reps": args.reps,
        "root_box_diagonal": round(diag, 4),
        "displacement": round(disp, 6),
        "radii_in_displacements": radii,
        "cases": res,
    }
    if args.out and not args.probe:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
