"""Box-overlap query throughput on the C5 scene.

    python scripts/overlap_bench.py [--out profiles/overlap_bench.json] [--reps 5] [--extents 4,10]
    python scripts/overlap_bench.py --probe --extents 2,4,8      # ids per box of each half-extent only, no file

Builds C5 and the near-surface device points of scripts/nearest_bench.py (the primary rays' hit points displaced by
`--displace` of the root box's diagonal) as box centres and, for each half-extent h of `--extents` (in displacements,
the same on the three axes: within_bench's two radii), with and without RTBVH_OVERLAP_TRIANGLE, times with HIP events,
the median of `reps` repetitions after one warm-up:

  sizes   RTBVH_OVERLAP_SIZES alone;
  fill    RTBVH_OVERLAP_FILL alone, on the offsets of the sizes call;
  both    mode 0 with capacity = the exact total;

each also with OVERLAP_SORT (the offsets must be the same bytes and the ids have the same order-sensitive digest).  One
OVERLAP_COUNT call per form gives the steps per box.  For orientation, in the same process: Context.within's SIZES
pass on the same points with the circumscribed radius (max_dist2 = 3 x half-extent^2), what a caller had before.
Writes ms, Mboxes/s, Mids/s, ids per box and steps per box as JSON.  No gate.  Not part of bench.py.
RTBVH_LIB=<an A/B build of the library> measures that build.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "overlap_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--displace", type=float, default=1e-3)
    ap.add_argument("--extents", default="4,10", help="half-extents in displacements, comma-separated")
    ap.add_argument("--probe", action="store_true", help="ids per box of each half-extent only")
    args = ap.parse_args()
    extents = [float(r) for r in args.extents.split(",")]

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
        w_offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")

        def ptr(t):
            return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

        def overlap(boxes, ids, mode):
            st = L.rtbvh_overlap_async(ctx._h, ptr(boxes), n, ptr(offsets), ptr(ids),
                                       0 if ids is None else ids.shape[0], mode, sh)
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

        def digest(ids, chunk=1 << 26):
            """An order-sensitive 64-bit sum of the ids (a list may be many GB: no second copy)."""
            acc = 0
            for b in range(0, ids.numel(), chunk):
                x = ids[b:b + chunk].to(torch.int64)
                k = torch.arange(b, b + x.numel(), device=x.device, dtype=torch.int64) * 2 + 1
                acc = (acc + int((x * k).sum().item())) & 0xFFFFFFFFFFFFFFFF
            return acc

        def figures(ms, total):
            med = float(np.median(ms))
            return {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                    "ms_median": round(med, 4), "mboxes_per_s": round(n / med / 1e3, 1),
                    "mids_per_s": round(total / med / 1e3, 1)}

        res = {}
        for r in extents:
            h = r * disp
            boxes = rt.make_boxes(near - h, near + h)
            torch.cuda.synchronize()   # (made on torch's stream, read on `stream`)
            case ={"half_extent_in_displacements": r, "half_extent": h}
            res[f"h{r:g}"] = case
            for tname, tri in (("boxes", 0), ("triangles", rt.OVERLAP_TRIANGLE)):
                overlap(boxes, None, rt.OVERLAP_SIZES | rt.OVERLAP_COUNT | tri)
                c_sizes = ctx.overlap_counts()
                total = int(offsets[n].item())
                assert c_sizes["boxes"] == n and c_sizes["ids"] == total, c_sizes
                sub = {"ids": total, "ids_per_box": round(total / n, 3),
                       "sizes_internal_steps_per_box": round(c_sizes["internal_steps"] / n, 3),
                       "sizes_leaf_steps_per_box": round(c_sizes["leaf_steps"] / n, 3)}
                case[tname] = sub
                if args.probe:
                    continue
                ids = torch.empty(total, dtype=torch.int32, device="cuda")
                first = None
                for label, sort in (("", 0), ("_sort", rt.OVERLAP_SORT)):
                    runs = {"sizes": lambda: overlap(boxes, None, rt.OVERLAP_SIZES | sort | tri),
                            "fill": lambda: overlap(boxes, ids, rt.OVERLAP_FILL | sort | tri),   # (offsets: the sizes call's)
                            "both": lambda: overlap(boxes, ids, sort | tri)}
                    for name, f in runs.items():
                        sub[name + label] = figures(timed(f), total)
                    got = (offsets.clone(), digest(ids))
                    if first is None:
                        first = got
                    else:   # the same output, byte for byte
                        assert torch.equal(got[0], first[0]) and got[1] == first[1], (r, tname)
                    ids.zero_()
                    torch.cuda.synchronize()
                del first, got
                overlap(boxes, ids, rt.OVERLAP_COUNT | tri)
                c_both = ctx.overlap_counts()
                assert c_both["ids"] == total, (c_both, total)
                sub["both_internal_steps_per_box"] = round(c_both["internal_steps"] / n, 3)
                sub["both_leaf_steps_per_box"] = round(c_both["leaf_steps"] / n, 3)
                del ids
            if args.probe:
                continue
            # for orientation: the radius query's sizes pass with the circumscribed radius on the same points
            pts = rt.make_points(near, 3 * h * h)
            torch.cuda.synchronize()

            def within(mode):
                st = L.rtbvh_within_async(ctx._h, ptr(pts), n, ptr(w_offsets), None, 0, rt.WITHIN_SIZES | mode, sh)
                assert st == 0, st

            within(rt.WITHIN_COUNT)
            cw = ctx.within_counts()
            wtotal = int(w_offsets[n].item())
            case["within_circumscribed"] = {"max_dist2": 3 * h * h, "pairs": wtotal, "pairs_per_point": round(wtotal / n, 3),
                                            "sizes_internal_steps_per_point": round(cw["internal_steps"] / n, 3),
                                            "sizes_leaf_steps_per_point": round(cw["leaf_steps"] / n, 3)}
            for label, sort in (("", 0), ("_sort", rt.WITHIN_SORT)):
                ms = timed(lambda: within(sort))
                med = float(np.median(ms))
                case["within_circumscribed"]["sizes" + label] = {
                    "ms": [round(v, 4) for v in ms], "ms_median": round(med, 4), "mpoints_per_s": round(n / med / 1e3, 1),
                    "time_over_overlap_sizes": round(med / case["boxes"]["sizes" + label]["ms_median"], 3)}
            del pts, boxes
        ctx.synchronize()
    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under the {W}x{H} reference "
                    "camera, node records; box centres: the primary rays' hit points displaced by "
                    f"{args.displace} of the root box's diagonal (nearest_bench's near_surface); half-extent = "
                    "h displacements on every axis for each h of half_extents_in_displacements",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "boxes": n,
        "reps": args.reps,
        "root_box_diagonal": round(diag, 4),
        "displacement": round(disp, 6),
        "half_extents_in_displacements": extents,
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
