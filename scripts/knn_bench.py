"""k-nearest query throughput on the C5 scene.

    python scripts/knn_bench.py [--out profiles/knn_bench.json] [--reps 5] [--no-baselines]

Builds C5 (10M synthetic triangles under the 3840 x 2160 reference camera, node records: as bench.py builds it)
and times Context.knn on device tensors with HIP events, `reps` repetitions after one warm-up, for

  (a) near_surface: nearest_bench's points -- the hit points of the frame's 3840 x 2160 primary rays, each displaced
      by `--displace` (default 1e-3) of the root box's diagonal in a random direction (the same generator), no bound;
  (b) uniform: as many points uniform in the root box, no bound;

with k = 1, 8 and 32, each in the given order and with KNN_SORT, and reads the steps per point of one KNN_COUNT query
per case (the order does not change a point's walk).  The sorted and the unsorted lists must be the same bits, and
the k = 8 list must start with the k = 1 one.  Beside them, in the same process, what a caller had before:

  - Context.nearest on the same points, both orders (what k = 1 costs over the dedicated kernel);
  - Context.within's WITHIN_SIZES pass on the same points, both orders, at the radius -- of `--radii`, in
    displacements -- whose mean list is closest to 8 pairs a point (the first of the two walks a caller needed
    before selecting a top k on the host; the fill pass and the selection come on top).

Writes ms, Mpoints/s, the steps and the run-to-run spread as JSON.  There is nothing earlier that answers the
question: no gate.  Not part of bench.py.  RTBVH_LIB=<an A/B build of the library> measures that build.
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

KS = (1, 8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "knn_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--displace", type=float, default=1e-3)
    ap.add_argument("--radii", default="0.5,0.75,1,1.25,1.5,2,2.5,3",
                    help="candidate radii of the `within` baseline, in displacements")
    ap.add_argument("--no-baselines", action="store_true", help="the k-nearest cases only (an A/B of the kernel)")
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    L = rt.lib()
    W, H = args.width, args.height
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    wvp, wv = rt.camera_reference(W, H)
    # the root box: the vertices in the space of the build (positions times WVP, .xyz)
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
        # nearest_bench's points, from the same generator
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
        uniform = lo + torch.rand((n, 3), device="cuda", generator=gen) * (hi - lo)
        del surf, u
        inf = float("inf")
        sets = {"near_surface": near, "uniform": uniform}
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
                    "ms_median": round(med, 4), "mpoints_per_s": round(n / med / 1e3, 1)}

        res = {}
        for name, xyz in sets.items():
            pts = rt.make_points(xyz, inf)
            stream.wait_stream(torch.cuda.current_stream())   # (make_points ran on the current stream)
            head = None   # the k = 1 list
            for k in KS:
                out = torch.empty((n, k, 2), dtype=torch.float32, device="cuda")
                first = None
                case = {}
                for label, mode in (("", 0), ("_sort", rt.KNN_SORT)):
                    case["knn" + label] = timed(lambda: ctx.knn(pts, k, mode=mode, out=out, stream=stream))
                    if first is None:
                        first = out.clone()
                    else:   # the same lists, bit for bit
                        assert torch.equal(out.view(torch.int32), first.view(torch.int32)), (name, k)
                if head is None:
                    head = first[:, 0].clone()
                else:
                    assert torch.equal(first[:, 0].view(torch.int32), head.view(torch.int32)), (name, k)
                ctx.knn(pts, k, mode=rt.KNN_COUNT, out=out, stream=stream)
                c = ctx.knn_counts()
                assert c["points"] == n and c["found"] == n * k, c
                case["internal_steps_per_point"] = round(c["internal_steps"] / n, 3)
                case["leaf_steps_per_point"] = round(c["leaf_steps"] / n, 3)
                d2 = first[:, k - 1, 1]
                case["median_kth_distance_over_displacement"] = round(float(d2.sqrt().median()) / disp, 4)
                res[f"{name}_k{k}"] = case
                del out, first
            if args.no_baselines:
                continue
            # what a caller had before: the closest-point query (k = 1's dedicated kernel) ...
            base = {}
            near_out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            for label, mode in (("", 0), ("_sort", rt.NEAREST_SORT)):
                base["nearest" + label] = timed(lambda: ctx.nearest(pts, mode=mode, out=near_out, stream=stream))
            assert torch.equal(near_out[:, 6].view(torch.int32), head[:, 0].view(torch.int32)), name
            assert torch.equal(near_out[:, 3].view(torch.int32), head[:, 1].view(torch.int32)), name
            ctx.nearest(pts, mode=rt.NEAREST_COUNT, out=near_out, stream=stream)
            cn = ctx.nearest_counts()
            base["nearest"]["internal_steps_per_point"] = round(cn["internal_steps"] / n, 3)
            base["nearest"]["leaf_steps_per_point"] = round(cn["leaf_steps"] / n, 3)
            del near_out
            # ... and the radius query's sizes pass at the radius that lists about 8 pairs a point
            offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            sh = ctypes.c_void_p(stream.cuda_stream)

            def sizes(p, mode):
                st = L.rtbvh_within_async(ctx._h, ctypes.c_void_p(p.data_ptr()), n, ctypes.c_void_p(offsets.data_ptr()),
                                          None, 0, rt.WITHIN_SIZES | mode, sh)
                assert st == 0, st

            probe = {}
            for r in (float(x) for x in args.radii.split(",")):
                bp = rt.make_points(xyz, (r * disp) ** 2)
                stream.wait_stream(torch.cuda.current_stream())
                sizes(bp, rt.WITHIN_COUNT)
                cw = ctx.within_counts()
                probe[r] = (cw["pairs"] / n, cw)
            r = min(probe, key=lambda x: abs(probe[x][0] - 8))
            bp = rt.make_points(xyz, (r * disp) ** 2)
            stream.wait_stream(torch.cuda.current_stream())
            w = {"radius_in_displacements": r, "pairs_per_point": round(probe[r][0], 3),
                 "pairs_per_point_of_each_radius": {f"{x:g}": round(v[0], 3) for x, v in probe.items()},
                 "internal_steps_per_point": round(probe[r][1]["internal_steps"] / n, 3),
                 "leaf_steps_per_point": round(probe[r][1]["leaf_steps"] / n, 3)}
            for label, mode in (("", 0), ("_sort", rt.WITHIN_SORT)):
                w["sizes" + label] = timed(lambda: sizes(bp, mode))
            base["within_sizes"] = w
            for k in KS:
                for label in ("", "_sort"):
                    t = res[f"{name}_k{k}"]["knn" + label]
                    t["time_over_nearest"] = round(t["ms_median"] / base["nearest" + label]["ms_median"], 3)
            res[name + "_before"] = base
            del offsets
        ctx.synchronize()
    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under the {W}x{H} reference "
                    "camera, node records; points: the primary rays' hit points displaced by "
                    f"{args.displace} of the root box's diagonal (near_surface), as many uniform in the root box "
                    "(uniform), no bound; k = 1, 8, 32",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "points": n,
        "reps": args.reps,
        "root_box_diagonal": round(diag, 4),
        "displacement": round(disp, 6),
        "not_measured": "node-box trees (FLAG_AUTO_WALK builds), finite bounds, k other than 1, 8 and 32, the "
                        "radius query's fill pass and the host-side selection of the earlier route",
        "cases": res,
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
