"""Closest-point query throughput on the C5 scene.

    python scripts/nearest_bench.py [--out profiles/nearest_bench.json] [--reps 5]

Builds C5 (10M synthetic triangles under the 3840 x 2160 reference camera, node records: as bench.py builds it)
and times Context.nearest on device tensors with HIP events, `reps` repetitions after one warm-up, for

  (a) near_surface: the hit points of the frame's 3840 x 2160 primary rays (a closest-hit ray query), each displaced
      by `--displace` (default 1e-3) of the root box's diagonal in a random direction, no bound;
  (b) uniform: as many points uniform in the root box, no bound;
  (c) near_surface_bounded: the points of (a) with max_dist2 = (4 displacements)^2;

each in the given order and with NEAREST_SORT, and reads the steps per point of one NEAREST_COUNT query per case
(the order does not change a point's walk).  The sorted and the unsorted results must be the same bits.
Writes Mpoints/s, the steps and the run-to-run spread as JSON, beside the closest-hit ray-query rate of
profiles/query_bench.json for orientation (other rays, the same scene).  There is nothing to compare against:
no gate.  Not part of bench.py.  RTBVH_LIB=<an A/B build of the library> measures that build.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nearest_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--displace", type=float, default=1e-3)
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

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
        # the primary rays (pixel (x, y): origin ((x - W/2) / 4, (y - H/2) / 4, 0), direction +z) and their hits
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
        cases = {"near_surface": rt.make_points(near, inf), "uniform": rt.make_points(uniform, inf),
                 "near_surface_bounded": rt.make_points(near, (4 * disp) ** 2)}
        del near, uniform
        out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        res = {}
        for name, pts in cases.items():
            first = None
            for label, mode in (("", 0), ("_sort", rt.NEAREST_SORT)):
                ms = []
                for k in range(args.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    ctx.nearest(pts, mode=mode, out=out, stream=stream)
                    e1.record(stream)
                    e1.synchronize()
                    if k:   # (the first is the warm-up)
                        ms.append(e0.elapsed_time(e1))
                if first is None:
                    first = out.clone()
                else:   # the same results, bit for bit
                    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), name
                med = float(np.median(ms))
                res[name + label] = {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4),
                                     "ms_max": round(max(ms), 4), "ms_median": round(med, 4),
                                     "mpoints_per_s": round(n / med / 1e3, 1)}
            ctx.nearest(pts, mode=rt.NEAREST_COUNT, out=out, stream=stream)
            c = ctx.nearest_counts()
            assert c["points"] == n, c
            res[name]["counts"] = c
            res[name]["found_fraction"] = round(c["found"] / n, 6)
            res[name]["internal_steps_per_point"] = round(c["internal_steps"] / n, 3)
            res[name]["leaf_steps_per_point"] = round(c["leaf_steps"] / n, 3)
            d2 = first[:, 3]
            res[name]["median_distance_over_displacement"] = round(float(d2[d2 >= 0].sqrt().median()) / disp, 4)
            del first
        ctx.synchronize()
    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under the {W}x{H} reference "
                    "camera, node records; points: the primary rays' hit points displaced by "
                    f"{args.displace} of the root box's diagonal (near_surface), as many uniform in the root box "
                    "(uniform), the first with max_dist2 = (4 displacements)^2 (near_surface_bounded)",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "points": n,
        "reps": args.reps,
        "root_box_diagonal": round(diag, 4),
        "displacement": round(disp, 6),
        "cases": res,
    }
    qb = os.path.join(REPO, "profiles", "query_bench.json")
    if os.path.exists(qb):   # for orientation only: other rays (the frame's reflection rays), the same scene
        with open(qb) as f:
            q = json.load(f)
        result["ray_query_closest_hit_mrays_per_s"] = q["modes"]["closest"]["mrays_per_s"]
        result["ray_query_closest_hit_rays"] = q["rays"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
