"""Triangle query throughput: a second soup against the C5 scene, and one icosphere against the other's tree.

    python scripts/cross_bench.py [--out profiles/cross_bench.json] [--reps 5]
    python scripts/cross_bench.py --ntris 100000 --nqueries 20000 --subdiv 5 --out ''      # a quick look, no file

Two cases.  c5: the synthetic 10M-triangle soup under the reference camera, built; the queries are the triangles of
a second soup of `--nqueries` (1M) triangles drawn by the same generator from another seed, taken to the space the
BVH was built in (times WVP).  shells: scripts/collide_bench.py's two icospheres (`--subdiv` 8: 1,310,720 triangles
each, the second moved by a quarter radius along x) under an identity camera, with only the first one built and the
second one's triangles for queries: the shells cross along a circle.  For each, in the callers' order and with
RTBVH_CROSS_SORT, timed with HIP events around the call on a side stream, the median of `reps` repetitions after
one warm-up, with the min-max spread:

  sizes   RTBVH_CROSS_SIZES alone;
  fill    RTBVH_CROSS_FILL alone, on the offsets of the sizes call;
  both    mode 0 with capacity = the exact total;
  first   rtbvh_cross_first_async;

and ids per query and the RTBVH_CROSS_COUNT steps per query of the sizes pass and of the first pass.  The route
before these entries, for the same queries in the same process, device part only: rtbvh_overlap_async with
RTBVH_OVERLAP_TRIANGLE over the query triangles' boxes, SIZES and FILL -- it lists a superset (scene triangle
against query BOX) and still owes the host the triangle tests, so the comparison flatters it.
Writes the figures as JSON; every timing in it was measured in the run that wrote it.  No gate.  Not part of bench.py.
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
from scripts.collide_bench import welded_scene   # noqa: E402
from scripts.signed_bench import icosphere   # noqa: E402


def built_space(scene, wvp):
    """(T, 3, 3) float32: the scene's triangles in the space a BVH under `wvp` is built in (position times WVP)."""
    p = scene.vertices[:, :3].astype(np.float32)
    m = np.ascontiguousarray(wvp, np.float32).reshape(4, 4)
    c = (p @ m[:3, :3] + m[3, :3]).astype(np.float32)
    return c[np.asarray(scene.indices, np.int64).reshape(-1, 3)]


def measure(rt, torch, ctx, queries, reps):
    """The figures of one built context and one (n, 3, 3) query set."""
    L = rt.lib()
    n = len(queries)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    sh = ctypes.c_void_p(stream.cuda_stream)
    tris = torch.from_numpy(rt.make_tris(queries).view(np.float32).reshape(n, 12)).cuda()
    lo, hi = queries.min(1), queries.max(1)
    boxes = torch.from_numpy(rt.make_boxes(lo, hi).view(np.float32).reshape(n, 8)).cuda()
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    first = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    def cross(ids, mode):
        st = L.rtbvh_cross_async(ctx._h, ptr(tris), n, ptr(offsets), ptr(ids), 0 if ids is None else ids.shape[0],
                                 mode, sh)
        assert st == 0, st

    def cross_first(mode):
        st = L.rtbvh_cross_first_async(ctx._h, ptr(tris), n, ptr(first), mode, sh)
        assert st == 0, st

    def overlap(ids, mode):
        st = L.rtbvh_overlap_async(ctx._h, ptr(boxes), n, ptr(offsets), ptr(ids), 0 if ids is None else ids.shape[0],
                                   mode | rt.OVERLAP_TRIANGLE, sh)
        assert st == 0, st

    def timed(f):
        ms = []
        for k in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            e1.synchronize()
            if k:   # (the first is the warm-up)
                ms.append(e0.elapsed_time(e1))
        return ms

    def figures(ms):
        med = float(np.median(ms))
        return {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "ms_median": round(med, 4), "mqueries_per_s": round(n / med / 1e3, 1)}

    res = {}
    for oname, sort in (("callers_order", 0), ("sorted", rt.CROSS_SORT)):
        cross(None, rt.CROSS_SIZES | rt.CROSS_COUNT | sort)
        c = ctx.cross_counts()
        total = int(offsets[n].item())
        assert c["queries"] == n and c["ids"] == total, c
        sub = {"ids": total, "ids_per_query": round(total / n, 4),
               "sizes_internal_steps_per_query": round(c["internal_steps"] / n, 3),
               "sizes_leaf_steps_per_query": round(c["leaf_steps"] / n, 3)}
        ids = torch.empty(total, dtype=torch.int32, device="cuda")
        sub["sizes"] = figures(timed(lambda: cross(None, rt.CROSS_SIZES | sort)))
        sub["fill"] = figures(timed(lambda: cross(ids, rt.CROSS_FILL | sort)))   # (offsets: the sizes call's)
        sub["both"] = figures(timed(lambda: cross(ids, sort)))
        cross_first(rt.CROSS_COUNT | sort)
        c = ctx.cross_counts()
        sub["queries_with_a_member"] = c["ids"]
        sub["first_internal_steps_per_query"] = round(c["internal_steps"] / n, 3)
        sub["first_leaf_steps_per_query"] = round(c["leaf_steps"] / n, 3)
        sub["first"] = figures(timed(lambda: cross_first(sort)))
        del ids
        # the route before: triangle-box overlap over the queries' boxes, device part only
        osort = rt.OVERLAP_SORT if sort else 0
        overlap(None, rt.OVERLAP_SIZES | osort)
        stream.synchronize()   # (offsets is read on torch's stream)
        ototal = int(offsets[n].item())
        ids = torch.empty(ototal, dtype=torch.int32, device="cuda")
        early = {"ids": ototal, "ids_per_query": round(ototal / n, 4), "ids_over_cross_ids": round(ototal / max(total, 1), 3),
                 "sizes": figures(timed(lambda: overlap(None, rt.OVERLAP_SIZES | osort))),
                 "fill": figures(timed(lambda: overlap(ids, rt.OVERLAP_FILL | osort)))}
        early["sizes_plus_fill_ms_median"] = round(early["sizes"]["ms_median"] + early["fill"]["ms_median"], 4)
        early["earlier_route_over_cross_both"] = round(early["sizes_plus_fill_ms_median"] / sub["both"]["ms_median"], 3)
        sub["overlap_of_query_boxes"] = early
        del ids
        res[oname] = sub
    ctx.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cross_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--nqueries", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--subdiv", type=int, default=8)
    ap.add_argument("--shift", type=float, default=0.25, help="the second shell's offset in radii")
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    cases = {}
    wvp, wv = rt.camera_reference(args.width, args.height)
    queries = built_space(rt.synthetic(args.nqueries, seed=0x5EED0105, half_extent=(100.0, 100.0, 50.0)), wvp)
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(wvp, wv)
        ctx.build()
        cases["c5"] = measure(rt, torch, ctx, queries, args.reps)
    del scene, queries

    verts, faces = icosphere(args.subdiv)
    second = verts.copy()
    second[:, 0] += np.float32(args.shift)
    queries = second[np.asarray(faces, np.int64).reshape(-1, 3)].astype(np.float32)
    scene = welded_scene(rt, verts, faces)
    T = scene.num_tris
    eye = np.eye(4, dtype=np.float32)
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(eye, eye)
        ctx.build()
        cases["shells"] = measure(rt, torch, ctx, queries, args.reps)
    result = {
        "workload": f"c5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under the {args.width}x"
                    f"{args.height} reference camera, node records; queries: the {args.nqueries} triangles of the same "
                    f"generator's seed 0x5EED0105, times WVP.  shells: an icosphere subdivided {args.subdiv} times "
                    f"({T} tris, welded) built under an identity camera; queries: its copy moved by {args.shift} radii "
                    "along x.",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "triangles": {"c5": args.ntris, "shells": T},
        "queries": {"c5": args.nqueries, "shells": T},
        "reps": args.reps,
        "timings": "every ms in this file was measured in the run that wrote it",
        "cases": cases,
    }
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
