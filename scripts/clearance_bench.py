"""Clearance query throughput: a second soup against the C5 scene, and one icosphere against the other's tree,
crossing and apart.

    python scripts/clearance_bench.py [--out profiles/clearance_bench.json] [--reps 5]
    python scripts/clearance_bench.py --ntris 100000 --nqueries 20000 --subdiv 5 --out ''      # a quick look, no file

Three cases.  c5 and shells are scripts/cross_bench.py's: the synthetic 10M-triangle soup under the reference camera
with the `--nqueries` (1M) triangles of a second soup for queries, and two icospheres (`--subdiv` 8: 1,310,720
triangles each) under an identity camera, the first one built, the second one moved by `--shift` (a quarter) radii
along x for queries: they cross along a circle.  gap: the same spheres with the second moved by 2 + `--gap` radii, so
that `--gap` (0.02) radii separate them.  For each, under max_dist2 = +inf and under a narrow band --
(`--band` (0.01) times the root box's diagonal) squared -- in the callers' order and with RTBVH_CLEARANCE_SORT, timed
with HIP events around the call on a side stream, the median of `reps` repetitions after one warm-up, with the
min-max spread: ms, Mqueries/s, the RTBVH_CLEARANCE_COUNT steps per query, the share of queries with a result and the
share with dist2 == 0.
Beside it, for the same queries in the same process, the route before this entry, device part only:
rtbvh_nearest_async over the 3N query vertices with the same bound.  Its time; the share of queries whose vertex-only
distance (the least of its three vertices') exceeds the clearance by more than 10^-3 of the root diagonal (a query
the route finds nothing for counts when the clearance has a result); and the share of crossing queries (dist2 == 0)
to which it gives a positive distance, or none.
Writes the figures as JSON; every figure in it was measured in the run that wrote it.  No gate.  Not part of bench.py.
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
from scripts.cross_bench import built_space   # noqa: E402
from scripts.signed_bench import icosphere   # noqa: E402


def measure(rt, torch, ctx, queries, diagonal, band, reps):
    """The figures of one built context and one (n, 3, 3) query set."""
    L = rt.lib()
    n = len(queries)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    sh = ctypes.c_void_p(stream.cuda_stream)
    tris = torch.from_numpy(rt.make_tris(queries).view(np.float32).reshape(n, 12)).cuda()
    out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    points = torch.zeros((3 * n, 4), dtype=torch.float32, device="cuda")
    points[:, :3] = torch.from_numpy(np.ascontiguousarray(queries.reshape(-1, 3))).cuda()
    near = torch.empty((3 * n, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    def clearance(bound, mode):
        st = L.rtbvh_clearance_async(ctx._h, ptr(tris), n, ctypes.c_float(bound), ptr(out), mode, sh)
        assert st == 0, st

    def nearest(mode):
        st = L.rtbvh_nearest_async(ctx._h, ptr(points), 3 * n, ptr(near), mode, sh)
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

    def figures(ms, m):
        med = float(np.median(ms))
        return {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "ms_median": round(med, 4), "mqueries_per_s": round(m / med / 1e3, 1)}

    res = {}
    for bname, bound in (("inf", float("inf")), ("band", float(np.float32((band * diagonal) ** 2)))):
        per = {"max_dist2": bound if np.isfinite(bound) else "inf"}
        for oname, sort in (("callers_order", 0), ("sorted", rt.CLEARANCE_SORT)):
            clearance(bound, rt.CLEARANCE_COUNT | sort)
            c = ctx.clearance_counts()
            assert c["queries"] == n, c
            with torch.cuda.stream(stream):
                found = out[:, 7].view(torch.int32) != -1
                d = torch.where(found, out[:, 3], torch.full_like(out[:, 3], float("inf")))
                zero = found & (out[:, 3] == 0)
                nfound, nzero = int(found.sum().item()), int(zero.sum().item())
            assert nfound == c["found"], (nfound, c)
            sub = {"found_share": round(nfound / n, 6), "dist2_zero_share": round(nzero / n, 6),
                   "internal_steps_per_query": round(c["internal_steps"] / n, 3),
                   "leaf_steps_per_query": round(c["leaf_steps"] / n, 3)}
            sub.update(figures(timed(lambda: clearance(bound, sort)), n))
            # the route before: nearest over the 3n vertices, device part only
            points[:, 3] = bound
            stream.wait_stream(torch.cuda.current_stream())
            nsort = rt.NEAREST_SORT if sort else 0
            early = figures(timed(lambda: nearest(nsort)), n)
            with torch.cuda.stream(stream):
                nd = near[:, 3].reshape(n, 3)
                nd = torch.where(nd < 0, torch.full_like(nd, float("inf")), nd).min(1).values   # (-1: no result)
                excess = torch.sqrt(nd) - torch.sqrt(d)       # (inf - inf: NaN, compares false)
                over = found & (excess > 1e-3 * diagonal)
                missed = zero & (nd > 0)
                early["over_clearance_by_1e-3_diagonal_share"] = round(int(over.sum().item()) / n, 6)
                early["crossing_queries_given_a_positive_distance_share"] = round(int(missed.sum().item()) / max(nzero, 1), 6)
                finite = found & torch.isfinite(nd)
                if int(finite.sum().item()):
                    early["worst_excess_over_diagonal"] = round(float(excess[finite].max().item()) / diagonal, 6)
            early["earlier_route_over_clearance"] = round(early["ms_median"] / sub["ms_median"], 3)
            sub["nearest_of_the_3n_vertices"] = early
            per[oname] = sub
        res[bname] = per
    ctx.synchronize()
    return res


def diagonal_of(tris):
    p = tris.reshape(-1, 3)
    return float(np.linalg.norm(p.max(0).astype(np.float64) - p.min(0).astype(np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clearance_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--nqueries", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--subdiv", type=int, default=8)
    ap.add_argument("--shift", type=float, default=0.25, help="shells: the second shell's offset in radii")
    ap.add_argument("--gap", type=float, default=0.02, help="gap: the space between the shells in radii")
    ap.add_argument("--band", type=float, default=0.01, help="the narrow bound's distance in root diagonals")
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    cases, diagonals = {}, {}
    wvp, wv = rt.camera_reference(args.width, args.height)
    queries = built_space(rt.synthetic(args.nqueries, seed=0x5EED0105, half_extent=(100.0, 100.0, 50.0)), wvp)
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    diagonals["c5"] = diagonal_of(built_space(scene, wvp))
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(wvp, wv)
        ctx.build()
        cases["c5"] = measure(rt, torch, ctx, queries, diagonals["c5"], args.band, args.reps)
    del scene, queries

    verts, faces = icosphere(args.subdiv)
    scene = welded_scene(rt, verts, faces)
    T = scene.num_tris
    diagonals["shells"] = diagonals["gap"] = diagonal_of(verts.astype(np.float32))
    eye = np.eye(4, dtype=np.float32)
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(eye, eye)
        ctx.build()
        for name, shift in (("shells", args.shift), ("gap", 2.0 + args.gap)):
            second = verts.copy()
            second[:, 0] += np.float32(shift)
            queries = second[np.asarray(faces, np.int64).reshape(-1, 3)].astype(np.float32)
            cases[name] = measure(rt, torch, ctx, queries, diagonals[name], args.band, args.reps)
    result = {
        "workload": f"c5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under the {args.width}x"
                    f"{args.height} reference camera, node records; queries: the {args.nqueries} triangles of the same "
                    f"generator's seed 0x5EED0105, times WVP.  shells: an icosphere subdivided {args.subdiv} times "
                    f"({T} tris, welded) built under an identity camera; queries: its copy moved by {args.shift} radii "
                    f"along x.  gap: the copy moved by {2.0 + args.gap} radii.  band: max_dist2 = ({args.band} root "
                    "diagonals) squared.",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "triangles": {"c5": args.ntris, "shells": T, "gap": T},
        "queries": {"c5": args.nqueries, "shells": T, "gap": T},
        "root_diagonal": {k: round(v, 6) for k, v in diagonals.items()},
        "reps": args.reps,
        "timings": "every figure in this file was measured in the run that wrote it",
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
