"""Animated geometry on the C5 scene: the vertex update, a rebuild against a topology-keeping refit, and what
each tree costs the certified trace as the mesh moves away from the shape it was built for.

    python scripts/dynamic_bench.py [--out profiles/dynamic_bench.json] [--frames 16] [--reps 5]

The scene is bench.py's C5 (10M synthetic triangles, seed 0x5EED0005, box 100 x 100 x 50, 3840 x 2160, primary
+ 1 bounce, RTBVH_FLAG_AUTO_WALK: the certified walks).  The positions live in a device tensor; frame f moves
every vertex to p + a_f sin(k p.yzx + 0.3 f) with a_f = (f + 1) * `--step` of the mesh box (default 0.5% a
frame: 8% at frame 16), computed by torch on the context's stream.

1. Per frame, in two contexts on one stream -- one rebuilds (rtbvh_build_async), one was built once over the
   undeformed mesh and refits (rtbvh_refit_async) -- timed with device events on that stream, the median of
   `reps` repetitions after a warm-up: the update (rtbvh_update_vertices_async from the tensor), the rebuild
   or the refit, and the certified trace over the resulting tree.  The trace column is the point: a refitted
   tree's boxes grow as the mesh deforms.  `crossover_frame` is the first frame at which rebuild + trace is
   below refit + trace (null: never within the run).
2. The camera orbit (static geometry, CPUTests Morton codes): rtbvh_set_camera, then a rebuild against a
   refit; the two trees are compared field by field once (`orbit.identical_trees`).
3. The rebuilt frame as one hipGraph (RTBVH_FLAG_GRAPH | RTBVH_FLAG_AUTO_WALK): bench.py's c5_frame_rebuild
   loop (wall clock per synchronous rtbvh_compute_bvh), static; then with a vertex update of the same positions
   before every frame -- the same frame, so the difference is what the update costs a rebuilt frame
   (`update_on_top_ms`); then deforming every frame (the torch deformation and the deformed mesh's slower
   trace included).  `graph_captures` stays 1.

Writes one JSON file and prints it.  Not part of bench.py.  RTBVH_LIB=<an A/B build> measures that build.
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


def summary(ms):
    return {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "ms_median": round(float(np.median(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dynamic_bench.json"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", type=float, default=0.005, help="amplitude growth per frame, as a share of the mesh box")
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--graph-frames", type=int, default=10)
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    assert torch.cuda.is_available(), "dynamic_bench.py measures on a GPU"
    W, H, bounces = args.width, args.height, 1
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    wvp, wv = rt.camera_reference(W, H)
    stream = torch.cuda.Stream()
    handle = stream.cuda_stream
    with torch.cuda.stream(stream):
        p0 = torch.from_numpy(np.ascontiguousarray(scene.vertices[:, :3])).cuda()
        lo, hi = p0.min(0).values, p0.max(0).values
        ext = hi - lo
        wav = 2 * np.pi / ext
        pos = torch.empty_like(p0)

    def deform(f):   # on `stream`: the update that follows reads it in stream order
        with torch.cuda.stream(stream):
            torch.add(p0, (args.step * (f + 1)) * ext * torch.sin(wav[[1, 2, 0]] * p0[:, [1, 2, 0]] + 0.3 * f), out=pos)

    def timed(fn):   # ms of what fn enqueues on `stream`
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50), {W}x{H}, primary+1 bounce, "
                    f"RTBVH_FLAG_AUTO_WALK; vertices displaced by (f + 1) * {args.step} of the mesh box at frame f",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "frames": args.frames, "reps": args.reps,
    }
    kw = dict(device=0, flags=rt.FLAG_AUTO_WALK, stream=handle)
    with rt.Context(**kw) as reb, rt.Context(**kw) as ref:
        for c in (reb, ref):
            c.set_scene(scene)
            c.set_camera(wvp, wv)
            c.build()
            c.trace(W, H, bounces)   # warm-up: every buffer exists
        base_trace = summary([timed(lambda: reb.trace(W, H, bounces, sync=False)) for _ in range(args.reps)])
        base_build = summary([timed(lambda: reb.build(sync=False)) for _ in range(args.reps)])
        base_refit = summary([timed(lambda: ref.refit(sync=False)) for _ in range(args.reps)])
        result["undeformed"] = {"build": base_build, "refit": base_refit, "trace": base_trace,
                                "refit_over_build": round(base_refit["ms_median"] / base_build["ms_median"], 4)}
        frames = []
        crossover = None
        for f in range(args.frames):
            deform(f)
            row = {"frame": f, "amplitude_share": round(args.step * (f + 1), 5)}
            for name, c, step in (("rebuild", reb, lambda: reb.build(sync=False)),
                                  ("refit", ref, lambda: ref.refit(sync=False))):
                up, bd, tr = [], [], []
                for k in range(args.reps + 1):
                    u = timed(lambda: c.update_vertices(pos, stream=stream))
                    b = timed(step)
                    t = timed(lambda: c.trace(W, H, bounces, sync=False))
                    if k:   # (the first is the warm-up)
                        up.append(u), bd.append(b), tr.append(t)
                st = c.stats()
                row[name] = {"update": summary(up), "boxes": summary(bd), "trace": summary(tr),
                             "redo_total": st["redo_total"],
                             "boxes_plus_trace_ms": round(float(np.median(bd)) + float(np.median(tr)), 4)}
            if crossover is None and row["rebuild"]["boxes_plus_trace_ms"] < row["refit"]["boxes_plus_trace_ms"]:
                crossover = f
            frames.append(row)
        diff = int((reb.read_framebuffer().view(np.uint32) != ref.read_framebuffer().view(np.uint32)).any(-1).sum())
        result["animation"] = frames
        result["crossover_frame"] = crossover
        result["last_frame_differing_pixels"] = diff   # (two valid trees: ties may resolve to another triangle)

        # 2. the camera orbit over the undeformed mesh
        for c in (reb, ref):
            c.update_vertices(p0, stream=stream)
            c.build()
        eye = rt.EYE_REFERENCE
        ob, orf, otb, otr = [], [], [], []
        for k in range(args.reps + 1):
            eye = rt.camera_orbit(eye, rt.KEY_LEFT)
            cam = rt.camera_look(eye, W, H)
            reb.set_camera(*cam)
            ref.set_camera(*cam)
            b = timed(lambda: reb.build(sync=False))
            tb = timed(lambda: reb.trace(W, H, bounces, sync=False))
            r = timed(lambda: ref.refit(sync=False))
            tr = timed(lambda: ref.trace(W, H, bounces, sync=False))
            if k:
                ob.append(b), orf.append(r), otb.append(tb), otr.append(tr)
        ta, tb_ = reb.read_bvh(), ref.read_bvh()
        same = all(np.array_equal(ta[f].view(np.uint32), tb_[f].view(np.uint32)) for f in ta.dtype.names)
        del ta, tb_
        same_frame = bool(np.array_equal(reb.read_framebuffer().view(np.uint32), ref.read_framebuffer().view(np.uint32)))
        result["orbit"] = {"rebuild": summary(ob), "refit": summary(orf), "trace_after_rebuild": summary(otb),
                           "trace_after_refit": summary(otr), "identical_trees": bool(same),
                           "identical_frames": same_frame,
                           "refit_over_rebuild": round(float(np.median(orf)) / float(np.median(ob)), 4)}

    # 3. the rebuilt frame as one hipGraph, static and animated (bench.py's c5_frame_rebuild loop)
    with rt.Context(device=0, flags=rt.FLAG_GRAPH | rt.FLAG_AUTO_WALK, stream=handle) as g:
        g.set_scene(scene)
        g.set_camera(wvp, wv)
        g.compute_bvh(W, H, bounces)
        g.compute_bvh(W, H, bounces)
        n = args.graph_frames

        def loop(positions):   # None: static; a tensor: updated with it; "deform": a new deformation per frame
            per = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                for f in range(n):
                    if positions is not None:
                        if positions is pos:
                            deform(f)
                        g.update_vertices(positions, stream=stream)
                    g.compute_bvh(W, H, bounces)
                per.append((time.perf_counter() - t0) / n * 1e3)
            return summary(per)

        static = loop(None)
        updated = loop(p0)
        static2 = loop(None)   # (the spread: the same loop again)
        upd = summary([timed(lambda: g.update_vertices(p0, stream=stream)) for _ in range(args.reps + 2)][2:])
        animated = loop(pos)
        g.update_vertices(p0, stream=stream)
        g.compute_bvh(W, H, bounces)
        result["graph_frame"] = {
            "frames_per_loop": n, "static_ms_per_frame": static, "static_again_ms_per_frame": static2,
            "updated_same_positions_ms_per_frame": updated, "update_kernel": upd,
            "update_on_top_ms": round(updated["ms_median"] - (static["ms_median"] + static2["ms_median"]) / 2, 4),
            "deforming_ms_per_frame": animated,
            "graph_captures": g.stats()["graph_captures"],
        }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
