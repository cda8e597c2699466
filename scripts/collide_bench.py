"""Self-collision query throughput: the C5 scene, and two interpenetrating icospheres.

    python scripts/collide_bench.py [--out profiles/collide_bench.json] [--reps 5] [--frames 20]
    python scripts/collide_bench.py --ntris 100000 --subdiv 5 --out ''      # a quick look, no file

Two scenes: C5 (the synthetic 10M-triangle soup under the reference camera), and scripts/signed_bench.py's icosphere
(`--subdiv` 8: 1,310,720 triangles) taken twice as one welded mesh each -- the second copy moved by a quarter radius
along x, with its own vertex range -- under an identity camera: the two shells interpenetrate along a circle and
nothing else crosses.  For each, with and without RTBVH_COLLIDE_TRIANGLE and with and without RTBVH_COLLIDE_SYMMETRIC,
timed with HIP events, the median of `reps` repetitions after one warm-up:

  sizes   RTBVH_COLLIDE_SIZES alone;
  fill    RTBVH_COLLIDE_FILL alone, on the offsets of the sizes call;
  both    mode 0 with capacity = the exact total;

and entries per triangle and the RTBVH_COLLIDE_COUNT steps per triangle of the sizes pass and of the one call.
The earlier route's device part, in the same process: rtbvh_overlap_async over the T leaf boxes (read back once with
read_bvh, outside the timing), SIZES and FILL; `earlier_route_over_collide_both` is its time over the one-call
box-mode collide's.  For the shells also the host time of a frame -- update_vertices of the second shell, refit, one
collide call (TRIANGLE, capacity fixed), synchronize -- while the second shell moves, over `frames` frames.
Writes the figures as JSON; every timing in it was measured in the run that wrote it.  No gate.  Not part of bench.py.
RTBVH_LIB=<an A/B build of the library> measures that build.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from scripts.signed_bench import icosphere   # noqa: E402


def welded_scene(rt, verts, faces):
    v = np.zeros((len(verts), 8), np.float32)
    v[:, :3] = verts
    v[:, 5] = -1
    T = len(faces)
    return rt.Scene(v, np.ascontiguousarray(faces, np.uint32).reshape(-1), np.zeros(T, np.uint32),
                    np.zeros(1, rt.MATERIAL_DTYPE))


def measure(rt, torch, ctx, T, reps):
    """The figures of one built context."""
    L = rt.lib()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    sh = ctypes.c_void_p(stream.cuda_stream)
    offsets = torch.empty(T + 1, dtype=torch.int64, device="cuda")

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    def collide(ids, mode):
        st = L.rtbvh_collide_async(ctx._h, ptr(offsets), ptr(ids), 0 if ids is None else ids.shape[0], mode, sh)
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

    def figures(ms, total):
        med = float(np.median(ms))
        return {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "ms_median": round(med, 4), "mtris_per_s": round(T / med / 1e3, 1),
                "mentries_per_s": round(total / med / 1e3, 1)}

    res = {}
    for tname, tri in (("boxes", 0), ("triangles", rt.COLLIDE_TRIANGLE)):
        for oname, sym in (("default", 0), ("symmetric", rt.COLLIDE_SYMMETRIC)):
            m = tri | sym
            collide(None, rt.COLLIDE_SIZES | rt.COLLIDE_COUNT | m)
            c = ctx.collide_counts()
            total = int(offsets[T].item())
            assert c["triangles"] == T and c["entries"] == total, c
            sub = {"entries": total, "entries_per_triangle": round(total / T, 4),
                   "sizes_internal_steps_per_triangle": round(c["internal_steps"] / T, 3),
                   "sizes_leaf_steps_per_triangle": round(c["leaf_steps"] / T, 3)}
            ids = torch.empty(total, dtype=torch.int32, device="cuda")
            sub["sizes"] = figures(timed(lambda: collide(None, rt.COLLIDE_SIZES | m)), total)
            sub["fill"] = figures(timed(lambda: collide(ids, rt.COLLIDE_FILL | m)), total)   # (offsets: the sizes call's)
            sub["both"] = figures(timed(lambda: collide(ids, m)), total)
            collide(ids, rt.COLLIDE_COUNT | m)
            c = ctx.collide_counts()
            assert c["entries"] == total, (c, total)
            sub["both_internal_steps_per_triangle"] = round(c["internal_steps"] / T, 3)
            sub["both_leaf_steps_per_triangle"] = round(c["leaf_steps"] / T, 3)
            res[f"{tname}_{oname}"] = sub
            del ids
    # the earlier route's device part: overlap over the leaf boxes, which lists every triangle itself, every pair
    # twice and the neighbours, for the host to throw away
    nodes = ctx.read_bvh()
    boxes = torch.from_numpy(rt.make_boxes(nodes["bb_min"][:T], nodes["bb_max"][:T]).view(np.float32).reshape(T, 8)).cuda()
    del nodes
    torch.cuda.synchronize()

    def overlap(ids, mode):
        st = L.rtbvh_overlap_async(ctx._h, ptr(boxes), T, ptr(offsets), ptr(ids), 0 if ids is None else ids.shape[0],
                                   mode, sh)
        assert st == 0, st

    overlap(None, rt.OVERLAP_SIZES)
    stream.synchronize()   # (offsets is read on torch's stream)
    total = int(offsets[T].item())
    ids = torch.empty(total, dtype=torch.int32, device="cuda")
    early = {"ids": total, "ids_per_box": round(total / T, 4),
             "sizes": figures(timed(lambda: overlap(None, rt.OVERLAP_SIZES)), total),
             "fill": figures(timed(lambda: overlap(ids, rt.OVERLAP_FILL)), total)}
    early["sizes_plus_fill_ms_median"] = round(early["sizes"]["ms_median"] + early["fill"]["ms_median"], 4)
    early["earlier_route_over_collide_both"] = round(early["sizes_plus_fill_ms_median"] /
                                                     res["boxes_default"]["both"]["ms_median"], 3)
    res["overlap_of_leaf_boxes"] = early
    del ids, boxes
    ctx.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "collide_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--subdiv", type=int, default=8)
    ap.add_argument("--shift", type=float, default=0.25, help="the second shell's offset in radii")
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    cases = {}
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(*rt.camera_reference(args.width, args.height))
        ctx.build()
        cases["c5"] = measure(rt, torch, ctx, scene.num_tris, args.reps)
    del scene

    verts, faces = icosphere(args.subdiv)
    V = len(verts)
    second = verts.copy()
    second[:, 0] += np.float32(args.shift)
    scene = welded_scene(rt, np.concatenate([verts, second]), np.concatenate([faces, faces + V]))
    T = scene.num_tris
    eye = np.eye(4, dtype=np.float32)
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(eye, eye)
        ctx.build()
        shells = measure(rt, torch, ctx, T, args.reps)
        # the second shell moves: update, refit, collide, every frame
        base = torch.from_numpy(verts).cuda()
        capacity = 4 * shells["triangles_default"]["entries"] + 1024
        ms, entries = [], []
        stream = torch.cuda.Stream()
        for f in range(args.frames + 1):
            dx = args.shift * (1.0 + 0.5 * np.sin(0.3 * f))
            pos = (base + torch.tensor([dx, 0.0, 0.0], dtype=torch.float32, device="cuda")).contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.update_vertices(pos, first=V, stream=stream)
            ctx.refit(sync=False)
            off, _ = ctx.collide(rt.COLLIDE_TRIANGLE, capacity=capacity, stream=stream, device=True)
            stream.synchronize()
            ctx.synchronize()
            t1 = time.perf_counter()
            total = int(off[T].item())
            assert total <= capacity, (total, capacity)
            if f:   # (the first is the warm-up)
                ms.append((t1 - t0) * 1e3)
                entries.append(total)
        shells["moving_second_shell"] = {
            "frame": "update_vertices of the second shell, refit, one collide call (TRIANGLE), synchronize; host time",
            "frames": args.frames, "ms": [round(v, 4) for v in ms], "ms_median": round(float(np.median(ms)), 4),
            "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "entries_min": min(entries),
            "entries_max": max(entries)}
        cases["shells"] = shells
    result = {
        "workload": f"c5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under the {args.width}x"
                    f"{args.height} reference camera, node records.  shells: an icosphere subdivided {args.subdiv} "
                    f"times ({len(faces)} tris, welded) twice, the second moved by {args.shift} radii along x with its "
                    "own vertices, identity camera.",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "triangles": {"c5": args.ntris, "shells": T},
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
