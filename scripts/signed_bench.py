"""Signed-distance query throughput on the C5 scene and on a closed mesh.

    python scripts/signed_bench.py [--out profiles/signed_bench.json] [--reps 5] [--no-baselines]

Two workloads, each timed with HIP events on device tensors, `reps` repetitions after one warm-up:

  C5      10M synthetic triangles under the 3840 x 2160 reference camera, node records (as bench.py builds it), with
          nearest_bench's points: near_surface (the primary rays' hit points displaced by `--displace` of the root
          box's diagonal) and as many uniform in the root box.  An open triangle soup: the counts are work, not sides.
  sphere  an icosphere subdivided `--subdiv` (8: 1,310,720 triangles) times under an identity camera, `--sphere-points`
          points uniform in [-1.3, 1.3]^3 and as many within 1e-3 of the surface.  A closed surface: `inside` is also
          checked against |p| < r_in on the points away from the surface.

For each point set: Context.signed in modes 0, SIGNED_VOTE3 and SIGNED_INSIDE_ONLY, each in the given order and with
SIGNED_SORT (the same bits), and the steps per point of one SIGNED_COUNT query per mode.  Beside them, in the same
process, what a caller had before: Context.nearest, plus one all-hits sizes pass (rtbvh_allhits_async with
ALLHITS_SIZES: n + 1 offsets and their scan) per ray along the same directions, on a ray buffer built outside the timed
region.  `baseline` sums nearest and the R sizes passes; `signed_over_baseline` is the new call's median over it.
Writes ms, Mpoints/s, the steps and the run-to-run spread as JSON.  No gate.  Not part of bench.py.
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

D = np.array([[0.75, 0.5, 0.4375], [-0.5, 0.75, -0.4375], [0.4375, -0.5, -0.75]], np.float32)   # include/rtbvh.h


def icosphere(subdiv):
    """The icosahedron subdivided `subdiv` times onto the unit sphere, vectorised: (V, 3) float32, (F, 3) int64."""
    t = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
                  (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
                  (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11),
                  (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.int64)
    for _ in range(subdiv):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[ue[:, 0]] + v[ue[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)   # the midpoints' indices: of (a, b), (b, c), (c, a)
        v = np.concatenate([v, mid])
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        f = np.concatenate([np.stack([a, m[0], m[2]], 1), np.stack([b, m[1], m[0]], 1), np.stack([c, m[2], m[1]], 1),
                            np.stack([m[0], m[1], m[2]], 1)])
    return v.astype(np.float32), f


def scene_of(rt, verts, faces):
    tris = verts[faces].reshape(-1, 3)
    v = np.zeros((len(tris), 8), np.float32)
    v[:, :3] = tris
    v[:, 5] = -1
    T = len(faces)
    return rt.Scene(v, np.arange(3 * T, dtype=np.uint32), np.zeros(T, np.uint32), np.zeros(1, rt.MATERIAL_DTYPE))


def c5_points(rt, torch, ctx, scene, wvp, W, H, displace):
    """nearest_bench's two point sets on a built C5 context, and (root box diagonal, displacement)."""
    m = torch.from_numpy(np.ascontiguousarray(wvp, np.float32).reshape(4, 4)).cuda()
    pos = torch.from_numpy(np.ascontiguousarray(scene.vertices[:, :3])).cuda()
    clip = pos @ m[:3, :3] + m[3, :3]
    lo, hi = clip.min(0).values, clip.max(0).values
    del pos, clip
    diag = float(torch.linalg.norm(hi - lo))
    disp = displace * diag
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    o = torch.stack([(xs.reshape(-1) - W // 2) / 4.0, (ys.reshape(-1) - H // 2) / 4.0,
                     torch.zeros(W * H, device="cuda")], 1).float()
    d = torch.zeros_like(o)
    d[:, 2] = 1
    hits = ctx.query(rt.make_rays(o, d))
    hit = hits[:, 0] != -1
    gen = torch.Generator(device="cuda").manual_seed(5)
    surf = o[hit] + hits[hit, 0:1] * d[hit]
    n = int(surf.shape[0])
    u = torch.randn((n, 3), device="cuda", generator=gen)
    near = surf + disp * u / torch.linalg.norm(u, dim=1, keepdim=True)
    uniform = lo + torch.rand((n, 3), device="cuda", generator=gen) * (hi - lo)
    return {"near_surface": near, "uniform": uniform}, diag, disp


def sphere_points(torch, n):
    gen = torch.Generator(device="cuda").manual_seed(7)
    uniform = (torch.rand((n, 3), device="cuda", generator=gen) * 2 - 1) * 1.3
    u = torch.randn((n, 3), device="cuda", generator=gen)
    u = u / torch.linalg.norm(u, dim=1, keepdim=True)
    near = u * (1 + (torch.rand((n, 1), device="cuda", generator=gen) * 2 - 1) * 1e-3)
    return {"near_surface": near, "uniform": uniform}


def make_timed(torch, stream, reps, n):
    def timed(f):
        ms = []
        for rep in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            e1.synchronize()
            if rep:   # (the first is the warm-up)
                ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        return {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "ms_median": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4),
                "mpoints_per_s": round(n / med / 1e3, 1)}
    return timed


def measure(rt, torch, ctx, sets, reps, baselines, r_in=None):
    """Every mode on every point set of one built context; r_in: check `inside` against a sphere's."""
    L = rt.lib()
    stream = torch.cuda.Stream()
    res = {}
    modes = (("signed", 0), ("signed_vote3", rt.SIGNED_VOTE3), ("inside_only", rt.SIGNED_INSIDE_ONLY))
    for name, xyz in sets.items():
        n = int(xyz.shape[0])
        timed = make_timed(torch, stream, reps, n)
        pts = rt.make_points(xyz, float("inf"))
        stream.wait_stream(torch.cuda.current_stream())   # (make_points ran on the current stream)
        out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        case = {"points": n}
        for label, mode in modes:
            first = None
            for order, sort in (("", 0), ("_sort", rt.SIGNED_SORT)):
                case[label + order] = timed(lambda: ctx.signed(pts, mode=mode | sort, out=out, stream=stream))
                if first is None:
                    first = out.clone()
                else:   # the same records, bit for bit
                    assert torch.equal(out.view(torch.int32), first.view(torch.int32)), (name, label)
            ctx.signed(pts, mode=mode | rt.SIGNED_COUNT, out=out, stream=stream)
            c = ctx.signed_counts()
            assert c["points"] == n, c
            case[label]["internal_steps_per_point"] = round(c["internal_steps"] / n, 3)
            case[label]["leaf_steps_per_point"] = round(c["leaf_steps"] / n, 3)
            case[label]["inside_share"] = round(c["inside"] / n, 5)
            if r_in is not None:   # away from the surface the answer is known
                r = torch.linalg.norm(xyz.double(), dim=1)
                keep = ~((0.999 * r_in <= r) & (r <= 1.001))
                got = (first[:, 7].contiguous().view(torch.int32) & 1) != 0
                case[label]["wrong_inside_away_from_the_surface"] = int((got != (r < r_in))[keep].sum())
                case[label]["points_away_from_the_surface"] = int(keep.sum())
        if baselines:
            near_out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
            sh = ctypes.c_void_p(stream.cuda_stream)
            rays = []
            for j in range(3):
                dj = torch.from_numpy(D[j]).cuda().expand(n, 3)
                rays.append(rt.make_rays(xyz, dj))   # t_max = +inf
            stream.wait_stream(torch.cuda.current_stream())

            def sizes(j, mode):
                st = L.rtbvh_allhits_async(ctx._h, ctypes.c_void_p(rays[j].data_ptr()), n,
                                           ctypes.c_void_p(offsets.data_ptr()), None, 0, rt.ALLHITS_SIZES | mode, sh)
                assert st == 0, st

            base = {}
            for order, nsort, asort in (("", 0, 0), ("_sort", rt.NEAREST_SORT, rt.ALLHITS_SORT)):
                base["nearest" + order] = timed(lambda: ctx.nearest(pts, mode=nsort, out=near_out, stream=stream))
                for j in range(3):
                    base[f"allhits_sizes_ray{j}" + order] = timed(lambda: sizes(j, asort))
                for label, rays_cast, near in (("signed", 1, 1), ("signed_vote3", 3, 1), ("inside_only", 1, 0)):
                    parts = ["nearest" + order] * near + [f"allhits_sizes_ray{j}" + order for j in range(rays_cast)]
                    ms = sum(base[p]["ms_median"] for p in parts)
                    spread = max(base[p]["spread"] for p in parts)
                    t = case[label + order]
                    t["baseline_ms"] = round(ms, 4)
                    t["baseline_parts"] = parts
                    t["baseline_spread"] = spread
                    t["signed_over_baseline"] = round(t["ms_median"] / ms, 4)
            case["before"] = base
            del near_out, offsets, rays
        res[name] = case
        del out, pts
    ctx.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "signed_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--displace", type=float, default=1e-3)
    ap.add_argument("--subdiv", type=int, default=8)
    ap.add_argument("--sphere-points", type=int, default=4_000_000)
    ap.add_argument("--no-baselines", action="store_true", help="the signed-distance cases only (an A/B of the kernel)")
    args = ap.parse_args()

    import torch

    import raytracebvh_amd as rt

    W, H = args.width, args.height
    res = {}
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    wvp, wv = rt.camera_reference(W, H)
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene)
        ctx.set_camera(wvp, wv)
        ctx.build()
        sets, diag, disp = c5_points(rt, torch, ctx, scene, wvp, W, H, args.displace)
        res["c5"] = measure(rt, torch, ctx, sets, args.reps, not args.no_baselines)
    del scene, sets
    verts, faces = icosphere(args.subdiv)
    t = verts.astype(np.float64)[faces]
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    r_in = float(np.abs((nrm * t[:, 0]).sum(1)).min())
    del t, nrm
    eye = np.eye(4, dtype=np.float32)
    with rt.Context(device=0) as ctx:
        ctx.set_scene(scene_of(rt, verts, faces))
        ctx.set_camera(eye, eye)
        ctx.build()
        res["sphere"] = measure(rt, torch, ctx, sphere_points(torch, args.sphere_points), args.reps,
                                not args.no_baselines, r_in)
    result = {
        "workload": f"c5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50) under the {W}x{H} reference "
                    "camera, node records; points: the primary rays' hit points displaced by "
                    f"{args.displace} of the root box's diagonal (near_surface), as many uniform in the root box "
                    f"(uniform).  sphere: an icosphere subdivided {args.subdiv} times ({len(faces)} tris) under an "
                    f"identity camera; {args.sphere_points} points within 1e-3 of the unit sphere (near_surface) and "
                    "uniform in [-1.3, 1.3]^3 (uniform).  No bound.",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "device": torch.cuda.get_device_name(0),
        "reps": args.reps,
        "c5_root_box_diagonal": round(diag, 4),
        "c5_displacement": round(disp, 6),
        "sphere_inradius": r_in,
        "baseline": "Context.nearest plus one rtbvh_allhits_async ALLHITS_SIZES pass per ray along the same "
                    "directions (reference crossing test, EPSILON 0.01); the ray buffers are built outside the timing",
        "not_measured": "node-box trees (FLAG_AUTO_WALK builds), finite bounds, the baseline's ray-buffer build",
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
