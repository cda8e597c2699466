"""Split region queries against the plain ones on the C5 scene.

    python scripts/region_split_bench.py [--out profiles/region_split_bench.json] [--reps 5] [--parts a,b,c]

One process, HIP events, the one-call form.  Per case a warm-up of both, then `reps` rounds of [plain, split] in turn:
the median of each with its min-max.  Every split run is checked against the plain run's offsets and the ids'
order-sensitive digest.  scripts/region_bench.py's workloads:

  (b) `--slabs` zero-thickness slabs across C5's root box along z, REGION_TRIANGLE;
  (c) C5 under the identity camera: the reference camera's whole frustum as one region and as `--tiles` x `--tiles`
      tile frusta; boxes and REGION_TRIANGLE, accepting and REGION_NO_ACCEPT; on the one frustum also K = 64, 1024, 4096;
  (a) the primary rays' hit points as boxes of ten displacements, as plane sets, under REGION_SPLIT_AUTO: so many
      regions that K comes out as 1 and the plain path runs.

`beats`: the split median is below the plain one by more than the two runs' min-max spreads together; `inside`: the
split median lies within the plain run's min-max.  One REGION_COUNT call per form gives the steps, the pieces and the
longest piece walk.  No gate.  Not part of bench.py.  RTBVH_LIB=<an A/B build of the library> measures that build.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "region_split_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--displace", type=float, default=1e-3)
    ap.add_argument("--extent", type=float, default=10.0, help="(a): the boxes' half-extent in displacements")
    ap.add_argument("--slabs", type=int, default=4096)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--parts", default="b,c,a")
    args = ap.parse_args()
    parts = set(args.parts.split(","))

    import torch

    import raytracebvh_amd as rt

    L = rt.lib()
    W, H = args.width, args.height
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    wvp, wv = rt.camera_reference(W, H)
    stream = torch.cuda.Stream()
    sh = ctypes.c_void_p(stream.cuda_stream)
    NOACC, TRI, SIZES, COUNT, AUTO = (rt.REGION_NO_ACCEPT, rt.REGION_TRIANGLE, rt.REGION_SIZES, rt.REGION_COUNT,
                                      rt.REGION_SPLIT_AUTO)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    def note(*what):   # progress, on stderr: the result line stays alone on stdout
        print("region_split_bench:", *what, file=sys.stderr, flush=True)

    def once(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

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
                "ms_median": round(med, 4), "mids_per_s": round(total / med / 1e3, 1)}

    def compare(ctx, regions, mode, fields, label):
        """The one-call query of `regions` ((n, 24) device tensor) under `mode`, plain and with each split field of
        `fields` ({name: bits}), interleaved."""
        n = int(regions.shape[0])
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def region(ids, m):
            st = L.rtbvh_region_async(ctx._h, ptr(regions), n, ptr(offsets), ptr(ids), 0 if ids is None else ids.shape[0],
                                      m, sh)
            assert st == 0, st

        region(None, mode | SIZES | AUTO)
        stream.synchronize()
        total = int(offsets[n].item())
        ids = torch.empty(total, dtype=torch.int32, device="cuda")
        forms = {"plain": 0, **fields}
        want = None
        for name, bits in forms.items():   # the warm-up, and the check of every form against the plain one
            ids.zero_()
            offsets.fill_(-1)
            torch.cuda.synchronize()   # (cleared on torch's stream, queried on ours)
            region(ids, mode | bits)
            stream.synchronize()
            got = (offsets.clone(), digest(ids))
            if want is None:
                want = got
            assert torch.equal(got[0], want[0]) and got[1] == want[1], f"{label} {name}: not the plain query's lists"
        ms = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, bits in forms.items():
                ms[name].append(once(lambda: region(ids, mode | bits)))
        out = {"regions": n, "ids": total}
        for name, bits in forms.items():
            sub = figures(ms[name], total)
            region(ids, mode | bits | COUNT)
            stream.synchronize()
            c = ctx.region_counts()
            assert c["regions"] == n and c["ids"] == total, c
            sub["steps"] = c["internal_steps"] + c["leaf_steps"]
            sub["accepted_subtrees"] = c["accepted_subtrees"]
            if bits:
                sub["split_counts"] = ctx.region_split_counts()
            out[name] = sub
            note(label, name, sub["ms_median"], "ms", sub.get("split_counts", ""))
        p = out["plain"]
        for name in fields:
            s = out[name]
            spread = (p["ms_max"] - p["ms_min"]) + (s["ms_max"] - s["ms_min"])
            s["plain_over_split"] = round(p["ms_median"] / s["ms_median"], 3)
            s["beats_plain"] = bool(p["ms_median"] - s["ms_median"] > spread)
            s["inside_plain_spread"] = bool(p["ms_min"] <= s["ms_median"] <= p["ms_max"])
        del ids, offsets
        torch.cuda.synchronize()
        return out

    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50), node records, the one-call form",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "reps": args.reps,
        "split_max_pieces": rt.REGION_SPLIT_MAX_PIECES,
    }
    auto = {"auto": AUTO}
    if "c" in parts:
        ident = np.eye(4, dtype=np.float32)
        with rt.Context(device=0) as ctx:
            ctx.set_scene(scene)
            ctx.set_camera(ident, ident)
            ctx.build()
            result["device"] = torch.cuda.get_device_name(0)
            m = np.asarray(wvp, np.float64).reshape(4, 4)
            cx, cy, cz, cw = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
            nt = args.tiles
            edges = -1.0 + 2.0 * np.arange(nt + 1) / nt
            planes = np.zeros((nt, nt, 6, 4))
            for j in range(nt):
                for i in range(nt):
                    planes[j, i] = [-(cx - edges[i] * cw), -(edges[i + 1] * cw - cx), -(cy - edges[j] * cw),
                                    -(edges[j + 1] * cw - cy), -cz, -(cw - cz)]
            tiles = torch.from_numpy(planes.reshape(nt * nt, 24).astype(np.float32)).cuda()
            one = torch.from_numpy(rt.frustum_planes(wvp).reshape(1, 24)).cuda()
            stream.wait_stream(torch.cuda.current_stream())
            ks = {**auto, **{f"k{k}": rt.region_split(k) for k in (64, 1024, 4096)}}
            res = {}
            for tname, tri in (("boxes", 0), ("triangles", TRI)):
                for aname, acc in (("accept", 0), ("no_accept", NOACC)):
                    res[f"{tname}_{aname}"] = {
                        "single_frustum": compare(ctx, one, tri | acc, ks, f"one frustum {tname} {aname}"),
                        "tiles": compare(ctx, tiles, tri | acc, auto, f"tile frusta {tname} {aname}")}
            result["c_frustum"] = {"tiles_per_side": nt, **res}
            ctx.synchronize()
    if parts & {"a", "b"}:
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
            result["device"] = torch.cuda.get_device_name(0)
            if "b" in parts:
                ns = args.slabs
                z = torch.linspace(float(lo[2]), float(hi[2]), ns + 2, device="cuda")[1:-1]
                planes = torch.zeros((ns, 6, 4), dtype=torch.float32, device="cuda")
                planes[:, 0, 2], planes[:, 0, 3] = -1.0, z
                planes[:, 1, 2], planes[:, 1, 3] = 1.0, -z
                stream.wait_stream(torch.cuda.current_stream())
                result["b_slices"] = compare(ctx, planes.reshape(ns, 24), TRI, auto, "slabs")
                del planes
            if "a" in parts:   # region_bench's boxes, from the same generator
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
                h = args.extent * disp
                boxes = rt.make_boxes(near - h, near + h)
                planes = torch.zeros((n, 6, 4), dtype=torch.float32, device="cuda")   # box_region's planes
                for k in range(3):
                    planes[:, 2 * k, k], planes[:, 2 * k, 3] = -1.0, boxes[:, k]
                    planes[:, 2 * k + 1, k], planes[:, 2 * k + 1, 3] = 1.0, -boxes[:, 4 + k]
                regions = planes.reshape(n, 24)
                del planes, boxes, near
                stream.wait_stream(torch.cuda.current_stream())
                case = compare(ctx, regions, 0, auto, "boxes as regions")
                assert case["auto"]["split_counts"]["k"] == 1, case["auto"]["split_counts"]
                case["half_extent_in_displacements"] = args.extent
                result["a_boxes_as_regions"] = case
            ctx.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
