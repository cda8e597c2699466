"""Region query throughput on the C5 scene.

    python scripts/region_bench.py [--out profiles/region_bench.json] [--reps 5] [--extents 4,10] [--parts a,b,c]

One process, HIP events, the median of `reps` repetitions after one warm-up, min-max recorded.

  (a) against overlap: scripts/overlap_bench.py's boxes (the primary rays' hit points displaced by `--displace` of the
      root box's diagonal, half-extent h displacements) as six axis planes each (box_region's planes, made on the
      device).  Sizes / fill / one call, taking subtrees whole (the default) and with REGION_NO_ACCEPT, beside
      Context.overlap's three on the same boxes; the lists must have overlap's offsets and order-sensitive digest.
      One REGION_COUNT call per form gives the steps and accepts per region.
  (b) slicing: `--slabs` zero-thickness slabs across C5's root box along z with REGION_TRIANGLE.
  (c) frustum: C5 built under the identity camera, the reference camera's frustum split into `--tiles` x `--tiles`
      sub-frusta (one region each), and the whole frustum as one region (one lane walks it: latency-bound).

Writes ms, Mregions/s, Mids/s, ids and steps per region as JSON.  No gate.  Not part of bench.py.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "region_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ntris", type=int, default=10_000_000)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--displace", type=float, default=1e-3)
    ap.add_argument("--extents", default="4,10", help="half-extents in displacements, comma-separated")
    ap.add_argument("--slabs", type=int, default=4096)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--parts", default="a,b,c")
    args = ap.parse_args()
    extents = [float(r) for r in args.extents.split(",")]
    parts = set(args.parts.split(","))

    import torch

    import raytracebvh_amd as rt

    L = rt.lib()
    W, H = args.width, args.height
    scene = rt.synthetic(args.ntris, seed=0x5EED0005, half_extent=(100.0, 100.0, 50.0))
    wvp, wv = rt.camera_reference(W, H)
    stream = torch.cuda.Stream()
    sh = ctypes.c_void_p(stream.cuda_stream)
    NOACC, TRI, SIZES, FILL, COUNT = (rt.REGION_NO_ACCEPT, rt.REGION_TRIANGLE, rt.REGION_SIZES, rt.REGION_FILL,
                                      rt.REGION_COUNT)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    def note(*what):   # progress, on stderr: the result line stays alone on stdout
        print("region_bench:", *what, file=sys.stderr, flush=True)

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

    def figures(ms, n, total):
        med = float(np.median(ms))
        return {"ms": [round(v, 4) for v in ms], "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "ms_median": round(med, 4), "mregions_per_s": round(n / med / 1e3, 3),
                "mids_per_s": round(total / med / 1e3, 1)}

    def measure(ctx, regions, tri, with_no_accept=True):
        """sizes / fill / one call of `regions` ((n, 24) device tensor) with and without accepts, and the counts."""
        n = int(regions.shape[0])
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def region(ids, mode):
            st = L.rtbvh_region_async(ctx._h, ptr(regions), n, ptr(offsets), ptr(ids), 0 if ids is None else ids.shape[0],
                                      mode | tri, sh)
            assert st == 0, st

        region(None, SIZES)
        stream.synchronize()
        total = int(offsets[n].item())
        ids = torch.empty(total, dtype=torch.int32, device="cuda")
        out = {"regions": n, "ids": total, "ids_per_region": round(total / max(n, 1), 3)}
        first = None
        for label, acc in (("accept", 0), ("no_accept", NOACC)) if with_no_accept else (("accept", 0),):
            sub = {}
            runs = {"sizes": lambda: region(None, SIZES | acc), "fill": lambda: region(ids, FILL | acc),
                    "both": lambda: region(ids, acc)}
            for name, f in runs.items():
                sub[name] = figures(timed(f), n, total)
                note(n, "regions", total, "ids", label, name, sub[name]["ms_median"], "ms")
            got = (offsets.clone(), digest(ids))
            if first is None:
                first = got
            else:   # the same output, byte for byte
                assert torch.equal(got[0], first[0]) and got[1] == first[1], label
            ids.zero_()
            region(ids, COUNT | acc)
            stream.synchronize()
            c = ctx.region_counts()
            assert c["regions"] == n and c["ids"] == total, c
            sub["both_steps_per_region"] = {k: round(v / max(n, 1), 3) for k, v in c.items() if k not in ("regions", "ids")}
            sub["ids_from_accepts"] = round(c["accepted_ids"] / max(total, 1), 4)
            out[label] = sub
            ids.zero_()
            torch.cuda.synchronize()
        return out, first[0], first[1]

    result = {
        "workload": f"C5: synthetic {args.ntris} tris (seed 0x5EED0005, box 100x100x50), node records",
        "library": os.environ.get("RTBVH_LIB", "librtbvh.so"),
        "reps": args.reps,
    }
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
            if "a" in parts:
                # overlap_bench's boxes, from the same generator
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
                stream.wait_stream(torch.cuda.current_stream())
                cases = {}
                for r in extents:
                    h = r * disp
                    boxes = rt.make_boxes(near - h, near + h)
                    planes = torch.zeros((n, 6, 4), dtype=torch.float32, device="cuda")   # box_region's planes
                    for k in range(3):
                        planes[:, 2 * k, k], planes[:, 2 * k, 3] = -1.0, boxes[:, k]
                        planes[:, 2 * k + 1, k], planes[:, 2 * k + 1, 3] = 1.0, -boxes[:, 4 + k]
                    regions = planes.reshape(n, 24)
                    del planes
                    case, off_r, dig_r = measure(ctx, regions, 0)
                    case["half_extent_in_displacements"] = r
                    del regions
                    # overlap itself on the same boxes
                    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
                    total = case["ids"]
                    ids = torch.empty(total, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()

                    def overlap(ids_, mode):
                        st = L.rtbvh_overlap_async(ctx._h, ptr(boxes), n, ptr(offsets), ptr(ids_),
                                                   0 if ids_ is None else ids_.shape[0], mode, sh)
                        assert st == 0, st

                    ov = {}
                    for name, f in {"sizes": lambda: overlap(None, rt.OVERLAP_SIZES),
                                    "fill": lambda: overlap(ids, rt.OVERLAP_FILL), "both": lambda: overlap(ids, 0)}.items():
                        ov[name] = figures(timed(f), n, total)
                        note(n, "boxes", total, "ids", "overlap", name, ov[name]["ms_median"], "ms")
                    assert torch.equal(offsets, off_r) and digest(ids) == dig_r, "region lists differ from overlap's"
                    overlap(ids, rt.OVERLAP_COUNT)
                    stream.synchronize()
                    c = ctx.overlap_counts()
                    ov["both_steps_per_box"] = {k: round(c[k] / n, 3) for k in ("internal_steps", "leaf_steps")}
                    case["overlap"] = ov
                    for name in ("sizes", "fill", "both"):
                        case[f"accept_over_overlap_{name}"] = round(case["accept"][name]["ms_median"] / ov[name]["ms_median"], 3)
                        case[f"no_accept_over_overlap_{name}"] = round(case["no_accept"][name]["ms_median"] / ov[name]["ms_median"], 3)
                    cases[f"h{r:g}"] = case
                    del ids, offsets, boxes, off_r
                    torch.cuda.synchronize()
                result["a_boxes_as_regions"] = {"boxes": n, "displacement": round(disp, 6), "cases": cases}
                del near
            if "b" in parts:
                ns = args.slabs
                z = torch.linspace(float(lo[2]), float(hi[2]), ns + 2, device="cuda")[1:-1]
                planes = torch.zeros((ns, 6, 4), dtype=torch.float32, device="cuda")
                planes[:, 0, 2], planes[:, 0, 3] = -1.0, z
                planes[:, 1, 2], planes[:, 1, 3] = 1.0, -z
                stream.wait_stream(torch.cuda.current_stream())
                case, _, _ = measure(ctx, planes.reshape(ns, 24), TRI)
                result["b_slices"] = case
            ctx.synchronize()
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
            res = {}
            for tname, tri in (("boxes", 0), ("triangles", TRI)):
                case, _, _ = measure(ctx, tiles, tri)
                single, _, _ = measure(ctx, one, tri)
                res[tname] = {"tiles": case, "single_frustum": single}
            result["c_frustum"] = {"tiles_per_side": nt, **res}
            ctx.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
