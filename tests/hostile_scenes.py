"""Scenes of hostile geometry (plain numpy + rt.Scene; used from CPU and GPU tests).  A helper, not a test.

The base is a wavy G x G grid of quads (2 G^2 triangles) over [-2.2, 2.2]^2 around z = 2, facing the camera: under
the reference camera of a 64 x 48 frame it fills most of the frame, under the identity a tenth of it, in front of the
primary rays' origins (z = 0) either way.  Its vertex coordinates are multiples of 2^-12, so the sum of two of them
is exact in fp32 and the midpoint of an edge is exactly collinear with it.

The hostile triangles are derived from randomly picked base triangles (A, B, C), so they lie on and near the surface,
where answers compete:

    points           three equal vertices: A (every other one displaced off the surface)
    needles          (A, A, B)
    collinear        (A, B, the exact midpoint of AB)
    duplicates       (A, B, C) again, as vertices of its own (no shared index: the copies are no index neighbours)
    reversed         (A, C, B)
    repeated-index   the index triple (i, i, j) of two base vertices
    slivers          (A, B, nextafter(midpoint of AB, C))
    denormal         (A, B, C) * 1e-41: every coordinate a denormal
    huge             (A, B, C) * 1e25: finite, every product of two coordinates overflows
    one-NaN          (A, B, C) with one component NaN, cycling through vertex and axis
    all-NaN          nine NaNs
    one-inf          (A, B, C) with one component +inf or -inf in turn, cycling through vertex and axis

(A camera matrix spreads a non-finite component: x * 0 is NaN for x = NaN or +-inf, so in BVH space a vertex with
one NaN component is NaN in all three, and one with an infinite component is infinite in that one and NaN in the
others.  That holds under the identity too.)

Every hostile triangle but the repeated-index ones owns its three vertices, so `clean` -- the same index buffer with
the source triangle's own positions in those slots -- is a well-formed scene of the same topology (the refit tests
move between the two).  The triangle order is shuffled: the classes spread over the ids and over the Morton order.

The query inputs of each kind come from the kind's own sampler, run on the FINITE PART of the BVH-space triangles
(finite, and not of the `huge` class: the samplers work in the root box, which is NaN, infinite or 1e25 wide
otherwise), plus inputs aimed at the hostile triangles: points at their vertices and box corners, rays through their
centroids and along needles, boxes around them, copies of them as triangle queries.
"""
import functools

import numpy as np

import raytracebvh_amd as rt
from tests import allhits_ref as ar
from tests import cross_ref as xr
from tests import nearest_ref as nr
from tests import overlap_ref as ovr
from tests import ray_walk_ref as rw

W, H = 64, 48
CLASSES = ["base", "points", "needles", "collinear", "duplicates", "reversed", "repeated-index", "slivers", "denormal",
           "huge", "one-NaN", "all-NaN", "one-inf"]
BASE = 0
COUNTS = {"points": 16, "needles": 16, "collinear": 16, "duplicates": 16, "reversed": 8, "repeated-index": 8,
          "slivers": 8, "denormal": 8, "huge": 8, "one-NaN": 12, "all-NaN": 4, "one-inf": 12}   # at G = 12
_FINITE = ["points", "needles", "collinear", "duplicates", "reversed", "repeated-index", "slivers", "denormal"]
_NONFINITE = ["one-NaN", "all-NaN", "one-inf"]
VARIANTS = {"degenerate": _FINITE, "huge": _FINITE + ["huge"], "nonfinite": _FINITE + _NONFINITE,
            "all": _FINITE + ["huge"] + _NONFINITE}
NONFINITE_VARIANTS = ("nonfinite", "all")
CAMERAS = ["reference", "identity"]
# classes whose triangles have an area to speak of (the winners the float64 sanity bound of test_hostile_cpu.py keeps)
WELL_FORMED = ("base", "duplicates", "reversed")


def cls(name):
    return CLASSES.index(name)


def camera(name, w=W, h=H):
    if name == "reference":
        return rt.camera_reference(w, h)
    return np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)


def _grid(G):
    """The wavy grid: ((G + 1)^2, 3) float32 vertices, multiples of 2^-12, and (2 G^2, 3) index triples."""
    s = np.linspace(-2.2, 2.2, G + 1)
    x, y = np.meshgrid(s, s, indexing="ij")
    z = 2.0 + 0.3 * np.sin(1.7 * x + 0.4) * np.cos(1.3 * y - 0.2)
    v = np.round(np.stack([x, y, z], -1).reshape(-1, 3) * 4096.0) / 4096.0
    i, j = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    a, b, c, d = (i * (G + 1) + j).ravel(), ((i + 1) * (G + 1) + j).ravel(), ((i + 1) * (G + 1) + j + 1).ravel(), \
        (i * (G + 1) + j + 1).ravel()
    return v.astype(np.float32), np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])


class Hostile:
    """scene, clean (the same indices over well-formed positions), labels (T,) (indices into CLASSES), and the
    positions (V, 3) of both."""

    def __init__(self, variant, G, seed):
        rng = np.random.default_rng(seed)
        gv, gi = _grid(G)
        mult = 8 if G >= 64 else 1     # COUNTS at G = 12, eight times them at G = 64
        pos, clean, idx, lab = [gv], [gv], [gi], [np.zeros(len(gi), np.int64)]
        nv = len(gv)
        f32 = np.float32
        for name in VARIANTS[variant]:
            n = COUNTS[name] * mult
            src = gi[rng.integers(0, len(gi), n)]
            A, B, C = gv[src[:, 0]], gv[src[:, 1]], gv[src[:, 2]]
            mid = ((A + B) * f32(0.5)).astype(f32)
            assert (mid.astype(np.float64) == (A.astype(np.float64) + B) / 2).all()    # exact
            k = np.arange(n)
            if name == "repeated-index":
                idx.append(np.stack([src[:, 0], src[:, 0], src[:, 1]], 1))
                lab.append(np.full(n, cls(name)))
                continue
            if name == "points":
                off = (rng.standard_normal((n, 3)) * 0.05).astype(f32) * (k % 2 == 1)[:, None].astype(f32)
                t = np.repeat((A + off).astype(f32)[:, None, :], 3, 1)
            elif name == "needles":
                t = np.stack([A, A, B], 1)
            elif name == "collinear":
                t = np.stack([A, B, mid], 1)
            elif name == "duplicates":
                t = np.stack([A, B, C], 1)
            elif name == "reversed":
                t = np.stack([A, C, B], 1)
            elif name == "slivers":
                t = np.stack([A, B, np.nextafter(mid, C)], 1)
            elif name == "denormal":
                t = (np.stack([A, B, C], 1).astype(np.float64) * 1e-41).astype(f32)
            elif name == "huge":
                t = (np.stack([A, B, C], 1).astype(np.float64) * 1e25).astype(f32)
            elif name == "one-NaN":
                t = np.stack([A, B, C], 1).copy()
                t[k, k % 3, (k // 3) % 3] = np.nan
            elif name == "all-NaN":
                t = np.full((n, 3, 3), np.nan, f32)
            elif name == "one-inf":
                t = np.stack([A, B, C], 1).copy()
                t[k, k % 3, (k // 3) % 3] = np.where(k % 2 == 0, np.inf, -np.inf)
            pos.append(t.reshape(-1, 3).astype(f32))
            clean.append(np.stack([A, B, C], 1).reshape(-1, 3))
            idx.append(nv + np.arange(3 * n).reshape(n, 3))
            nv += 3 * n
            lab.append(np.full(n, cls(name)))
        idx, lab = np.concatenate(idx), np.concatenate(lab)
        order = rng.permutation(len(idx))
        self.variant, self.G = variant, G
        self.indices = idx[order].reshape(-1).astype(np.uint32)
        self.labels = lab[order]
        self.positions = np.concatenate(pos).astype(f32)
        self.clean_positions = np.concatenate(clean).astype(f32)
        self.scene = scene_of(self.positions, self.indices)
        self.clean = scene_of(self.clean_positions, self.indices)
        self.T = len(self.labels)

    def tris(self, wvp, clean=False):
        """The BVH-space triangles (T, 3, 3)."""
        s = self.clean if clean else self.scene
        with np.errstate(all="ignore"):
            return rw.clip_triangles(s.vertices, s.indices, wvp)


def scene_of(positions, indices):
    """collide_ref.scene_of's scene (positions, one grey material) with every vertex normal tilted a little off -z:
    a primary ray's reflection then has no zero component, so the certified bounce walk takes it (cert_scenes.py)."""
    from tests.collide_ref import scene_of as bare
    s = bare(positions, indices)
    k = np.arange(len(positions), dtype=np.float64)
    n = np.stack([0.08 * np.sin(0.7 * k + 0.3), 0.08 * np.cos(1.1 * k), -np.ones(len(k))], 1)
    v = s.vertices.copy()
    v[:, 3:6] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return rt.Scene(v, s.indices, s.mat_indices, s.materials)


@functools.lru_cache(maxsize=None)
def hostile(variant, G=12, seed=1):
    """The scene of a variant: a Hostile (scene, labels, ...).  Cached: treat it as read-only."""
    return Hostile(variant, G, seed)


def finite_part(tris, labels):
    """The mask of the triangles the samplers run on: finite in BVH space and not of the `huge` class."""
    return np.isfinite(tris).all((1, 2)) & (labels != cls("huge"))


def _aimed(tris, labels, limit, rng):
    """Up to `limit` hostile triangles with finite BVH-space vertices, spread over the classes."""
    ok = np.nonzero((labels != BASE) & np.isfinite(tris).all((1, 2)))[0]
    return ok if len(ok) <= limit else np.sort(rng.choice(ok, limit, replace=False))


class Inputs:
    """The query inputs of every kind for (T, 3, 3) BVH-space triangles with labels: a few hundred of each."""

    def __init__(self, tris, labels, seed=3):
        rng = np.random.default_rng(seed)
        fin = tris[finite_part(tris, labels)]
        hostile_ids = np.nonzero(labels != BASE)[0]
        # points: the sampler's, then every finite vertex and box corner of (a sample of) the hostile triangles --
        # the finite corners of non-finite ones too: the clamp sends a NaN closest point there
        lo = np.fmin(np.fmin(tris[:, 0], tris[:, 1]), tris[:, 2])
        hi = np.fmax(np.fmax(tris[:, 0], tris[:, 1]), tris[:, 2])
        pick = hostile_ids if len(hostile_ids) <= 160 else np.sort(rng.choice(hostile_ids, 160, replace=False))
        extra = np.concatenate([tris[pick].reshape(-1, 3), lo[pick], hi[pick]])
        extra = extra[np.isfinite(extra).all(1)]
        extra = extra[np.sort(np.unique(extra, axis=0, return_index=True)[1])][:320]
        self.points = np.concatenate([nr.sample_points(fin, seed, n_random=192, n_each=32)[0], extra]).astype(np.float32)
        # rays: the sampler's, then rays through the centroids of hostile triangles and along their first edge
        aim = _aimed(tris, labels, 96, rng)
        o, d = ar.sample_rays(fin, 192, 24, 96, 16, seed=seed)
        cen = ((tris[aim, 0] + tris[aim, 1] + tris[aim, 2]) / np.float32(3)).astype(np.float32)
        cd = rng.standard_normal((len(aim), 3)).astype(np.float32)
        cd /= np.sqrt((cd * cd).sum(1, keepdims=True))
        edge = (tris[aim, 1] - tris[aim, 0]).astype(np.float32)
        edge = np.where((edge == 0).all(1, keepdims=True), tris[aim, 2] - tris[aim, 0], edge).astype(np.float32)
        with np.errstate(all="ignore"):
            self.ray_o = np.concatenate([o, (cen - np.float32(3) * cd), (tris[aim, 0] - edge)]).astype(np.float32)
        self.ray_d = np.concatenate([d, cd, edge]).astype(np.float32)
        # boxes: the sampler's, then the boxes of hostile triangles, exact and grown
        qlo, qhi = ovr.sample_boxes(fin, seed, n_random=160, n_each=24)
        grow = np.float32(0.02)
        self.qlo = np.concatenate([qlo, lo[aim], lo[aim] - grow]).astype(np.float32)
        self.qhi = np.concatenate([qhi, hi[aim], hi[aim] + grow]).astype(np.float32)
        # triangle queries: the sampler's, then copies of hostile triangles (a few non-finite ones: no walk)
        bad = np.nonzero(~np.isfinite(tris).all((1, 2)))[0][:8]
        self.queries = np.concatenate([xr.random_queries(fin, n=192, seed=seed), tris[aim], tris[bad]]).astype(np.float32)


def oracle_scene(s):
    from oracle import lib as orc
    return orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob)


# ---------------------------------------------------------------- what the references answer, by class
WITHIN_BOUND = np.float32(0.05)     # lists about ten triangles a point at G = 64, about four at G = 12
KNN_K, KHITS_K = 8, 4


def reference_answers(tris, labels, indices, nodes, inp):
    """{kind: (ids, can)} from the restatements alone: `ids`, the triangle ids of the kind's answers over `inp` (the
    brute forces; for `query` the walk of the oracle's `nodes`), and `can`, the set of classes the kind's restatement
    can return at all on these inputs -- the classes with at least one (input, triangle) pair that passes the kind's
    membership conditions when the pair is evaluated on its own, whatever the other triangles do."""
    from tests import collide_ref as cr
    from tests import khits_ref as kh
    from tests import knn_ref as kr
    from tests import signed_ref as sr
    from tests import within_ref as wr
    T = len(tris)
    rank = wr.rank_of(nodes["index"][:T] // 3)
    out = {}

    def classes(mask_by_tri):
        return set(labels[np.asarray(mask_by_tri)].tolist())

    def real(ids):
        ids = np.asarray(ids).ravel()
        return ids[ids != 0xFFFFFFFF].astype(np.int64)

    # the point kinds: a pair is returnable when its dist2 is no NaN
    d, finite = kr.dist2_matrix(tris, inp.points)
    can = classes(~np.isnan(d[finite]).all(0))
    near = nr.brute(tris, inp.points)
    out["nearest"] = (real(near["tri"]), can)
    out["knn"] = (real(kr.select_k(d, finite, KNN_K)[0]), can)
    with np.errstate(all="ignore"):
        out["within"] = (real(wr.brute_within(tris, inp.points, WITHIN_BOUND, rank)[1]["tri"]),
                         classes((d[finite] <= WITHIN_BOUND).any(0)))
    out["signed"] = (real(sr.brute(tris, inp.points, vote3=True)["tri"]), can)
    # the ray kinds: a pair is returnable when the leaf box and the triangle test accept it
    n = len(inp.ray_o)
    k, t = np.repeat(np.arange(n), T), np.tile(np.arange(T), n)
    ok = ar.pair_tests(tris, t, inp.ray_o[k], inp.ray_d[k], ar.INF)[0].reshape(n, T)
    can = classes(ok.any(0))
    out["allhits"] = (real(ar.brute_allhits(tris, inp.ray_o, inp.ray_d, ar.INF, rank)[1]["tri"]), can)
    out["khits"] = (real(kh.brute_k(tris, inp.ray_o, inp.ray_d, KHITS_K)["tri"]), can)
    out["query"] = (real(rw.walk(nodes, tris, inp.ray_o, inp.ray_d)["tri"]), can)
    # the box and triangle kinds: the lists are the member pairs
    lo, hi = nr.leaf_data(tris)[3:]
    walk = ovr.valid_boxes(inp.qlo, inp.qhi)
    meet = ovr.boxes_meet(inp.qlo[walk, None], inp.qhi[walk, None], lo[None], hi[None])
    out["overlap"] = (real(ovr.brute_overlap(tris, inp.qlo, inp.qhi, rank)[1]), classes(meet.any(0)))
    kk, jj = np.nonzero(meet)
    a, e1, e2 = nr.leaf_data(tris)[:3]
    tm = ovr.triangle_meets(inp.qlo[walk][kk], inp.qhi[walk][kk], a[jj], e1[jj], e2[jj])
    out["overlap-triangle"] = (real(ovr.brute_overlap(tris, inp.qlo, inp.qhi, rank, True)[1]),
                               classes(np.bincount(jj[tm], minlength=T) > 0))
    kq, jq = xr.member_pairs(tris, inp.queries)
    out["cross"] = (real(xr.brute_cross(tris, inp.queries, rank)[1]), classes(np.bincount(jq, minlength=T) > 0))
    for name, tri in (("collide", False), ("collide-triangle", True)):
        x, y = cr.member_pairs(tris, indices, tri)
        out[name] = (real(cr.csr((x, y), rank, T, True)[1]),
                     classes(np.bincount(np.concatenate([x, y]), minlength=T) > 0))
    return out


def hostile_share(ids, labels):
    ids = np.asarray(ids)
    return float((labels[ids] != BASE).mean()) if len(ids) else 0.0
