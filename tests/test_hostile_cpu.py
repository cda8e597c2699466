"""The hostile scenes (tests/hostile_scenes.py) without a GPU: by the references alone, that the scenes can expose a
wrong kernel -- the conditions tests/test_hostile_gpu.py rests on.  Every class of hostile triangle that a query kind
can return is returned; the oracle's tree over them is a tree; a restatement with a mistake a kernel could make
(NaN-keeping min / max, no NaN -> 0 rule, negated comparisons, an open interval) answers differently here and the same
on the golden scenes -- each test says on which variants, and the open interval's says why the golden scenes do tell
it; and the float32 restatement stays accurate where the winner has an area.

Also here: oracle/lib.py's lib() builds a missing liboracle.so (on a temporary copy of oracle/)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import lib as orc
from tests import allhits_ref as ar
from tests import hostile_scenes as hs
from tests import nearest_ref as nr
from tests import overlap_ref as ovr
from tests import ray_walk_ref as rw
from tests.conftest import REPO, load_scene_fixture
from tests.test_nearest_cpu import MEASURED_WORST

GOLDEN = ["Test", "Rect", "Image_Test"]
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module", params=[(v, c) for v in hs.VARIANTS for c in hs.CAMERAS], ids=lambda p: "-".join(p))
def case(request):
    """A variant at G = 12 under one camera: the Hostile, its BVH-space triangles, the oracle's tree and the inputs."""
    variant, cam = request.param
    h = hs.hostile(variant)
    wvp, _ = hs.camera(cam)
    tris = h.tris(wvp)
    nodes = orc.build(hs.oracle_scene(h.scene), wvp)
    return h, wvp, tris, nodes, hs.Inputs(tris, h.labels)


# ---------------------------------------------------------------- 1. the scenes
def test_scene_shape():
    for variant, names in hs.VARIANTS.items():
        h = hs.hostile(variant)
        assert h.T == 288 + sum(hs.COUNTS[n] for n in names)
        counts = np.bincount(h.labels, minlength=len(hs.CLASSES))
        assert counts[hs.BASE] == 288
        for n in names:
            assert counts[hs.cls(n)] == hs.COUNTS[n]
        where = np.nonzero(h.labels != hs.BASE)[0]
        assert (np.bincount(where * 8 // h.T, minlength=8) >= 4).all()      # shuffled over the ids
        # `clean` is the same topology over well-formed positions (the repeated-index triples aside)
        assert np.isfinite(h.clean_positions).all() and np.abs(h.clean_positions).max() < 4
        t = h.tris(np.eye(4, dtype=np.float32), clean=True)
        area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
        assert (area[h.labels != hs.cls("repeated-index")] > 1e-3).all()
        if variant in hs.NONFINITE_VARIANTS:
            assert not np.isfinite(h.positions).all()
        else:
            assert np.isfinite(h.positions).all()
    big = hs.hostile("all", 64)
    assert big.T == 8192 + 8 * sum(hs.COUNTS.values())


def test_reference_camera_frame_hits_the_base():
    """The oracle's 64 x 48 frame under the reference camera hits the scene in at least a tenth of the pixels, with
    no NaN pixel and no stack overflow, for every variant."""
    wvp, wv = hs.camera("reference")
    for variant in hs.VARIANTS:
        h = hs.hostile(variant)
        osc = hs.oracle_scene(h.scene)
        fb, _, st = orc.trace(osc, orc.build(osc, wvp), wvp, wv, hs.W, hs.H, 1)
        assert st["hits"] >= hs.W * hs.H // 10 and st["stack_overflows"] == 0
        assert not np.isnan(fb).any()


# ---------------------------------------------------------------- 2. every class appears
def test_every_returnable_class_is_returned(case):
    """For every kind: each class that the kind's restatement can return at all (hostile_scenes.reference_answers,
    pair by pair) is among the kind's answers at least once, and the hostile share of the answers is not zero."""
    h, wvp, tris, nodes, inp = case
    got = hs.reference_answers(tris, h.labels, h.indices, nodes, inp)
    assert set(got) == {"nearest", "knn", "within", "signed", "allhits", "khits", "query", "overlap",
                        "overlap-triangle", "cross", "collide", "collide-triangle"}
    for kind, (ids, can) in got.items():
        share = hs.hostile_share(ids, h.labels)
        print(f"{h.variant} {kind}: {len(ids)} answers, {100 * share:.1f}% hostile, classes "
              f"{sorted(hs.CLASSES[c] for c in can)}")
        counts = np.bincount(h.labels[ids], minlength=len(hs.CLASSES))
        assert hs.BASE in can and len(can) >= 3, kind
        for c in can:
            assert counts[c] >= 1, f"{kind}: no answer of class {hs.CLASSES[c]}"
        assert set(np.nonzero(counts)[0].tolist()) <= can, kind          # (and nothing that no pair can give)
        assert share > 0, kind
    # the point kinds reach every class but the all-NaN one, the box kinds' boxes every class with a box
    finite_classes = {hs.cls(n) for n in hs.VARIANTS[h.variant] if n != "all-NaN"} | {hs.BASE}
    assert got["nearest"][1] == finite_classes and got["overlap"][1] == finite_classes


# ---------------------------------------------------------------- 3. the oracle's tree
@pytest.mark.parametrize("morton", [orc.MORTON_CPUTESTS, orc.MORTON_HLSL], ids=["cputests", "hlsl"])
def test_oracle_tree_is_valid(case, morton):
    """Every node has one parent; the NaN-boxed nodes are exactly the all-NaN leaves and the internal nodes whose
    whole subtree is all-NaN."""
    h, wvp, tris, _, _ = case
    T = h.T
    nodes = orc.build(hs.oracle_scene(h.scene), wvp, morton_mode=morton)
    assert len(nodes) == 2 * T - 1
    leaf = (nodes["child_l"] == NONE) & (nodes["child_r"] == NONE)
    assert leaf[:T].all() and not leaf[T:].any()
    kids = np.concatenate([nodes["child_l"][T:], nodes["child_r"][T:]]).astype(np.int64)
    assert np.array_equal(np.sort(kids), np.delete(np.arange(2 * T - 1), T))       # every node but the root, once
    parent_of = np.full(2 * T - 1, NONE, np.int64)
    parent_of[nodes["child_l"][T:].astype(np.int64)] = np.arange(T, 2 * T - 1)
    parent_of[nodes["child_r"][T:].astype(np.int64)] = np.arange(T, 2 * T - 1)
    np.testing.assert_array_equal(nodes["parent"].astype(np.int64), parent_of)
    assert np.array_equal(np.sort(nodes["index"][:T] // 3), np.arange(T))           # every triangle in one leaf
    # all-NaN below: leaves by class, internal nodes bottom-up (a child's depth is below its parent's: climb by rounds)
    below = np.zeros(2 * T - 1, bool)
    below[:T] = h.labels[nodes["index"][:T] // 3] == hs.cls("all-NaN")
    done = leaf.copy()
    cl, cr_ = nodes["child_l"].astype(np.int64), nodes["child_r"].astype(np.int64)
    for _ in range(2 * T):
        ready = ~done & ~leaf
        ready[T:] &= done[cl[T:]] & done[cr_[T:]]
        if not ready.any():
            break
        below[ready] = below[cl[ready]] & below[cr_[ready]]
        done |= ready
    assert done.all()                                                               # no cycle: the climb ends
    nan_box = np.isnan(nodes["bb_min"]).any(1) | np.isnan(nodes["bb_max"]).any(1)
    np.testing.assert_array_equal(nan_box, below)
    assert int(nan_box.sum()) >= (4 if h.variant in hs.NONFINITE_VARIANTS else 0)
    if h.variant in hs.NONFINITE_VARIANTS:
        root = nodes[T]
        assert np.isinf(root["bb_min"]).all() and np.isinf(root["bb_max"]).all()
    else:
        assert np.isfinite(nodes["bb_min"]).all() and np.isfinite(nodes["bb_max"]).all()


# ---------------------------------------------------------------- 4. mutations a kernel could carry
def tri_dist2_copy(p, a, e1, e2, lo, hi, fmin=np.fmin, fmax=np.fmax, nan_to_zero=True):
    """A copy of nearest_ref.tri_dist2 (dist2 only) with its two NaN rules as parameters: the clamp's min / max
    (np.fmin / np.fmax drop a NaN as fminf / fmaxf do; np.minimum / np.maximum keep it) and `u, v: NaN -> 0`."""
    f = p.dtype.type
    p, a, e1, e2, lo, hi = (nr._split(x) for x in (p, a, e1, e2, lo, hi))
    dot = nr._dot
    with np.errstate(all="ignore"):
        ap = tuple(p[k] - a[k] for k in range(3))
        d1, d2 = dot(e1, ap), dot(e2, ap)
        e11, e12, e22 = dot(e1, e1), dot(e1, e2), dot(e2, e2)
        d3, d4, d5, d6 = d1 - e11, d2 - e12, d1 - e12, d2 - e22
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        den = f(1) / ((va + vb) + vc)
        u, v = vb * den, vc * den
        w = d43 / (d43 + d56)
        r = (va <= 0) & (d43 >= 0) & (d56 >= 0)
        u, v = np.where(r, f(1) - w, u), np.where(r, w, v)
        r = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        u, v = np.where(r, f(0), u), np.where(r, d2 / (d2 - d6), v)
        r = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        u, v = np.where(r, d1 / (d1 - d3), u), np.where(r, f(0), v)
        r = (d6 >= 0) & (d5 <= d6)
        u, v = np.where(r, f(0), u), np.where(r, f(1), v)
        r = (d3 >= 0) & (d4 <= d3)
        u, v = np.where(r, f(1), u), np.where(r, f(0), v)
        r = (d1 <= 0) & (d2 <= 0)
        u, v = np.where(r, f(0), u), np.where(r, f(0), v)
        if nan_to_zero:
            u = np.where(np.isnan(u), f(0), u)
            v = np.where(np.isnan(v), f(0), v)
        q = tuple(fmax(lo[k], fmin(hi[k], (a[k] + e1[k] * u) + e2[k] * v)) for k in range(3))
        e = tuple(p[k] - q[k] for k in range(3))
        return dot(e, e)


POINT_MUTANTS = {"NaN-keeping clamp": dict(fmin=np.minimum, fmax=np.maximum), "no NaN -> 0": dict(nan_to_zero=False)}


def nearest_answers(tris, pts, **mutant):
    """(tri, dist2 bits) of every point with tri_dist2_copy: the (dist2, id) minimum, a NaN dist2 never winning."""
    a, e1, e2, lo, hi = nr.leaf_data(tris)
    d = tri_dist2_copy(pts[:, None, :], a[None], e1[None], e2[None], lo[None], hi[None], **mutant)
    dk = np.where(np.isnan(d), np.float32(np.inf), d)
    tri = np.argmin(dk, 1)
    return tri, nr.bits(d[np.arange(len(pts)), tri]), d


def changed(x, y):
    return int(((x[0] != y[0]) | (x[1] != y[1])).sum())


def golden_tris(name, cam):
    d = load_scene_fixture(name)
    return rw.clip_triangles(d["vertices"], d["indices"], hs.camera(cam)[0]), d


def test_the_copy_is_the_restatement(case):
    h, wvp, tris, nodes, inp = case
    tri, bits, d = nearest_answers(tris, inp.points)
    a, e1, e2, lo, hi = nr.leaf_data(tris)
    want = nr.tri_dist2(inp.points[:, None, :], a[None], e1[None], e2[None], lo[None], hi[None])[0]
    np.testing.assert_array_equal(nr.bits(d), nr.bits(want))
    ref = nr.brute(tris, inp.points)
    np.testing.assert_array_equal(tri, ref["tri"])
    np.testing.assert_array_equal(bits, nr.bits(ref["dist2"]))


@pytest.mark.parametrize("mutant", list(POINT_MUTANTS))
def test_point_mutants_change_hostile_answers(case, mutant):
    """Closest-point answers under each of the two mistakes.  Without the `NaN -> 0` rule answers change on every
    variant (0 / 0 barycentrics of needles, collinear and point triangles).  The NaN-keeping clamp changes answers
    where a vertex is not finite (`nonfinite`, `all`) and ONLY there: once u and v are no NaN the closest point is
    a finite combination of finite vectors unless u or v is infinite, which takes a face denominator that cancels
    to exactly 0 under a nonzero numerator -- no (point, triangle) pair of `degenerate` or `huge` does that (nor
    any of 600,000 random points about their slivers, needles and collinear triangles), so there the two clamps
    agree and a kernel with this mistake cannot be told from a right one: asserted as found."""
    h, wvp, tris, nodes, inp = case
    good = nearest_answers(tris, inp.points)
    n = changed(good, nearest_answers(tris, inp.points, **POINT_MUTANTS[mutant]))
    print(f"{h.variant}: {mutant} changes {n} of {len(inp.points)} answers")
    if mutant == "NaN-keeping clamp" and h.variant not in hs.NONFINITE_VARIANTS:
        assert n == 0
    else:
        assert n > 0


@pytest.mark.parametrize("cam", hs.CAMERAS)
@pytest.mark.parametrize("name", GOLDEN)
def test_point_mutants_leave_the_golden_scenes_alone(name, cam):
    tris, _ = golden_tris(name, cam)
    pts = nr.sample_points(tris)[0]
    good = nearest_answers(tris, pts)
    for mutant, kw in POINT_MUTANTS.items():
        assert changed(good, nearest_answers(tris, pts, **kw)) == 0, mutant


def tri_test_negated(tris, tri, o, d):
    """ray_walk_ref.tri_test with every comparison written as the negated opposite one: !(a < b) as a >= b, a < b as
    !(a >= b).  The same for ordered operands; a NaN operand turns each around."""
    EPS, _dot, _cross = rw.EPS, rw._dot, rw._cross
    with np.errstate(all="ignore"):
        p = tris[tri]
        p0 = p[:, 0]
        e1, e2 = p[:, 1] - p0, p[:, 2] - p0
        tmp = _cross(d, e2)
        dx = _dot(e1, tmp)
        ok = np.abs(dx) >= EPS
        idx = np.float32(1) / dx
        rt_ = o - p0
        u = _dot(rt_, tmp) * idx
        ok &= (u >= 0) & (np.float32(1) >= u)
        tmp = _cross(rt_, e1)
        v = _dot(d, tmp) * idx
        ok &= (v >= 0) & (np.float32(1) >= u + v)
        t = _dot(e2, tmp) * idx
        ok &= ~(EPS >= t)
    return np.where(ok, t, np.float32(-1)).astype(np.float32), u.astype(np.float32), v.astype(np.float32)


def ray_members(tris, o, d, test):
    """(n, T) bool and float32: which (ray, triangle) pairs `test` accepts, and their t (all-hits' condition (T))."""
    n, T = len(o), len(tris)
    k, j = np.repeat(np.arange(n), T), np.tile(np.arange(T), n)
    t = test(tris, j, o[k], d[k])[0]
    return (t != -1).reshape(n, T), rw.bits(t).reshape(n, T)


def test_negated_comparisons_change_the_ray_answers(case):
    """The ray side's pair.  The two forms differ only where an operand is a NaN, and then the original accepts
    at each of the first three tests and rejects at the last (`EPS < t`), the negated form the other way round.  So
    they part only where `t` is a NaN after three tests on ordered operands: products that overflow (`huge`, `all`
    -- also for base triangles, under the rays aimed at the huge ones from 1e25 away).  With finite products no
    operand is a NaN (`degenerate`), and a NaN or infinite vertex makes the determinant a NaN, or infinite with a
    NaN u or v, or t = 0 (`nonfinite`): there both forms reject the same pairs, asserted."""
    h, wvp, tris, nodes, inp = case
    w = ar.walked(inp.ray_o, inp.ray_d, ar.INF)
    good = ray_members(tris, inp.ray_o[w], inp.ray_d[w], rw.tri_test)
    bad = ray_members(tris, inp.ray_o[w], inp.ray_d[w], tri_test_negated)
    n = int((good[0] != bad[0]).sum())
    by_class = np.bincount(h.labels[np.nonzero(good[0] != bad[0])[1]], minlength=len(hs.CLASSES))
    print(f"{h.variant}: negated comparisons change {n} of {good[0].size} (ray, triangle) pairs, by class {by_class}")
    if "huge" in hs.VARIANTS[h.variant]:
        assert n > 0
    else:
        assert n == 0


@pytest.mark.parametrize("cam", hs.CAMERAS)
@pytest.mark.parametrize("name", GOLDEN)
def test_negated_comparisons_leave_the_golden_scenes_alone(name, cam):
    tris, _ = golden_tris(name, cam)
    o, d = ar.sample_rays(tris, 192, 24, 96, 16)
    walked = ar.walked(o, d, ar.INF)                       # (the sampler's six degenerate rays are never walked)
    good = ray_members(tris, o[walked], d[walked], rw.tri_test)
    bad = ray_members(tris, o[walked], d[walked], tri_test_negated)
    np.testing.assert_array_equal(good[0], bad[0])
    np.testing.assert_array_equal(good[1][good[0]], bad[1][good[0]])


def boxes_meet_open(qlo, qhi, lo, hi):
    """overlap_ref.boxes_meet with < for <=."""
    with np.errstate(all="ignore"):
        return ((qlo < hi) & (lo < qhi)).all(-1)


def box_pairs_changed(tris, qlo, qhi):
    lo, hi = nr.leaf_data(tris)[3:]
    walk = ovr.valid_boxes(qlo, qhi)
    a = ovr.boxes_meet(qlo[walk, None], qhi[walk, None], lo[None], hi[None])
    b = boxes_meet_open(qlo[walk, None], qhi[walk, None], lo[None], hi[None])
    return int((a != b).sum()), int(a.sum())


def test_open_intervals_change_the_box_answers(case):
    h, wvp, tris, nodes, inp = case
    n, total = box_pairs_changed(tris, inp.qlo, inp.qhi)
    print(f"{h.variant}: open intervals drop {n} of {total} (box, triangle) pairs")
    assert n > 0


@pytest.mark.parametrize("cam", hs.CAMERAS)
@pytest.mark.parametrize("name", GOLDEN)
def test_open_intervals_on_the_golden_scenes(name, cam):
    """The `no change` half does NOT hold for the box side on the golden scenes: overlap_ref.sample_boxes centres
    every fourth box, a point box, on a sampled point, and 64 of those points are mesh vertices -- such a box touches
    the leaf boxes of the vertex's triangles in a face, which only the closed test lists.  (The existing overlap
    tests catch this mistake already; here it is pinned as what it is.)  Away from the point and flat boxes (classes
    1 and 2 of the sampler) the open and closed tests do agree on these scenes."""
    tris, _ = golden_tris(name, cam)
    qlo, qhi = ovr.sample_boxes(tris, 5)
    n, total = box_pairs_changed(tris, qlo, qhi)
    assert 0 < n < total
    fat = np.isin(np.arange(len(qlo)) % 4, (0, 3))
    assert box_pairs_changed(tris, qlo[fat], qhi[fat])[0] == 0


# ---------------------------------------------------------------- 5. accuracy where the winner has an area
@pytest.mark.parametrize("cam", hs.CAMERAS)
def test_restatement_is_accurate_where_the_winner_is_well_formed(cam):
    """tests/test_nearest_cpu.py's bound -- the float32 winner's distance against the smallest distance of a float64
    evaluation of the same formulas, 4 x 98.5 x 2^-24 of the root box's diagonal -- on `degenerate`, over the points
    whose float32 winner is a base triangle or a copy of one."""
    h = hs.hostile("degenerate")
    tris = h.tris(hs.camera(cam)[0])
    pts = hs.Inputs(tris, h.labels).points
    want = nr.brute(tris, pts)
    keep = np.isin(h.labels[want["tri"]], [hs.cls(n) for n in hs.WELL_FORMED])
    assert keep.sum() >= 200 and (~keep).sum() >= 50
    a, e1, e2, lo, hi = nr.leaf_data(tris, np.float64)
    d64 = nr.tri_dist2(pts.astype(np.float64)[:, None, :], a[None], e1[None], e2[None], lo[None], hi[None])[0]
    rlo, rhi = nr.root_box(tris)
    diag = float(np.sqrt(((rhi.astype(np.float64) - rlo) ** 2).sum()))
    err = np.abs(np.sqrt(want["dist2"].astype(np.float64)) - np.sqrt(np.nanmin(d64, 1))) / diag * 2.0 ** 24
    print(f"worst error, well-formed winners: {err[keep].max():.2f}; others: {err[~keep].max():.2f} (x 2^-24 diagonal)")
    assert err[keep].max() <= 4 * MEASURED_WORST


# ---------------------------------------------------------------- 6. oracle/lib.py makes a missing library
def test_lib_builds_a_missing_library(tmp_path):
    """lib() on a tree without liboracle.so makes it: a temporary copy of oracle/, in a fresh interpreter."""
    src = os.path.join(REPO, "oracle")
    dst = tmp_path / "oracle"
    shutil.copytree(src, dst, ignore=shutil.ignore_patterns("*.so", "_ref", "__pycache__", "*.o"))
    assert not (dst / "liboracle.so").exists()
    code = ("import os, oracle.lib as L\n"
            "assert not os.path.exists(L.LIB_PATH)\n"
            "assert L.lib().orc_expand_bits(1023) == 0x09249249\n"
            "assert os.path.exists(L.LIB_PATH)\n"
            "assert callable(L.build_lib) and L.build.__code__.co_argcount >= 2\n"
            "print(L.LIB_PATH)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, capture_output=True, text=True,
                       env={**os.environ, "PYTHONPATH": str(tmp_path)})
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(dst / "liboracle.so")
