"""The walk-only tree: the built tree's top with every maximal subtree of <= 512 leaves rebuilt by
binned SAH, which the certified 4-wide bounce walk reads from the third trace of a build on (RTBVH_WALK_TREE=1: from
the first).  Its structure (rtbvh_read_walk_qnodes walked on the host), its frames (bit for bit the reference
order's), its visit counts and the policy that makes, keeps and drops it; and every QNode the walk can reach
compared, entry word for entry word and edge code for edge code, with the rebuild's sequential model in the CPU
oracle (oracle.lib.walk_tree, written from DESIGN.md 6c) under the built tree's own QNode checks."""
import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import deep_scenes as ds
from tests import hostile_scenes as hs
from tests import walk_tree_scenes as ws
from tests.cert_scenes import camera
from tests.conftest import load_scene_fixture
from tests.test_gpu_parity import _edge_bound_np, _huge_scene, check_qnode_array, leaf_edge_bounds
from tests.walk_tree_scenes import identical_scene

pytestmark = pytest.mark.gpu

CERT = rt.FLAG_CERTIFIED
LEAF, NONE = 0x80000000, 0xFFFFFFFF
SEED = 0x5EED0004


def cert_ctx(monkeypatch, knob="1", flags=CERT):
    """A certified context with RTBVH_WALK_TREE as given (None: the policy's default), read at create."""
    if knob is None:
        monkeypatch.delenv("RTBVH_WALK_TREE", raising=False)
    else:
        monkeypatch.setenv("RTBVH_WALK_TREE", knob)
    return rt.Context(device=0, flags=flags)


def fixture_scene(name):
    d = load_scene_fixture(name)
    return rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])


def leaf_edge_codes(s, wvp, nodes, T):
    """margin.h's edge code (rounded up) of every sorted leaf, from the clip-space triangles (numpy float32)."""
    M = np.asarray(wvp, np.float32).reshape(4, 4)
    P = s.vertices[:, :3].astype(np.float32)
    with np.errstate(under="ignore"):
        clip = ((P[:, 0:1] * M[0] + P[:, 1:2] * M[1]) + P[:, 2:3] * M[2]) + M[3]
    tri = clip[s.indices.reshape(-1, 3), :3]
    eb = _edge_bound_np(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])[nodes["index"][:T] // 3]
    return ((eb.view(np.uint32).astype(np.uint64) + 0xFFFF) >> 16).astype(np.uint32)


def check_walk_qnodes(q, nodes, leaf_codes, T):
    """From the root's slot: every leaf 0..T-1 reached exactly once, every entry's decoded box contains the exact
    boxes of the leaves below it, every node's edge code >= those of the leaves below it.  Returns the depth."""
    assert q.shape == (2 * T - 1, 16)
    bmin, bmax = nodes["bb_min"][:T], nodes["bb_max"][:T]
    f = (q & np.uint32(0xFF800000)).view(np.float32)
    org, scl = q[:, 0:3].view(np.float32), f[:, 3:6]
    shifts = np.arange(4, dtype=np.uint32) * 8
    lo = ((q[:, 6:9, None] >> shifts) & 255).astype(np.float32)   # [slot, axis, c]
    hi = ((q[:, 9:12, None] >> shifts) & 255).astype(np.float32)
    with np.errstate(all="ignore"):   # (the slots of leaves hold nothing)
        dlo = org[:, :, None] + lo * scl[:, :, None]
        dhi = org[:, :, None] + hi * scl[:, :, None]
    code_e = q[:, 4] & 0xFFFF
    seen = np.zeros(T, np.int64)
    # pre-order over the slots, then the exact union and the largest leaf code of every entry bottom-up
    order, stack, depth = [], [(2 * T - 2, 1)], 0
    while stack:
        sl, d = stack.pop()
        order.append(sl)
        depth = max(depth, d)
        assert scl[sl, 0] != 0, "these scenes' nodes all have a finite grid"
        ids = q[sl, 12:16]
        assert ids[0] != NONE and ids[2] != NONE
        for e in map(int, ids):
            if e == NONE:
                continue
            if e & LEAF:
                seen[e & ~LEAF] += 1
            else:
                assert e < 2 * T - 2
                stack.append((int(e), d + 1))
    assert len(order) == len(set(order)), "a slot is reached twice"
    np.testing.assert_array_equal(seen, 1, "every leaf exactly once")
    u_lo, u_hi, u_code = {}, {}, {}
    for sl in reversed(order):
        los, his, codes = [], [], []
        for c, e in enumerate(map(int, q[sl, 12:16])):
            if e == NONE:
                continue
            if e & LEAF:
                j = int(e & ~LEAF)
                l, h, cd = bmin[j], bmax[j], leaf_codes[j]
            else:
                l, h, cd = u_lo.pop(int(e)), u_hi.pop(int(e)), u_code.pop(int(e))
            assert (dlo[sl, :, c] <= l).all() and (dhi[sl, :, c] >= h).all(), (sl, c)
            los.append(l), his.append(h), codes.append(cd)
        u_lo[sl], u_hi[sl], u_code[sl] = np.min(los, 0), np.max(his, 0), max(codes)
        assert code_e[sl] >= u_code[sl], sl
    return depth


@pytest.mark.parametrize("T", [1, 2, 3, 5, 512, 513, 2049, 70_000, "identical"])
def test_structure(T, monkeypatch):
    s = identical_scene() if T == "identical" else rt.synthetic(T, seed=SEED)
    T = s.num_tris
    W, H = 64, 64
    wvp, wv = rt.camera_reference(W, H)
    with rt.Context(device=0, flags=0) as r:
        r.set_scene(s)
        r.set_camera(wvp, wv)
        r.build()
        r.trace(W, H, 2)
        want = r.read_framebuffer()
    with cert_ctx(monkeypatch) as c:
        c.set_scene(s)
        c.set_camera(wvp, wv)
        c.build()
        c.trace(W, H, 2)
        st = c.stats()
        np.testing.assert_array_equal(c.read_framebuffer(), want)
        assert st["stack_overflows"] == 0
        if T == 1:   # one leaf: the walk starts at it, there is no node to rebuild and no walk tree
            assert st["walk_tree_builds"] == 0 and st["walk_tree_used"] == 0
            with pytest.raises(rt.RtbvhError):
                c.read_walk_qnodes()
            return
        assert st["walk_tree_builds"] == 1 and st["walk_tree_used"] == 1
        nodes, q = c.read_bvh(), c.read_walk_qnodes()
        c.trace(W, H, 2)   # the same tree again: nothing is made
        assert c.stats()["walk_tree_builds"] == 1
        q2 = c.read_walk_qnodes()
    depth = check_walk_qnodes(q, nodes, leaf_edge_codes(s, wvp, nodes, T), T)
    assert depth <= 64
    with cert_ctx(monkeypatch) as d:   # another context: the same tree, word for word
        d.set_scene(s)
        d.set_camera(wvp, wv)
        d.build()
        d.trace(W, H, 1)
        q3 = d.read_walk_qnodes()
    reach = [2 * T - 2]   # (the slots of leaves hold nothing)
    while reach:
        sl = reach.pop()
        np.testing.assert_array_equal(q[sl], q2[sl])
        np.testing.assert_array_equal(q[sl], q3[sl])
        reach.extend(e for e in map(int, q[sl, 12:16]) if e != NONE and not (e & LEAF))


def walk_tree_equals_the_model(c, s, wvp, finite=True):
    """The walk-tree QNodes a context holds (its last trace made or used them) against the model of the rebuild run on
    the context's own built tree and the scene as it is now: check_qnode_array from the root's slot -- at every
    slot the walk can reach the four entry words and the E code exactly, and the grid, containment and tcap
    properties of the built tree's QNodes.  Returns (built tree, model tree, how each node came about, nodes read)."""
    nodes, q = c.read_bvh(), c.read_walk_qnodes()
    wt, how = orc.walk_tree(nodes)
    ws.check_tree_over_the_same_leaves(wt, nodes)
    read, _ = check_qnode_array(q, wt, leaf_edge_bounds(s, wvp, nodes)[0], finite)
    return nodes, wt, how, read


def scaled_thirds(s, big=10.0, small=0.1):
    """Positions with every third triangle scaled by `big` about its first vertex and every third by `small` (each
    vertex belongs to one triangle in the synthetic scenes): edge bounds that rise and fall, boxes that move."""
    P = s.vertices[:, :3].astype(np.float32).copy()
    idx = s.indices.reshape(-1, 3)
    f = np.ones(len(idx), np.float32)
    f[0::3], f[1::3] = big, small
    for k in (1, 2):
        P[idx[:, k]] = P[idx[:, 0]] + f[:, None] * (P[idx[:, k]] - P[idx[:, 0]])
    return np.ascontiguousarray(P)


def with_positions(s, P):
    v = s.vertices.copy()
    v[:, :3] = P
    return rt.Scene(v, s.indices, s.mat_indices, s.materials)


MK = rt.FLAG_MULTI_KERNEL_BUILD
MODEL_CASES = ["syn513", "syn2049", "syn6000", "lattice", "planar", "identical", "nonfinite", "fan", "crossing",
               "budget", "syn2049 refitted"]


@pytest.mark.parametrize("case", MODEL_CASES)
def test_rebuild_equals_the_model(case, monkeypatch):
    """The smallest scenes that reach each branch of k_wt_select / k_wt_rebuild: one top node over two subtrees of a
    one-workgroup build (513); several top levels, subtrees near 512 leaves and ranges above and below a wave's 64
    (2,049 and 6,000, multi-kernel builds); exact costs that tie on all three axes (a lattice of 8 x 8 x 16
    identical triangles at unit spacing under the identity camera) and on two (a planar one); no plane at all
    (identical triangles); halves under non-finite corners; the deep-tree scenes (the fan: one subtree of 15
    levels; the crossing scene: 65 subtrees of up to 29 levels, none of them deep enough in the built tree to run out
    of levels); a subtree root 31 levels deep whose planes peel, so that the level budget refuses some and the 32-level
    limit others (walk_tree_scenes.budget_scene); a refitted tree."""
    cam, flags, finite, moved = rt.camera_reference(64, 64), CERT | MK, True, None
    if case.startswith("syn"):
        n = int(case.split()[0][3:])
        s = rt.synthetic(n, seed=SEED)
        if n == 513:
            flags = CERT   # the one-workgroup build: the top node's edge bound is k_build_small's
        if "refitted" in case:
            moved = scaled_thirds(s)
    elif case == "lattice":
        s, cam = ws.lattice_scene(8, 8, 16, seed=3), ws.IDENTITY
    elif case == "planar":
        s, cam = ws.lattice_scene(32, 32, 1, seed=3), ws.IDENTITY
    elif case == "identical":
        s = identical_scene()
    elif case == "nonfinite":
        s, cam, finite = hs.hostile("nonfinite").scene, hs.camera("reference"), False
    elif case == "fan":
        s, cam = ds.fan_scene(), camera("A")
    elif case == "crossing":
        s, cam, flags = ds.crossing_scene(), ds.crossing_camera(), CERT
    else:
        s, cam = ws.budget_scene(), ws.IDENTITY
    with cert_ctx(monkeypatch, "1", flags) as c:
        c.set_scene(s)
        c.set_camera(*cam)
        c.build()
        if moved is not None:
            c.trace(64, 64, 1)   # (a walk tree of the old geometry first)
            c.update_vertices(moved)
            c.refit()
            s = with_positions(s, moved)
        c.trace(64, 64, 1)
        st = c.stats()
        assert st["walk_tree_used"] == 1 and st["walk_tree_builds"] == (2 if moved is not None else 1)
        nodes, wt, how, read = walk_tree_equals_the_model(c, s, cam[0], finite)
    T = s.num_tris
    first, last, _ = ws.leaf_ranges(wt)
    size = (last - first + 1)[T:]
    kept, sah, budget = (how["how"] == k for k in (orc.WT_KEPT, orc.WT_SAH, orc.WT_HALVES_BUDGET))
    halves = ~kept & ~sah
    print(f"{case}: T = {T}, {kept.sum()} kept, {sah.sum()} SAH, {halves.sum()} halves ({budget.sum()} for the "
          f"level budget), {len(read)} QNodes read, deepest level {how['level'].max()}")
    if case == "syn513":
        assert kept.sum() == 1 and (how["level"][~kept] == 0).sum() == 2
    if case in ("syn2049", "syn6000", "syn2049 refitted"):
        assert kept.sum() > 2 and size[~kept].max() > 256
        assert (sah & (size > 64)).any() and (sah & (size < 64) & (size > 2)).any()
    if case == "lattice":
        assert set(how["axis"][sah]) == {0, 1, 2}
    if case == "planar":
        assert set(how["axis"][sah]) == {0, 1}
    if case == "identical":
        assert not sah.any()
    if case == "nonfinite":
        assert sah.any() and (halves & (size > 2)).any()
    if case == "budget":
        assert budget.any() and how["level"].max() == 32


def frames(s, cam, W, H, bounces, monkeypatch, flags=CERT, multi_kernel=False):
    """(reference-order frame, certified frame without the walk tree and its stats, with it and its stats)."""
    extra = rt.FLAG_MULTI_KERNEL_BUILD if multi_kernel else 0
    out = []
    for knob, fl in ((None, 0), ("0", flags), ("1", flags)):
        with cert_ctx(monkeypatch, knob, fl | extra) as c:
            c.set_scene(s)
            c.set_camera(*cam)
            c.build()
            c.trace(W, H, bounces)
            out.append((c.read_framebuffer(), c.read_intensity(), c.stats()))
    return out


def assert_frames(s, cam, W, H, bounces, monkeypatch, **kw):
    (ref, rint, _), (f0, i0, s0), (f1, i1, s1) = frames(s, cam, W, H, bounces, monkeypatch, **kw)
    assert s0["walk_tree_builds"] == 0 and s0["walk_tree_used"] == 0
    assert s1["walk_tree_builds"] == 1 and s1["walk_tree_used"] == 1
    np.testing.assert_array_equal(f1.view(np.uint32), ref.view(np.uint32))
    np.testing.assert_array_equal(i1.view(np.uint32), rint.view(np.uint32))
    np.testing.assert_array_equal(f0.view(np.uint32), ref.view(np.uint32))
    if s0["stack_overflows"] == 0:
        assert s1["stack_overflows"] == 0
    for k in ("bounce_rays", "textured_hits"):
        assert s1[k] == s0[k], k
    return s0, s1


@pytest.mark.parametrize("bounces", [1, 3])
def test_frames_synthetic(bounces, monkeypatch):
    assert_frames(rt.synthetic(70_000, seed=SEED), rt.camera_reference(256, 256), 256, 256, bounces, monkeypatch)


def test_frames_test_obj(monkeypatch):
    assert_frames(fixture_scene("Test"), rt.camera_reference(320, 240), 320, 240, 3, monkeypatch)
    assert_frames(fixture_scene("Test"), rt.camera_reference(320, 240), 320, 240, 3, monkeypatch, multi_kernel=True)


@pytest.mark.parametrize("variant", list(hs.VARIANTS))
@pytest.mark.parametrize("cam", hs.CAMERAS)
def test_frames_hostile(variant, cam, monkeypatch):
    """tests/hostile_scenes.py through the rebuild: points, needles, duplicates (equal centroids), denormal and huge
    extents, NaN and inf corners (the halves path)."""
    assert_frames(hs.hostile(variant).scene, hs.camera(cam), hs.W, hs.H, 2, monkeypatch, multi_kernel=True)


def test_frames_nodes_without_a_grid(monkeypatch):
    """Triangles spanning +-1e31: the nodes above them carry no grid, the certified walk ends there and the ray is
    re-traced on the built tree -- with the walk tree as without."""
    s0, s1 = assert_frames(_huge_scene(), rt.camera_reference(320, 240), 320, 240, 2, monkeypatch, multi_kernel=True)
    assert s1["redo_total"] > 0 and s0["redo_total"] > 0


@pytest.mark.parametrize("scene", ["fan", "crossing"])
def test_frames_deep_trees(scene, monkeypatch):
    """The deep-tree scenes (tests/deep_scenes.py): a root path near the 64-level limit keeps the rebuilt subtrees
    within the walk's stack (k_wt_rebuild's level budget)."""
    if scene == "fan":
        assert_frames(ds.fan_scene(), camera("A"), ds.W, ds.H, 2, monkeypatch, multi_kernel=True)
    else:
        assert_frames(ds.crossing_scene(), ds.crossing_camera(), 64, 48, 2, monkeypatch)


def test_visits(monkeypatch):
    """The bounce pass's internal visits with the walk tree are not more than without it (the CPU study,
    tools/collapse_study.cpp REBUILD=bottom, predicts fewer on this scene: profiles/walk_tree_study.jsonl)."""
    s = rt.synthetic(70_000, seed=SEED)
    _, (_, _, s0), (_, _, s1) = frames(s, rt.camera_reference(256, 256), 256, 256, 1, monkeypatch,
                                       flags=CERT | rt.FLAG_COUNT_VISITS)
    print(f"bounce internal visits: built tree {s0['internal_visits'][1]}, walk tree {s1['internal_visits'][1]}, "
          f"leaf visits {s0['leaf_visits'][1]} / {s1['leaf_visits'][1]}")
    assert s0["internal_visits"][1] > 0
    assert s1["internal_visits"][1] <= s0["internal_visits"][1]


def test_policy_third_trace_builds_it_once(monkeypatch):
    s = rt.synthetic(20_000, seed=SEED)
    W, H = 128, 128
    with cert_ctx(monkeypatch, None) as c:
        c.set_scene(s)
        c.set_camera(*rt.camera_reference(W, H))
        c.build()
        seen, fbs = [], []
        for _ in range(5):
            c.trace(W, H, 2)
            st = c.stats()
            seen.append((st["walk_tree_builds"], st["walk_tree_used"]))
            fbs.append(c.read_framebuffer())
        assert seen == [(0, 0), (0, 0), (1, 1), (1, 1), (1, 1)]
        for fb in fbs[1:]:
            np.testing.assert_array_equal(fb, fbs[0])
        c.trace(W, H, 0)   # no bounce pass: nothing to walk it
        assert c.stats()["walk_tree_used"] == 0


def test_knob_off(monkeypatch):
    s = rt.synthetic(20_000, seed=SEED)
    with cert_ctx(monkeypatch, "0") as c:
        c.set_scene(s)
        c.set_camera(*rt.camera_reference(128, 128))
        c.build()
        for _ in range(4):
            c.trace(128, 128, 2)
        st = c.stats()
        assert st["walk_tree_builds"] == 0 and st["walk_tree_used"] == 0
        with pytest.raises(rt.RtbvhError):
            c.read_walk_qnodes()


def test_rebuild_refit_and_update_drop_it(monkeypatch):
    """A build under a moved camera, a refit and a vertex update each make the walk tree one of an old tree: the
    next frame equals the reference order's of the new tree, from a walk tree made anew."""
    s = rt.synthetic(20_000, seed=SEED)
    W, H = 128, 128
    camA = rt.camera_reference(W, H)
    wvpB = np.asarray(camA[0], np.float32).copy().reshape(4, 4)
    wvpB[3, 0] += 3.0
    camB = (wvpB, camA[1])
    moved = s.vertices[:, :3].copy()
    moved[:, 2] += (0.25 * np.sin(np.arange(len(moved)) * 0.01)).astype(np.float32)

    def reference(cam, pos=None):
        with rt.Context(device=0, flags=0) as r:
            r.set_scene(s)
            r.set_camera(*cam)
            r.build()
            if pos is not None:
                r.update_vertices(pos)
                r.refit()
            r.trace(W, H, 2)
            return r.read_framebuffer()

    with cert_ctx(monkeypatch) as c:
        c.set_scene(s)
        c.set_camera(*camA)
        c.build()
        c.trace(W, H, 2)
        np.testing.assert_array_equal(c.read_framebuffer(), reference(camA))
        assert c.stats()["walk_tree_builds"] == 1
        c.set_camera(*camB)
        c.build()
        with pytest.raises(rt.RtbvhError):   # (the one it holds is of the last tree)
            c.read_walk_qnodes()
        c.trace(W, H, 2)
        np.testing.assert_array_equal(c.read_framebuffer(), reference(camB))
        assert c.stats()["walk_tree_builds"] == 2
        c.refit()
        c.trace(W, H, 2)
        np.testing.assert_array_equal(c.read_framebuffer(), reference(camB))
        assert c.stats()["walk_tree_builds"] == 3
        c.update_vertices(moved)
        with pytest.raises(rt.RtbvhError):   # stale: no trace until a refit or build
            c.trace(W, H, 2)
        c.refit()
        c.trace(W, H, 2)
        st = c.stats()
        assert st["walk_tree_builds"] == 4 and st["walk_tree_used"] == 1
        np.testing.assert_array_equal(c.read_framebuffer(), reference(camB, moved))


def test_four_streams_share_one(monkeypatch):
    """Four streams with frames in flight (the context's and three callers': every buffer set a context has) under
    the default policy: one walk tree, made before the third trace, every frame identical to the one traced alone
    on the built tree's QNodes."""
    import torch

    s = rt.synthetic(70_000, seed=SEED)
    W, H = 256, 256
    dev = torch.device("cuda:0")
    with cert_ctx(monkeypatch, None) as c:
        c.set_scene(s)
        c.set_camera(*rt.camera_reference(W, H))
        c.build()
        alone = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        c.trace_band_async(W, H, 2, 0, 1, alone.data_ptr())
        c.synchronize()
        assert c.stats()["walk_tree_used"] == 0
        streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
        bufs = [torch.zeros_like(alone) for _ in range(8)]
        torch.cuda.synchronize()   # (torch fills them on its own stream)
        for i, b in enumerate(bufs):
            if i % 4 == 0:
                c.trace_band_async(W, H, 2, 0, 1, b.data_ptr())
            else:
                c.trace_band_async(W, H, 2, 0, 1, b.data_ptr(), stream_ptr=streams[i % 4 - 1].cuda_stream)
        c.synchronize()
        st = c.stats()
        assert st["walk_tree_builds"] == 1 and st["walk_tree_used"] == 1 and st["stack_overflows"] == 0
        for i, b in enumerate(bufs):
            assert torch.equal(b, alone), i


def test_graph_capture_never_uses_it(monkeypatch):
    """AUTO_WALK | GRAPH on a scene past the AUTO threshold (certified walks): the plain frame before the capture
    may make a walk tree (RTBVH_WALK_TREE=1), the captured frame holds none, and every replay is the reference
    order's frame of its camera."""
    s = rt.synthetic(70_000, seed=SEED)
    W, H = 128, 128
    camA = rt.camera_reference(W, H)
    wvpB = np.asarray(camA[0], np.float32).copy().reshape(4, 4)
    wvpB[3, 0] += 2.0
    want = []
    for cam in (camA, (wvpB, camA[1])):
        with rt.Context(device=0, flags=0) as r:
            r.set_scene(s)
            r.set_camera(*cam)
            r.compute_bvh(W, H, 2)
            want.append(r.read_framebuffer())
    with cert_ctx(monkeypatch, "1", rt.FLAG_AUTO_WALK | rt.FLAG_GRAPH) as g:
        g.set_scene(s)
        for k in (0, 1, 0, 1):
            g.set_camera(*(camA if k == 0 else (wvpB, camA[1])))
            g.compute_bvh(W, H, 2)
            st = g.stats()
            np.testing.assert_array_equal(g.read_framebuffer(), want[k])
            assert st["walk_tree_used"] == 0 and st["graph_captures"] == 1
        assert st["walk_tree_builds"] <= 1
