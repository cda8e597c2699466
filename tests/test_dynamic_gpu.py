"""Animated geometry on the GPU: vertex updates from host and device memory (rtbvh_update_vertices_*) and the
topology-keeping refit (rtbvh_refit*), against a fresh context, the CPU oracle and the numpy restatement of
findCollision (tests/ray_walk_ref.py).  Every comparison is bit-exact; frames are 64 x 64.

Scenes: Rect (12 triangles), Test (1,952: the one-workgroup build), Image_Test (3,072: the one-workgroup sort,
the multi-kernel rest), rt.synthetic(20000) (radix sort, several refit workgroups, crossing nodes), the crossing
scene of tests/deep_scenes.py (the grouped refit's fallback), and scenes of 1 and 2 triangles.

Section 8 runs the QNode model of tests/test_gpu_parity.py (entries, grids, containment, the E code exactly, the tcap
code) on live contexts after every transition that rewrites the QNodes, and the walk-only tree of the same state
against its model (tests/test_walk_tree_gpu.py)."""
import functools

import numpy as np
import pytest

import raytracebvh_amd as rt
from oracle import lib as orc
from tests import deep_scenes as ds
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_gpu_parity import check_qnodes_live
from tests.test_query_gpu import assert_genuine, assert_hits_equal, random_rays, tiny_scene
from tests.test_walk_tree_gpu import scaled_thirds, walk_tree_equals_the_model, with_positions

pytestmark = pytest.mark.gpu
W = H = 64
SCENES = ["Rect", "Test", "Image_Test", "syn20k", "crossing", "tiny1", "tiny2"]
FLAGS = {"plain": 0, "certified": rt.FLAG_CERTIFIED, "auto": rt.FLAG_AUTO_WALK}
FIELDS = ("parent", "child_l", "child_r", "code", "index", "bb_min", "bb_max")
NOT_READY, INVALID_ARG = rt._lib.ERR_NOT_READY, rt._lib.ERR_INVALID_ARG


# ---------------------------------------------------------------- scenes, cameras, deformations
@functools.lru_cache(maxsize=None)
def scene_of(name):
    """(scene, (wvp, wv) of the build camera, (wvp, wv) of another camera)."""
    ref = rt.camera_reference(W, H)
    other = rt.camera_look(rt.camera_orbit(rt.EYE_REFERENCE, rt.KEY_LEFT), W, H)
    if name == "syn20k":
        return rt.synthetic(20000), ref, other
    if name == "crossing":
        m = np.array(ds.crossing_camera()[0], np.float32).reshape(4, 4)
        m[3, :3] += (0.75, -0.5, 2.0)   # the same scaling, the mesh slid under the rays' grid
        return ds.crossing()[0], ds.crossing_camera(), (m.ravel(), m.ravel().copy())
    if name.startswith("tiny"):
        return tiny_scene(int(name[4:])), ref, other
    d = load_scene_fixture(name)
    return rt.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"]), ref, other


def deform(p, phase):
    """p' = p + a sin(k p.yzx + phase) in float32, a = 2% of the mesh box per axis, one wave across it."""
    p = np.ascontiguousarray(p, np.float32)
    ext = (p.max(0) - p.min(0)).astype(np.float32)
    a = np.float32(0.02) * ext
    k = np.where(ext > 0, np.float32(2 * np.pi) / np.where(ext > 0, ext, 1), 0).astype(np.float32)
    yzx = [1, 2, 0]
    return np.ascontiguousarray((p + a * np.sin(k[yzx] * p[:, yzx] + np.float32(phase))).astype(np.float32))


def new_normals(v, phase):
    """The scene's normals turned a little about x (their z, which the shading weighs, changes)."""
    n = v[:, 3:6]
    c, s = np.float32(np.cos(0.3 + phase)), np.float32(np.sin(0.3 + phase))
    return np.ascontiguousarray(np.stack([n[:, 0], c * n[:, 1] - s * n[:, 2], s * n[:, 1] + c * n[:, 2]], 1), np.float32)


@functools.lru_cache(maxsize=None)
def moved(name, step, normals=False):
    """Deformation `step` (1, 2, ...) of a scene: (positions, normals or None, the scene with them)."""
    s = scene_of(name)[0]
    P = deform(s.vertices[:, :3], 0.7 * step)
    N = new_normals(s.vertices, 0.2 * step) if normals else None
    v = s.vertices.copy()
    v[:, :3] = P
    if N is not None:
        v[:, 3:6] = N
    for a in (P, N, v):
        if a is not None:
            a.setflags(write=False)
    return P, N, rt.Scene(v, s.indices, s.mat_indices, s.materials)


def oscene(s):
    return orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob)


@functools.lru_cache(maxsize=None)
def oracle_of(name, step, normals=False, cam=0, bounces=1):
    """The oracle's tree and frame of a scene's deformation `step` (0: as it is) at camera `cam`; read-only."""
    s = moved(name, step, normals)[2] if step else scene_of(name)[0]
    wvp, wv = scene_of(name)[1 + cam]
    os_ = oscene(s)
    nodes = orc.build(os_, wvp)
    fb = orc.trace(os_, nodes, wvp, wv, W, H, bounces)[0]
    nodes.setflags(write=False)
    fb.setflags(write=False)
    return nodes, fb


def make_ctx(name, flags=0, cam=0, scene=None, **kw):
    c = rt.Context(device=0, flags=flags, **kw)
    c.set_scene(scene if scene is not None else scene_of(name)[0])
    c.set_camera(*scene_of(name)[1 + cam])
    return c


def assert_tree_equal(got, want, fields=FIELDS, what=""):
    for f in fields:
        np.testing.assert_array_equal(got[f].view(np.uint32), want[f].view(np.uint32), err_msg=f"{what} field {f}")


def assert_frame_equal(got, want, what=""):
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what + " frame")


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the cached arrays are read-only)


# ---------------------------------------------------------------- 1. update + rebuild = a fresh scene
def _update(ctx, how, P, N):
    """The update of all vertices through one of the paths."""
    import torch
    if how == "numpy":
        ctx.update_vertices(P, N)
    elif how == "partial":   # two calls: [0, h) and [h, V)
        h = max(1, len(P) // 2)
        ctx.update_vertices(P[:h], None if N is None else N[:h])
        ctx.update_vertices(P[h:], None if N is None else N[h:], first=h)
    elif how == "torch":     # device tensors on a stream of the caller's
        s = torch.cuda.Stream()
        tp, tn = cuda(P), None if N is None else cuda(N)
        s.wait_stream(torch.cuda.current_stream())
        ctx.update_vertices(tp, tn, stream=s)
        s.synchronize()      # (the tensors stay alive until the update has read them)
    elif how == "strided":   # an rtbvh_vertex-shaped tensor: positions at 0, normals at 3, stride 8
        v = np.zeros((len(P), 8), np.float32)
        v[:, :3] = P
        v[:, 3:6] = 0 if N is None else N
        tv = cuda(v)
        assert tv[:, :3].stride(0) == 8
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        ctx.update_vertices(tv[:, :3], None if N is None else tv[:, 3:6], stream=s)
        s.synchronize()
    else:
        raise AssertionError(how)


@pytest.mark.parametrize("normals", [False, True], ids=["positions", "normals"])
@pytest.mark.parametrize("how", ["numpy", "torch", "strided", "partial"])
@pytest.mark.parametrize("name", SCENES)
def test_update_then_rebuild_equals_a_fresh_scene(name, how, normals):
    P, N, s1 = moved(name, 1, normals)
    nodes, fb = oracle_of(name, 1, normals)
    with make_ctx(name) as a, make_ctx(name, scene=s1) as b:
        a.compute_bvh(W, H, 1)          # a tree and a frame of the old geometry first
        _update(a, how, P, N)
        a.compute_bvh(W, H, 1)
        b.compute_bvh(W, H, 1)
        np.testing.assert_array_equal(a.read_morton(), b.read_morton())
        for x, y in zip(a.read_sorted(), b.read_sorted()):
            np.testing.assert_array_equal(x, y)
        ta = a.read_bvh()
        assert_tree_equal(ta, b.read_bvh(), what="fresh context")
        assert_tree_equal(ta, nodes, what="oracle")
        fa = a.read_framebuffer()
        assert_frame_equal(fa, b.read_framebuffer(), "fresh context")
        assert_frame_equal(fa, fb, "oracle")
    if normals and name == "syn20k":   # the normals matter: the frame is not that of the old ones
        assert not np.array_equal(fb, oracle_of(name, 1, False)[1])


def test_hlsl_morton_update_needs_no_mesh_box():
    P, _, s1 = moved("Image_Test", 1)
    kw = dict(morton_mode=rt.MORTON_HLSL)
    with make_ctx("Image_Test", **kw) as a, make_ctx("Image_Test", scene=s1, **kw) as b:
        a.build()
        a.update_vertices(cuda(P))
        a.compute_bvh(W, H, 1)
        b.compute_bvh(W, H, 1)
        assert_tree_equal(a.read_bvh(), b.read_bvh())
        assert_frame_equal(a.read_framebuffer(), b.read_framebuffer())


# ---------------------------------------------------------------- 2. graph replay
@pytest.mark.parametrize("name", ["Test", "syn20k"])
def test_update_replays_the_captured_frame(name):
    import torch
    with make_ctx(name, flags=rt.FLAG_GRAPH) as ctx:
        s = torch.cuda.Stream()
        for step in (1, 2, 3):
            tp = cuda(moved(name, step)[0])
            s.wait_stream(torch.cuda.current_stream())
            ctx.update_vertices(tp, stream=s)
            ctx.compute_bvh(W, H, 1)
            s.synchronize()
            nodes, fb = oracle_of(name, step)
            assert_frame_equal(ctx.read_framebuffer(), fb, f"step {step}")
            assert_tree_equal(ctx.read_bvh(), nodes, what=f"step {step}")
            assert ctx.stats()["graph_captures"] == 1


# ---------------------------------------------------------------- 3. a camera-only refit = a rebuild
@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("name", SCENES)
def test_camera_only_refit_equals_a_rebuild(name, mode):
    nodes, fb = oracle_of(name, 0, cam=1)
    with make_ctx(name, FLAGS[mode]) as ctx, make_ctx(name, FLAGS[mode], cam=1) as fresh:
        ctx.build()
        before = ctx.read_sorted()
        ctx.set_camera(*scene_of(name)[2])
        ctx.refit()
        fresh.build()
        got = ctx.read_bvh()
        assert_tree_equal(got, fresh.read_bvh(), what="fresh build")
        assert_tree_equal(got, nodes, what="oracle")
        for x, y in zip(before, ctx.read_sorted()):
            np.testing.assert_array_equal(x, y)
        ctx.trace(W, H, 1)
        assert_frame_equal(ctx.read_framebuffer(), fb, "oracle")
        ctx.refit(sync=False)   # and again, enqueued only: the same tree
        ctx.trace(W, H, 1)
        assert_frame_equal(ctx.read_framebuffer(), fb, "second refit")


# ---------------------------------------------------------------- 4. a refit after a deformation
def check_refitted(ctx, name, step, tree0, sorted0, mode, rays=1024, full=True):
    """The context's tree after update(step) + refit: the build's topology, exact boxes of the moved triangles, and
    frames and hits that are the reference walk's over that tree."""
    s1 = moved(name, step)[2]
    wvp, wv = scene_of(name)[1]
    for x, y in zip(sorted0, ctx.read_sorted()):
        np.testing.assert_array_equal(x, y)
    tree = ctx.read_bvh()
    assert_tree_equal(tree, tree0, ("parent", "child_l", "child_r", "index", "code"), "kept")
    n = s1.num_tris
    tris = rw.clip_triangles(s1.vertices, s1.indices, wvp)
    t = tris[tree["index"][:n] // 3]
    lo = np.minimum(np.minimum(t[:, 0], t[:, 1]), t[:, 2])
    hi = np.maximum(np.maximum(t[:, 0], t[:, 1]), t[:, 2])
    np.testing.assert_array_equal(tree["bb_min"][:n].view(np.uint32), lo.view(np.uint32))
    np.testing.assert_array_equal(tree["bb_max"][:n].view(np.uint32), hi.view(np.uint32))
    if n > 1:
        bmin, bmax = np.zeros((2 * n - 1, 3), np.float32), np.zeros((2 * n - 1, 3), np.float32)
        bmin[:n], bmax[:n] = lo, hi
        # (packed copies, kept alive here: the binding passes on the pointers of the arrays it is given)
        par, cl, cr = (np.ascontiguousarray(tree[f]) for f in ("parent", "child_l", "child_r"))
        bmin, bmax, _ = orc.refit(n, par, cl, cr, bmin, bmax)
        np.testing.assert_array_equal(tree["bb_min"].view(np.uint32), bmin.view(np.uint32))
        np.testing.assert_array_equal(tree["bb_max"].view(np.uint32), bmax.view(np.uint32))
    os1 = oscene(s1)
    for b in (1, 3) if full else (1,):
        ctx.trace(W, H, b)
        assert_frame_equal(ctx.read_framebuffer(), orc.trace(os1, tree, wvp, wv, W, H, b)[0], f"{b} bounces")
    if mode == "certified":
        assert ctx.stats()["walk_state"] == 2   # (the certified walks read the refitted QNodes and footprints)
    o, d = random_rays(tree, rays, seed=step)
    want = rw.walk(tree, tris, o, d)
    r = rt.make_rays(o, d)
    assert_hits_equal(ctx.query(r), want, "closest")
    assert_hits_equal(ctx.query(r, rt.QUERY_CERTIFIED), want, "certified")
    if full:
        got = ctx.query(r, rt.QUERY_ANY)
        np.testing.assert_array_equal(got["t"] != -1, want["hit"])
        assert_genuine(got, tris, o, d)
    return tree


@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("name", SCENES)
def test_refit_after_deformation(name, mode):
    with make_ctx(name, FLAGS[mode]) as ctx:
        ctx.build()
        tree0, sorted0 = ctx.read_bvh(), ctx.read_sorted()
        ctx.trace(W, H, 1)             # (a bin set of the built tree, for the binned walks)
        bins = [ctx.bin_builds()]
        for step in (1, 2):            # the second refit starts from the first one's tickets and footprints
            ctx.update_vertices(moved(name, step)[0])
            ctx.refit()
            tree = check_refitted(ctx, name, step, tree0, sorted0, mode, full=step == 1)
            bins.append(ctx.bin_builds())
            assert not np.array_equal(tree["bb_min"], tree0["bb_min"])
        if bins[0]:                    # a binned primary pass: every refitted tree got a bin set of its own
            assert bins[0] < bins[1] < bins[2]
        ctx.build()                    # then a rebuild is the fresh tree of the last geometry
        assert_tree_equal(ctx.read_bvh(), oracle_of(name, 2)[0], what="rebuild")
        ctx.trace(W, H, 1)
        assert_frame_equal(ctx.read_framebuffer(), oracle_of(name, 2)[1], "rebuild")


# ---------------------------------------------------------------- 5. records and node-box trees
def test_refitted_records_and_node_box_trees_agree():
    s = rt.synthetic(70_000, seed=0x5EED0004)
    wvp, wv = rt.camera_reference(W, H)
    P = deform(s.vertices[:, :3], 0.7)
    v = s.vertices.copy()
    v[:, :3] = P
    s1 = rt.Scene(v, s.indices, s.mat_indices, s.materials)
    with rt.Context(device=0, flags=rt.FLAG_AUTO_WALK) as auto, rt.Context(device=0) as plain:
        for c in (auto, plain):
            c.set_scene(s)
            c.set_camera(wvp, wv)
            c.build()
            c.update_vertices(cuda(P))
            c.refit()
        nodes = plain.read_bvh()
        assert_tree_equal(auto.read_bvh(), nodes, what="node boxes against records")
        tris = rw.clip_triangles(s1.vertices, s1.indices, wvp)
        o, d = random_rays(nodes, 20_000, seed=3)
        rays = rt.make_rays(o, d)
        a, p = auto.query(rays, rt.QUERY_COUNT), plain.query(rays, rt.QUERY_COUNT)
        np.testing.assert_array_equal(a.view(np.uint32), p.view(np.uint32))
        assert auto.query_counts() == plain.query_counts()
        want = rw.walk(nodes, tris, o, d)
        assert want["hit"].any() and not want["hit"].all()
        assert_hits_equal(a, want)
        np.testing.assert_array_equal(auto.query(rays, rt.QUERY_CERTIFIED).view(np.uint32), p.view(np.uint32))
        auto.trace(W, H, 1)
        plain.trace(W, H, 1)
        fb = auto.read_framebuffer()
        assert auto.stats()["walk_state"] == 2   # (the certified walks: the refit wrote node boxes, no records)
        assert_frame_equal(fb, plain.read_framebuffer(), "records against node boxes")
        ofb = orc.trace(oscene(s1), nodes, wvp, wv, W, H, 1, row_begin=0, row_end=16)[0]
        assert_frame_equal(fb[0:16], ofb, "oracle over the refitted tree")


# ---------------------------------------------------------------- 6. state and errors
def test_state_and_errors():
    name = "Test"
    s = scene_of(name)[0]
    V = len(s.vertices)
    P = moved(name, 1)[0]
    rays = rt.make_rays(np.zeros((4, 3)), np.ones((4, 3)))
    L = rt.lib()

    def status(f):
        with pytest.raises(rt.RtbvhError) as e:
            f()
        return e.value.status

    with rt.Context(device=0) as ctx:
        assert status(lambda: ctx.update_vertices(P)) == NOT_READY       # before set_scene
        assert status(ctx.refit) == NOT_READY
        ctx.set_scene(s)
        ctx.set_camera(*scene_of(name)[1])
        assert status(ctx.refit) == NOT_READY                            # before any build
        assert status(lambda: ctx.refit(sync=False)) == NOT_READY
        ctx.update_vertices(s.vertices[:, :3])                           # before a build: allowed (stride 8)
        ctx.build()
        tree0 = ctx.read_bvh()
        ctx.trace(W, H, 1)
        fb0 = ctx.read_framebuffer()
        ctx.query(rays)
        # count == 0 touches nothing: the tree stays usable
        ctx.update_vertices(P[:0])
        assert L.rtbvh_update_vertices_async(ctx._h, None, 3, None, 0, 0, 0, None) == rt._lib.OK
        assert L.rtbvh_update_vertices_host(ctx._h, None, 0, None, 0, V + 5, 0) == rt._lib.OK
        ctx.trace(W, H, 1)
        # range and stride errors, computed without overflow; none makes the tree stale
        p = P.ctypes.data
        for first, count in ((0, V + 1), (V, 1), (1, V), (0xFFFFFFFF, 2), (2, 0xFFFFFFFF), (V + 1, 1)):
            assert L.rtbvh_update_vertices_host(ctx._h, p, 3, None, 0, first, count) == INVALID_ARG
            assert L.rtbvh_update_vertices_async(ctx._h, p, 3, None, 0, first, count, None) == INVALID_ARG
        assert "exceeds" in L.rtbvh_last_error(ctx._h).decode()
        assert L.rtbvh_update_vertices_host(ctx._h, p, 2, None, 0, 0, 1) == INVALID_ARG
        assert L.rtbvh_update_vertices_host(ctx._h, p, 3, p, 2, 0, 1) == INVALID_ARG
        assert "stride" in L.rtbvh_last_error(ctx._h).decode()
        assert L.rtbvh_update_vertices_host(ctx._h, None, 3, None, 0, 0, 1) == INVALID_ARG
        assert L.rtbvh_update_vertices_async(ctx._h, None, 3, None, 0, 0, 1, None) == INVALID_ARG
        assert status(lambda: ctx.update_vertices(P, first=1)) == INVALID_ARG
        ctx.trace(W, H, 1)
        assert_frame_equal(ctx.read_framebuffer(), fb0)
        # after an update: traces and queries are refused and say why, the readbacks keep the last build's tree
        ctx.update_vertices(P)
        for f in (lambda: ctx.trace(W, H, 1), lambda: ctx.trace(W, H, 1, sync=False), lambda: ctx.query(rays),
                  lambda: ctx.verify_walk(W, H, 1), lambda: ctx.query(rays, rt.QUERY_ANY),
                  lambda: ctx.trace_band_async(W, H, 1, 0, 1, ctx.framebuffer_device_ptr())):
            assert status(f) == NOT_READY
            assert "updated" in L.rtbvh_last_error(ctx._h).decode()
        assert_tree_equal(ctx.read_bvh(), tree0, what="stale readback")
        assert_frame_equal(ctx.read_framebuffer(), fb0, "stale readback")
        ctx.refit()
        ctx.trace(W, H, 1)
        assert not np.array_equal(ctx.read_framebuffer(), fb0)
        ctx.update_vertices(P)
        assert status(lambda: ctx.query(rays)) == NOT_READY
        ctx.build()                                                      # a build clears it too
        assert_tree_equal(ctx.read_bvh(), oracle_of(name, 1)[0])
        ctx.update_vertices(P)
        ctx.compute_bvh(W, H, 1)                                         # and compute_bvh
        assert_frame_equal(ctx.read_framebuffer(), oracle_of(name, 1)[1])
        ctx.set_scene(s)                                                 # set_scene resets the tree, as before
        assert status(ctx.refit) == NOT_READY


def test_query_after_async_refit_sees_the_new_tree():
    import torch
    name = "Image_Test"
    wvp, _ = scene_of(name)[1]
    with make_ctx(name) as ctx:
        ctx.build()
        tree0 = ctx.read_bvh()
        o, d = random_rays(tree0, 4096)
        rays = cuda(rt.make_rays(o, d).view(np.float32).reshape(-1, 8))
        tp = cuda(moved(name, 1)[0])
        s1 = torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        before = ctx.query(rays, stream=s1)        # outstanding while the update and the refit are enqueued
        ctx.update_vertices(tp, stream=s1)
        ctx.refit(sync=False)
        after = ctx.query(rays, stream=s1)
        s1.synchronize()
        ctx.synchronize()
        s1v = moved(name, 1)[2]
        tree1 = ctx.read_bvh()
        s0 = scene_of(name)[0]
        want0 = rw.walk(tree0, rw.clip_triangles(s0.vertices, s0.indices, wvp), o, d)
        want1 = rw.walk(tree1, rw.clip_triangles(s1v.vertices, s1v.indices, wvp), o, d)
        assert_hits_equal(before.cpu().numpy().view(rt.HIT_DTYPE).reshape(-1), want0, "before the refit")
        assert_hits_equal(after.cpu().numpy().view(rt.HIT_DTYPE).reshape(-1), want1, "after the refit")
        assert not np.array_equal(before.cpu().numpy(), after.cpu().numpy())


# ---------------------------------------------------------------- 8. the QNodes after every transition
MK, CERT = rt.FLAG_MULTI_KERNEL_BUILD, rt.FLAG_CERTIFIED
QN_KINDS = {"one workgroup": (1000, 0), "records": (2049, MK), "node boxes": (2049, CERT | MK)}


def qn_states(n):
    """(scene, positions) of the three geometries: as made; a third of the triangles scaled up tenfold and a third
    down (E rises and falls); and from there the other way and further."""
    s0 = rt.synthetic(n, seed=0x5EED0004)
    P1 = scaled_thirds(s0, 10.0, 0.1)
    s1 = with_positions(s0, P1)
    P2 = scaled_thirds(s1, 0.03, 40.0)
    return s0, (s1, P1), (with_positions(s0, P2), P2)


def qn_cameras():
    """The reference camera, and one whose WVP has another scale (every clip-space edge three times as long)."""
    wvp, wv = rt.camera_reference(W, H)
    return (wvp, wv), ((np.asarray(wvp, np.float32) * np.float32(3)).astype(np.float32), wv)


def assert_rose_and_fell(before, after):
    (r0, e0), (r1, e1) = before, after
    both = np.intersect1d(r0, r1)
    assert (e1[both] > e0[both]).any() and (e1[both] < e0[both]).any()


def walk_tree_now(c, s, cam, bounces=1):
    """The walk tree the next trace makes (RTBVH_WALK_TREE=1, a certified context) against its model."""
    builds = c.stats()["walk_tree_builds"]
    c.trace(W, H, bounces)
    st = c.stats()
    assert st["walk_tree_used"] == 1 and st["walk_tree_builds"] == builds + 1
    walk_tree_equals_the_model(c, s, cam[0])


@pytest.mark.parametrize("kind", list(QN_KINDS))
def test_qnodes_after_refits_and_a_rebuild(kind, monkeypatch):
    """The built tree's QNodes against their model after update + refit (E rises and falls), a second refit from
    there, a camera-only refit under a WVP of another scale, and the rebuild that follows: on a one-workgroup
    tree, a multi-kernel records tree and a certified context's node-box tree (there also the walk tree)."""
    monkeypatch.setenv("RTBVH_WALK_TREE", "1")
    n, flags = QN_KINDS[kind]
    s0, (s1, P1), (s2, P2) = qn_states(n)
    cam, cam2 = qn_cameras()
    with rt.Context(device=0, flags=flags) as c:
        c.set_scene(s0)
        c.set_camera(*cam)
        c.build()
        built = check_qnodes_live(c, s0, cam)
        if flags & CERT:
            walk_tree_now(c, s0, cam)   # (one of the old geometry: the refit has to drop it)
        c.update_vertices(P1)
        c.refit()
        first = check_qnodes_live(c, s1, cam)
        assert_rose_and_fell(built, first)
        if flags & CERT:
            walk_tree_now(c, s1, cam)
        c.update_vertices(P2)
        c.refit()
        second = check_qnodes_live(c, s2, cam)
        assert_rose_and_fell(first, second)
        c.set_camera(*cam2)
        c.refit()
        scaled = check_qnodes_live(c, s2, cam2)
        assert scaled[1][0] > second[1][0]   # (the root's E: the longest edge, three times as long)
        c.build()
        check_qnodes_live(c, s2, cam2)


def test_qnodes_after_graph_replays(monkeypatch):
    """CERTIFIED | GRAPH: the captured frame replayed under a moved camera, then after a vertex update; the QNodes
    and, from a trace outside the graph, the walk tree of each state; then a rebuild."""
    monkeypatch.setenv("RTBVH_WALK_TREE", "1")
    s0, (s1, P1), _ = qn_states(2049)
    cam, cam2 = qn_cameras()
    with rt.Context(device=0, flags=CERT | MK | rt.FLAG_GRAPH) as c:
        c.set_scene(s0)
        c.set_camera(*cam)
        c.compute_bvh(W, H, 1)
        c.compute_bvh(W, H, 1)
        assert c.stats()["graph_captures"] == 1
        built = check_qnodes_live(c, s0, cam)
        c.set_camera(*cam2)
        c.compute_bvh(W, H, 1)
        assert c.stats()["graph_captures"] == 1   # a replay
        moved = check_qnodes_live(c, s0, cam2)
        assert moved[1][0] > built[1][0]   # (the root's E: the longest edge, three times as long)
        walk_tree_now(c, s0, cam2)
        c.update_vertices(P1)
        c.compute_bvh(W, H, 1)
        assert c.stats()["graph_captures"] == 1
        check_qnodes_live(c, s1, cam2)
        walk_tree_now(c, s1, cam2)
        c.build()
        check_qnodes_live(c, s1, cam2)


@pytest.mark.parametrize("kind", ["one workgroup", "records"])
def test_qnodes_derived_on_a_plain_context(kind, monkeypatch):
    """A plain context (the reference-order walks: its build quantizes no node): the QNodes the first certified
    query derives, those after a refit, the walk tree a certified trace then makes of that tree, and a rebuild."""
    monkeypatch.setenv("RTBVH_WALK_TREE", "1")
    n, flags = QN_KINDS[kind]
    s0, (s1, P1), _ = qn_states(n)
    cam, _ = qn_cameras()
    with rt.Context(device=0, flags=flags) as c:
        c.set_scene(s0)
        c.set_camera(*cam)
        c.build()
        tree = c.read_bvh()
        o, d = random_rays(tree, 256)
        rays = rt.make_rays(o, d)
        tris = rw.clip_triangles(s0.vertices, s0.indices, cam[0])
        assert_hits_equal(c.query(rays, rt.QUERY_CERTIFIED), rw.walk(tree, tris, o, d), "certified")
        derived = check_qnodes_live(c, s0, cam)
        c.set_flags(flags | CERT)
        walk_tree_now(c, s0, cam)
        c.set_flags(flags)
        c.update_vertices(P1)
        c.refit()
        refitted = check_qnodes_live(c, s1, cam)
        assert_rose_and_fell(derived, refitted)
        tris = rw.clip_triangles(s1.vertices, s1.indices, cam[0])
        assert_hits_equal(c.query(rays, rt.QUERY_CERTIFIED), rw.walk(c.read_bvh(), tris, o, d), "after the refit")
        c.set_flags(flags | CERT)
        walk_tree_now(c, s1, cam)
        c.set_flags(flags)
        c.build()
        check_qnodes_live(c, s1, cam)


# ---------------------------------------------------------------- 7. the C++ host's --animate mode
@pytest.mark.parametrize("refit", [False, True], ids=["rebuild", "refit"])
def test_tool_animates_over_the_c_abi(tmp_path, refit):
    import json
    import subprocess

    from tests.test_tools import TOOL, _build_tool
    _build_tool()
    out = tmp_path / "last.bmp"
    r = subprocess.run([TOOL, "--synthetic", "5000", "--width", "64", "--height", "64", "--animate", "3",
                        "--bmp", str(out)] + (["--refit"] if refit else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["animate"] == 3 and rec["refit"] is refit and rec["tris"] == 5000 and rec["update_ms_median"] > 0
    assert out.stat().st_size == 54 + 64 * 64 * 3   # the last frame, as a 24-bit BMP
