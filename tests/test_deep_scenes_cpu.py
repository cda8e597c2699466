"""The deep-tree scenes (tests/deep_scenes.py) do what the GPU tests need of them, by the CPU oracle and the numpy
restatement of its walk alone: the fan's rays need stack entries far past the part the walks keep in LDS (16 for
the one-ray-per-lane walks, 13 for the 4-wide bounce walk) in the primary pass and in every bounce pass, beside
shallow rays in the same waves; the crossing scene's tree gives one group of refit workgroups more crossing nodes
than k_refit_group climbs in LDS.  Without this the GPU tests (tests/test_deep_trees_gpu.py) could pass on scenes
that reach neither."""
import functools

import numpy as np
import pytest

from oracle import lib as orc
from tests import cert_scenes as cs
from tests import deep_scenes as ds
from tests import ray_walk_ref as rw
from tests.conftest import load_scene_fixture
from tests.test_query_cpu import primary_rays

BOUNCES = 3


@functools.lru_cache(maxsize=None)
def _fan_passes():
    """[(origins, directions, the restated reference-order walk)]: the primary rays, then the rays entering each
    of the BOUNCES bounce passes."""
    s, os_, nodes, wvp, wv = ds.fan()
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    rays = [primary_rays(ds.W, ds.H)]
    rays += [cs.entering_rays(os_, nodes, wvp, wv, ds.W, ds.H, b)[1:] for b in range(BOUNCES)]
    return [(o, d, rw.walk(nodes, tris, o, d)) for o, d in rays]


def test_fan_restatement_matches_the_oracle():
    """max_stack comes from the restatement: its walks are the oracle's (hits, visits, the deepest stack)."""
    want = ds.fan_oracle(BOUNCES)["stats"]
    walks = [r for _, _, r in _fan_passes()]
    assert sum(int(r["hit"].sum()) for r in walks) == want["hits"]
    assert sum(int(r["internal"].sum()) for r in walks) == want["internal_visits"]
    assert sum(int(r["leaf"].sum()) for r in walks) == want["leaf_visits"]
    assert max(int(r["max_stack"].max()) for r in walks) == want["max_stack"]
    assert sum(len(r["hit"]) for r in walks[1:]) == want["bounce"]


def test_fan_primary_rays_are_deep():
    ms = _fan_passes()[0][2]["max_stack"]
    print(f"primary: {(ms >= 30).sum()} rays at >= 30, max {ms.max()}, {(ms < 8).sum()} below 8")
    assert (ms >= 30).sum() >= 5000
    assert (ms < 8).sum() >= 5000
    # a wave of the lane walk is 8 x 8 pixels: some hold deep and shallow rays
    tiles = ms.reshape(ds.H // 8, 8, ds.W // 8, 8)
    assert ((tiles.max(axis=(1, 3)) >= 30) & (tiles.min(axis=(1, 3)) < 8)).sum() >= 10
    # with the reference's own 32 entries (RayTraceTraversal.hlsl:9) the walk would overflow here ...
    assert (ms >= 32).sum() > 0


def test_reference_stack_is_enough_on_its_own_mesh():
    """... although it does not on Test.obj (what tests/test_deep_trees_gpu.py asserts of stack_limit=32)."""
    d = load_scene_fixture("Test")
    s = orc.Scene(d["vertices"], d["indices"], d["mat_indices"], d["material_blob"])
    wvp, wv = orc.camera_reference(ds.W, ds.H)
    st = orc.trace(s, orc.build(s, wvp), wvp, wv, ds.W, ds.H, BOUNCES)[2]
    assert st["max_stack"] < 16


@pytest.mark.parametrize("p", [1, 2, 3])
def test_fan_bounce_passes_are_deep(p):
    ms = _fan_passes()[p][2]["max_stack"]
    print(f"pass {p}: {len(ms)} rays, {(ms >= 24).sum()} at >= 24, max {ms.max()}, {(ms < 8).sum()} below 8")
    assert (ms >= 24).sum() >= 1000
    assert (ms < 8).sum() >= 256


@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_fan_is_deep_in_the_nearest_first_order_too(p):
    """The binary nearest-first rule (ray_walk_ref.walk order="nearest") on the primary rays and on the rays
    entering each bounce pass: the reference order's hits, and stacks as deep -- a nearest-first walk that ended
    at its first hit's distance would stay shallow here, so the GPU probes of the nearest-first modes at
    stack_limit = 20 have rays to answer them in every pass."""
    s, _, nodes, wvp, _ = ds.fan()
    o, d, ref = _fan_passes()[p]
    q = rw.walk(nodes, rw.clip_triangles(s.vertices, s.indices, wvp), o, d, order="nearest")
    np.testing.assert_array_equal(rw.bits(q["t"]), rw.bits(ref["t"]))
    np.testing.assert_array_equal(q["tri"], ref["tri"])
    print(f"pass {p}: {(q['max_stack'] >= 24).sum()} rays at >= 24, max {q['max_stack'].max()}")
    assert (q["max_stack"] >= 24).sum() >= 1000
    assert (q["max_stack"] < 8).sum() >= 256


def test_fan_oracle_has_no_overflow_and_defers_rays():
    want = ds.fan_oracle(BOUNCES)["stats"]
    assert want["stack_overflows"] == 0
    assert 30 <= want["max_stack"] < rw.STACK - 1
    o, d, _ = _fan_passes()[1]
    assert cs.deferred_mask(o, d).sum() >= 1000   # the flat normals: rays for k_bounce_redo, deep ones among them


def test_fan_hits_lie_inside_their_leaf_slabs():
    """Containment (tests/containment.py): every ray's closest hit enters its leaf's box no later than it meets the
    triangle.  Where that fails, the uncertified nearest-first walks may answer with another triangle than the
    reference order; the fan's triangles have a little depth so that it holds."""
    s, _, nodes, _, _ = ds.fan()
    n = s.num_tris
    leaf_of_tri = np.empty(n, np.int64)
    leaf_of_tri[nodes["index"][:n] // 3] = np.arange(n)
    for p, (o, d, r) in enumerate(_fan_passes()):
        h = r["hit"]
        lf = leaf_of_tri[r["tri"][h].astype(np.int64)]
        with np.errstate(all="ignore"):
            inv = (np.float32(1) / d[h]).astype(np.float32)
        ok, mn = rw._box(nodes["bb_min"][lf], nodes["bb_max"][lf], o[h], inv)
        assert ok.all(), p
        assert (mn <= r["t"][h]).all(), p


def test_fan_tree_is_a_caterpillar_over_a_balanced_subtree():
    s, _, nodes, _, _ = ds.fan()
    n = s.num_tris
    assert n == 64 + 1 + 28 + 4
    codes = nodes["code"][:n]
    assert (codes == 0).sum() == 66                       # cell (0, 0, 0): 1 + dups triangles and a pin
    power = codes[(codes != 0) & (codes & (codes - 1) == 0)]
    assert len(power) == 28 and len(set(power.tolist())) == 28
    depth = np.zeros(2 * n - 1, np.int64)
    for x in range(n, 2 * n - 1):                         # (a node's parent has the smaller index or is the root)
        k, dd = x, 0
        while nodes["parent"][k] != 0xFFFFFFFF:
            k, dd = nodes["parent"][k], dd + 1
        depth[x] = dd
    assert depth.max() + 1 >= 35


def test_crossing_codes_are_the_scenes():
    s, _, nodes, _, _ = ds.crossing()
    assert s.num_tris == ds.CROSSING_T > 8192             # past the one-workgroup build
    np.testing.assert_array_equal(nodes["code"][:s.num_tris], ds.crossing_codes())
    p = s.vertices[:, :3]
    assert (p.min(0) == 0).all() and (p.max(0) == 1024).all()


def test_crossing_scene_fills_one_group_past_gcap():
    per_group = ds.crossing_per_group(ds.crossing()[2])
    print("crossing nodes per group:", per_group)
    assert per_group.max() > ds.GCAP
    assert (np.sort(per_group)[:-1] < ds.GCAP).all()
    # the count is the tree's, not the triangles': the codes alone give it
    codes = ds.crossing_codes()
    t = np.zeros(2 * len(codes) - 1, orc.NODE_DTYPE)
    t["parent"], t["child_l"], t["child_r"] = orc.karras(codes)
    np.testing.assert_array_equal(ds.crossing_per_group(t), per_group)


def test_crossing_helper_on_a_random_tree():
    """A random tree stays far below GCAP (the other builds of the suite never take the branch), and the helper
    counts what a direct walk of the definition counts."""
    rng = np.random.default_rng(1)
    codes = np.sort(rng.integers(0, 1 << 30, 70_000, dtype=np.uint32))
    t = np.zeros(2 * len(codes) - 1, orc.NODE_DTYPE)
    t["parent"], t["child_l"], t["child_r"] = orc.karras(codes)
    per_group = ds.crossing_per_group(t)
    assert len(per_group) == 3 and 0 < per_group.max() < ds.GCAP
    n = len(codes)

    def span(x):   # the leaves below node x, by descent
        a = b = x
        while a >= n:
            a = t["child_l"][a]
        while b >= n:
            b = t["child_r"][b]
        return a, b
    first, last = ds.leaf_ranges(t)
    for k in rng.integers(0, n - 1, 200):
        assert span(n + k) == (first[k], last[k])


def test_crossing_frame_has_hits_and_misses():
    _, os_, nodes, wvp, wv = ds.crossing()
    st = orc.trace(os_, nodes, wvp, wv, 64, 48, 1)[2]
    assert 64 * 48 // 4 < st["hits"] and st["bounce"] > 500 and st["stack_overflows"] == 0
