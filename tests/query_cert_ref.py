"""Numpy restatements for the certified ray queries (QUERY_CERTIFIED; trace.hip k_query_wide).

A helper of tests/test_query_certified_cpu.py and tests/test_query_certified_gpu.py, not a test: the claim test
that decides which rays the 4-wide walk takes, the per-ray certificate, the initial-key encoding of t_max, and
the rays the two test files share.
"""
import functools

import numpy as np

from tests import cert_scenes as cs
from tests import deep_scenes as ds
from tests import ray_walk_ref as rw
from tests.test_query_gpu import random_rays

MT_DD = np.float32(1.0 + 2.0 ** -18)   # margin.h: the largest d.d the margin's A covers
SENTINEL = np.uint64(0xFFFFFFFF)


def uncovered_mask(o, d):
    """The walk's claim test, !(qnode_fast_ray(o, 1 / d) && dot(d, d) <= MT_DD): max |1 / d_k| <= 2^20 and
    max |o_k| <= 2^90 (maxima that drop NaN, comparisons that are false for NaN), and d.d summed left to right."""
    o = np.ascontiguousarray(o, np.float32)
    d = np.ascontiguousarray(d, np.float32)
    with np.errstate(all="ignore"):
        inv = np.abs((np.float32(1) / d).astype(np.float32))
        mi = np.fmax(np.fmax(inv[:, 0], inv[:, 1]), inv[:, 2])
        ao = np.abs(o)
        mo = np.fmax(np.fmax(ao[:, 0], ao[:, 1]), ao[:, 2])
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return ~((mi <= np.float32(2.0 ** 20)) & (mo <= np.float32(2.0 ** 90)) & (dd <= MT_DD))


def leaf_box_passes(tris, tri, o, d, bound):
    """The certificate: the own box of triangle tri[k] (min / max of its clip-space vertices) passes the reference
    slab test of ray k with the bound bound[k]: 0 <= tmax, tmin <= tmax, tmin <= bound."""
    p = tris[tri]
    with np.errstate(all="ignore"):
        inv = (np.float32(1) / d).astype(np.float32)
        ok, mn = rw._box(p.min(1), p.max(1), o, inv)
        return ok & (mn <= bound)


def cert_failures(tris, want, o, d):
    """Rays whose restated closest hit (want: rw.walk's dict) fails its own certificate: whatever a walk that finds
    this hit does, it cannot vouch for it, and one that finds another hit differs from the reference."""
    h = np.nonzero(want["hit"])[0]
    bad = np.zeros(len(o), bool)
    bad[h] = ~leaf_box_passes(tris, want["tri"][h].astype(np.int64), o[h], d[h], want["t"][h])
    return bad


def brute_force_keys(nodes, tris, o, d, t_max):
    """The walk's u64 key without a tree: start at (t_max, 0xFFFFFFFF), take the lexicographic (t, leaf) minimum over
    every leaf's triangle test.  Returns (key, tri): a key whose low word is still the sentinel is a miss."""
    n = (len(nodes) + 1) // 2
    key = rw.bits(np.asarray(t_max, np.float32)).astype(np.uint64) << np.uint64(32) | SENTINEL
    tri = np.full(len(o), rw.NONE, np.uint32)
    for j in range(n):
        k3 = int(nodes["index"][j]) // 3
        t, _, _ = rw.tri_test(tris, np.full(len(o), k3, np.int64), o, d)
        k = np.where(t == -1, ~np.uint64(0), rw.bits(t).astype(np.uint64) << np.uint64(32) | np.uint64(j))
        better = k < key
        key = np.where(better, k, key)
        tri = np.where(better, np.uint32(k3), tri)
    return key, tri


def key_t(key):
    return (key >> np.uint64(32)).astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------- shared inputs
HALL_RAYS = {"small": 4096, "large": 8192}
# (hits, certificate failures) of the halls' rays, seed 7: what the CPU test pins and the GPU test relies on
HALL_EXPECT = {"small": (1602, 89), "large": (3526, 59)}


@functools.lru_cache(maxsize=None)
def hall_case(variant):
    """(tris, o, d, want, bad) of hall(variant, "A") with HALL_RAYS[variant] random rays, seed 7: the restated
    closest hits and the rays whose hit fails its certificate.  Computed once, read-only."""
    s, _, nodes, wvp, _ = cs.hall(variant, "A")
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    o, d = random_rays(nodes, HALL_RAYS[variant], seed=7)
    want = rw.walk(nodes, tris, o, d)
    bad = cert_failures(tris, want, o, d)
    for a in (o, d, bad, *want.values()):
        a.setflags(write=False)
    return tris, o, d, want, bad


def fan_window_rays(count=2048, seed=1):
    """Rays from z = -0.1 through the fan's window (deep_scenes.P, .R shrunk by half a unit), nearly along +z."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(12.5, 27.5, count), rng.uniform(4.5, 19.5, count), np.full(count, -0.1)], 1)
    d = np.stack([rng.uniform(-.004, .004, count), rng.uniform(-.004, .004, count), np.ones(count)], 1)
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    return o.astype(np.float32), d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def fan_case():
    """(tris, o, d, want) of deep_scenes.fan() with fan_window_rays()."""
    s, _, nodes, wvp, _ = ds.fan()
    tris = rw.clip_triangles(s.vertices, s.indices, wvp)
    o, d = fan_window_rays()
    want = rw.walk(nodes, tris, o, d)
    for a in (o, d, *want.values()):
        a.setflags(write=False)
    return tris, o, d, want


def extra_uncovered_rays(nodes):
    """Rays beside test_query_gpu.edge_rays: a direction component of 1e-8 (|1 / d| = 1e8 > 2^20), origins at
    2^100 (> 2^90), both uncovered; and unit rays shortened to |d| = 0.5, covered.  Returns (o, d)."""
    o, d = random_rays(nodes, 48, seed=21)
    o, d = o.copy(), d.copy()
    d[0:16, 0] = np.float32(1e-8)
    d[0:16] /= np.sqrt((d[0:16] * d[0:16]).sum(1, keepdims=True))
    d[0:16, 0] = np.float32(1e-8)
    o[16:32, 1] = np.float32(2.0 ** 100)
    d[32:48] *= np.float32(0.5)
    return o.astype(np.float32), d.astype(np.float32)
