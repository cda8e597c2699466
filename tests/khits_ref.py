"""The first-k ray query (include/rtbvh.h rtbvh_khits_*) restated in numpy float32.

A helper of the first-k tests, not a test.  It builds on tests/allhits_ref.py: a ray's members are the all-hits
query's (conditions (B) and (T)), a member's key is (tk, triangle id) with tk = fmax(t, mn), mn the slab entry of
the member's own leaf box, and the answer is the first k members in key order, each as its genuine {t, u, v, tri},
padded with the miss record {-1, 0, 0, 0xFFFFFFFF}.  No tree.
"""
import numpy as np

from tests import allhits_ref as ar
from tests import ray_walk_ref as rw

NONE = np.uint32(0xFFFFFFFF)
INF = ar.INF
HIT_DTYPE = ar.HIT_DTYPE


def members(tris, origins, directions):
    """(offsets, hits, mn) of every ray for t_max = +inf: brute_allhits' lists in triangle order with each member's
    leaf-box slab entry.  select_k cuts them to a smaller t_max."""
    return ar.brute_allhits(tris, origins, directions, INF, np.arange(len(tris)), with_mn=True)


def key_t(hits, mn):
    """tk of each member: fmax drops a NaN, as fmaxf does."""
    return np.fmax(hits["t"], mn).astype(np.float32)


def keys(hits, mn):
    """The uint64 keys tk bits << 32 | tri: tk > 0, so the bits order as the floats."""
    return rw.bits(key_t(hits, mn)).astype(np.uint64) << np.uint64(32) | hits["tri"].astype(np.uint64)


def misses(n, k):
    out = np.zeros((n, k), HIT_DTYPE)
    out["t"], out["tri"] = -1, NONE
    return out


def select_k(lists, k, t_max=INF):
    """The answer from members()' lists: an (n, k) HIT_DTYPE array, each ray's k members with the smallest keys
    among those within t_max (one value or one per ray), ascending, then misses."""
    off, hits, mn = lists
    n = len(off) - 1
    tm = np.broadcast_to(np.asarray(t_max, np.float32), (n,))
    cnt = np.diff(off.astype(np.int64))
    per = np.repeat(tm, cnt)
    with np.errstate(all="ignore"):
        keep = (hits["t"] <= per) & ~(mn > per) & (per > 0)     # allhits_ref.cut's rule
    ray = np.repeat(np.arange(n), cnt)[keep]
    hits, key = hits[keep], keys(hits[keep], mn[keep])
    order = np.lexsort((key, ray))
    ray, hits = ray[order], hits[order]
    start = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(ray, minlength=n), out=start[1:])
    pos = np.arange(len(ray)) - start[ray]
    out = misses(n, k)
    first = pos < k
    out[ray[first], pos[first]] = hits[first]
    return out


def brute_k(tris, origins, directions, k, t_max=INF):
    return select_k(members(tris, origins, directions), k, t_max)


def found(out):
    return out["tri"] != NONE
