"""The split region query (include/rtbvh.h, the split field of rtbvh_region_async) in plain Python on the oracle's tree.

A helper of the split-region tests, not a test.  A region is cut along the tree into at most K pieces -- `expand`,
trace.hip k_region_expand's rounds -- and every piece is walked on its own with an empty stack -- `walk_piece`,
k_region_piece -- the lists laid end to end.  The plane tests are tests/region_ref.py's, made once per region for every
node and every triangle (`Masks`); the model itself is tree logic on those booleans.

Nodes are the oracle's: leaves [0, n), internal nodes [n, 2n - 1), the root n; leaf k holds triangle order[k].
A piece is ("node", x), ("leaf", k) or ("range", lo, length).
"""
import numpy as np

from tests import deep_scenes as ds
from tests import nearest_ref as nr
from tests import region_ref as rr

ROUNDS = 64                 # rtbvh_internal.h REGION_SPLIT_ROUNDS
MAX_PIECES = 1 << 20        # RTBVH_REGION_SPLIT_MAX_PIECES
STACK_SIZE = 66             # rtbvh_device.h


def auto_k(n, field=15):
    """The K the library uses for n regions and a split field value: the field is an upper limit."""
    shift = 12 if field == 15 else field
    while shift > 0 and (n << shift) > MAX_PIECES:
        shift -= 1
    return 1 << shift


class Tree:
    """The oracle's nodes with what the walks need: children, leaf ranges, the leaf order, the leaf data."""

    def __init__(self, nodes, tris):
        self.T = T = len(tris)
        self.nodes = nodes
        self.order = nodes["index"][:T] // 3
        self.first, self.last = ds.leaf_ranges(nodes) if T > 1 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        self.left = nodes["child_l"].astype(np.int64)
        self.right = nodes["child_r"].astype(np.int64)
        self.leaf = nr.leaf_data(tris)
        lo, hi = self.leaf[3], self.leaf[4]
        self.nan_free = not (np.isnan(lo).any() or np.isnan(hi).any())


class Masks:
    """One region against the whole tree: enter / inside per node (the root's box for the root), member per leaf."""

    def __init__(self, tree, planes6, triangle):
        a, e1, e2, lo, hi = tree.leaf
        self.finite = bool(np.isfinite(planes6).all())
        bmin, bmax = tree.nodes["bb_min"], tree.nodes["bb_max"]
        self.enter = rr.box_enter(planes6, bmin, bmax)
        self.inside = rr.box_inside(planes6, bmin, bmax)
        t = tree.order
        member = rr.box_enter(planes6, lo[t], hi[t])               # (B) on the leaf's own box
        if triangle:
            member &= rr.vertices_pass(planes6, a[t], e1[t], e2[t], lo[t], hi[t])
        self.member = member                                       # by leaf position


def expand(tree, m, K, accept, rounds=ROUNDS):
    """(pieces, node tests): the ordered frontier of at most K pieces."""
    n = tree.T
    acc = accept and tree.nan_free
    if not m.finite:
        return [], 0
    if n == 1:
        return [("leaf", 0)], 0
    if not m.enter[n]:
        return [], 0
    if acc and m.inside[n]:
        return [("range", 0, n)], 0
    items, tests = [("node", n)], 0

    def child(x):
        if not m.enter[x]:
            return []
        if x < n:
            return [("leaf", x)]
        if acc and m.inside[x]:
            return [("range", int(tree.first[x - n]), int(tree.last[x - n] - tree.first[x - n] + 1))]
        return [("node", x)]

    for _ in range(rounds):
        if not items or len(items) >= K:
            break
        budget = K - len(items)
        out, nnode = [], 0
        for it in items:
            if it[0] == "node":
                nnode += 1
                if nnode <= budget:                                 # the first K - len NODEs
                    tests += 1
                    out += child(int(tree.left[it[1]])) + child(int(tree.right[it[1]]))
                    continue
            out.append(it)
        items = out
        assert len(items) <= K
        if nnode == 0:
            break
    return items, tests


def walk_piece(tree, m, piece, accept, out, stats, limit=STACK_SIZE):
    """k_region's step loop from the piece's own node with an empty stack; returns the piece's steps."""
    n = tree.T
    acc = accept and tree.nan_free
    steps = 0

    def take(x):
        stats["accepted"] += 1
        out.extend(int(t) for t in tree.order[tree.first[x - n]:tree.last[x - n] + 1])

    if piece[0] == "range":
        stats["accepted"] += 1
        out.extend(int(t) for t in tree.order[piece[1]:piece[1] + piece[2]])
        return 0
    stack = [piece[1]]
    while stack:
        k = stack.pop()
        steps += 1
        if k < n:
            stats["leaf"] += 1
            if m.member[k]:
                out.append(int(tree.order[k]))
            continue
        stats["internal"] += 1
        l, r = int(tree.left[k]), int(tree.right[k])
        lh, rh = bool(m.enter[l]), bool(m.enter[r])
        la = lh and acc and l >= n and bool(m.inside[l])
        ra = rh and acc and r >= n and bool(m.inside[r]) and (la or not lh)
        if la:
            take(l)
        if ra:
            take(r)
        le, re = lh and not la, rh and not ra
        if le and re and len(stack) + 1 >= limit:                   # (k_region: sp + 1 >= limit loses both children)
            stats["overflow"] += 1
            continue
        if re:
            stack.append(r)
        if le:
            stack.append(l)
    return steps


def split_lists(tree, regions, triangle, K, accept=True, limit=STACK_SIZE):
    """(offsets, ids, stats, pieces per region): the split query of every region."""
    got, off, per_region = [], [0], []
    stats = dict(internal=0, leaf=0, accepted=0, overflow=0, tests=0, pieces=0, longest=0)
    for p in rr.as_planes(regions):
        m = Masks(tree, p, triangle)
        items, tests = expand(tree, m, K, accept)
        stats["tests"] += tests
        stats["pieces"] += len(items)
        for it in items:
            stats["longest"] = max(stats["longest"], walk_piece(tree, m, it, accept, got, stats, limit))
        per_region.append(items)
        off.append(len(got))
    return np.array(off, np.uint64), np.array(got, np.uint32), stats, per_region


def plain_steps(tree, regions, triangle, accept=True):
    """internal and leaf steps of the plain walk (one pass): k_region's, the root handled at the claim."""
    stats = dict(internal=0, leaf=0, accepted=0, overflow=0)
    got = []
    n = tree.T
    for p in rr.as_planes(regions):
        m = Masks(tree, p, triangle)
        if not m.finite:
            continue
        if n == 1:
            walk_piece(tree, m, ("leaf", 0), accept, got, stats)
        elif m.enter[n]:
            if accept and tree.nan_free and m.inside[n]:
                continue
            walk_piece(tree, m, ("node", n), accept, got, stats)
    return stats


def leaf_span(tree, piece):
    """[first, last] leaf positions a piece covers."""
    n = tree.T
    if piece[0] == "range":
        return piece[1], piece[1] + piece[2] - 1
    if piece[0] == "leaf" or piece[1] < n:
        return piece[1], piece[1]
    return int(tree.first[piece[1] - n]), int(tree.last[piece[1] - n])


def is_subsequence(sub, full):
    it = iter(full)
    return all(any(x == y for y in it) for x in sub)
