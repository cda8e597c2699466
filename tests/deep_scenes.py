"""Scenes with deep trees (plain numpy + rt.Scene; used from CPU and GPU tests, like tests/cert_scenes.py).

fan_scene: about a hundred triangles whose tree is some 36 levels deep, and whose leaf boxes all hold one window
of the frame.  The one-ray-per-lane walks keep their stack entries [0, 16) in LDS and the rest in scratch, the
4-wide bounce walk entries [0, 13) (trace.hip LANE_LSB, SB, SW); the OBJ and uniform-soup scenes of the other
tests need at most 12 entries, so only a scene like this one reaches the scratch part and the hand-over.

The camera is the identity (clip space = object space), so the primary ray of pixel (x, y) of a 320 x 240 frame
is o = ((x - 160) / 4, (y - 120) / 4, 0), d = +z.  Two pin triangles at (0, 0, Z0) and (1024 U, 1024 U, Z0 +
1024 UZ) fix the mesh box, and with it the CPUTests Morton grid: a triangle whose centroid is ((qx + .5) U,
(qy + .5) U, Z0 + (qz + .5) UZ) has the code of cell (qx, qy, qz).  The fan's cells are (0, 0, 0), (2^j, 0, 0),
(0, 2^j, 0) (j = 0..8) and (0, 0, 2^j) (j = 0..9): their codes but 0 are powers of two, so an internal node
above the cell-0 subtree has ONE leaf as its right child and everything below as its left child.  `dups` more
triangles in cell (0, 0, 0) hang a balanced subtree (split by index) under the last of them.

Every fan triangle is v0 = (P - R, z - DZ), v1 = (P + R, z + DZ), v2 = (3 c - 2 P, z): its centroid is (c, z), its
box holds the window [P - R, P + R] in xy, and only the rays on one side of the window's diagonal meet it.  A ray
along +z through the window therefore passes the box test of both children at every level and pushes the right
one -- in the reference order always, and in a nearest-first order because each right leaf lies behind its left
sibling's subtree (the z-cell-0 leaves take z in rising code order, the cell-(0, 0, 0) triangles first).

The mesh box begins behind the camera (Z0 < 0): the fan lies in z > 0, a mirror at z = 300 behind it, another
at z = -0.2 behind the camera, both a little tilted.  A ray that meets no fan triangle goes to and fro between
the mirrors through all the boxes, so every bounce pass has rays as deep as the primary pass: the reference
order on both ways, a nearest-first order on the way up (on the way down the single leaf is the nearer child,
and the walk pushes the subtree instead and pops it at once).

crossing_scene: 32,770 triangles whose sorted codes give the grouped refit (build.hip k_refit_group) a group of
64 refit workgroups with more than GCAP = 1024 crossing nodes -- the branch that runs the global protocol for
all of them, which no random tree reaches (about 600 at most).
"""
import functools
import os

import numpy as np

import raytracebvh_amd as rt
from oracle import lib as orc
from tests.cert_scenes import _material, _painted, camera, oscene_of

W, H = 320, 240
U, UZ = 64.0, 0.5          # the Morton cell: U in x and y, UZ in z (the mesh box is 1024 cells a side)
Z0 = -0.25                 # the mesh box's least z: z-cell qz is [Z0 + qz UZ, Z0 + (qz + 1) UZ)
P, R = (20.0, 12.0), 8.0   # the window's centre and half side
DZ = 0.0005                # half the depth of a fan triangle (see fan_scene)
MIRROR_Z, MIRROR_NORMAL = 300.0, (0.004, 0.0026, -1.0)    # behind the fan
FRONT_Z, FRONT_NORMAL = -0.2, (-0.003, 0.002, -1.0)       # behind the camera


def _tiny(at, sign):
    """A pin: a small triangle with one vertex at `at`, the others `sign` * 1/8 away in x and in y."""
    x, y, z = at
    return [(x, y, z), (x + sign * 0.125, y, z), (x, y + sign * 0.125, z)]


def fan_scene(dups=64):
    """The fan (module docstring) as an rt.Scene: 1 + dups + 9 + 9 + 10 fan triangles, the two mirrors, the two
    pins.  Every third triangle has the shading normal (0, 0, -1) (a ray along z leaves it along z: the certified
    bounce walk defers it, trace.hip DEFER_*), the others' are tilted; five colours in turn, as the halls of
    tests/cert_scenes.py.  dups = 64 gives a 36-level tree; 4096 gives 42 levels, and an oracle frame of minutes.

    A fan triangle is not quite flat: v0 and v1 are DZ below and above its z.  A flat triangle's box has no depth,
    its slab entry along +z is exactly z, and Moller-Trumbore's t may round below it -- the containment failure
    of tests/containment.py, which the uncertified nearest-first walks answer differently.
    tests/test_deep_scenes_cpu.py checks that every hit of the frame lies inside its leaf's slab interval."""
    cells = [(0, 0, 0)] * (1 + dups)
    for j in range(9):
        cells += [(1 << j, 0, 0), (0, 1 << j, 0)]
    zcells = [(0, 0, 1 << j) for j in range(10)]
    # the z-cell-0 leaves: distinct z in Z0 + (0.56, 0.94) UZ rising with the Morton code (ties: with the index)
    # -- the cell-(0, 0, 0) triangles first, then y0, x0, y1, x1, ...
    code = lambda q: sum(((q[0] >> b & 1) << (3 * b + 2)) | ((q[1] >> b & 1) << (3 * b + 1)) for b in range(10))
    order = sorted(range(len(cells)), key=lambda k: (code(cells[k]), k))
    zs = np.empty(len(cells))
    zs[order] = Z0 + np.linspace(0.56, 0.94, len(cells)) * UZ   # (in front of the camera: z in [0.03, 0.22])
    tris = []
    for (qx, qy, qz), z in list(zip(cells, zs)) + [(q, Z0 + (q[2] + 0.5) * UZ) for q in zcells]:
        cx, cy = (qx + 0.5) * U, (qy + 0.5) * U
        tris.append([(P[0] - R, P[1] - R, z - DZ), (P[0] + R, P[1] + R, z + DZ), (3 * cx - 2 * P[0], 3 * cy - 2 * P[1], z)])
    nfan = len(tris)
    tris.append([(0.0, 0.0, MIRROR_Z - 1.0), (400.0, 0.0, MIRROR_Z + 0.5), (0.0, 400.0, MIRROR_Z + 0.5)])
    # the front mirror: over the window, its centroid (338, 12) in z-cell 0
    tris.append([(8.0, 0.0, FRONT_Z - 0.02), (8.0, 24.0, FRONT_Z + 0.01), (998.0, 12.0, FRONT_Z + 0.01)])
    tris.append(_tiny((0.0, 0.0, Z0), 1.0))
    tris.append(_tiny((1024 * U, 1024 * U, Z0 + 1024 * UZ), -1.0))
    tris = np.array(tris, np.float32)
    rng = np.random.default_rng(36)
    nrm = np.concatenate([rng.uniform(0.01, 0.03, (len(tris), 2)) * rng.choice([-1.0, 1.0], (len(tris), 2)),
                          np.full((len(tris), 1), -1.0)], 1)
    nrm[np.arange(len(tris)) % 3 == 0, :2] = 0.0   # flat normals: rays the certified bounce walk defers
    nrm[nfan], nrm[nfan + 1] = MIRROR_NORMAL, FRONT_NORMAL
    v = np.zeros((3 * len(tris), 8), np.float32)
    v[:, :3] = tris.reshape(-1, 3)
    v[:, 3:6] = np.repeat(nrm.astype(np.float32), 3, axis=0)
    s = rt.Scene(v, np.arange(3 * len(tris), dtype=np.uint32), np.zeros(len(tris), np.uint32), _material(900.0))
    return _painted(s)


@functools.lru_cache(maxsize=None)
def fan(dups=64):
    """(scene, oracle scene, oracle tree, wvp, wv) of the fan under the identity camera; built once."""
    s = fan_scene(dups)
    wvp, wv = camera("A")
    os_ = oscene_of(s)
    return s, os_, orc.build(os_, wvp), wvp, wv


@functools.lru_cache(maxsize=None)
def fan_oracle(bounces=3, width=W, height=H, dups=64):
    """The oracle's whole frame of the fan: dict(fb, inten, stats).  Computed once, read-only: shared."""
    _, os_, nodes, wvp, wv = fan(dups)
    orc.set_threads(max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or 0) or (os.cpu_count() or 1))))
    try:   # (the oracle's result does not depend on its threads: tests/test_oracle_threads.py)
        fb, inten, st = orc.trace(os_, nodes, wvp, wv, width, height, bounces, want_intensity=True)
    finally:
        orc.set_threads(1)
    for a in (fb, inten):
        a.setflags(write=False)
    return dict(fb=fb, inten=inten, stats=st)


# ---------------------------------------------------------------- the grouped refit's fallback
RBLOCK = 512             # build.hip RBLOCK (RTBVH_REFIT_BLOCK): node indices per refit workgroup
GSPAN = 64 * RBLOCK      # build.hip GSPAN = RGROUP * RBLOCK: node indices per group of refit workgroups
GCAP = 1024              # build.hip GCAP: the crossing nodes a group climbs in LDS
CLUSTERS = 63
CROSSING_T = GSPAN + 2


def crossing_codes():
    """The crafted sorted sequence of CROSSING_T 30-bit codes.  Index 0 is the pin's code 0 and the last index the
    other pin's 2^30 - 1.  Around each multiple B = 512 c of RBLOCK (c = 1..63) sits a cluster of 19 codes with
    the upper 12 bits 64 c, at indices [B - 10, B + 8]: over the low 18 bits an alternating caterpillar -- the
    cluster's leftmost code alone has bit 17 clear, of the rest the rightmost alone has bit 16 set, of the rest
    the leftmost alone has bit 15 clear, ... and the last two differ in bit 0 and sit at B - 1 and B.  Each of
    the 18 nested ranges holds B - 1 and B, and its node's index is one of the range's ends, within 10 of B: 18
    crossing nodes (build.hip crossing()) a cluster, and the nodes that join a cluster to its neighbours.
    Between the clusters, runs of one duplicate code (upper bits 64 c + 32), split by index inside one
    workgroup's span."""
    codes = np.zeros(CROSSING_T, np.uint32)
    codes[1:] = 32 << 18                       # the run before the first cluster
    for c in range(1, CLUSTERS + 1):
        B = RBLOCK * c
        lo, hi = B - 10, B + 8                 # the caterpillar's remaining range
        fixed = 0                              # the low bits every remaining code shares
        low = np.zeros(19, np.uint32)
        for bit in range(17, 0, -1):
            if bit % 2:                        # peel the leftmost: it alone has the bit clear
                low[lo - (B - 10)] = fixed | ((1 << bit) - 1)   # (the bits below: any; all set keeps it < the rest)
                fixed |= 1 << bit
                lo += 1
            else:                              # peel the rightmost: it alone has the bit set
                low[hi - (B - 10)] = fixed | (1 << bit)
                hi -= 1
        assert (lo, hi) == (B - 1, B)
        low[lo - (B - 10)], low[hi - (B - 10)] = fixed, fixed | 1
        codes[B - 10:B + 9] = ((64 * c) << 18) | low
        codes[B + 9:] = (64 * c + 32) << 18    # the run after it (overwritten by the next cluster)
    codes[-1] = (1 << 30) - 1
    assert (np.diff(codes.astype(np.int64)) >= 0).all()
    return codes


def _cells_of(codes):
    """CPUTests Morton code -> cell (qx, qy, qz): x in bits 3j + 2, y in 3j + 1, z in 3j."""
    c = codes.astype(np.int64)
    q = np.zeros((len(c), 3), np.int64)
    for j in range(10):
        q[:, 0] |= (c >> (3 * j + 2) & 1) << j
        q[:, 1] |= (c >> (3 * j + 1) & 1) << j
        q[:, 2] |= (c >> (3 * j) & 1) << j
    return q


def crossing_camera():
    """The mesh box [0, 1024]^3 scaled into a 64 x 48 frame's rays (x in [-8, 8), y in [-6, 6)), z in [1, 65]."""
    m = np.zeros((4, 4), np.float32)
    m[0, 0], m[1, 1], m[2, 2], m[3, 3] = 1 / 64, 3 / 256, 1 / 16, 1
    m[3, :3] = (-8, -6, 1)
    return m.ravel(), m.ravel().copy()


def crossing_scene(seed=5):
    """Triangles whose CPUTests Morton codes, once sorted, are crossing_codes(): the two pins at (0, 0, 0) and
    (1024, 1024, 1024) (cells of size 1), and one triangle a code with its centroid within 0.3 of its cell's
    centre (the duplicates of a run differ in it) and vertices up to 120 away, kept inside the mesh box.  The
    triangles are dealt in a shuffled order, so the sort has work to do."""
    codes = crossing_codes()[1:-1]
    rng = np.random.default_rng(seed)
    n = len(codes)
    cen = _cells_of(codes) + 0.5 + rng.uniform(-0.3, 0.3, (n, 3))
    off = rng.uniform(-1.0, 1.0, (n, 3, 3))
    off -= off.mean(axis=1, keepdims=True)                        # the centroid stays
    room = np.minimum(cen, 1024 - cen).min(axis=1)                # to the mesh box's nearest face
    off *= (np.minimum(120.0, 0.5 * room) / np.abs(off).max(axis=(1, 2)))[:, None, None]
    tris = (cen[:, None, :] + off)[rng.permutation(n)]
    tris = np.concatenate([tris, [_tiny((0.0, 0.0, 0.0), 1.0), _tiny((1024.0, 1024.0, 1024.0), -1.0)]]).astype(np.float32)
    nrm = np.concatenate([rng.uniform(-0.3, 0.3, (len(tris), 2)), np.full((len(tris), 1), -1.0)], 1)
    v = np.zeros((3 * len(tris), 8), np.float32)
    v[:, :3] = tris.reshape(-1, 3)
    v[:, 3:6] = np.repeat(nrm.astype(np.float32), 3, axis=0)
    s = rt.Scene(v, np.arange(3 * len(tris), dtype=np.uint32), np.zeros(len(tris), np.uint32), _material())
    return _painted(s)


@functools.lru_cache(maxsize=None)
def crossing():
    """(scene, oracle scene, oracle tree, wvp, wv) of the crossing scene; built once."""
    s = crossing_scene()
    wvp, wv = crossing_camera()
    os_ = oscene_of(s)
    nodes = orc.build(os_, wvp)
    nodes.setflags(write=False)
    return s, os_, nodes, wvp, wv


def leaf_ranges(nodes):
    """(first, last) leaf of every internal node of a NODE_DTYPE tree (leaves [0, n), internal k at n + k)."""
    n = (len(nodes) + 1) // 2
    cl, cr = nodes["child_l"].astype(np.int64), nodes["child_r"].astype(np.int64)
    first, last = np.arange(2 * n - 1), np.arange(2 * n - 1)
    order, todo = [], [n]
    while todo:
        x = todo.pop()
        order.append(x)
        todo.extend(c for c in (cl[x], cr[x]) if c >= n)
    for x in reversed(order):   # children before parents
        first[x], last[x] = first[cl[x]], last[cr[x]]
    return first[n:], last[n:]


def crossing_per_group(nodes):
    """The crossing nodes of each group of 64 refit workgroups, as build.hip counts them (crossing(), k_refit's
    xlist, k_refit_group's m): internal node k crosses when its leaf range is not inside [k & ~(RBLOCK - 1),
    + RBLOCK), and it is listed in the group of its own index, k // GSPAN."""
    first, last = leaf_ranges(nodes)
    k = np.arange(len(first))
    base = k & ~(RBLOCK - 1)
    cross = ~((first >= base) & (last < base + RBLOCK))
    return np.bincount(k[cross] // GSPAN, minlength=(len(k) + GSPAN - 1) // GSPAN)
