"""Scenes for the certified walks' multi-bounce tests (plain numpy + rt.Scene; used from CPU and GPU tests).

Hall of mirrors.  The camera is the identity (clip space = object space; tests/containment.py), so the
primary ray of pixel (x, y) is o = ((x - W/2) / 4, (y - H/2) / 4, 0), d = +z.  Two walls of small triangles
face each other over the whole frame: at z = +30 with shading normals (tx, ty, -1), at z = -30 with
(tx, ty, +1); shininess 900 keeps a ray's intensity above 0 for many passes.  Triangle k of a wall is FLAT
(tx = ty = 0) when k % every == 0, otherwise |tx|, |ty| are drawn from [0.01, 0.03] with random signs.

A ray along +-z that hits a flat triangle reflects along -+z with two exact zero components: |1/d| is
infinite, the certified bounce walk's slack test cannot take it (trace.hip qnode_fast_ray), and the walk
DEFERS it (trace.hip DEFER_*).  With every_back = 2 * every_front, half of a pass's deferred rays are
deferred again in the next pass, the other half join the certified walk with a tilted direction: every
pass has deferred rays, rays the walk takes, and rays of both kinds feeding the next queue.  The triangles
take five colours in turn, so a pixel tells which triangles its ray met, pass by pass.
"""
import functools
import os

import numpy as np

import raytracebvh_amd as rt
from oracle import lib as orc

W, H = 320, 240
# the rtbvh_stats fields the multi-bounce tests compare (tests/test_certified_bounces_gpu.py _check_stats)
STATS_CHECKED = ("hits", "bounce_rays", "textured_hits", "stack_overflows", "redo_deferred", "redo_rays", "redo_total")

# cells (x, y), cell size, every (front, back)
VARIANTS = {
    "small": ((44, 34), 2.0, (3, 6)),       # 5,984 triangles: the one-workgroup build
    # 141,688: the multi-kernel build, above AUTO's 65,536.  (Not 200 x 180: with a row count that is a multiple
    # of `every`, whole rows of cells are flat, and the frame holds a whole number of such periods -- a moved
    # camera then defers exactly as many rays, and a count left over from the other camera could not be told.)
    "large": ((199, 178), 0.5, (3, 6)),
    "few": ((200, 180), 0.5, (97, 194)),    # the same walls, about 1% of the rays deferred
}


def _material(ns=300.0):
    m = np.zeros(1, rt.MATERIAL_DTYPE)
    m[0]["diffuse"] = (0.64, 0.64, 0.64, 1.0)
    m[0]["specular"] = (0.5, 0.5, 0.5, 1.0)
    m[0]["shininess"] = ns
    m[0]["alpha"] = 1.0
    m[0]["tex_num"] = -1
    return m


def _mesh(tris, normals, ns=300.0):
    """rt.Scene from (n, 3, 3) positions and (n, 3) per-triangle vertex normals, one material."""
    n = len(tris)
    v = np.zeros((3 * n, 8), np.float32)
    v[:, :3] = tris.reshape(-1, 3)
    v[:, 3:6] = np.repeat(normals, 3, axis=0)
    return rt.Scene(v, np.arange(3 * n, dtype=np.uint32), np.zeros(n, np.uint32), _material(ns))


def _grid(n0, n1, lo0, lo1, step):
    """Two triangles per cell of an n0 x n1 grid (cell corners at lo + step * i): (2 n0 n1, 3, 2)."""
    i, j = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    a0, a1 = (lo0 + step * i).ravel(), (lo1 + step * j).ravel()
    b0, b1 = a0 + step, a1 + step
    t1 = np.stack([np.stack([a0, a1], 1), np.stack([b0, a1], 1), np.stack([b0, b1], 1)], 1)
    t2 = np.stack([np.stack([a0, a1], 1), np.stack([b0, b1], 1), np.stack([a0, b1], 1)], 1)
    return np.concatenate([t1, t2])


def camera(name):
    """A: the identity.  B: the identity moved by (3.25, -1.75) -- the walls slide under the rays' grid, so
    other pixels meet the flat triangles."""
    m = np.eye(4, dtype=np.float32).ravel()
    if name == "B":
        m[12], m[13] = 3.25, -1.75
    else:
        assert name == "A"
    return m, m.copy()


def _wall_normals(rng, n, every, nz):
    mag = rng.uniform(0.01, 0.03, (n, 2))
    sign = rng.choice([-1.0, 1.0], (n, 2))
    nrm = np.concatenate([mag * sign, np.full((n, 1), nz)], 1)
    nrm[np.arange(n) % every == 0, :2] = 0.0
    return nrm


def hall_of_mirrors(variant, seed=20):
    (n0, n1), size, (every_front, every_back) = VARIANTS[variant]
    rng = np.random.default_rng(seed)
    # (the grid's origin is off the rays' quarter grid by 0.1: no cell's side under a ray)
    g = _grid(n0, n1, -0.5 * n0 * size - 0.1, -0.5 * n1 * size - 0.1, size)
    n = len(g)
    front = np.concatenate([g, np.full(g.shape[:2] + (1,), 30.0)], 2)
    back = np.concatenate([g, np.full(g.shape[:2] + (1,), -30.0)], 2)
    nrm = np.concatenate([_wall_normals(rng, n, every_front, -1.0), _wall_normals(rng, n, every_back, 1.0)])
    return _painted(_mesh(np.concatenate([front, back]).astype(np.float32), nrm.astype(np.float32), ns=900.0))


def _painted(s):
    """Five colours dealt over the triangles (5 is coprime to every `every`): which triangle a ray hit in which pass
    shows in its pixel -- with one colour, a ray left unshaded or walked for another ray would not."""
    mats = np.repeat(s.materials, 5)
    mats["diffuse"][:, :3] = [(0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.2, 0.3, 0.9), (0.8, 0.8, 0.1), (0.5, 0.1, 0.7)]
    return rt.Scene(s.vertices, s.indices, np.arange(s.num_tris, dtype=np.uint32) % 5, mats)


def strip_scene(tall=False, cells=4100):
    """A strip of 4 * cells = 16,400 small triangles (two rows of cells of size 2) along x -- with `tall`, along
    y -- under every pixel of a 32,776 x 16 frame (x in [-4097, 4096.75], y in [-2, 1.75]), the first and last
    columns included.  It lies in the plane z = 30 + x / 2048 (the mesh box keeps a depth); every third
    triangle's shading normal is (0, 0, -1), the others' tilted as the hall's; coloured as the hall."""
    g = _grid(cells, 2, -cells - 0.05, -2.05, 2.0)
    tris = np.concatenate([g, 30.0 + g[:, :, 0:1] / 2048.0], 2)
    if tall:
        tris = tris[:, :, [1, 0, 2]]
    nrm = _wall_normals(np.random.default_rng(7), len(tris), 3, -1.0)
    return _painted(_mesh(tris.astype(np.float32), nrm.astype(np.float32)))


def oscene_of(s):
    return orc.Scene(s.vertices, s.indices, s.mat_indices, s.material_blob)


def entering_rays(oscene, nodes, wvp, wv, W, H, b):
    """The rays that enter bounce pass b + 1 (b = 0: the first): the oracle's reflectRay records after b passes
    with intensity > 0 -- bit for bit the GPU's queue (test_gpu_parity.py test_ray_records_match_oracle).
    Returns (live mask (H, W), origins (n, 3), directions (n, 3)), float32."""
    refl = orc.trace(oscene, nodes, wvp, wv, W, H, b, want_records=True)[3]
    live = refl[..., 0] > 0
    return live, refl[live][:, 1:4], refl[live][:, 4:7]


def deferred_mask(o, d):
    """The certified walk's claim-time test (trace.hip k_bounce_trav: !(qnode_fast_ray && dot(d, d) <= MT_DD)) for
    rays that pass its |o| <= 2^90 and |d| parts (test_cert_scenes_cpu.py asserts they do, with room): a ray is
    deferred when max_k |float32(1) / d_k| > 2^20.  The library is built with -fno-fast-math, so the device's
    division is the IEEE one numpy makes here."""
    with np.errstate(divide="ignore"):
        inv = np.float32(1) / d.astype(np.float32)
    return np.abs(inv).max(axis=1) > np.float32(2.0 ** 20)


def expected_deferred(oscene, nodes, wvp, wv, W, H, bounces):
    """rtbvh_stats.redo_deferred of a certified frame of `bounces` passes: the deferred rays of every pass."""
    return sum(int(deferred_mask(*entering_rays(oscene, nodes, wvp, wv, W, H, b)[1:]).sum()) for b in range(bounces))


@functools.lru_cache(maxsize=None)
def hall(variant, cam):
    """(scene, oracle scene, oracle tree, wvp, wv) of a variant under camera "A" or "B"; built once."""
    s = hall_of_mirrors(variant)
    wvp, wv = camera(cam)
    os_ = oscene_of(s)
    return s, os_, orc.build(os_, wvp), wvp, wv


@functools.lru_cache(maxsize=None)
def hall_oracle(variant, cam, bounces=3, width=W, height=H):
    """The oracle's whole frame of a hall: dict(fb, inten, stats, deferred).  Computed once, read-only: shared."""
    _, os_, nodes, wvp, wv = hall(variant, cam)
    orc.set_threads(max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or 0) or (os.cpu_count() or 1))))
    try:   # (the oracle's result does not depend on its threads: tests/test_oracle_threads.py)
        fb, inten, st = orc.trace(os_, nodes, wvp, wv, width, height, bounces, want_intensity=True)
        deferred = expected_deferred(os_, nodes, wvp, wv, width, height, bounces)
    finally:
        orc.set_threads(1)
    for a in (fb, inten):
        a.setflags(write=False)
    return dict(fb=fb, inten=inten, stats=st, deferred=deferred)
