"""The halls of mirrors (tests/cert_scenes.py) do what the GPU tests need of them, by the CPU oracle alone:
every one of the first three bounce passes has deferred rays AND rays the certified walk takes, no ray sits
near the walk's thresholds, and the two cameras defer different pixels.  Without this the GPU tests
(tests/test_certified_bounces_gpu.py) could pass with nothing deferred."""
import functools

import numpy as np
import pytest

from tests import cert_scenes as cs

CASES = [(v, c) for v in cs.VARIANTS for c in ("A", "B")]


@functools.lru_cache(maxsize=None)
def _passes(variant, cam):
    """Per pass 1..3: (live mask, origins, directions, deferred mask over the live rays)."""
    _, os_, nodes, wvp, wv = cs.hall(variant, cam)
    out = []
    for b in range(3):
        live, o, d = cs.entering_rays(os_, nodes, wvp, wv, cs.W, cs.H, b)
        out.append((live, o, d, cs.deferred_mask(o, d)))
    return out


@pytest.mark.parametrize("variant,cam", CASES)
def test_every_pass_has_deferred_rays_and_walked_rays(variant, cam):
    every = cs.VARIANTS[variant][2]
    for p, (live, o, d, deferred) in enumerate(_passes(variant, cam), start=1):
        n, nd = int(live.sum()), int(deferred.sum())
        print(f"{variant} {cam} pass {p}: live {n}, deferred {nd}")
        assert n > 0.8 * cs.W * cs.H, p
        if every == (3, 6):
            assert nd >= 0.05 * n and n - nd >= 0.5 * n, (p, n, nd)
        else:
            assert 0.001 * n <= nd <= 0.02 * n, (p, n, nd)


@pytest.mark.parametrize("variant,cam", CASES)
def test_no_ray_near_the_walks_thresholds(variant, cam):
    """|1/d_k| > 2^20 decides deferral: no non-zero component within a relative 2^-18 of 2^-20 (a last-bit
    difference in the division could not change the count); and the other parts of the walk's test -- d.d <=
    1 + 2^-18 (margin.h MT_DD), |o| <= 2^90 -- hold with room, in float64."""
    for p, (live, o, d, _) in enumerate(_passes(variant, cam), start=1):
        a = np.abs(d.astype(np.float64))
        near = (a != 0) & (np.abs(a - 2.0 ** -20) <= 2.0 ** -18 * 2.0 ** -20)
        assert not near.any(), p
        assert ((d.astype(np.float64) ** 2).sum(1) < 1 + 2.0 ** -19).all(), p
        assert (np.abs(o.astype(np.float64)) < 2.0 ** 20).all(), p
        assert np.isfinite(o).all() and np.isfinite(d).all(), p


@pytest.mark.parametrize("variant", list(cs.VARIANTS))
def test_camera_b_defers_fewer_rays_at_other_pixels(variant):
    def first_pass(cam):
        live, _, _, deferred = _passes(variant, cam)[0]
        m = np.zeros(live.shape, bool)
        m[live] = deferred
        return m
    a, b = first_pass("A"), first_pass("B")
    assert 0 < b.sum() < a.sum()
    assert not np.array_equal(a, b)
    assert (a != b).sum() > 0.1 * a.sum()


def test_expected_deferred_sums_the_passes():
    _, os_, nodes, wvp, wv = cs.hall("small", "A")
    per_pass = [int(p[3].sum()) for p in _passes("small", "A")]
    assert cs.expected_deferred(os_, nodes, wvp, wv, cs.W, cs.H, 3) == sum(per_pass)
    assert cs.expected_deferred(os_, nodes, wvp, wv, cs.W, cs.H, 1) == per_pass[0]
    assert cs.expected_deferred(os_, nodes, wvp, wv, cs.W, cs.H, 0) == 0


@pytest.mark.parametrize("tall", [False, True])
def test_strip_scene_spans_the_largest_frame(tall):
    """tests/test_certified_bounces_gpu.py test_frames_past_the_binned_pass_size: about 20,000 triangles under
    every column (row) of a 32,776-pixel side, a third of them with flat normals."""
    s = cs.strip_scene(tall)
    assert 15_000 <= s.num_tris <= 25_000
    p = s.vertices[:, :3]
    along, across = (p[:, 1], p[:, 0]) if tall else (p[:, 0], p[:, 1])
    assert along.min() < -32776 / 8 and along.max() > 32776 / 8 - 0.25
    assert across.min() < -2 and across.max() > 1.75
    flat = (s.vertices[::3, 3:5] == 0).all(1)
    assert abs(flat.mean() - 1 / 3) < 0.01
