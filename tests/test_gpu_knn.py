"""The k-NN kernels (fr_knn.hip) at every grid tier and on degenerate geometry.

The search is exact, so every comparison is bit for bit: against plain float32 brute force (tests/util.py:knn_brute_force)
where P allows it, and against the CPU oracle, which test_oracle_golden.py pins to that brute force on the same point sets.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from fateavatar_amd import scenes
from tests import util

pytestmark = pytest.mark.gpu

SETS = util.knn_point_sets()


def _both(pts, dev):
    from fateavatar_amd.knn import nearest_dist2
    from simple_knn._C import distCUDA2
    t = torch.from_numpy(pts).to(dev)
    return distCUDA2(t).cpu().numpy(), nearest_dist2(t).cpu().numpy()


@pytest.mark.parametrize("name", sorted(SETS))
def test_knn_equals_brute_force_and_oracle(gpu_device, name):
    """distCUDA2 and nearest_dist2 == float32 brute force == oracle on the small and the degenerate point sets."""
    from oracle import oracle
    pts = SETS[name]
    mean, nearest = _both(pts, gpu_device)
    want_mean, want_nearest = util.knn_brute_force(pts)
    np.testing.assert_array_equal(mean, want_mean)
    np.testing.assert_array_equal(nearest, want_nearest)
    o_mean, o_nearest = oracle.knn_dist2(pts)
    np.testing.assert_array_equal(mean, o_mean)
    np.testing.assert_array_equal(nearest, o_nearest)


def _tier_points(kind, P):
    if kind == "cube":
        return np.random.default_rng(P).uniform(-1, 1, (P, 3)).astype(np.float32)
    verts, faces, _ = scenes.head_geometry()       # a surface: most of the grid stays empty, searches walk several shells
    return scenes.sample_mesh(verts, faces, P, seed=5)


@pytest.mark.parametrize("kind", ["cube", "head_mesh"])
@pytest.mark.parametrize("P,G", [(40_000, 64), (300_000, 128), (2_100_000, 256)])
def test_knn_grid_tiers_equal_the_oracle(gpu_device, P, G, kind):
    """The grid tiers the other tests never reach (G = 8 .. 32 there), in a filled cube and on a surface."""
    from oracle import oracle
    g = 8
    while g < 256 and g ** 3 < P:                  # fr_knn.hip:knn_grid_size, restated
        g *= 2
    assert g == G
    pts = _tier_points(kind, P)
    mean, nearest = _both(pts, gpu_device)
    o_mean, o_nearest = oracle.knn_dist2(pts)
    np.testing.assert_array_equal(mean, o_mean)
    np.testing.assert_array_equal(nearest, o_nearest)
    assert np.all(np.isfinite(mean)) and np.all(nearest <= mean)


@pytest.mark.parametrize("name", ["normal_257", "lattice_18", "two_clusters", "plane_z0"])
def test_knn_does_not_depend_on_the_input_order(gpu_device, name):
    pts = SETS[name]
    perm = np.random.default_rng(3).permutation(len(pts))
    mean, nearest = _both(pts, gpu_device)
    mean_p, nearest_p = _both(np.ascontiguousarray(pts[perm]), gpu_device)
    np.testing.assert_array_equal(mean_p, mean[perm])
    np.testing.assert_array_equal(nearest_p, nearest[perm])
    big = _tier_points("head_mesh", 40_000)
    perm = np.random.default_rng(4).permutation(len(big))
    a, b = _both(big, gpu_device), _both(np.ascontiguousarray(big[perm]), gpu_device)
    np.testing.assert_array_equal(b[0], a[0][perm])
    np.testing.assert_array_equal(b[1], a[1][perm])


@pytest.mark.parametrize("P", [1, 3, 257, 5000, 40_000, 300_000])
@pytest.mark.parametrize("fn", ["fr_knn_mean_dist2", "fr_knn_nearest_dist2"])
def test_knn_stays_inside_the_workspace_it_asks_for(gpu_device, P, fn):
    """fr_knn_workspace_bytes(P) is all the search touches: a patterned guard region behind a workspace of exactly that
    size (and in front of it) is intact afterwards, the result is the oracle's, and one byte less is refused."""
    from fateavatar_amd import _lib
    from oracle import oracle
    L = _lib.lib()
    need = int(L.fr_knn_workspace_bytes(P))
    assert need % 256 == 0
    guard = 1 << 16
    pts = np.random.default_rng(P).normal(size=(P, 3)).astype(np.float32)
    t = torch.from_numpy(pts).to(gpu_device)
    buf = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device=gpu_device)
    assert buf.data_ptr() % 256 == 0
    out = torch.full((P + 64,), -7.0, device=gpu_device)
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    rc = getattr(L, fn)(P, t.data_ptr(), out.data_ptr(), buf.data_ptr() + guard, need, stream)
    assert rc == _lib.FR_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need:] == 0xA5).all())
    assert bool((out[P:] == -7.0).all())
    mean, nearest = oracle.knn_dist2(pts)
    np.testing.assert_array_equal(out[:P].cpu().numpy(), mean if fn == "fr_knn_mean_dist2" else nearest)
    assert getattr(L, fn)(P, t.data_ptr(), out.data_ptr(), buf.data_ptr() + guard, need - 1, stream) != _lib.FR_OK
