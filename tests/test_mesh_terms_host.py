"""CPU: the uniform Laplacian of a mesh as `binding.mesh_laplacian` builds it against the dense restatement
(tests/mesh_terms_ref.py) and against matrices written out by hand, the restated loss against a value computed by hand, and
the C ABI of the mesh-terms launch (`fr_mesh_terms`, include/fr_rasterizer.h)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.mesh_terms_ref import (displaced, flame_distance, float64_terms, float64_terms_sparse, laplacian_dense, laplacian_smoothing,
                                  random_mesh, random_mesh_drawn_at_once)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fr_rasterizer.h")

T = 1.0 / 3.0
CASES = {
    # one triangle: every off-diagonal 1/2
    "triangle": (3, [[0, 1, 2]], [[-1, .5, .5], [.5, -1, .5], [.5, .5, -1]]),
    # a tetrahedron: 1/3
    "tetrahedron": (4, [[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], [[-1, T, T, T], [T, -1, T, T], [T, T, -1, T], [T, T, T, -1]]),
    # two triangles on the shared edge 1-2: degrees 2, 3, 3, 2
    "two_triangles": (4, [[0, 1, 2], [2, 1, 3]], [[-1, .5, .5, 0], [T, -1, T, T], [T, T, -1, T], [0, .5, .5, -1]]),
    # vertex 4 unused, face (0,1,2) listed twice, face (2,1,3) in both windings: the matrix of the two triangles, and an
    # empty row with its -1
    "unused_repeated_both_windings": (5, [[0, 1, 2], [0, 1, 2], [2, 1, 3], [3, 1, 2]],
                                      [[-1, .5, .5, 0, 0], [T, -1, T, T, 0], [T, T, -1, T, 0], [0, .5, .5, -1, 0], [0, 0, 0, 0, -1]]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_laplacian_of_small_meshes_equals_the_hand_written_matrix(name):
    from fateavatar_amd.binding import mesh_laplacian
    V, faces, want = CASES[name]
    want = torch.tensor(want, dtype=torch.float64)
    lap = mesh_laplacian(torch.tensor(faces), V)
    assert lap.V == V and lap.row_ptr.dtype == torch.int32 and lap.col.dtype == torch.int32 and lap.row_ptr.numel() == V + 1
    assert int(lap.row_ptr[-1]) == lap.col.numel() == int((want > 0).sum())
    assert torch.equal(lap.to_dense(torch.float64), want)            # (1/2 and the rounded 1/3 of the literal: the same doubles)
    assert torch.equal(laplacian_dense(faces, V, torch.float64), want)
    assert torch.equal(lap.to_dense(torch.float32), laplacian_dense(faces, V, torch.float32))
    for i in range(V):                                               # rows ascending and duplicate-free
        row = lap.col[int(lap.row_ptr[i]):int(lap.row_ptr[i + 1])].tolist()
        assert row == sorted(set(row)) and i not in row


def test_laplacian_of_the_head_template():
    """15 024 unique edges, nnz 30 048, degrees 3 .. 32 (six vertices of degree >= 30: the eyeball poles), no isolated
    vertex, no self-edge; symmetric; equal to the dense restatement."""
    from fateavatar_amd import scenes
    from fateavatar_amd.binding import mesh_laplacian
    verts, faces, _ = scenes.head_geometry()
    V = int(verts.shape[0])
    lap = mesh_laplacian(torch.from_numpy(np.asarray(faces)), V)
    rp, col = lap.row_ptr.long(), lap.col.long()
    deg = rp[1:] - rp[:-1]
    assert V == 5023 and col.numel() == 30048 and int(rp[-1]) == 30048 and int(rp[0]) == 0
    assert int(deg.min()) == 3 and int(deg.max()) == 32 and int((deg >= 30).sum()) == 6
    row = torch.repeat_interleave(torch.arange(V), deg)
    assert not bool((row == col).any()) and int(col.min()) >= 0 and int(col.max()) < V
    key = row * V + col
    assert bool((key[1:] > key[:-1]).all())                          # rows ascending, duplicate-free
    assert torch.equal(torch.sort(col * V + row).values, key)        # symmetric
    assert int((row < col).sum()) == 15024
    assert torch.equal(lap.to_dense(torch.float32), laplacian_dense(faces, V, torch.float32))


def test_laplacian_refuses_faces_outside_the_mesh():
    from fateavatar_amd.binding import mesh_laplacian
    with pytest.raises(ValueError):
        mesh_laplacian(torch.tensor([[0, 1, 3]]), 3)
    with pytest.raises(ValueError):
        mesh_laplacian(torch.tensor([[0, -1, 2]]), 3)
    lap = mesh_laplacian(torch.zeros((0, 3), dtype=torch.int64), 2)   # no faces: two empty rows
    assert lap.row_ptr.tolist() == [0, 0, 0] and lap.col.numel() == 0
    assert torch.equal(lap.to_dense(), -torch.eye(2))


def test_restated_losses_on_the_tetrahedron_by_hand():
    """verts_orig = 0, verts = d with d_0 = (3,0,0), d_1 = (0,3,0), d_2 = (0,0,3), d_3 = 0.  Every vertex has the other three
    as neighbours: r_i = -d_i + (S - d_i) / 3 = S / 3 - (4/3) d_i with S = (3,3,3), so r_0 = (-3,1,1), r_1 = (1,-3,1),
    r_2 = (1,1,-3), r_3 = (1,1,1): |r|^2 = 11, 11, 11, 3, their mean 36 / 4 = 9.  flame: 27 / 12 = 2.25.  The gradient of the
    Laplacian term is (2/V) L^T r: row 0 = 0.5 * (-r_0 + (r_1 + r_2 + r_3) / 3) = 0.5 * ((3,-1,-1) + (1,-1/3,-1/3)) = (2,-2/3,-2/3)."""
    V, faces, _ = CASES["tetrahedron"]
    L = laplacian_dense(faces, V, torch.float64)
    vo = torch.zeros(V, 3, dtype=torch.float64)
    v = torch.tensor([[3., 0, 0], [0, 3, 0], [0, 0, 3], [0, 0, 0]], dtype=torch.float64, requires_grad=True)
    lap = laplacian_smoothing(L, vo, v)
    assert abs(lap.item() - 9.0) < 1e-12 and abs(flame_distance(vo, v).item() - 2.25) < 1e-12
    assert abs(laplacian_smoothing(L, vo[None], v[None]).item() - 9.0) < 1e-12          # [1,V,3]
    lap.backward()
    assert torch.allclose(v.grad[0], torch.tensor([2.0, -2.0 / 3.0, -2.0 / 3.0], dtype=torch.float64), atol=1e-12)
    # a constant shift of the whole mesh is in the Laplacian's null space
    assert abs(float(laplacian_smoothing(L, vo, vo + 0.25))) < 1e-24


@pytest.mark.parametrize("weights", [(1e5, 0.0), (1e5, 0.3)])
def test_sparse_restatement_is_the_dense_one(weights):
    """`float64_terms_sparse` (what the GPU test is held to where V x V does not fit) against `float64_terms` on the drawn meshes
    of tests/test_gpu_mesh_terms.py, a mesh drawn at once and the hand-written cases: `grad`, `lap`, `flame` (and the
    magnitudes the bounds are written in) to 1e-12 relative, `deg` exactly."""
    from tests.test_gpu_mesh_terms import SEED, SIZES
    meshes = [random_mesh(V, SEED[V]) + (SEED[V],) for V in SIZES] + [random_mesh_drawn_at_once(300, 5) + (5,)]
    meshes += [(0.1 * np.random.default_rng(3).standard_normal((V, 3)).astype(np.float32), np.asarray(faces, np.int64), 9)
               for V, faces, _ in CASES.values()]
    empty = 0
    for vo, faces, seed in meshes:
        V = vo.shape[0]
        vo_t, v_t = torch.from_numpy(vo), torch.from_numpy(displaced(vo, seed))
        dense, sparse = float64_terms(faces, V, vo_t, v_t, *weights), float64_terms_sparse(faces, V, vo_t, v_t, *weights)
        assert sorted(dense) == sorted(sparse)
        assert sparse["deg"].dtype == dense["deg"].dtype and torch.equal(sparse["deg"], dense["deg"])
        empty += int((sparse["deg"] == 0).sum())
        for k in ("lap", "flame"):
            assert dense[k] > 0 and abs(sparse[k] - dense[k]) <= 1e-12 * dense[k], (V, k)
        for k in ("grad", "r", "d", "Mr", "Mg"):
            assert sparse[k].shape == dense[k].shape and sparse[k].dtype == torch.float64
            assert float((sparse[k] - dense[k]).norm()) <= 1e-12 * float(dense[k].norm()), (V, k)
            assert float((sparse[k] - dense[k]).abs().max()) <= 1e-12 * float(dense[k].abs().max()), (V, k)
    assert empty >= 5                                # rows without a neighbour were among them


def test_new_entries_are_declared_exported_and_listed():
    from fateavatar_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in ("fr_mesh_terms", "fr_mesh_terms_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    # 17 x 128 bytes of done-counters + two rows of per-workgroup partials
    assert _lib.lib().fr_mesh_terms_workspace_bytes() >= 17 * 128 + 2 * 4


def test_config_struct_has_the_c_compilers_layout(tmp_path):
    from fateavatar_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu\n", sizeof(fr_mesh_terms_config), offsetof(fr_mesh_terms_config, laplacian_weight),
        offsetof(fr_mesh_terms_config, flame_weight));
 return 0; }'''
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = _lib.fr_mesh_terms_config
    assert got == [C.sizeof(S), S.laplacian_weight.offset, S.flame_weight.offset]
    assert [n for n, _ in S._fields_] == ["laplacian_weight", "flame_weight"]


def test_validation_refuses_bad_arguments_before_anything_is_enqueued():
    """No GPU: every call below fails its argument check, which runs in front of the first HIP call.  (The non-null
    pointers are never dereferenced.)  Arguments: cfg, V, verts, verts_orig, row_ptr, col, d_verts, loss, workspace, stream."""
    from fateavatar_amd import _lib
    L = _lib.lib()
    cfg = _lib.fr_mesh_terms_config(1e5, 0.0)
    p = 0x1000      # stands for "a non-null device pointer"
    bad = dict(null_config=(None, 8, p, p, p, p, p, p, p, None),
               negative_V=(C.byref(cfg), -1, p, p, p, p, p, p, p, None),
               null_verts=(C.byref(cfg), 8, None, p, p, p, p, p, p, None),
               null_verts_orig=(C.byref(cfg), 8, p, None, p, p, p, p, p, None),
               null_row_ptr=(C.byref(cfg), 8, p, p, None, p, p, p, p, None),
               null_row_ptr_V0=(C.byref(cfg), 0, p, p, None, None, None, p, p, None),
               null_col=(C.byref(cfg), 8, p, p, p, None, p, p, p, None),
               null_loss=(C.byref(cfg), 8, p, p, p, p, p, None, p, None),
               null_loss_V0=(C.byref(cfg), 0, p, p, p, None, None, None, p, None),
               null_workspace=(C.byref(cfg), 8, p, p, p, p, None, p, None, None),
               null_workspace_V0=(C.byref(cfg), 0, p, p, p, None, None, p, None, None))
    for what, args in bad.items():
        assert L.fr_mesh_terms(*args) == _lib.FR_ERR_INVALID_ARGUMENT, what
        assert b"fr_mesh_terms" in L.fr_last_error(), what
    # V == 0 with a null `col` and a null `d_verts` is a valid call that launches nothing
    assert L.fr_mesh_terms(C.byref(cfg), 0, p, p, p, None, None, p, p, None) == _lib.FR_OK
