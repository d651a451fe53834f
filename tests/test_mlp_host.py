"""CPU: the host side of the fused deformation MLP (fateavatar_amd/mlp.py, FlashStep(deformer=...)) — the embedding's column
order, the flat nn.Linear layout and its state_dict, the C ABI's struct and size formula, and every refusal that is decided
before the device is touched.  The kernels themselves: tests/test_gpu_mlp.py."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest
import torch

from tests import mlp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_embedding_column_order_on_two_hand_computed_points():
    from fateavatar_amd.mlp import embed_points
    pts = torch.tensor([[0.5, -0.25, 1.0], [0.0, 2.0, -1.5]])
    e = embed_points(pts, n_freqs=2)
    assert tuple(e.shape) == (2, 3 * (1 + 2 * 2))
    s, c = math.sin, math.cos
    want = [[0.5, -0.25, 1.0, s(0.5), s(-0.25), s(1.0), c(0.5), c(-0.25), c(1.0), s(1.0), s(-0.5), s(2.0), c(1.0), c(-0.5), c(2.0)],
            [0.0, 2.0, -1.5, s(0.0), s(2.0), s(-1.5), c(0.0), c(2.0), c(-1.5), s(0.0), s(4.0), s(-3.0), c(0.0), c(4.0), c(-3.0)]]
    assert torch.allclose(e.double(), torch.tensor(want, dtype=torch.float64), atol=1e-7, rtol=0)
    # the reference's default: 8 frequencies -> 51 columns, the same as the restatement's, bit for bit
    big = torch.randn(7, 3, generator=torch.Generator().manual_seed(0))
    assert tuple(embed_points(big).shape) == (7, 51) and torch.equal(embed_points(big), mlp_ref.embed(big))
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        embed_points(torch.zeros(4, 2))


def test_flat_layout_and_state_dict_round_trip_with_the_references_keys():
    from fateavatar_amd.mlp import DeformMLP
    torch.manual_seed(3)
    ref = mlp_ref.RefMLP(51 + 59, 10, hidden_layers=6)
    E = torch.randn(5, 51)
    mlp = DeformMLP.from_torch(ref, E, 59)
    assert (mlp.N, mlp.point_dim, mlp.cond_dim, mlp.layers, mlp.out_dim) == (5, 51, 59, 6, 10)
    sd = ref.state_dict()
    assert list(mlp.state_dict()) == list(sd)                      # fcs.0.weight, fcs.0.bias, ..., output_linear.bias
    # the flat buffer is the state_dict's tensors one after the other: no transpose, no padding
    assert torch.equal(mlp.flat.detach(), torch.cat([t.reshape(-1) for t in sd.values()]))
    assert mlp.flat.numel() == 256 * 110 + 256 + 5 * (256 * 256 + 256) + 10 * 256 + 10 == mlp.flat_grad.numel()
    assert mlp.flat.requires_grad and not mlp.flat_grad.requires_grad
    for i in range(6):
        assert torch.equal(mlp.weight(i), ref.fcs[i].weight) and torch.equal(mlp.bias(i), ref.fcs[i].bias)
    assert torch.equal(mlp.weight(6), ref.output_linear.weight) and tuple(mlp.grad_weight(0).shape) == (256, 110)
    assert mlp.weight(2).data_ptr() == mlp.flat.data_ptr() + 4 * (256 * 111 + 257 * 256)     # views, not copies
    # out through the model's names, back into a fresh network and into a fresh reference module
    other = DeformMLP(E, 59, layers=6, out_dim=10)
    assert not torch.equal(other.flat, mlp.flat)
    ptr = other.flat.data_ptr()
    other.load_state_dict(mlp.state_dict("deformNet."))            # (the prefix is recognised)
    assert torch.equal(other.flat, mlp.flat) and other.flat.data_ptr() == ptr
    fresh = mlp_ref.RefMLP(110, 10, hidden_layers=6)
    fresh.load_state_dict(other.state_dict())
    x = torch.randn(3, 110)
    assert torch.equal(fresh(x), ref(x))
    with pytest.raises(KeyError, match="fcs.5.bias"):
        other.load_state_dict({k: v for k, v in sd.items() if k != "fcs.5.bias"})
    with pytest.raises(ValueError, match="fcs.0.weight"):
        other.load_state_dict({**sd, "fcs.0.weight": torch.zeros(256, 111)})


def test_default_initialisation_is_nn_linears_in_the_references_order():
    from fateavatar_amd.mlp import DeformMLP
    torch.manual_seed(11)
    ref = mlp_ref.RefMLP(3 + 4, 10, hidden_layers=2)
    torch.manual_seed(11)
    mlp = DeformMLP(torch.zeros(9, 3), 4, layers=2)
    assert torch.equal(mlp.flat.detach(), torch.cat([t.reshape(-1) for t in ref.state_dict().values()]))


def test_refusals_come_before_the_device():
    from fateavatar_amd.mlp import DeformMLP
    E = torch.zeros(4, 51)
    with pytest.raises(ValueError, match="width"):
        DeformMLP.from_torch(mlp_ref.RefMLP(110, 10, hidden_dim=128, hidden_layers=2), E, 59)
    with pytest.raises(ValueError, match="width"):
        DeformMLP(E, 59, width=128)
    for layers in (0, 9):
        with pytest.raises(ValueError, match="hidden layers"):
            DeformMLP(E, 59, layers=layers)
    with pytest.raises(ValueError, match="<= 256"):
        DeformMLP(E, 206)
    DeformMLP(E, 205, layers=1)                                     # 51 + 205 = 256 is allowed
    with pytest.raises(ValueError, match="output columns"):
        DeformMLP(E, 59, out_dim=17)
    with pytest.raises(TypeError, match="float32"):
        DeformMLP(E.double(), 59)
    with pytest.raises(ValueError, match="requires grad"):
        DeformMLP(E.clone().requires_grad_(True), 59)
    with pytest.raises(ValueError, match="input is 110 wide"):
        DeformMLP.from_torch(mlp_ref.RefMLP(110, 10, hidden_layers=2), E, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeformMLP(E, 59, layers=1)(torch.zeros(59))


def test_abi_struct_limits_and_workspace_formula():
    from fateavatar_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu %zu\n", sizeof(fr_mlp), offsetof(fr_mlp, D_out), offsetof(fr_mlp, E), offsetof(fr_mlp, weights));
 printf("%d %d %d %d %d\n", FR_MLP_WIDTH, FR_MLP_MAX_LAYERS, FR_MLP_MAX_OUT, FR_MLP_POINT_TILE, FR_MLP_CHUNK);
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out[:4] == [C.sizeof(_lib.fr_mlp), _lib.fr_mlp.D_out.offset, _lib.fr_mlp.E.offset, _lib.fr_mlp.weights.offset]
    assert out[4:] == [_lib.FR_MLP_WIDTH, _lib.FR_MLP_MAX_LAYERS, _lib.FR_MLP_MAX_OUT, _lib.FR_MLP_POINT_TILE, _lib.FR_MLP_CHUNK]
    L = _lib.lib()
    r256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for N, layers in ((16384, 6), (1, 1), (1541, 8), (100000, 6)):
        want = (layers + 2) * r256(N * 1024) + r256(-(-N // _lib.FR_MLP_CHUNK) * 257 * 256 * 4) + 1024
        assert L.fr_mlp_workspace_bytes(N, layers) == want
    assert L.fr_mlp_workspace_bytes(16384, 6) >= 16384 * 256 * 4 * 6       # the saved activations the issue counts
    assert L.fr_mlp_workspace_bytes(10, 0) == 0 and L.fr_mlp_workspace_bytes(10, 9) == 0


def test_entry_points_refuse_shapes_outside_the_limits_before_anything_is_enqueued():
    from fateavatar_amd import _lib
    L = _lib.lib()
    ws = (C.c_char * 1024)()
    addr = (C.addressof(ws) + 255) // 256 * 256
    good = dict(N=0, L=6, De=51, Dc=59, D_out=10)
    for bad in (dict(L=0), dict(L=9), dict(De=0), dict(Dc=-1), dict(De=200, Dc=57), dict(D_out=0), dict(D_out=17), dict(N=-1)):
        d = _lib.fr_mlp(**{**good, **bad})
        assert L.fr_mlp_forward(C.byref(d), None, addr, None) == _lib.FR_ERR_INVALID_ARGUMENT, bad
        assert "fr_mlp_forward" in _lib.last_error()
        assert L.fr_mlp_backward(C.byref(d), None, addr, None, addr, None) == _lib.FR_ERR_INVALID_ARGUMENT, bad
    d = _lib.fr_mlp(**good)
    assert L.fr_mlp_forward(C.byref(d), None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT            # no workspace
    assert L.fr_mlp_forward(C.byref(d), None, addr + 4, None) == _lib.FR_ERR_INVALID_ARGUMENT        # misaligned
    assert L.fr_mlp_backward(C.byref(d), None, None, None, addr, None) == _lib.FR_ERR_INVALID_ARGUMENT  # no d_weights
    d = _lib.fr_mlp(**{**good, "N": 4})
    assert L.fr_mlp_forward(C.byref(d), addr, addr, None) == _lib.FR_ERR_INVALID_ARGUMENT            # N > 0 and null arrays
    assert L.fr_mlp_forward(None, None, addr, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert L.fr_mlp_forward(C.byref(_lib.fr_mlp(**good)), None, addr, None) == _lib.FR_OK             # N == 0: nothing to launch


def test_flash_step_checks_its_deformer_before_the_device():
    from fateavatar_amd.flash import FlashGaussians, FlashStep
    from fateavatar_amd.mlp import DeformMLP
    N = 6
    pc = FlashGaussians(torch.zeros(N, dtype=torch.int64), torch.full((N, 3), 1 / 3), -4.0, "cpu")
    faces = torch.zeros((1, 3), dtype=torch.int32)
    E = torch.zeros(N, 51)
    with pytest.raises(TypeError, match="DeformMLP"):
        FlashStep(pc, faces, None, None, torch.zeros(3, 3), deformer=torch.nn.Linear(3, 10))
    with pytest.raises(ValueError, match=r"\[6,10\]"):
        FlashStep(pc, faces, None, None, torch.zeros(3, 3), deformer=DeformMLP(torch.zeros(N + 1, 51), 59, layers=1))
    with pytest.raises(ValueError, match=r"\[6,10\]"):
        FlashStep(pc, faces, None, None, torch.zeros(3, 3), deformer=DeformMLP(E, 59, layers=1, out_dim=9))
    with pytest.raises(ValueError, match="deformer_lr"):
        FlashStep(pc, faces, None, None, torch.zeros(3, 3), deformer=DeformMLP(E, 59, layers=1), deformer_lr=0.0)
