"""CPU: the C ABI of GaussianAvatars' regulariser launch (`fr_gaussian_regularise`, include/fr_rasterizer.h) and the torch
restatement the GPU tests of the rigged set's regularisers and density control are held to (tests/rigged_density_ref.py):
its regulariser gradient against finite differences, its maintenance against the `binding_counter` invariants."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import torch

from tests.rigged_density_ref import NAMES, RiggedRef, draw_gate_inputs, regulariser_grads, regularisers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fr_rasterizer.h")
G = np.load(os.path.join(ROOT, "tests", "golden", "golden_binding.npz"))


def test_new_entries_are_declared_exported_and_listed():
    from fateavatar_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in ("fr_gaussian_regularise", "fr_regularise_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    # 17 x 128 bytes of done-counters + two rows of per-workgroup partials
    assert _lib.lib().fr_regularise_workspace_bytes() >= 17 * 128 + 2 * 4


def test_config_struct_has_the_c_compilers_layout(tmp_path):
    from fateavatar_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu %zu %zu\n", sizeof(fr_regularise_config), offsetof(fr_regularise_config, scale_weight),
        offsetof(fr_regularise_config, xyz_weight), offsetof(fr_regularise_config, threshold_scale),
        offsetof(fr_regularise_config, threshold_xyz));
 return 0; }'''
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = _lib.fr_regularise_config
    assert got == [C.sizeof(S), S.scale_weight.offset, S.xyz_weight.offset, S.threshold_scale.offset, S.threshold_xyz.offset]
    assert [n for n, _ in S._fields_] == ["scale_weight", "xyz_weight", "threshold_scale", "threshold_xyz"]


def test_validation_refuses_bad_arguments_before_anything_is_enqueued():
    """No GPU: every call below fails its argument check, which runs in front of the first HIP call.  (The non-null
    pointers are never dereferenced.)"""
    from fateavatar_amd import _lib
    L = _lib.lib()
    cfg = _lib.fr_regularise_config(1.0, 0.01, 0.6, 1.0)
    p = 0x1000      # stands for "a non-null device pointer"
    bad = dict(negative_P=(C.byref(cfg), -1, p, p, p, p, p, p, None),
               null_scaling=(C.byref(cfg), 8, None, p, p, p, p, p, None),
               null_xyz=(C.byref(cfg), 8, p, None, p, p, p, p, None),
               null_workspace=(C.byref(cfg), 8, p, p, p, p, p, None, None),
               null_workspace_P0=(C.byref(cfg), 0, None, None, None, None, p, None, None),
               null_loss=(C.byref(cfg), 8, p, p, p, p, None, p, None),
               null_loss_P0=(C.byref(cfg), 0, None, None, None, None, None, p, None),
               null_config=(None, 8, p, p, p, p, p, p, None))
    for what, args in bad.items():
        assert L.fr_gaussian_regularise(*args) == _lib.FR_ERR_INVALID_ARGUMENT, what
        assert b"fr_gaussian_regularise" in L.fr_last_error(), what


def test_restatement_regulariser_gradient_agrees_with_central_finite_differences():
    """float64 autograd of weight_s * scale_loss + weight_x * xyz_loss against central differences (h = 1e-6: truncation ~h^2,
    rounding ~1e-16 / h) to 1e-6 relative to the largest entry — on rows whose gates are at least 1e-3 from their
    thresholds, so that no difference straddles a kink.  Pins the gate conventions: components with exp(s) <= threshold and
    rows with |xyz| <= threshold have a zero gradient, exactly."""
    P, ws, wx, ts, tx = 64, 1.0, 0.01, 0.6, 1.0
    scaling, xyz = draw_gate_inputs(P, torch.Generator().manual_seed(3), ts, tx, torch.float64)
    e, n = torch.exp(scaling), xyz.norm(dim=1)
    assert float(((e - ts).abs()).min()) > 1e-3 and float((n - tx).abs().min()) > 1e-3
    assert bool((e > ts).any()) and bool((e <= ts).any()) and bool((n > tx).any()) and bool((n <= tx).any())
    assert bool((e <= ts).all(dim=1).any())          # a row clipped to zero entirely
    _, _, gs, gx = regulariser_grads(scaling, xyz, ws, wx, ts, tx)

    def f(s, x):
        a, b = regularisers(s, x, ts, tx)
        return float(ws * a + wx * b)

    h = 1e-6
    for t, g, which in ((scaling, gs, 0), (xyz, gx, 1)):
        fd = torch.zeros_like(t)
        for i in range(P):
            for k in range(3):
                tp, tm = t.clone(), t.clone()
                tp[i, k] += h
                tm[i, k] -= h
                fd[i, k] = ((f(tp, xyz) - f(tm, xyz)) if which == 0 else (f(scaling, tp) - f(scaling, tm))) / (2 * h)
        assert float(g.abs().max()) > 0
        assert float((g - fd).abs().max()) <= 1e-6 * float(g.abs().max()), which
    assert bool((gs[e <= ts] == 0).all()) and bool((gx[n <= tx] == 0).all())
    # the corner cases autograd defines: a component exactly AT the threshold, and xyz = 0
    s0 = torch.log(torch.tensor([[0.6, 0.6, 0.6], [0.6, 2.0, 0.1]], dtype=torch.float64))
    x0 = torch.zeros(2, 3, dtype=torch.float64)
    _, _, g0, gx0 = regulariser_grads(s0, x0, ws, wx, float(torch.exp(s0[0, 0])), tx)
    assert bool((g0[0] == 0).all()) and float(g0[1, 0]) == 0 and float(g0[1, 2]) == 0 and float(g0[1, 1]) > 0
    assert bool((gx0 == 0).all()) and bool(torch.isfinite(gx0).all())


def _random_ref(rng, F, P, gen):
    binding = torch.from_numpy(np.concatenate([np.arange(F), rng.integers(0, F, P - F)]).astype(np.int64))
    params = {"_xyz": torch.randn(P, 3, generator=gen), "_opacity": torch.randn(P, 1, generator=gen) * 3 - 2,
              "_features_dc": torch.rand(P, 1, 3, generator=gen), "_features_rest": torch.randn(P, 15, 3, generator=gen),
              "_rotation": torch.randn(P, 4, generator=gen), "_scaling": torch.randn(P, 3, generator=gen) - 4.0}
    ref = RiggedRef(params, binding, F)
    ref.step({n: torch.randn(ref.p[n].shape, generator=gen) for n in NAMES})      # (creates the Adam state)
    return ref


def test_restatement_maintenance_keeps_binding_counter_and_every_face_populated():
    """300 random operations (guarded prune with a random mask of random density — up to everything —, densify_and_prune on
    random statistics, reset_opacity) on the golden mesh's 90 faces: after each one `binding_counter == bincount(binding)`,
    `binding_counter.min() >= 1`, every parameter, both Adam moments and the statistics have one row per Gaussian."""
    F = int(G["faces"].shape[0])
    rng = np.random.default_rng(5)
    gen = torch.Generator().manual_seed(5)
    ref = _random_ref(rng, F, 4 * F, gen)
    did = {"prune": 0, "densify": 0, "reset": 0, "guard": 0}
    for it in range(300):
        op = rng.integers(0, 10)
        if op < 6 or ref.P > 3000:
            mask = torch.from_numpy(rng.random(ref.P) < rng.choice([0.05, 0.5, 0.95, 1.0]))
            marked = int(mask.sum())
            did["guard"] += int(ref.prune(mask) < marked)
            did["prune"] += 1
        elif op < 9:
            ref.xyz_gradient_accum = torch.from_numpy(rng.random((ref.P, 1)).astype(np.float32) * 3e-4)
            ref.denom = torch.from_numpy(rng.integers(0, 3, (ref.P, 1)).astype(np.float32))
            with torch.no_grad():       # scales on both sides of percent_dense * extent = 0.02
                ref.p["_scaling"].copy_(torch.from_numpy(rng.normal(-4.0, 1.0, (ref.P, 3)).astype(np.float32)))
            n_clone, n_split, _ = ref.densify_and_prune(1e-4, 0.005, 2.0, 20 if it % 2 else None, gen)
            did["densify"] += int(n_clone > 0 and n_split > 0)
            assert float(ref.xyz_gradient_accum.abs().max()) == 0 and float(ref.denom.abs().max()) == 0
        else:
            ref.reset_opacity()
            did["reset"] += 1
            assert float(torch.sigmoid(ref.p["_opacity"].detach()).max()) <= 0.01 * (1 + 1e-6)
            assert float(ref.moments("_opacity")[0].abs().max()) == 0
        assert torch.equal(ref.binding_counter.long(), torch.bincount(ref.binding, minlength=F)), it
        assert int(ref.binding_counter.min()) >= 1, it
        for n in NAMES:
            m, v, _ = ref.moments(n)
            assert ref.p[n].shape[0] == ref.P == m.shape[0] == v.shape[0], (it, n)
        assert ref.xyz_gradient_accum.shape == (ref.P, 1) == ref.denom.shape
    assert min(did.values()) > 0, did


def test_rigged_gaussians_resize_carries_the_binding_and_returns_the_row_map():
    """RiggedGaussians.resize: FlatGaussians.resize's contract (old_index, -1 for appended rows) with `binding` carried."""
    from fateavatar_amd.rigged import REFERENCE_REGULARISERS, RiggedGaussians
    assert tuple(REFERENCE_REGULARISERS) == (1.0, 0.01, 0.6, 1.0)
    pc = RiggedGaussians(np.array([0, 1, 2, 2, 1], np.int32), "cpu")
    with torch.no_grad():
        pc._xyz.copy_(torch.arange(15.0).reshape(5, 3))
    keep = torch.tensor([True, False, True, True, False])
    rows = [torch.full((2,) + pc.SHAPES[n], 7.0) for n, _ in pc.FIELDS]
    old_index = pc.resize(keep_mask=keep, new_rows=rows, new_binding=torch.tensor([2, 0]))
    assert old_index.tolist() == [0, 2, 3, -1, -1] and pc.P == 5
    assert pc.binding.tolist() == [0, 2, 2, 2, 0] and pc.binding.dtype == torch.int32
    assert pc._xyz[:3].tolist() == [[0, 1, 2], [6, 7, 8], [9, 10, 11]] and bool((pc._xyz[3:] == 7).all())
    assert pc.flat.numel() == 5 * sum(pc.widths()) == pc.flat_grad.numel()
    assert pc.grad_view("_scaling").data_ptr() == pc.flat_grad[5 * 56:].data_ptr() and pc.grad_view("_xyz").shape == (5, 3)


def test_build_rotation_is_the_restatements_matrix_and_a_rotation():
    """`gs_utils.build_rotation` against tests/rigged_density_ref.build_rotation (general_utils.py:78-99 restated entry by entry) on
    257 raw, unnormalised float64 quaternions.  The two differ only in how the norm's four squares are summed and in the order of
    the products: every entry is <= 1 in magnitude and is reached in fewer than 16 roundings, so |got - want| <= 16 x 2^-52;
    R R^T = I and det R = 1 to the same count times the three terms of a row product."""
    from fateavatar_amd.gs_utils import build_rotation
    from tests.rigged_density_ref import build_rotation as want_rotation
    q = torch.randn(257, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(12)) * 3.0
    got, want = build_rotation(q), want_rotation(q)
    eps = 2.0 ** -52
    assert got.shape == (257, 3, 3) and got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 16 * eps
    assert float((got @ got.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 48 * eps
    assert float((torch.linalg.det(got) - 1).abs().max()) <= 48 * eps
    assert torch.equal(build_rotation(torch.tensor([[2.0, 0.0, 0.0, 0.0]])), torch.eye(3).unsqueeze(0))
