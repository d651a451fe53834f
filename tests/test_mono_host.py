"""CPU: the restatement of MonoGaussianAvatar's per-point arithmetic (tests/mono_ref.py) pinned by hand cases, gradcheck, the
written backward and the kernels' closed forms; the host logic of fateavatar_amd/mono.py; the new ABI structs' layout."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest
import torch

from fateavatar_amd import _lib, mono
from tests import mono_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _identity_bones(J):
    return torch.eye(4, dtype=torch.float64).repeat(J, 1, 1)


def test_identity_bones_give_the_point_plus_the_blendshape_differences():
    p, S, P, w, c, f, _ = R.recipe(33, 50, 6)
    I = _identity_bones(6)
    xyz = R.deform_points(p, S, P, w / w.sum(1, keepdim=True), (c[0], c[1], I), (f[0], f[1], I))
    want = p + torch.einsum("nkl,l->nk", S, f[0] - c[0]) + torch.einsum("nik,i->nk", P, f[1] - c[1])
    assert float((xyz - want).abs().max()) < 1e-14


def test_one_hot_weights_give_a_rigid_transform():
    p, S, P, w, c, f, _ = R.recipe(33, 7, 5)
    assert bool((w[:5] == torch.eye(5, dtype=torch.float64)).all())           # the recipe's first rows are one-hot, one per bone
    zero = torch.zeros_like
    xyz = R.deform_points(p[:5], zero(S[:5]), zero(P[:5]), w[:5], c, f)
    for j in range(5):
        h = torch.cat([p[j], torch.ones(1, dtype=torch.float64)])
        want = (f[2][j] @ torch.inverse(c[2][j]) @ h)[:3]
        assert float((xyz[j] - want).abs().max()) < 1e-14
    assert float((xyz[0] - p[0]).abs().max()) < 1e-15                           # bone 0 is the identity in both poses


def test_frame_equal_to_canonical_gives_the_point_back():
    p, S, P, w, c, _, _ = R.recipe(65, 50, 6)
    xyz = R.deform_points(p, S, P, w, c, c)
    # (rows whose weights do not sum to 1 come back as T3 (z3, 1) with z4 = 1 / s, not as p: the reference does not divide)
    s = w.sum(1)
    unit = (s - 1).abs() < 1e-12
    assert int(unit.sum()) >= 40 and int((~unit).sum()) >= 8
    assert float((xyz[unit] - p[unit]).abs().max()) < 1e-14
    assert float((xyz[~unit] - p[~unit]).abs().max()) > 1e-3


def test_the_recipe_has_the_rows_the_design_asks_for():
    for N, E, J in ((1, 50, 6), (63, 7, 5), (4099, 50, 6)):
        p, S, P, w, c, f, g = R.recipe(N, E, J)
        assert p.shape == (N, 3) and S.shape == (N, 3, E) and P.shape == (N, 36, 3) and w.shape == (N, J) and g.shape == (N, 3)
        for A in (c[2], f[2]):
            assert bool((A[:, 3] == torch.tensor([0, 0, 0, 1.0], dtype=torch.float64)).all())
            assert bool((A[0] == torch.eye(4, dtype=torch.float64)).all())
            assert float((A[:, :3, :3] @ A[:, :3, :3].transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
        if N >= 63:
            s = w.sum(1)
            assert float(s[8:24].min()) >= 0.5 - 1e-12 and float(s[8:24].max()) <= 2 + 1e-12 and float((s[8:24] - 1).abs().max()) > 0.05
            assert bool((w[24:40, 0] == 0).all()) and float((w[24:40].sum(1) - 1).abs().max()) < 1e-12
            assert bool((w[:J] == torch.eye(J, dtype=torch.float64)).all())
            T_c = torch.einsum("nj,jab->nab", w, c[2])[:, :3, :3]
            assert float(torch.linalg.cond(T_c / w.sum(1)[:, None, None]).max()) < 1.5


def _recipe_digest(*args, **kw):
    """sha256 (first 16 hex digits) over every tensor of the recipe, rounded to float32 (the values the GPU tests feed)."""
    import hashlib
    p, S, P, w, c, f, g = R.recipe(*args, **kw)
    h = hashlib.sha256()
    for t in (p, S, P, w, *c, *f, g):
        h.update(t.float().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def test_the_recipe_keeps_its_values_and_is_valid_for_one_bone():
    """The digests were taken BEFORE the recipe learnt J = 1 (the rows without bone 0 are skipped there: with one bone the row would
    be 0 / 0, and the points are drawn smaller): every (N, E, J) in use then gives the same float32 bits now.  With J = 1 every
    tensor is finite, the weights are the softmax's 1 apart from the scaled block, and the deformation and its gradients are
    finite."""
    want = {(1, 50, 6): "0b22257940740a6f", (63, 7, 5): "f6eb026b67683433", (65, 50, 6): "a190ca7814dbc539",
            (4099, 50, 6): "a1770f02762c83a1", (4099, 7, 5): "d6b26c3fa37bd498", (33, 7, 5): "ee731b9948b4b382"}
    assert {k: _recipe_digest(*k) for k in want} == want
    assert _recipe_digest(40, 7, 5, seed=1) == "f65b7b9d4e7cf8c7" and _recipe_digest(5, 4, 3, seed=3) == "dc6d99d20b22d751"
    for N, E in ((1, 1), (30, 3), (4099, 1), (4099, 16)):
        p, S, P, w, c, f, g = R.recipe(N, E, 1)
        assert w.shape == (N, 1) and all(bool(torch.isfinite(t).all()) for t in (p, S, P, w, *c, *f, g)), (N, E)
        s = w[:, 0]
        assert bool((s[:8] == 1).all()) and bool((s[24:] == 1).all())
        if N > 24:
            assert float(s[8:24].min()) >= 0.5 and float(s[8:24].max()) <= 2.0 and float((s[8:24] - 1).abs().max()) > 0.05
        leaves = [t.clone().requires_grad_(True) for t in (p, S, P, w)]
        xyz = R.deform_points(*leaves, c, f)
        grads = torch.autograd.grad(xyz, leaves, g)
        assert bool(torch.isfinite(xyz).all()) and all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in grads)


def test_gradcheck_of_the_restatement():
    p, S, P, w, c, f, _ = R.recipe(5, 4, 3, seed=3)
    leaves = [t.clone().requires_grad_(True) for t in (p, S, P, w)]
    assert torch.autograd.gradcheck(lambda *x: R.deform_points(*x, c, f), leaves, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("N,E,J", [(65, 50, 6), (40, 7, 5)])
def test_the_written_backward_and_the_closed_forms_are_autograd(N, E, J):
    p, S, P, w, c, f, g = R.recipe(N, E, J, seed=1)
    leaves = [t.clone().requires_grad_(True) for t in (p, S, P, w)]
    xyz = R.deform_points(*leaves, c, f)
    want = torch.autograd.grad(xyz, leaves, g)
    written = R.deform_points_backward(p, S, P, w, c, f, g)
    closed = R.deform_points_closed_form(p, S, P, w, c, f, g)
    assert float((closed[0] - xyz.detach()).abs().max()) < 1e-13
    for name, a, b, r in zip(("points", "shapedirs", "posedirs", "weights"), written, closed[1:], want):
        assert float(r.abs().max()) > 0
        assert _rel(a, r) < 1e-13, name
        assert _rel(b, r) < 1e-13, name


def test_nearest_vertex_restatement_breaks_ties_towards_the_lowest_index():
    verts = torch.tensor([[0.0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0]])
    pts = torch.tensor([[0.5, 0, 0], [0.875, 0, 0], [0.5, 0.5, 0], [0, 2, 0]])
    idx, d2 = R.nearest_vertex(pts, verts)
    assert idx.tolist() == [0, 1, 0, 3] and d2.tolist() == [0.25, 0.015625, 0.5, 1.0]


def test_lbs_terms_restatement():
    g = torch.Generator().manual_seed(0)
    gw, gP, gS = torch.rand((7, 6), generator=g), torch.rand((7, 36, 3), generator=g), torch.rand((7, 3, 5), generator=g)
    idx = torch.tensor([3, 3, 0, 6])
    out = R.lbs_terms(idx, gw[idx] + 1.0, gP[idx] * 0 + gP[idx] - 2.0, gS[idx], gw, gP, gS)
    assert torch.allclose(out, torch.tensor([1.0, 4.0, 0.0]))


def test_the_counted_roundings_of_the_lbs_terms():
    """The formula the GPU test bounds the three losses with (tests/test_gpu_mono.py), on the sizes its docstring names."""
    from tests.test_gpu_mono import TERMS_GRID_CAP, _terms_roundings
    assert TERMS_GRID_CAP == 16384
    assert _terms_roundings(1027, 50, 6) == [1 + 1 + 1 + 18, 7 + 1 + 1 + 18, 10 + 1 + 1 + 18]
    assert _terms_roundings(TERMS_GRID_CAP, 50, 6)[2] == 10 + 1 + 4 + 18 and _terms_roundings(TERMS_GRID_CAP + 1, 64, 8)[2] == 12 + 2 + 4 + 18
    assert _terms_roundings(3 * TERMS_GRID_CAP + 5, 50, 6) == [1 + 4 + 4 + 18, 7 + 4 + 4 + 18, 36]
    assert _terms_roundings(1027, 1, 1) == [21, 27, 21]


def test_reference_lbs_weights():
    assert tuple(mono.reference_lbs_weights()) == pytest.approx((1.0, 10000.0, 10000.0))
    assert tuple(mono.reference_lbs_weights(5.0)) == pytest.approx((0.5, 5000.0, 5000.0))
    var = torch.tensor([0.5, 2.0, 4.0])
    got = mono.reference_lbs_weights(10.0, var)
    assert got.shapedirs == pytest.approx(1000 * 10 * ((2 + 0.5 + 0.25) / 3) / 50) and got.weights == 1.0 and got.posedirs == 10000.0
    # the folded coefficients against the reference's own composition (train/loss.py:439-445, :484-514) on random rows
    g = torch.Generator().manual_seed(1)
    pred, gt = [torch.randn((9, n), generator=g, dtype=torch.float64) for n in (6, 108, 150)], \
               [torch.randn((9, n), generator=g, dtype=torch.float64) for n in (6, 108, 150)]
    mse = lambda a, b: ((a - b) ** 2).mean()  # noqa: E731
    w = 10.0
    total = mse(pred[0], gt[0]) * w * 0.1 + mse(pred[1] * 10, gt[1] * 10) * w * 10.0 \
        + torch.mean(mse(pred[2] * 10, gt[2] * 10) / var.double() / 50) * w * 10.0
    folded = sum(c * mse(a, b) for c, a, b in zip(got, pred, gt))
    assert float(total) == pytest.approx(float(folded), rel=1e-12)


def test_upsample_table_and_radius_schedule():
    want = {0: 400, 4: 400, 5: 800, 9: 800, 10: 1600, 15: 3200, 20: 6400, 25: 10000, 29: 10000, 30: 20000, 39: 20000, 40: 40000,
            50: 80000, 59: 80000, 60: 100000, 61: 100000, 99: 100000}
    assert {e: mono.upsample_target(e) for e in want} == want
    assert [e for e in range(0, 81) if mono.radius_factor(e) == 0.75] == [5, 10, 15, 20, 25, 30, 40, 50, 65, 70, 75, 80]
    assert mono.radius_factor(60) == 0.9 and mono.radius_factor(61) == 1.0 and mono.radius_factor(0) == 1.0


def test_mono_points_init_prune_and_upsample():
    gen = torch.Generator().manual_seed(0)
    pc = mono.MonoPoints(n_init_points=400, scene_scale=1.0, device="cpu", generator=gen)
    assert pc.N == 400 and pc.points.requires_grad and pc.points.dtype == torch.float32
    assert float((pc.points.detach().norm(dim=1) - 0.5).abs().max()) < 1e-6                # the sphere of radius 0.5 / scene_scale
    assert pc.radius == pytest.approx(0.15 * 0.75 ** math.log2(4.0))
    assert pc.upsample(0, gen) == 0 and pc.N == 400 and pc.radius == pytest.approx(0.15 * 0.75 ** 2)
    r0, before = pc.radius, pc.points.detach().clone()
    assert pc.upsample(5, gen) == 400 and pc.N == 800 and pc.radius == pytest.approx(0.75 * r0)
    assert torch.equal(pc.points.detach()[:400], before) and pc.points.requires_grad
    # a new point is an old one jittered by at most half the OLD radius per axis
    d = (pc.points.detach()[400:, None, :] - before[None]).abs().amax(dim=2).amin(dim=1)
    assert float(d.max()) <= 0.5 * r0 + 1e-7 and float(d.max()) > 0
    opacity = torch.linspace(0, 1, 800).reshape(800, 1)
    pc.mark_visible(opacity)
    assert int(pc.visible.sum()) == int((opacity >= 0.1).sum()) and not bool(pc.visible[0])
    kept = pc.points.detach()[pc.visible].clone()
    pc.prune(pc.visible)
    assert pc.N == kept.shape[0] and torch.equal(pc.points.detach(), kept) and pc.points.requires_grad and not bool(pc.visible.any())
    with pytest.raises(RuntimeError, match="boolean mask"):
        pc.prune(torch.ones(3))
    small = mono.MonoPoints(n_init_points=100, max_points=150, device="cpu", generator=gen)
    assert small.upsample(70, gen) == 50 and small.N == 150                                   # never beyond max_points
    late = mono.MonoPoints(n_init_points=100, max_points=200, device="cpu", generator=gen)
    base = late.points.detach().clone()
    late.upsample(101, gen)                                                                    # after epoch 100: width 0.004
    d = (late.points.detach()[100:, None, :] - base[None]).abs().amax(dim=2).amin(dim=1)
    assert float(d.max()) <= 0.002 + 1e-7


def test_splat_attributes_is_the_reference_arithmetic():
    g = torch.Generator().manual_seed(0)
    f, o = torch.randn((9, 11), generator=g), torch.randn((9, 11), generator=g)
    rgb, op, sc, rot = mono.splat_attributes(f, o, radius=0.05, scene_scale=2.0)
    assert torch.allclose(rgb, torch.sigmoid(f[:, :3] + o[:, 8:]))
    assert torch.allclose(sc, torch.sigmoid(f[:, 3:6] + o[:, :3]) * 0.025 / 2.0 + 0.05)
    assert torch.allclose(rot, torch.nn.functional.normalize(f[:, 6:10] + o[:, 3:7])) and torch.allclose(op, torch.sigmoid(f[:, 10:] + o[:, 7:8]))
    assert rgb.shape == (9, 3) and op.shape == (9, 1) and sc.shape == (9, 3) and rot.shape == (9, 4)
    with pytest.raises(RuntimeError, match="features"):
        mono.splat_attributes(f[:, :10], o, 0.1)


def _f32_recipe(N=8, E=5, J=3):
    p, S, P, w, c, f, _ = R.recipe(N, E, J)
    f32 = lambda t: t.float()  # noqa: E731
    return [f32(t) for t in (p, S, P, w)], mono.PoseState(*map(f32, c)), mono.PoseState(*map(f32, f))


def test_deform_points_shape_dtype_and_device_errors():
    x, c, f = _f32_recipe()
    with pytest.raises(RuntimeError, match="float32"):
        mono.deform_points(x[0].double(), *x[1:], c, f)
    with pytest.raises(RuntimeError, match=r"shapedirs \[N,3,E\]"):
        mono.deform_points(x[0], x[1][:, :2], x[2], x[3], c, f)
    with pytest.raises(RuntimeError, match=r"posedirs \[N,36,3\]"):
        mono.deform_points(x[0], x[1], x[2][:, :35], x[3], c, f)
    with pytest.raises(RuntimeError, match="lbs_weights"):
        mono.deform_points(x[0], x[1], x[2], x[3][:7], c, f)
    with pytest.raises(RuntimeError, match="E in 1 .. 64"):
        mono.deform_points(x[0], torch.zeros(8, 3, 65), x[2], x[3], c, f)
    with pytest.raises(RuntimeError, match="J in 1 .. 8"):
        mono.deform_points(x[0], x[1], x[2], torch.zeros(8, 9), c, f)
    with pytest.raises(RuntimeError, match="canonical pose state"):
        mono.deform_points(*x, c._replace(betas=c.betas[:4]), f)
    with pytest.raises(RuntimeError, match="frame pose state"):
        mono.deform_points(*x, c, f._replace(transforms=f.transforms[:2]))
    with pytest.raises(RuntimeError, match="frame pose state requires grad"):
        mono.deform_points(*x, c, f._replace(betas=f.betas.clone().requires_grad_(True)))
    with pytest.raises(RuntimeError, match="canonical pose state requires grad"):
        mono.deform_points(*x, c._replace(transforms=c.transforms.clone().requires_grad_(True)), f)
    with pytest.raises(RuntimeError, match="a pose state is"):            # (before anything looks inside the state)
        mono.deform_points(*x, tuple(c)[:2], f)
    with pytest.raises(RuntimeError, match="a pose state is"):
        mono.deform_points(*x, c, f.betas)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mono.deform_points(*x, c, f)


def test_nearest_vertex_and_lbs_terms_argument_errors():
    p, v = torch.zeros(4, 3), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="float32"):
        mono.nearest_vertex(p.double(), v)
    with pytest.raises(RuntimeError, match=r"verts \[V,3\]"):
        mono.nearest_vertex(p, torch.zeros(5, 2))
    with pytest.raises(ValueError, match="V in 1 .. 8192"):
        mono.nearest_vertex(p, torch.zeros(0, 3))
    with pytest.raises(ValueError, match="V in 1 .. 8192"):
        mono.nearest_vertex(p, torch.zeros(8193, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mono.nearest_vertex(p, v)
    N, V, E, J = 4, 5, 7, 6
    idx = torch.zeros(N, dtype=torch.int32)
    a = [torch.zeros(N, J), torch.zeros(N, 36, 3), torch.zeros(N, 3, E), torch.zeros(V, J), torch.zeros(V, 36, 3), torch.zeros(V, 3, E)]
    with pytest.raises(RuntimeError, match="int32"):
        mono.lbs_terms_and_grad(idx.long(), *a)
    with pytest.raises(RuntimeError, match="gt_posedirs"):
        mono.lbs_terms_and_grad(idx, a[0], a[1], a[2], a[3], torch.zeros(V, 3, 36), a[5])
    with pytest.raises(RuntimeError, match="d_shapedirs"):
        mono.lbs_terms_and_grad(idx, *a, d_shapedirs=torch.zeros(N, E, 3))
    with pytest.raises(RuntimeError, match="float32"):
        mono.lbs_terms_and_grad(idx, a[0].double(), *a[1:])
    with pytest.raises(RuntimeError, match="no CPU path"):
        mono.lbs_terms_and_grad(idx, *a)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    d = _lib.fr_point_lbs()
    d.N, d.E, d.J = 0, 50, 6
    assert L.fr_point_lbs_forward(C.byref(d), None, None) == _lib.FR_ERR_INVALID_ARGUMENT      # null pose states
    d.E = 65
    assert L.fr_point_lbs_forward(C.byref(d), None, None) == _lib.FR_ERR_INVALID_ARGUMENT
    d.E, d.J = 50, 9
    assert L.fr_point_lbs_backward(C.byref(d), None, None, None, None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert L.fr_nearest_vertex(0, None, 0, None, None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert L.fr_nearest_vertex(0, None, _lib.FR_NEAREST_MAX_V + 1, 8, None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "FR_NEAREST_MAX_V" in _lib.last_error()
    assert L.fr_lbs_terms(None, 0, 1, 1, 1, *[None] * 11, None, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert L.fr_lbs_terms_workspace_bytes() >= 3 * 1024 * 4


def test_new_struct_layouts_match_the_c_compiler():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu\n", sizeof(fr_pose_state), sizeof(fr_point_lbs), sizeof(fr_lbs_terms_config));
 printf("%zu %zu %zu\n", offsetof(fr_pose_state, pose_feature), offsetof(fr_pose_state, transforms), offsetof(fr_point_lbs, J));
 printf("%zu %zu %zu %zu\n", offsetof(fr_point_lbs, points), offsetof(fr_point_lbs, weights), offsetof(fr_point_lbs, canonical), offsetof(fr_point_lbs, frame));
 printf("%zu %d %d %d %d\n", offsetof(fr_lbs_terms_config, shapedirs_weight), FR_LBS_MAX_E, FR_LBS_MAX_J, FR_LBS_POSE_FEATURES, FR_NEAREST_MAX_V);
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    ps, pl, tc = _lib.fr_pose_state, _lib.fr_point_lbs, _lib.fr_lbs_terms_config
    assert got == [C.sizeof(ps), C.sizeof(pl), C.sizeof(tc), ps.pose_feature.offset, ps.transforms.offset, pl.J.offset,
                   pl.points.offset, pl.weights.offset, pl.canonical.offset, pl.frame.offset, tc.shapedirs_weight.offset,
                   _lib.FR_LBS_MAX_E, _lib.FR_LBS_MAX_J, _lib.FR_LBS_POSE_FEATURES, _lib.FR_NEAREST_MAX_V]
