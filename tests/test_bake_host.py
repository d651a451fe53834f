"""CPU: the host side of the neural-baking kernels (csrc/fr_bake.hip, fateavatar_amd/texture.py `decode_attributes`,
fateavatar_amd/loss.py `rot_term_and_grad`): the exports, the argument checks of the C ABI (they run before any HIP call)
and of the Python interface, and the properties of the float64 restatements (tests/bake_ref.py) the GPU tests hold the
kernels to."""
import math
import os

import pytest
import torch

from fateavatar_amd import _lib, texture
from tests import bake_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_build_wiring():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fr_rasterizer.h")).read()
    for name in ("fr_bake_decode", "fr_bake_decode_backward", "fr_rot_term_workspace_bytes", "fr_rot_term"):
        assert name in _lib.EXPORTS and hasattr(L, name) and name + "(" in hdr
    mk = open(os.path.join(ROOT, "fateavatar_amd", "csrc", "Makefile")).read()
    strict = [l for l in mk.splitlines() if l.startswith("STRICT_UNITS")][0]
    assert "fr_bake" in strict.split() and "fr_tex_math.hpp" in mk          # built without FMA contraction, like fr_texture
    src = open(os.path.join(ROOT, "fateavatar_amd", "csrc", "fr_bake.hip")).read()
    assert '#include "fr_tex_math.hpp"' in src
    assert L.fr_rot_term_workspace_bytes() == 17 * 128 + 2 * 256 * 4        # the counters + two rows of per-workgroup partials


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    """Every check runs before the first HIP call, so it can be exercised without a GPU (the pointers are never followed)."""
    L = _lib.lib()
    f = 0x1000
    bad = _lib.FR_ERR_INVALID_ARGUMENT

    def refused(rc, *words):
        assert rc == bad, rc
        msg = _lib.last_error()
        for w in words:
            assert w in msg, msg

    dec = lambda N=10, uv=f, H=8, W=8, tex=f, outs=(f, f, f, f, f): L.fr_bake_decode(N, uv, H, W, tex, -5.0, -4.5, *outs, None)  # noqa: E731
    refused(dec(tex=None), "fr_bake_decode", "null tex_out")
    refused(dec(uv=None), "null uv")
    for k in range(5):
        refused(dec(outs=tuple(None if i == k else f for i in range(5))), "null output array")
    refused(dec(N=-1), "N must be")
    refused(dec(H=0), "H x W")
    refused(dec(W=-3), "H x W")
    refused(dec(H=1 << 15, W=1 << 15), "H x W")
    refused(dec(outs=(f, f, f, f + 4, f)), "16-byte aligned")
    assert dec(N=0, uv=None, outs=(None,) * 5) == _lib.FR_OK                 # nothing to do is not an error (launches nothing)

    def bwd(N=10, uv=f, H=8, W=8, rs=f, en=f, tex=f, d=(f, f, f, f, f), d_tex=f):
        return L.fr_bake_decode_backward(N, uv, H, W, rs, en, tex, -5.0, -4.5, *d, d_tex, None)
    refused(bwd(tex=None), "fr_bake_decode_backward", "null tex_out")
    refused(bwd(uv=None), "null uv")
    refused(bwd(d_tex=None), "null d_tex_out")
    refused(bwd(rs=None), "null plan")
    refused(bwd(en=None), "null plan")
    refused(bwd(N=-2), "N must be")
    refused(bwd(H=0), "H x W")
    refused(bwd(H=1 << 15, W=1 << 15), "H x W")
    refused(bwd(d=(f, f, f, f + 8, f)), "16-byte aligned")

    ws = L.fr_rot_term
    refused(ws(0.1, -1, f, f, f, f, None), "fr_rot_term", "negative N")
    refused(ws(0.1, 4, None, f, f, f, None), "null rotation array")
    refused(ws(0.1, 4, f, f, None, f, None), "null workspace or loss")
    refused(ws(0.1, 4, f, f, f, None, None), "null workspace or loss")
    refused(ws(0.1, 4, f + 4, f, f, f, None), "16-byte aligned")
    assert ws(0.1, 0, None, None, f, f, None) == _lib.FR_OK                  # N == 0: nothing is launched


def test_python_interface_refuses_bad_arguments():
    from fateavatar_amd.loss import rot_loss, rot_term_and_grad

    class _Plan:                      # (the checks need no device to refuse)
        H, W, N = 8, 8, 10
    with pytest.raises(RuntimeError, match=r"\[1,11,H,W\]"):
        texture.decode_attributes(torch.zeros(1, 10, 8, 8), _Plan(), -5.0, -4.5)
    with pytest.raises(RuntimeError, match=r"\[1,11,H,W\]"):
        texture.decode_attributes(torch.zeros(2, 11, 8, 8), _Plan(), -5.0, -4.5)
    with pytest.raises(RuntimeError, match="is 8 x 9, the plan was made for 8 x 8"):
        texture.decode_attributes(torch.zeros(1, 11, 8, 9), _Plan(), -5.0, -4.5)
    with pytest.raises(RuntimeError, match="float32"):
        texture.decode_attributes(torch.zeros(1, 11, 8, 8, dtype=torch.float64), _Plan(), -5.0, -4.5)
    with pytest.raises(RuntimeError, match=r"must be on a HIP device \(there is no CPU path\)"):
        texture.decode_attributes(torch.zeros(1, 11, 8, 8), _Plan(), -5.0, -4.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rot_term_and_grad(torch.zeros(4, 4), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rot_loss(torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match=r"\[N,4\]"):
        rot_loss(torch.zeros(4, 3))


def test_bake_step_says_what_it_takes_before_it_touches_a_device():
    from fateavatar_amd import bake
    from fateavatar_amd.loss import ScaleRatioTerm
    assert bake.REFERENCE_ROT_TERM == bake.RotTerm(0.1) and bake.BAKE_LR == 1e-3 and bake.N_CHANNELS == 11
    assert isinstance(ScaleRatioTerm(), tuple)
    with pytest.raises(TypeError, match="BakedAvatar"):
        bake.BakeStep(object(), None, None, None, None)


# ------------------------------------------------------------------ the rot-term restatement
def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 4, generator=g, dtype=torch.float64) * 2 - 1


def test_rot_restatement_gradient_agrees_with_central_differences():
    q = _rows(7, 3)
    _, grad = R.rot_loss_and_grad(q, torch.float64)
    h = 1e-6
    worst = 0.0
    for i in range(q.shape[0]):
        for j in range(4):
            p, m = q.clone(), q.clone()
            p[i, j] += h
            m[i, j] -= h
            fd = float(R.rot_loss(p) - R.rot_loss(m)) / (2 * h)
            # central differences: h^2 / 6 x the third derivative, and 2^-53 |loss| / h of rounding; both far below 1e-6 relative
            tol = 1e-6 * max(1.0, abs(fd))
            worst = max(worst, abs(fd - float(grad[i, j])) / tol)
            assert abs(fd - float(grad[i, j])) <= tol, (i, j, fd, float(grad[i, j]))
    print("rot restatement against central differences: worst error / tolerance", worst)


def test_rot_restatement_on_rows_without_a_vector_part():
    for row in ([1.0, 0, 0, 0], [0.0, 0, 0, 0], [-1.0, 0, 0, 0]):
        q = torch.cat([torch.tensor([row], dtype=torch.float64), _rows(3, 1)])
        loss_all, grad = R.rot_loss_and_grad(q, torch.float64)
        alone, g1 = R.rot_loss_and_grad(torch.tensor([row], dtype=torch.float64), torch.float64)
        assert float(alone) == 0.0 and bool((g1 == 0).all()) and bool(torch.isfinite(g1).all()), row
        assert bool((grad[0] == 0).all()) and bool(torch.isfinite(grad).all()) and float(loss_all) > 0, row


def test_rot_restatement_by_hand():
    """A rotation by theta about x with the real part first: raw = (theta, 0, 0), so one row's loss is theta^2."""
    theta = 0.7
    q = torch.tensor([[math.cos(theta / 2), math.sin(theta / 2), 0.0, 0.0]], dtype=torch.float64)
    assert abs(float(R.rot_loss(q)) - theta * theta) < 1e-14
    q = torch.tensor([[math.cos(theta / 2), 0.0, math.sin(theta / 2), 0.0]], dtype=torch.float64)    # about y: raw[1] is not in the loss
    assert float(R.rot_loss(q)) == 0.0


# ------------------------------------------------------------------ the rotation activation at a zero texel
def test_rotation_activation_jacobian_at_a_zero_texel_is_pi():
    """d q / d a = I / 2 at a = 0, a = tanh(t) 2 pi: the Jacobian of the emitted (z, w, x, y) with respect to t has pi on
    its three non-zero entries — (0, 2), (2, 0), (3, 1) — and is finite: nothing divides by theta."""
    t = torch.zeros(3, 1, 1, dtype=torch.float64)
    J = torch.autograd.functional.jacobian(lambda x: texture.rotation_activation(x).reshape(4), t).reshape(4, 3)
    want = torch.zeros(4, 3, dtype=torch.float64)
    want[0, 2] = want[2, 0] = want[3, 1] = math.pi
    assert bool(torch.isfinite(J).all()) and torch.equal(J, want), J
    # ... and the Taylor branch continues it: a texel of 1e-9 (theta below 1e-6) has the same Jacobian to 1e-6
    t = torch.full((3, 1, 1), 1e-9, dtype=torch.float64)
    J2 = torch.autograd.functional.jacobian(lambda x: texture.rotation_activation(x).reshape(4), t).reshape(4, 3)
    assert float((J2 - want).abs().max()) < 1e-6
