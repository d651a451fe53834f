"""CPU: the host side of the L1 + D-SSIM image loss — window taps, workspace sizes, argument checks of the wrappers and of
the C entry, the ABI struct, the steps' new argument — and the restatement the GPU tests use as their reference
(tests/image_loss_ref.py) against the formulas' closed-form gradient."""
import ctypes as C
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from fateavatar_amd import _lib
from tests import image_loss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_taps_are_the_reference_arithmetic_bit_for_bit():
    from fateavatar_amd.loss import ssim_window
    w = ssim_window()
    assert w.dtype == torch.float32 and w.shape == (11,) and w.device.type == "cpu"
    # the order the library defines: float32 roundings of the doubles, summed pairwise over the taps padded to 16, divided
    g = np.array([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)]).astype(np.float32)
    t = list(g) + [np.float32(0)] * 5
    while len(t) > 1:
        t = [np.float32(t[i] + t[i + 1]) for i in range(0, len(t), 2)]
    assert w.numpy().tolist() == (g / t[0]).astype(np.float32).tolist()
    # and the reference's own arithmetic (torch.sum's order is its build's and the CPU's; on its vectorised paths it is this one)
    assert torch.equal(w, ref.window_taps())
    assert torch.equal(w, w.flip(0)) and float(w[5]) == float(w.max())
    assert abs(float(w.double().sum()) - 1.0) <= 2 * 2.0 ** -23       # 2 ulp at 1
    out = (C.c_float * 11)()
    _lib.lib().fr_ssim_window(out)
    assert list(out) == w.tolist()


def test_workspace_bytes_cover_the_maps_and_the_partials():
    L = _lib.lib()
    ws = L.fr_image_loss_workspace_bytes
    T = ref.TILE
    for C_, H, W in [(1, 1, 1), (3, 1, 1), (3, 7, 5), (3, 128, 128), (3, 512, 512), (3, 1024, 1024), (1, 33, 47), (4, 2048, 1024)]:
        tiles = C_ * -(-H // T) * -(-W // T)
        assert ws(C_, H, W) >= 12 * C_ * H * W + 8 * tiles and ws(C_, H, W) >= L.fr_l1_workspace_bytes(), (C_, H, W)
        assert ws(C_, H, W) <= 12 * C_ * H * W + 8 * tiles + 16384          # sane: nothing else of size in it
        assert ws(C_, H + 1, W) > ws(C_, H, W) and ws(C_, H, W + 1) > ws(C_, H, W) and ws(C_ + 1, H, W) > ws(C_, H, W)
    assert 0 < ws(1, 1, 1) < 65536
    assert ws(0, 4, 4) == 0 and ws(3, 0, 4) == 0 and ws(3, 4, -1) == 0


def test_wrappers_refuse_bad_arguments():
    from fateavatar_amd.loss import ImageLoss, d_ssim, image_loss_and_grad, image_loss_and_grad_batch, image_loss_workspace
    assert ImageLoss(0.8, 0.2).rgb_weight == 0.8 and ImageLoss(0.8, 0.2).dssim_weight == 0.2 and ImageLoss._fields == ("rgb_weight", "dssim_weight")
    x, y = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        image_loss_and_grad(x, y, (0.8, 0.2))
    with pytest.raises(RuntimeError):
        image_loss_and_grad(x, torch.rand(3, 8, 9), (0.8, 0.2))
    need = _lib.lib().fr_image_loss_workspace_bytes(3, 8, 8)
    assert need > 12 * 3 * 8 * 8
    with pytest.raises(RuntimeError, match="no CPU path"):            # the device comes first, whatever else is wrong
        image_loss_and_grad(x, y, (0.8, 0.2), workspace=torch.zeros(need - 1, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        image_loss_and_grad_batch([x], [y], (0.8, 0.2), [torch.zeros(3)], [None], [torch.zeros(1, dtype=torch.uint8)])
    five = [x] * (_lib.FR_MAX_BATCH + 1)
    with pytest.raises(RuntimeError, match="1 .. 4 images"):
        image_loss_and_grad_batch(five, five, (0.8, 0.2), five, five, five)
    with pytest.raises(RuntimeError, match="1 .. 4 images"):
        image_loss_and_grad_batch([], [], (0.8, 0.2), [], [], [])
    with pytest.raises(RuntimeError, match="C, H, W >= 1"):
        image_loss_workspace(torch.device("cpu"), 3, 0, 8)
    with pytest.raises(RuntimeError, match="img2"):
        d_ssim(x, y.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="no CPU path"):
        d_ssim(x.clone().requires_grad_(), y)


def test_c_entry_refuses_bad_sizes_and_counts():
    L = _lib.lib()
    cfg = _lib.fr_image_loss_config(0.8, 0.2)
    one = (C.c_void_p * 4)(256, 256, 256, 256)      # never dereferenced: every call below fails its checks first
    two_ws = (C.c_void_p * 4)(256, 256, 512, 768)
    call = lambda n, c, h, w, ws=one, cfgp=C.byref(cfg): L.fr_image_loss_grad(cfgp, n, c, h, w, one, one, one, one, ws, None)  # noqa: E731
    for args, needle in (((0, 3, 8, 8), "FR_MAX_BATCH"), ((5, 3, 8, 8), "FR_MAX_BATCH"), ((1, 0, 8, 8), "C, H, W"),
                         ((1, 3, 0, 8), "C, H, W"), ((1, 3, 8, -1), "C, H, W"), ((2, 3, 8, 8), "one workspace per image")):
        assert call(*args) == _lib.FR_ERR_INVALID_ARGUMENT, args
        assert needle in _lib.last_error(), (args, _lib.last_error())
    assert call(1, 3, 8, 8, cfgp=None) == _lib.FR_ERR_INVALID_ARGUMENT and "configuration" in _lib.last_error()
    misaligned = (C.c_void_p * 4)(260, 256, 512, 768)
    assert call(1, 3, 8, 8, ws=misaligned) == _lib.FR_ERR_INVALID_ARGUMENT and "aligned" in _lib.last_error()
    assert L.fr_image_loss_grad(C.byref(cfg), 1, 3, 8, 8, None, one, one, one, two_ws, None) == _lib.FR_ERR_INVALID_ARGUMENT


def test_config_struct_matches_the_header(tmp_path):
    """tests/test_abi.py's mechanism: the C compiler's layout of the header's struct against the ctypes mirror."""
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu\n", sizeof(fr_image_loss_config), offsetof(fr_image_loss_config, rgb_weight), offsetof(fr_image_loss_config, dssim_weight));
 return 0; }'''
    src, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(src, "w").write(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    cfg = _lib.fr_image_loss_config
    assert out == [C.sizeof(cfg), cfg.rgb_weight.offset, cfg.dssim_weight.offset] == [8, 0, 4]
    assert {"fr_ssim_window", "fr_image_loss_workspace_bytes", "fr_image_loss_grad"} <= set(_lib.EXPORTS)


def test_steps_take_the_image_loss_argument():
    from fateavatar_amd import rigged, train
    from fateavatar_amd.loss import ImageLoss
    for cls in (rigged.RiggedStep, train.TrainStep):
        p = inspect.signature(cls.__init__).parameters
        assert "image_loss" in p and p["image_loss"].default is None, cls
    assert rigged.REFERENCE_IMAGE_LOSS == ImageLoss(0.8, 0.2)
    from fateavatar_amd.avatar import AvatarBatchStep, AvatarStep
    for cls in (AvatarStep, AvatarBatchStep):      # FateAvatar's own dssim weight is 0: its steps do not take the argument
        assert "image_loss" not in inspect.signature(cls.__init__).parameters


@pytest.mark.parametrize("kind", ref.KINDS)
def test_restatement_agrees_with_the_closed_form_gradient(kind):
    """The reference of the GPU tests pinned on the CPU: float64 autograd of the restatement against the closed form
        d d_ssim / dx = -(1/N) [conv(dM) + 2 x conv(dS11) + y conv(dS12)]
    written out with the window applied as 121 shifted, weighted copies of the padded map (another evaluation than the
    restatement's conv2d).  The window is the reference's: the taps' products ROUNDED TO float32 (`create_window` multiplies in
    float32), which a separable pair of float64 1-D passes is not — that form, which this test used before the restatement was
    held to a recorded run of the reference's d_ssim, is 5.6e-9 of d_ssim away."""
    import torch.nn.functional as F
    x, y, t64, t32 = ref.case((3, 33, 47), kind)
    l1, ds, g1, gs = t64
    X, Y = x.double(), y.double()
    g = ref.window_taps()
    w2 = (g[:, None] * g[None, :]).double()            # float32 products, then the images' dtype
    assert w2.dtype == torch.float64 and torch.equal(w2, w2.float().double()) and torch.equal(w2, w2.T)
    H, W = X.shape[1:]

    def conv(t):
        p = F.pad(t, (5, 5, 5, 5))
        return sum(w2[i, j] * p[:, i:i + H, j:j + W] for i in range(11) for j in range(11))

    mu1, mu2 = conv(X), conv(Y)
    s11, s22, s12 = conv(X * X) - mu1 ** 2, conv(Y * Y) - mu2 ** 2, conv(X * Y) - mu1 * mu2
    A, B, Cc, D = 2 * mu1 * mu2 + ref.C1, 2 * s12 + ref.C2, mu1 ** 2 + mu2 ** 2 + ref.C1, s11 + s22 + ref.C2
    dS11, dS12 = -A * B / (Cc * D * D), 2 * A / (Cc * D)
    dM = 2 * mu2 * B / (Cc * D) - 2 * mu1 * A * B / (Cc * Cc * D) - 2 * mu1 * dS11 - mu2 * dS12
    want = -(conv(dM) + 2 * X * conv(dS11) + Y * conv(dS12)) / X.numel()
    assert abs(float(1 - (A * B / (Cc * D)).mean()) - float(ds)) <= 1e-13
    assert float((gs - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(g1, torch.sign(X - Y) / X.numel()) and abs(float(l1) - float((X - Y).abs().mean())) <= 1e-15
    # and the float32 twin sits where the GPU bounds expect it: well inside them
    for w in ref.WEIGHTS:
        dl, rl2, ent = ref.errors(*ref.combine(t32, w), *ref.combine(t64, w))
        assert dl <= ref.LOSS_ATOL / 4 and rl2 <= ref.GRAD_REL_L2 / 4 and ent <= ref.GRAD_ENTRY / 4, (kind, w, dl, rl2, ent)
