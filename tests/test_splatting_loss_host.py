"""CPU: SplattingAvatar's loss terms — the restatement of tests/splatting_loss_ref.py on hand-computed cases (it is the reference of
tests/test_gpu_splatting_loss.py), and what the library's two entry points answer without a device: the layouts of their
configuration structs, their workspace sizes and their refusals."""
import ctypes as C
import math
import os
import subprocess
import tempfile
import types

import pytest
import torch

from fateavatar_amd import _lib
from tests import splatting_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = math.log


def _scaling(rows):
    return torch.tensor([[LOG(v) for v in r] for r in rows], dtype=torch.float64)


# ------------------------------------------------------------------ 1. the restatement on cases worked out by hand
def test_pixel_terms_by_hand():
    """d = (0.5, -0.25, 0, 1): l1 = 1.75 / 4, mse = (0.25 + 0.0625 + 1) / 4; gradient sign(d) / 4 + 10 * 2 d / 4, 0 at d = 0."""
    img = torch.tensor([[[0.75, 0.25, 0.5, 1.0]]], dtype=torch.float64)
    gt = torch.tensor([[[0.25, 0.5, 0.5, 0.0]]], dtype=torch.float64)
    loss, g = R.pixel_terms(img, gt, 1.0, 10.0)
    assert loss.tolist() == [0.4375 + 10.0 * 0.328125, 0.4375, 0.328125]
    assert g.reshape(-1).tolist() == [0.25 + 2.5, -0.25 - 1.25, 0.0, 0.25 + 5.0]
    loss, g = R.pixel_terms(img, gt, 1.0, 0.0)
    assert loss.tolist() == [0.4375, 0.4375, 0.328125] and g.reshape(-1).tolist() == [0.25, -0.25, 0.0, 0.25]
    loss, g = R.pixel_terms(img, gt, 0.0, 1.0)
    assert loss.tolist() == [0.328125, 0.4375, 0.328125] and g.reshape(-1).tolist() == [0.25, -0.125, 0.0, 0.5]


def test_scale_term_by_hand():
    """Gates 0.008 and 10.  Row A (0.1, 0.001, 0.001): selected, smax 0.1 at component 0.  Row B (0.004, 0.0001, 0.0001): ratio 40
    but smax <= max_scaling.  Row C (0.1, 0.05, 0.02): smax over the gate but ratio 5.  Row D (0.001, 0.002, 0.5): selected, smax
    0.5 at component 2.  Mean over A and D = 0.3; the gradient is weight * smax / 2 at the argmax of the selected rows only."""
    s = _scaling([[0.1, 0.001, 0.001], [0.004, 0.0001, 0.0001], [0.1, 0.05, 0.02], [0.001, 0.002, 0.5]])
    loss, n, g, sel = R.scale_term(s, 2.0, 10.0, 0.008)
    assert sel.tolist() == [True, False, False, True] and n == 2
    assert abs(float(loss) - 0.3) < 1e-15
    want = torch.zeros(4, 3, dtype=torch.float64)
    want[0, 0], want[3, 2] = 2.0 * 0.1 / 2, 2.0 * 0.5 / 2
    assert torch.allclose(g, want, rtol=1e-14, atol=0) and bool((g[~sel] == 0).all())
    # one row
    loss, n, g, sel = R.scale_term(s[:1], 1.0, 10.0, 0.008)
    assert n == 1 and abs(float(loss) - 0.1) < 1e-15 and abs(float(g[0, 0]) - 0.1) < 1e-15 and g[0, 1:].tolist() == [0.0, 0.0]
    # the empty selection: 0, no gradient, nothing divided by the empty count
    for rows in (s[1:3], _scaling([[1e-4, 1e-4, 1e-4]] * 5)):
        loss, n, g, sel = R.scale_term(rows, 1.0, 10.0, 0.008)
        assert n == 0 and float(loss) == 0.0 and not bool(g.any()) and bool(torch.isfinite(g).all())
    # the two gates are strict: smax == max_scaling and ratio == scale_threshold are not selected
    s = torch.tensor([[LOG(0.008), LOG(0.0001), LOG(0.0001)]], dtype=torch.float64)
    assert R.scale_term(s, 1.0, 10.0, float(torch.exp(s[0, 0])))[1] == 0 and R.scale_term(s, 1.0, 10.0, 0.0079)[1] == 1
    s = torch.tensor([[3.0, 1.0, 2.0]], dtype=torch.float64)      # exp(3) / exp(1): the ratio itself as the threshold
    ratio = float(torch.exp(s[0, 0]) / torch.exp(s[0, 1]))
    assert R.scale_term(s, 1.0, ratio, 0.008)[1] == 0 and R.scale_term(s, 1.0, ratio * (1 - 1e-12), 0.008)[1] == 1
    # a NaN row is not selected (its comparisons are false) and leaves the others' mean alone
    s = _scaling([[0.1, 0.001, 0.001], [0.2, 0.001, 0.001]])
    s[1, 1] = float("nan")
    loss, n, g, sel = R.scale_term(s, 1.0, 10.0, 0.008)
    assert sel.tolist() == [True, False] and abs(float(loss) - 0.1) < 1e-15


def test_redraw_rule():
    """draw_scaling leaves no undecided row, about 65 % selected; undecided_rows flags each of its three cases."""
    g = torch.Generator().manual_seed(1)
    s = R.draw_scaling(10_000, g)
    assert s.dtype == torch.float32 and not bool(R.undecided_rows(s, 10.0, 0.008).any())
    n = R.scale_term(s, 1.0, 10.0, 0.008)[1]
    assert 6000 < n < 7000, n
    rows = _scaling([[0.008 * (1 + 5e-5), 1e-4, 1e-4], [0.1, 0.01 * (1 - 5e-5), 0.02], [0.1, 0.1 * (1 - 5e-7), 1e-3], [0.1, 0.001, 0.002]])
    assert R.undecided_rows(rows, 10.0, 0.008).tolist() == [True, True, True, False]


# ------------------------------------------------------------------ 2. the ABI without a device
def test_config_struct_layouts_match_the_c_compiler():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu\n", sizeof(fr_pixel_loss_config), offsetof(fr_pixel_loss_config, rgb_weight), offsetof(fr_pixel_loss_config, mse_weight));
 printf("%zu %zu %zu %zu\n", sizeof(fr_scale_term_config), offsetof(fr_scale_term_config, weight),
        offsetof(fr_scale_term_config, scale_threshold), offsetof(fr_scale_term_config, max_scaling));
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    p, s = _lib.fr_pixel_loss_config, _lib.fr_scale_term_config
    assert sizes[:3] == [C.sizeof(p), p.rgb_weight.offset, p.mse_weight.offset] == [8, 0, 4]
    assert sizes[3:] == [C.sizeof(s), s.weight.offset, s.scale_threshold.offset, s.max_scaling.offset] == [12, 0, 4, 8]


def test_workspace_sizes_and_refusals():
    """Both workspaces are the last-workgroup counters (17 lines of 128 bytes) and two rows of 1 024 partials; the entry points
    refuse null arguments, misaligned images and a row count whose float count would not be exact — before anything is launched."""
    L = _lib.lib()
    assert L.fr_pixel_loss_workspace_bytes() == L.fr_huber_workspace_bytes() == 17 * 128 + 2 * 1024 * 4
    assert L.fr_scale_term_workspace_bytes() == L.fr_regularise_workspace_bytes() == 17 * 128 + 2 * 1024 * 4
    pcfg, scfg = _lib.fr_pixel_loss_config(1.0, 10.0), _lib.fr_scale_term_config(1.0, 10.0, 0.008)
    bad = _lib.FR_ERR_INVALID_ARGUMENT
    a = 4096     # (an aligned non-null address: every call below is refused before it is used)
    assert L.fr_pixel_loss_grad(None, 3, 4, 4, a, a, a, a, a, None) == bad
    for k in (0, 1, 3, 4):
        args = [a, a, a, a, a]
        args[k] = None
        assert L.fr_pixel_loss_grad(C.byref(pcfg), 3, 4, 4, *args, None) == bad, k
    assert b"fr_pixel_loss_grad" in L.fr_last_error()
    assert L.fr_pixel_loss_grad(C.byref(pcfg), -1, 4, 4, a, a, a, a, a, None) == bad
    for k in (0, 1, 2):
        args = [a, a, a, a, a]
        args[k] = a + 4
        assert L.fr_pixel_loss_grad(C.byref(pcfg), 3, 4, 4, *args, None) == bad, k
    assert L.fr_pixel_loss_grad(C.byref(pcfg), 3, 0, 4, a, a, None, a, a, None) == _lib.FR_OK      # n == 0: nothing is launched
    assert L.fr_scale_term(None, 4, a, a, a, a, None) == bad
    assert L.fr_scale_term(C.byref(scfg), -1, a, a, a, a, None) == bad
    assert L.fr_scale_term(C.byref(scfg), 4, None, a, a, a, None) == bad
    assert L.fr_scale_term(C.byref(scfg), 4, a, a, None, a, None) == bad
    assert L.fr_scale_term(C.byref(scfg), 4, a, a, a, None, None) == bad
    assert L.fr_scale_term(C.byref(scfg), 1 << 24, a, a, a, a, None) == bad and b"2^24" in L.fr_last_error()
    assert L.fr_scale_term(C.byref(scfg), 0, None, None, a, a, None) == _lib.FR_OK                  # P == 0: nothing is launched


def test_python_refusals():
    """No CPU path; a step takes an ImageLoss, a PixelLoss or None as its image term, and says so."""
    from fateavatar_amd.loss import (ImageLoss, PixelLoss, ScaleTerm, pixel_loss_and_grad, pixel_loss_workspace, scale_term_and_grad,
                                     scale_term_workspace)
    from fateavatar_amd.splatting import REFERENCE_IMAGE_LOSS, REFERENCE_SCALE_TERM
    from fateavatar_amd.train import TrainStep
    assert REFERENCE_IMAGE_LOSS == PixelLoss(1.0, 10.0) and isinstance(REFERENCE_IMAGE_LOSS, PixelLoss)
    assert REFERENCE_SCALE_TERM == ScaleTerm(1.0, 10.0, 0.008) and isinstance(REFERENCE_SCALE_TERM, ScaleTerm)
    assert (R.REFERENCE["rgb_weight"], R.REFERENCE["mse_weight"]) == tuple(REFERENCE_IMAGE_LOSS)
    assert (R.REFERENCE["scale_weight"], R.REFERENCE["scale_threshold"], R.REFERENCE["max_scaling"]) == tuple(REFERENCE_SCALE_TERM)
    x = torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pixel_loss_and_grad(x, x, PixelLoss(1.0, 10.0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        scale_term_and_grad(torch.zeros(4, 3), None)
    for maker in (pixel_loss_workspace, scale_term_workspace):
        with pytest.raises(RuntimeError, match="no CPU path"):
            maker(torch.device("cpu"))
    step = types.SimpleNamespace()
    for other in ((1.0, 10.0), [0.8, 0.2], 1.0, ScaleTerm()):
        with pytest.raises(TypeError, match=r"ImageLoss.*PixelLoss"):
            TrainStep._init_image_loss(step, other)
    assert ImageLoss(0.8, 0.2) != PixelLoss(1.0, 10.0)
