"""CPU: FateAvatar's scale-ratio term — the restatement of tests/fate_scale_ref.py against the recorded run of the reference's own
`FateAvatarLoss.accumulate_gradients` (tests/golden/reference_fate_scale.npz, written by tests/golden/make_fate_scale_runs.py),
the package's constants against the recorded parameters, and what the library's entry point answers without a device: the
layout of its configuration struct, its workspace size and its refusals."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

from fateavatar_amd import _lib
from tests import fate_scale_ref as R
from tests.reference_runs import Case, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["fatescale_mixed", "fatescale_none", "fatescale_init"]


# ------------------------------------------------------------------ 1. the restatement against the recorded run
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_recorded_run(name):
    """float64 on the fixture's float32 inputs: scale_loss and d_scaling (scale_weight applied) to 1e-12; the margins the
    generator asserted hold on the stored inputs; the cases that are to be exactly zero are."""
    c = Case(name)
    s = c.inp("scaling")
    assert tuple(s.shape) == (257, 3) and s.dtype == torch.float32
    loss, count, g = R.loss_count_grad(s, c.param("scale_weight"), c.param("scale_threshold"))
    assert rel(loss, c.out("scale_loss")) <= 1e-12 and rel(g, c.out("d_scaling")) <= 1e-12
    gate, tie = R.margins(s, c.param("scale_threshold"))
    assert gate >= 1e-2 and tie >= 1e-3 and abs(gate - c.scalar("margin_ratio")) <= 1e-12
    if name == "fatescale_mixed":
        assert 0.35 * 257 <= count <= 0.65 * 257 and float(c.out("scale_loss")) > 0
        assert abs(tie - c.scalar("margin_tie")) <= 1e-12
        assert int((c.out("d_scaling") != 0).sum()) == 2 * count      # one entry on the largest, one on the smallest component
    else:
        assert count == 0 and float(c.out("scale_loss")) == 0 and int(c.out("d_scaling").count_nonzero()) == 0
        assert float(loss) == 0 and int(g.count_nonzero()) == 0
    if name == "fatescale_init":
        assert bool((s == s[:, :1]).all())


def test_restatement_by_hand():
    """exp(log 20) / exp(log 2) = 10 against 9: loss 1 / 2 rows, gradient +- w / 2 x 10 on the largest / smallest component."""
    s = torch.log(torch.tensor([[2.0, 20.0, 5.0], [1.0, 2.0, 3.0]], dtype=torch.float64))
    loss, count, g = R.loss_count_grad(s, 0.1, 9.0)
    assert abs(float(loss) - 0.5) < 1e-14 and count == 1
    assert torch.allclose(g, torch.tensor([[-0.5, 0.5, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64), atol=1e-14, rtol=0)


def test_reference_constants_are_the_recorded_parameters():
    from fateavatar_amd.avatar import REFERENCE_SCALE_TERM
    from fateavatar_amd.loss import ScaleRatioTerm
    assert isinstance(REFERENCE_SCALE_TERM, ScaleRatioTerm) and ScaleRatioTerm() == REFERENCE_SCALE_TERM
    for name in CASES:
        c = Case(name)
        assert REFERENCE_SCALE_TERM == ScaleRatioTerm(c.param("scale_weight"), c.param("scale_threshold"))
        assert c.param("rgb_weight") == 1.0


# ------------------------------------------------------------------ 2. the ABI without a device
def test_header_ctypes_and_library_agree():
    header = open(os.path.join(ROOT, "include", "fr_rasterizer.h")).read()
    for sym in ("fr_scale_ratio_workspace_bytes", "fr_scale_ratio_term"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym) and sym + "(" in header
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu\n", sizeof(fr_scale_ratio_config), offsetof(fr_scale_ratio_config, weight), offsetof(fr_scale_ratio_config, scale_threshold));
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    s = _lib.fr_scale_ratio_config
    assert sizes == [C.sizeof(s), s.weight.offset, s.scale_threshold.offset] == [8, 0, 4]


def test_workspace_size_and_refusals():
    """The workspace is the siblings': the last-workgroup counters and two rows of 1 024 partials.  Null arguments and a row
    count whose float count would not be exact are refused before anything is launched, with fr_scale_term's messages."""
    L = _lib.lib()
    assert L.fr_scale_ratio_workspace_bytes() == L.fr_scale_term_workspace_bytes() == 17 * 128 + 2 * 1024 * 4
    cfg = _lib.fr_scale_ratio_config(0.1, 9.0)
    bad, a = _lib.FR_ERR_INVALID_ARGUMENT, 4096     # (a non-null address: every call below is refused before it is used)
    assert L.fr_scale_ratio_term(None, 4, a, a, a, a, None) == bad and b"fr_scale_ratio_term: null configuration" in L.fr_last_error()
    assert L.fr_scale_ratio_term(C.byref(cfg), -1, a, a, a, a, None) == bad
    assert L.fr_scale_ratio_term(C.byref(cfg), 4, None, a, a, a, None) == bad and b"null parameter array" in L.fr_last_error()
    assert L.fr_scale_ratio_term(C.byref(cfg), 4, a, a, None, a, None) == bad
    assert L.fr_scale_ratio_term(C.byref(cfg), 4, a, a, a, None, None) == bad and b"null workspace or loss" in L.fr_last_error()
    assert L.fr_scale_ratio_term(C.byref(cfg), 1 << 24, a, a, a, a, None) == bad and b"2^24" in L.fr_last_error()
    assert L.fr_scale_ratio_term(C.byref(cfg), 0, None, None, a, a, None) == _lib.FR_OK                # P == 0: nothing is launched


def test_python_refusals():
    """No CPU path; a step takes a ScaleRatioTerm or None, and says so before it touches a device."""
    from fateavatar_amd.avatar import AvatarBatchStep, AvatarStep
    from fateavatar_amd.loss import ScaleTerm, scale_ratio_loss, scale_ratio_term_and_grad
    s = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        scale_ratio_term_and_grad(s, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        scale_ratio_loss(s)
    with pytest.raises(RuntimeError, match=r"\[P,3\]"):
        scale_ratio_loss(torch.zeros(4, 2))
    for term in (3, (0.1, 9.0), ScaleTerm()):
        with pytest.raises(TypeError, match="ScaleRatioTerm or None"):
            AvatarStep(None, None, None, None, None, scale_term=term)
    with pytest.raises(TypeError, match="ScaleRatioTerm or None"):
        AvatarBatchStep(None, None, None, None, None, views_per_step=2, scale_term=3)
