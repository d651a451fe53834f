"""SplattingAvatar's closed-form loss terms in stock PyTorch with autograd: the reference of tests/test_gpu_splatting_loss.py, pinned
on hand-computed cases by tests/test_splatting_loss_host.py.

reference: `SplattingAvatarLoss` (train/loss.py:259-323) — `get_rgb_loss` / `get_mse_loss` (:279-283: nn.L1Loss and nn.MSELoss,
reduction 'mean') and the scale term of `accumulate_gradients` (:307-315) on `model_outputs['scale']` = exp(_scaling)
(model/baseline/splattingavatar.py:270), with the weights and gates of config/splattingavatar.yaml:13-20.  A restatement, written
anew — and pinned to the class itself: `SplattingAvatarLoss.accumulate_gradients` (made without its constructor, which builds
lpips.LPIPS) was run on recorded inputs, and tests/test_reference_runs_host.py holds `pixel_terms`, `scale_term` and `REFERENCE`
to its float64 results and `Params` (tests/golden/reference_image_terms.npz, case `splat`)."""
import math

import torch

REFERENCE = dict(rgb_weight=1.0, mse_weight=10.0, scale_weight=1.0, scale_threshold=10.0, max_scaling=0.008)


def pixel_terms(img, gt, rgb_weight, mse_weight, dtype=torch.float64):
    """((rgb_weight * l1 + mse_weight * mse, l1, mse) as a 3-element tensor, d of its first word / d img) in `dtype`."""
    x = img.detach().to(dtype).requires_grad_(True)
    y = gt.detach().to(dtype)
    l1 = torch.nn.L1Loss(reduction="mean")(x, y)       # :279-280
    mse = torch.nn.MSELoss(reduction="mean")(x, y)     # :282-283
    total = l1 * rgb_weight + mse * mse_weight         # :294-304
    (g,) = torch.autograd.grad(total, x)
    return torch.stack([total, l1, mse]).detach(), g


def scale_term(scaling, weight, scale_threshold, max_scaling, dtype=torch.float64):
    """(scale_loss UNWEIGHTED, number of selected rows, weight * d scale_loss / d _scaling [P,3], the selection [P] bool) of the
    raw `scaling` [P,3], in `dtype`."""
    s = scaling.detach().to(dtype).requires_grad_(True)
    scale = torch.exp(s)                               # splattingavatar.py:270
    scale_max, _ = torch.max(scale, dim=-1)            # :309
    scale_min, _ = torch.min(scale, dim=-1)            # :310
    ratio = scale_max / scale_min                      # :311
    sel = (scale_max > max_scaling) & (ratio > scale_threshold)   # :312
    if bool(sel.any()):                                # :313
        loss = scale_max[sel].mean()
        (g,) = torch.autograd.grad(loss * weight, s)
    else:
        loss, g = torch.zeros((), dtype=dtype), torch.zeros_like(s)
    return loss.detach(), int(sel.sum()), g.detach(), sel


def undecided_rows(scaling, scale_threshold, max_scaling):
    """[P] bool: rows a float32 evaluation may decide differently from float64 — smax / max_scaling or ratio / scale_threshold
    within 1e-4 of 1 (the selection), or the two largest components within 1e-6 relative of each other (the argmax)."""
    scale = torch.exp(scaling.double())
    top = torch.sort(scale, dim=-1, descending=True).values
    smax, smin = top[:, 0], top[:, 2]
    near = lambda v: (v - 1.0).abs() <= 1e-4  # noqa: E731
    return near(smax / max_scaling) | near(smax / smin / scale_threshold) | ((top[:, 0] - top[:, 1]) <= 1e-6 * top[:, 0])


def draw_scaling(P, generator, scale_threshold=REFERENCE["scale_threshold"], max_scaling=REFERENCE["max_scaling"]):
    """[P,3] float32 raw scales: log(max_scaling) + U(-3, 3) per component — about 65 % of the rows are selected — with every
    row of `undecided_rows` drawn again until none is left: THE redraw rule of the device tests, no row is left out of a
    comparison."""
    draw = lambda n: (math.log(max_scaling) + (torch.rand(n, 3, generator=generator) * 6.0 - 3.0)).float()  # noqa: E731
    s = draw(P)
    for _ in range(64):
        bad = undecided_rows(s, scale_threshold, max_scaling)
        if not bool(bad.any()):
            return s
        s[bad] = draw(int(bad.sum()))
    raise RuntimeError("draw_scaling: rows stayed undecided")
