"""TEST HELPER — FateAvatar's scale-ratio term restated in torch (FateAvatarLoss.accumulate_gradients, train/loss.py:144-151,
on model_outputs['scale'] = exp(_scaling), model/fateavatar.py:282), its gradient by autograd, and the draw of log-scales that
keep clear of the threshold and of ties.  Pinned to the recorded run of the reference's own method by
tests/test_fate_scale_host.py."""
import math

import torch

LOG_LO, LOG_HI = math.log(6e-4), math.log(1e-2)     # the span of the reference's starting scales (its knn estimate)


def scale_loss(scaling, scale_threshold):
    """The three lines: relu(scale.max(-1) / scale.min(-1) - scale_threshold).mean() with scale = exp(scaling)."""
    scale = torch.exp(scaling)
    ratio = scale.max(dim=-1).values / scale.min(dim=-1).values
    return torch.relu(ratio - scale_threshold).mean()


def loss_count_grad(scaling, weight, scale_threshold, dtype=torch.float64):
    """(scale_loss, rows over the threshold, weight x d scale_loss / d scaling) of `scaling` [P,3] computed in `dtype`."""
    s = scaling.detach().to(dtype).clone().requires_grad_(True)
    loss = scale_loss(s, scale_threshold)
    (g,) = torch.autograd.grad(weight * loss, s)
    scale = torch.exp(s.detach())
    count = int((scale.max(-1).values / scale.min(-1).values > scale_threshold).sum())
    return loss.detach(), count, g


def draw_scaling(P, gen, scale_threshold, over=0.5):
    """[P,3] float32 log-scales: the smallest component of a row uniform in [LOG_LO, LOG_HI], the largest above it by a
    log-ratio that puts about `over` of the rows past the threshold — under: [0.05, log thr - 0.05], over: [log thr + 0.05,
    log thr + 1.5] —, the third between them at 10 % .. 90 % of the way, the three in a random order."""
    lt = math.log(scale_threshold)
    base = LOG_LO + (LOG_HI - LOG_LO) * torch.rand(P, generator=gen, dtype=torch.float64)
    u, m = torch.rand(P, generator=gen, dtype=torch.float64), 0.1 + 0.8 * torch.rand(P, generator=gen, dtype=torch.float64)
    is_over = torch.rand(P, generator=gen) < over
    r = torch.where(is_over, lt + 0.05 + 1.45 * u, 0.05 + (lt - 0.1) * u)
    rows = torch.stack([base, base + m * r, base + r], dim=1)
    order = torch.argsort(torch.rand(P, 3, generator=gen), dim=1)
    return torch.gather(rows, 1, order).float()


def margins(scaling, scale_threshold):
    """(min over the rows of |ratio / threshold - 1|, min over the rows over the threshold of the relative gap between the two
    largest and between the two smallest activated components — inf without such a row), of the float32 inputs in float64."""
    scale = torch.exp(scaling.double())
    srt = scale.sort(dim=-1).values
    ratio = srt[:, 2] / srt[:, 0]
    gate = float((ratio / scale_threshold - 1).abs().min())
    sel = ratio > scale_threshold
    if not bool(sel.any()):
        return gate, math.inf
    tie = torch.minimum(srt[sel, 2] / srt[sel, 1] - 1, srt[sel, 1] / srt[sel, 0] - 1)
    return gate, float(tie.min())
