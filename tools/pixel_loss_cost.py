"""What SplattingAvatar's fused loss terms cost: `loss.pixel_loss_and_grad` (one launch of fr_pixel_loss_grad) and
`loss.scale_term_and_grad` (two launches of fr_scale_term).

    python tools/pixel_loss_cost.py [--iters 400] [--rounds 5] [--out profiles/r25_splatting_objective_kernels.json]

Image term at 3 x 512^2: the time per call of (fused) the launch, (torch) a float32 torch restatement of 1.0 L1 + 10.0 MSE,
forward and backward, (l1) `fr_l1_loss_grad` alone and (huber) `fr_huber_loss_grad` without a mask, which moves the same bytes
(two images read, one written: 12 n bytes).  Scale term at P = 10 000 and 300 000: (fused) both launches, (loss_only) the first
alone, (torch) the float32 torch restatement with its backward.  Back-to-back calls on one stream between two device events, the
variants alternated round by round in one process.  A call from Python costs the host more than these kernels cost the device, so every
fused variant is ALSO timed as twenty calls captured into one graph (time of a replay / 20: the device's time per call, what a
captured step pays); next to those the bytes model over the measured time as a fraction of the HBM peak (the scale term: 12 P
bytes read twice, one float per selected row read and written).
A run without a GPU fails."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FR_TUNE_RUNTIME", "1")

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification


def _median(v):
    return sorted(v)[len(v) // 2]


def torch_pixel(x, y):
    """1.0 L1 + 10.0 MSE in float32 torch ops, forward and backward (train/loss.py:279-283, :294-304)."""
    import torch
    x = x.detach().requires_grad_()
    loss = torch.nn.functional.l1_loss(x, y) + 10.0 * torch.nn.functional.mse_loss(x, y)
    (g,) = torch.autograd.grad(loss, x)
    return loss, g


def torch_scale(s, scale_threshold=10.0, max_scaling=0.008):
    """The scale term in float32 torch ops, forward and backward (train/loss.py:307-315; `if thresh_idxs.any()` is the
    reference's host synchronisation and stays)."""
    import torch
    s = s.detach().requires_grad_()
    scale = torch.exp(s)
    smax, _ = torch.max(scale, dim=-1)
    smin, _ = torch.min(scale, dim=-1)
    sel = (smax > max_scaling) & (smax / smin > scale_threshold)
    if not bool(sel.any()):
        return torch.zeros((), device=s.device), torch.zeros_like(s)
    loss = smax[sel].mean()
    (g,) = torch.autograd.grad(loss, s)
    return loss, g


def _alternate(run, n_it, rounds):
    """{name: [us per call, one per round]}: the variants of `run` alternated round by round, device events around each block."""
    import torch
    for f in run.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in run}
    order = list(run)
    for r in range(rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(n_it[name]):
                run[name]()
            b.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / n_it[name])
    return us


GRAPH_CALLS = 20           # launches per captured graph: a replay's time over this is the device's time per call


def _graphed(f):
    """`f` captured GRAPH_CALLS times into one graph: the replay has no host work between the launches."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(GRAPH_CALLS):
                f()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return g.replay


def _row(us):
    return {k: dict(median=round(_median(v), 2), rounds=[round(t, 2) for t in v]) for k, v in us.items()}


def pixel(iters, rounds):
    import torch
    from fateavatar_amd.loss import (HuberLoss, PixelLoss, huber_loss_and_grad, huber_workspace, l1_loss_and_grad, l1_workspace,
                                     pixel_loss_and_grad, pixel_loss_workspace)
    dev = torch.device("cuda:0")
    shape = (3, 512, 512)
    gen = torch.Generator().manual_seed(512)
    y = torch.rand(shape, generator=gen).to(dev)
    x = (y + 0.02 * torch.randn(shape, generator=gen).to(dev)).contiguous()
    grad, l3, l1 = torch.empty_like(x), torch.zeros(3, device=dev), torch.zeros((), device=dev)
    ws, ws1, wsh = pixel_loss_workspace(dev), l1_workspace(dev), huber_workspace(dev)
    run = {"fused": lambda: pixel_loss_and_grad(x, y, PixelLoss(1.0, 10.0), loss_out=l3, grad_out=grad, workspace=ws),
           "torch": lambda: torch_pixel(x, y),
           "l1": lambda: l1_loss_and_grad(x, y, loss_out=l1, grad_out=grad, workspace=ws1),
           "huber": lambda: huber_loss_and_grad(x, y, HuberLoss(0.1, 40.0), loss_out=l3, grad_out=grad, workspace=wsh)}
    n_it = {"fused": iters, "torch": max(10, iters // 10), "l1": iters, "huber": iters}
    us = _alternate(run, n_it, rounds)
    replay = {k: _graphed(run[k]) for k in ("fused", "l1", "huber")}
    us_dev = {k: [t / GRAPH_CALLS for t in v] for k, v in _alternate(replay, {k: iters for k in replay}, rounds).items()}
    n = x.numel()
    fused, dev_us = _median(us["fused"]), _median(us_dev["fused"])
    row = dict(shape="3 x 512 x 512", calls_per_round=n_it, us_per_call=_row(us), us_per_call_in_a_graph=_row(us_dev),
               torch_over_fused=round(_median(us["torch"]) / fused, 1),
               fused_minus_l1_us=round(fused - _median(us["l1"]), 2), fused_minus_huber_us=round(fused - _median(us["huber"]), 2),
               model_bytes=12 * n, model_GBps_in_a_graph=round(12 * n / dev_us / 1e3, 1),
               fraction_of_hbm_peak_in_a_graph=round(12 * n / (dev_us * 1e-6) / HBM_PEAK, 3))
    print(json.dumps(row), file=sys.stderr)
    return row


def scale(iters, rounds):
    import torch
    from fateavatar_amd.loss import ScaleTerm, scale_term_and_grad, scale_term_workspace
    dev = torch.device("cuda:0")
    out = []
    for P in (10_000, 300_000):
        gen = torch.Generator().manual_seed(P)
        s = (math.log(0.008) + (torch.rand(P, 3, generator=gen) * 6.0 - 3.0)).float().to(dev)     # about 65 % of the rows selected
        d, l2 = torch.zeros(P, 3, device=dev), torch.zeros(2, device=dev)
        ws = scale_term_workspace(dev)
        terms = ScaleTerm(1.0, 10.0, 0.008)
        run = {"fused": lambda: scale_term_and_grad(s, d, out=l2, terms=terms, workspace=ws),
               "loss_only": lambda: scale_term_and_grad(s, None, out=l2, terms=terms, workspace=ws),
               "torch": lambda: torch_scale(s)}
        n_it = {"fused": iters, "loss_only": iters, "torch": max(10, iters // 10)}
        us = _alternate(run, n_it, rounds)
        replay = {k: _graphed(run[k]) for k in ("fused", "loss_only")}
        us_dev = {k: [t / GRAPH_CALLS for t in v]
                  for k, v in _alternate(replay, {k: iters for k in replay}, rounds).items()}
        torch.cuda.synchronize()
        selected = int(l2[1])
        fused, dev_us = _median(us["fused"]), _median(us_dev["fused"])
        model = 2 * 12 * P + 8 * selected
        row = dict(P=P, selected=selected, calls_per_round=n_it, us_per_call=_row(us), us_per_call_in_a_graph=_row(us_dev),
                   torch_over_fused=round(_median(us["torch"]) / fused, 1),
                   gradient_launch_us_in_a_graph=round(dev_us - _median(us_dev["loss_only"]), 2), model_bytes=model,
                   model_GBps_in_a_graph=round(model / dev_us / 1e3, 1),
                   fraction_of_hbm_peak_in_a_graph=round(model / (dev_us * 1e-6) / HBM_PEAK, 4))
        print(json.dumps(row), file=sys.stderr)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pixel_loss_cost: needs a GPU (nothing here is measured without one)")
    doc = dict(what="SplattingAvatar's fused loss terms: time per call of fr_pixel_loss_grad and fr_scale_term against float32 torch "
                    "restatements with their backward (device events around back-to-back calls, alternated round by round)",
               device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK,
               pixel_loss=pixel(a.iters, a.rounds), scale_term=scale(a.iters, a.rounds))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
