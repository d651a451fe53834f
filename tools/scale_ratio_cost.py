"""What FateAvatar's scale-ratio term costs: `loss.scale_ratio_term_and_grad` (one launch of fr_scale_ratio_term).

    python tools/scale_ratio_cost.py [--iters 400] [--rounds 5] [--out profiles/r31_fate_scale_term_kernel.json]

At P = 100 000 and 65 536 rows, about half of them over the threshold (tests/fate_scale_ref.draw_scaling: needs the checkout's
tests/ next to tools/): the time per call of (fused) the launch with its gradient, (loss_only) without, (torch) a float32 torch
restatement of the three lines of train/loss.py:147-149 with its backward.  Measured as tools/pixel_loss_cost.py measures the
sibling terms — back-to-back calls on one stream between two device events, the variants alternated round by round, and the
fused variants also as twenty calls captured into one graph (a replay's time / 20: what a captured step pays) — with that file's
helpers.  The bytes model: 12 P bytes read, two floats read and written per row over the threshold.
A run without a GPU fails."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
os.environ.setdefault("FR_TUNE_RUNTIME", "1")

from pixel_loss_cost import GRAPH_CALLS, HBM_PEAK, _alternate, _graphed, _median, _row  # noqa: E402


def torch_scale_ratio(s, scale_threshold=9.0):
    """The term in float32 torch ops, forward and backward (train/loss.py:147-149)."""
    import torch
    s = s.detach().requires_grad_()
    scale = torch.exp(s)
    smax, _ = torch.max(scale, dim=-1)
    smin, _ = torch.min(scale, dim=-1)
    loss = torch.nn.functional.relu(smax / smin - scale_threshold).mean()
    (g,) = torch.autograd.grad(0.1 * loss, s)
    return loss, g


def measure(iters, rounds):
    import torch
    from fateavatar_amd.loss import ScaleRatioTerm, scale_ratio_term_and_grad, scale_ratio_workspace
    from tests.fate_scale_ref import draw_scaling
    dev = torch.device("cuda:0")
    out = []
    for P in (100_000, 65_536):
        s = draw_scaling(P, torch.Generator().manual_seed(P), 9.0, over=0.5).to(dev)
        d, l2 = torch.zeros(P, 3, device=dev), torch.zeros(2, device=dev)
        ws = scale_ratio_workspace(dev)
        terms = ScaleRatioTerm(0.1, 9.0)
        run = {"fused": lambda: scale_ratio_term_and_grad(s, d, out=l2, terms=terms, workspace=ws),
               "loss_only": lambda: scale_ratio_term_and_grad(s, None, out=l2, terms=terms, workspace=ws),
               "torch": lambda: torch_scale_ratio(s)}
        n_it = {"fused": iters, "loss_only": iters, "torch": max(10, iters // 10)}
        us = _alternate(run, n_it, rounds)
        replay = {k: _graphed(run[k]) for k in ("fused", "loss_only")}
        us_dev = {k: [t / GRAPH_CALLS for t in v] for k, v in _alternate(replay, {k: iters for k in replay}, rounds).items()}
        torch.cuda.synchronize()
        over = int(l2[1])
        fused, dev_us = _median(us["fused"]), _median(us_dev["fused"])
        model = 12 * P + 16 * over
        row = dict(P=P, rows_over_threshold=over, calls_per_round=n_it, us_per_call=_row(us), us_per_call_in_a_graph=_row(us_dev),
                   torch_over_fused=round(_median(us["torch"]) / fused, 1),
                   torch_over_fused_in_a_graph=round(_median(us["torch"]) / dev_us, 1), model_bytes=model,
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
        raise SystemExit("scale_ratio_cost: needs a GPU (nothing here is measured without one)")
    doc = dict(what="FateAvatar's scale-ratio term: time per call of fr_scale_ratio_term against a float32 torch restatement with its "
                    "backward (device events around back-to-back calls, alternated round by round)",
               device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, scale_ratio_term=measure(a.iters, a.rounds))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
