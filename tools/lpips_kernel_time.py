"""What the fused LPIPS term costs: `Lpips.loss_and_grad` (fr_lpips_loss_grad, csrc/fr_vgg.hip) on the 13-layer trunk, no resize.

    python tools/lpips_kernel_time.py [--res 512] [--iters 10] [--rounds 3] [--torch] [--vgg-l1] [--out profiles/r30_lpips_kernels.json]

Times, per call, between two device events around `iters` back-to-back calls on one stream, the variants alternated round by
round in one process (tools/vgg_kernel_time.py's scheme):
  forward      the two forwards and the five terms (grad_out=False: the metric)
  step         forward + the tap seeds + the data gradient of the rendered branch (what a training step pays)
  gradient     step - forward
--torch    the same weights through F.conv2d / F.max_pool2d, the unit normalisation from stock ops, and autograd on the device
           (the `lpips` package's route: vendor-library convolutions), forward alone and forward + backward.
--vgg-l1   the L1 perceptual term (fr_vgg_loss_grad) over the SAME 13 layers and taps: what the LPIPS tap and seed kernels add.
Seeded He-normal weights and uniform `lin` (the cost does not depend on the values).  A run without a GPU fails."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("FR_TUNE_RUNTIME", "1")

from vgg_kernel_time import F32_PEAK, _alternate, _median, macs  # noqa: E402


def torch_lpips(weights, biases, lin, layers, mean, std, eps=1e-10):
    """LPIPS through stock torch ops on the same weights: f(img, gt, backward) -> (loss, gradient of img or None)."""
    import torch
    import torch.nn.functional as F
    m = torch.tensor(mean, device=weights[0].device).view(1, 3, 1, 1)
    s = torch.tensor(std, device=weights[0].device).view(1, 3, 1, 1)
    lin = [w.view(1, -1, 1, 1) for w in lin]

    def run(img, gt, backward):
        x = img.detach().requires_grad_(backward)
        h = (torch.stack([x, gt]) - m) / s
        loss, k = 0.0, 0
        for y, w, b in zip(layers, weights, biases):
            if y.pool_before:
                h = F.max_pool2d(h, 2, 2)
            h = F.relu(F.conv2d(h, w, b, padding=1))
            if y.tap_after:
                u = h / (h.pow(2).sum(1, keepdim=True).sqrt() + eps)
                loss = loss + (lin[k] * (u[0:1] - u[1:2].detach()).pow(2)).sum(1).mean()
                k += 1
        if backward:
            (g,) = torch.autograd.grad(loss, x)
            return loss, g
        return loss, None
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--vgg-l1", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import fateavatar_amd
    from fateavatar_amd.perceptual import Lpips, Perceptual
    if not torch.cuda.is_available():
        raise SystemExit("lpips_kernel_time: needs a HIP device")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    size = (a.res, a.res)
    feats = Lpips.trunk(size, device=dev)
    gt = torch.rand(3, a.res, a.res, device=dev)
    img = (gt + 0.1 * torch.randn_like(gt)).clamp(0, 1)

    def fused(p):
        loss = torch.zeros(1 + p.n_terms, device=dev)
        grad = torch.zeros_like(img)
        return (lambda: p.loss_and_grad(img, gt, loss_out=loss, grad_out=False)), (lambda: p.loss_and_grad(img, gt, loss_out=loss, grad_out=grad))

    lp = Lpips(feats)
    run = {}
    run["forward"], run["step"] = fused(lp)
    if a.vgg_l1:
        run["vgg_l1_forward"], run["vgg_l1_step"] = fused(Perceptual(feats))
    if a.torch:
        t = torch_lpips(feats.weights, feats.biases, lp.lin, feats.layers, feats.mean, feats.std)
        run["torch_forward"] = lambda: t(img, gt, False)
        run["torch_step"] = lambda: t(img, gt, True)
    us = _alternate(run, a.iters, a.rounds)
    med = {k: _median(v) for k, v in us.items()}
    fwd, bwd = macs(feats.layers, size)
    flop_f, flop_b = 2 * 2 * sum(fwd), 2 * sum(bwd)
    res = {"config": {"res": a.res, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
                      "hip_env": fateavatar_amd.runtime_env(), "gflop_forward": flop_f / 1e9, "gflop_gradient": flop_b / 1e9,
                      "workspace_bytes": int(lp._workspace.numel())},
           "us_rounds": us, "us": med, "tflops": {}}

    def rate(flop, t_us):
        return flop / (t_us * 1e-6) / 1e12

    for prefix in ["", "vgg_l1_", "torch_"]:
        if prefix + "step" not in med:
            continue
        f, s = med[prefix + "forward"], med[prefix + "step"]
        g = s - f
        res["tflops"][prefix or "fused_"] = {"forward": rate(flop_f, f), "gradient": rate(flop_b, g), "step": rate(flop_f + flop_b, s)}
        print(f"{prefix or 'fused_'}: forward {f:9.1f} us ({rate(flop_f, f):5.1f} TF/s, {100 * rate(flop_f, f) * 1e12 / F32_PEAK:4.1f} % of peak)  "
              f"gradient {g:9.1f} us ({rate(flop_b, g):5.1f} TF/s)  step {s:9.1f} us  rounds {['%.0f' % v for v in us[prefix + 'step']]}")
    print(json.dumps({"lpips_kernel_time": res["us"]}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
