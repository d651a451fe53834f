"""What the fused L1 + D-SSIM image loss (`loss.image_loss_and_grad`, two launches of fr_image_loss_grad) costs.

    python tools/image_loss_cost.py [--iters 200] [--rounds 5] [--steps 300] [--out profiles/r12_image_loss.json]

Kernel time: at 3 x 512^2 and 3 x 1024^2, one image and four, the time per call of (fused) the launch pair, (torch) a float32
torch restatement of 0.8 L1 + 0.2 d_ssim, forward and backward, and (l1) `fr_l1_loss_grad` alone — back-to-back calls on one
stream between two device events, the three alternated round by round in one process.  Next to it the bytes model of the pair
(pass 1 reads 2 N floats and writes 3 N, pass 2 reads 5 N and writes N: 44 N bytes) over the measured time, as a fraction of the
HBM peak.
Step rate: `RiggedStep` steps/s at 512^2 on the template's 10 006 faces and on 100 000 Gaussians, `image_loss=None` against
`REFERENCE_IMAGE_LOSS`, two step objects alternated round by round in one process.
A run without a GPU fails."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FR_TUNE_RUNTIME", "1")

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification
HBM_COPY = 6.3e12          # bytes/s, what a float4 copy achieves


def _median(v):
    return sorted(v)[len(v) // 2]


def torch_loss(x, y, window):
    """0.8 L1 + 0.2 d_ssim in float32 torch ops (the restatement of tests/image_loss_ref.py), forward and backward."""
    import torch
    import torch.nn.functional as F
    x = x.detach().requires_grad_()
    C = x.shape[0]
    conv = lambda t: F.conv2d(t[None], window, padding=5, groups=C)[0]  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s11, s22, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    S = (2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))
    loss = 0.8 * (x - y).abs().mean() + 0.2 * (1 - S.mean())
    (g,) = torch.autograd.grad(loss, x)
    return loss, g


def kernels(iters, rounds):
    import torch
    from fateavatar_amd.loss import (image_loss_and_grad_batch, image_loss_workspace, l1_loss_and_grad_batch, l1_workspace,
                                     ssim_window)
    dev = torch.device("cuda:0")
    g = ssim_window().to(dev)
    out = []
    for res in (512, 1024):
        for K in (1, 4):
            shape = (3, res, res)
            gen = torch.Generator().manual_seed(res + K)
            ys = [torch.rand(shape, generator=gen).to(dev) for _ in range(K)]
            xs = [(y + 0.02 * torch.randn(shape, generator=gen).to(dev)).contiguous() for y in ys]
            window = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
            grads, l3 = [torch.empty_like(x) for x in xs], [torch.zeros(3, device=dev) for _ in xs]
            l1s = [torch.zeros((), device=dev) for _ in xs]
            ws, ws1 = [image_loss_workspace(dev, *shape) for _ in xs], [l1_workspace(dev) for _ in xs]
            run = {"fused": lambda: image_loss_and_grad_batch(xs, ys, (0.8, 0.2), l3, grads, ws),
                   "torch": lambda: [torch_loss(x, y, window) for x, y in zip(xs, ys)],
                   "l1": lambda: l1_loss_and_grad_batch(xs, ys, l1s, grads, ws1)}
            n_it = {"fused": iters, "torch": max(10, iters // 10), "l1": iters}
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
            n = K * 3 * res * res
            fused = _median(us["fused"])
            row = dict(shape=f"{K} x 3 x {res} x {res}", calls_per_round=n_it,
                       us_per_call={k: dict(median=round(_median(v), 2), rounds=[round(t, 2) for t in v]) for k, v in us.items()},
                       torch_over_fused=round(_median(us["torch"]) / fused, 1), fused_minus_l1_us=round(fused - _median(us["l1"]), 2),
                       model_bytes=44 * n, model_GBps=round(44 * n / fused / 1e3, 1),
                       fraction_of_hbm_peak=round(44 * n / (fused * 1e-6) / HBM_PEAK, 3),
                       fraction_of_hbm_copy_rate=round(44 * n / (fused * 1e-6) / HBM_COPY, 3))
            print(json.dumps(row), file=sys.stderr)
            out.append(row)
    return out


def steps(n_steps, rounds):
    import torch
    from fateavatar_amd.rigged import REFERENCE_IMAGE_LOSS
    from tools.train_synthetic import rigged_setup
    dev = torch.device("cuda:0")
    out = []
    for P in (10_006, 100_000):
        sus = {"l1": rigged_setup(P, 512, dev, image_loss=None), "dssim": rigged_setup(P, 512, dev, image_loss=REFERENCE_IMAGE_LOSS)}

        def run(su, n, start):
            st, nf = su["st"], su["n_frames"]
            for it in range(start, start + n):
                st.step(su["cams"][it % nf], su["posed"][it % nf], su["gts"][it % nf])
        for su in sus.values():
            run(su, 20, 0)
        torch.cuda.synchronize()
        rate = {k: [] for k in sus}
        it0 = 20
        for r in range(rounds):
            for name in (("l1", "dssim") if r % 2 == 0 else ("dssim", "l1")):
                torch.cuda.synchronize()
                t = time.perf_counter()
                run(sus[name], n_steps, it0)
                torch.cuda.synchronize()
                rate[name].append(n_steps / (time.perf_counter() - t))
            it0 += n_steps
        for su in sus.values():
            su["st"].check()
            assert su["st"]._graph is not None and su["st"].overflows == 0
        m = {k: _median(v) for k, v in rate.items()}
        row = dict(P=P, res=512, steps_per_round=n_steps,
                   steps_per_s={k: dict(median=round(m[k], 1), rounds=[round(x, 1) for x in v]) for k, v in rate.items()},
                   us_per_step={k: round(1e6 / m[k], 2) for k in m}, dssim_minus_l1_us_per_step=round(1e6 / m["dssim"] - 1e6 / m["l1"], 2),
                   loss_terms=[round(float(x), 6) for x in sus["dssim"]["st"].loss_terms])
        print(json.dumps(row), file=sys.stderr)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("image_loss_cost: needs a GPU (nothing here is measured without one)")
    doc = dict(what="fused L1 + D-SSIM image loss: time per call against a float32 torch restatement and against fr_l1_loss_grad "
                    "(device events around back-to-back calls, alternated round by round), and RiggedStep steps/s with and without it",
               device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, hbm_copy_bytes_per_s=HBM_COPY,
               kernels=kernels(a.iters, a.rounds), rigged_step=steps(a.steps, a.rounds))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
