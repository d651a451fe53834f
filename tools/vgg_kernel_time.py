"""What the fused perceptual term costs: `Perceptual.loss_and_grad` (fr_vgg_loss_grad, csrc/fr_vgg.hip) on VGG-16's stack.

    python tools/vgg_kernel_time.py [--res 512] [--size 224] [--iters 20] [--rounds 3] [--torch] [--tiles] [--layers]
                                    [--out profiles/r29_vgg_perceptual_kernels.json]

Times, per call, between two device events around `iters` back-to-back calls on one stream, the variants alternated round by
round in one process:
  forward      the two forwards and the terms (grad_out=False)
  step         forward + the data gradient of the rendered branch (what a training step pays)
  gradient     step - forward
and the rate against the f32 peak: forward = 2 images x the stack's multiply-adds x 2 FLOP, the gradient one image's (layer 0
has no data gradient worth counting: its input is the image).
--torch   the same weights through F.interpolate / F.conv2d / F.max_pool2d / F.l1_loss and autograd on the device (the
          reference's route: vendor-library convolutions), forward alone and forward + backward.
--tiles   the fused variants with the GEMM tile forced to 64 x 64 and to 128 x 64 (FR_VGG_TILE_*), next to the per-layer choice.
--layers  the per-layer split: the stack truncated behind every layer (its last layer made a tap), each prefix timed like the
          whole; a layer's cost is the difference of two prefixes (so it includes the pool in front of it, and the tap's
          reduction moves with the cut: read the differences as what a layer adds, to a few microseconds).
Seeded He-normal weights (pretrained ones are the caller's to supply; the cost does not depend on the values).
A run without a GPU fails."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FR_TUNE_RUNTIME", "1")

F32_PEAK = 157.3e12        # FLOP/s, MI355X f32 matrix / vector peak


def _median(v):
    return sorted(v)[len(v) // 2]


def macs(layers, size):
    """Multiply-adds of ONE image's forward per layer, and of its data gradient (0 for layer 0)."""
    h, w = size
    fwd, bwd = [], []
    for i, y in enumerate(layers):
        if y.pool_before:
            h, w = h // 2, w // 2
        n = 9 * y.c_in * y.c_out * h * w
        fwd.append(n)
        bwd.append(n if i > 0 else 0)
    return fwd, bwd


def torch_route(weights, biases, layers, size, mean, std):
    """The reference's route on the same weights: returns f(img, gt, backward) -> loss (and the gradient of img)."""
    import torch
    import torch.nn.functional as F
    m = torch.tensor(mean, device=weights[0].device).view(1, 3, 1, 1)
    s = torch.tensor(std, device=weights[0].device).view(1, 3, 1, 1)

    def run(img, gt, backward):
        x = img.detach().requires_grad_(backward)
        h = F.interpolate((torch.stack([x, gt]) - m) / s, mode="bilinear", size=size, align_corners=False)
        loss = 0.0
        for y, w, b in zip(layers, weights, biases):
            if y.pool_before:
                h = F.max_pool2d(h, 2, 2)
            h = F.relu(F.conv2d(h, w, b, padding=1))
            if y.tap_after:
                loss = loss + F.l1_loss(h[0:1], h[1:2].detach())
        if backward:
            (g,) = torch.autograd.grad(loss, x)
            return loss, g
        return loss, None
    return run


def _alternate(run, iters, rounds):
    import torch
    for f in run.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in run}
    order = list(run)
    for r in range(rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(iters):
                run[name]()
            b.record()
            torch.cuda.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / iters)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--tiles", action="store_true")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import fateavatar_amd
    from fateavatar_amd import _lib
    from fateavatar_amd.perceptual import VGG16_LAYERS, ConvLayer, Perceptual, VggFeatures
    if not torch.cuda.is_available():
        raise SystemExit("vgg_kernel_time: needs a HIP device")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    size = (a.size, a.size)
    feats = VggFeatures.vgg16(size=size, device=dev)
    gt = torch.rand(3, a.res, a.res, device=dev)
    img = (gt + 0.1 * torch.randn_like(gt)).clamp(0, 1)

    def fused(features, tile=_lib.FR_VGG_TILE_AUTO):
        p = Perceptual(features)
        p.tile = tile
        loss = torch.zeros(1 + p.n_terms, device=dev)
        grad = torch.zeros_like(img)
        return (lambda: p.loss_and_grad(img, gt, loss_out=loss, grad_out=False)), (lambda: p.loss_and_grad(img, gt, loss_out=loss, grad_out=grad))

    run = {}
    run["forward"], run["step"] = fused(feats)
    if a.tiles:
        run["forward_tile64"], run["step_tile64"] = fused(feats, _lib.FR_VGG_TILE_64)
        run["forward_tile128"], run["step_tile128"] = fused(feats, _lib.FR_VGG_TILE_128)
    if a.torch:
        t = torch_route(feats.weights, feats.biases, feats.layers, size, feats.mean, feats.std)
        run["torch_forward"] = lambda: t(img, gt, False)
        run["torch_step"] = lambda: t(img, gt, True)
    if a.layers:
        for k in range(1, len(VGG16_LAYERS)):
            cut = [ConvLayer(*y) for y in VGG16_LAYERS[:k]]
            cut[-1] = cut[-1]._replace(tap_after=True)
            f = VggFeatures(cut, feats.weights[:k], feats.biases[:k], size=size, device=dev)
            run[f"forward_upto{k - 1}"], run[f"step_upto{k - 1}"] = fused(f)
    us = _alternate(run, a.iters, a.rounds)
    med = {k: _median(v) for k, v in us.items()}
    fwd, bwd = macs(feats.layers, size)
    flop_f, flop_b = 2 * 2 * sum(fwd), 2 * sum(bwd)
    res = {"config": {"res": a.res, "size": a.size, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
                      "hip_env": fateavatar_amd.runtime_env(), "gflop_forward": flop_f / 1e9, "gflop_gradient": flop_b / 1e9},
           "us_rounds": us, "us": med}

    def rate(flop, t_us):
        return flop / (t_us * 1e-6) / 1e12

    def show(prefix, label):
        f, s = med[prefix + "forward" + label], med[prefix + "step" + label]
        g = s - f
        res.setdefault("tflops", {})[prefix + label] = {"forward": rate(flop_f, f), "gradient": rate(flop_b, g), "step": rate(flop_f + flop_b, s)}
        print(f"{prefix or 'fused_'}{label or ''}: forward {f:9.1f} us ({rate(flop_f, f):5.1f} TF/s, {100 * rate(flop_f, f) * 1e12 / F32_PEAK:4.1f} % of peak)  "
              f"gradient {g:9.1f} us ({rate(flop_b, g):5.1f} TF/s)  step {s:9.1f} us  rounds {['%.0f' % v for v in us[prefix + 'step' + label]]}")

    show("", "")
    if a.tiles:
        show("", "_tile64")
        show("", "_tile128")
    if a.torch:
        show("torch_", "")
    if a.layers:
        prev_f = prev_s = 0.0
        rows = []
        for k in range(len(VGG16_LAYERS)):
            last = k == len(VGG16_LAYERS) - 1
            f = med["forward"] if last else med[f"forward_upto{k}"]
            s = med["step"] if last else med[f"step_upto{k}"]
            df, dg = f - prev_f, (s - f) - (prev_s - prev_f)
            y = VGG16_LAYERS[k]
            rows.append({"layer": k, "c_in": y.c_in, "c_out": y.c_out, "forward_us": df, "gradient_us": dg,
                         "forward_tflops": rate(2 * 2 * fwd[k], df) if df > 0 else None,
                         "gradient_tflops": rate(2 * bwd[k], dg) if dg > 0 and bwd[k] else None})
            print(f"layer {k} ({y.c_in:3d} -> {y.c_out:3d}{', pooled' if y.pool_before else ''}): forward +{df:8.1f} us "
                  f"({rows[-1]['forward_tflops'] or 0:5.1f} TF/s)  gradient +{dg:8.1f} us ({rows[-1]['gradient_tflops'] or 0:5.1f} TF/s)")
            prev_f, prev_s = f, s
        res["layers"] = rows
    print(json.dumps({"vgg_kernel_time": res["us"]}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
