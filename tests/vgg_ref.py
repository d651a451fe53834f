"""A torch restatement of the reference's perceptual term (VGGPerceptualLoss.forward, tools/loss_utils/vgg_feature.py:24-47),
written by hand from stock ops — F.interpolate, F.conv2d, F.relu, F.max_pool2d, F.l1_loss — and parametrised by dtype, layer
list and size; and a PINNED backward: the backward of the same network with every decision (ReLU masks, pool argmaxes, tap
signs) taken from activations that are handed in instead of being recomputed, so that a device's gradient can be checked at the
device's own decisions.  Everything runs on the CPU.

`layers`: (c_in, c_out, pool_before, tap_after) records; `weights` / `biases`: per layer a Conv2d's [c_out,c_in,3,3] / [c_out].
Activations are NCHW with the rendered image at index 0 and the target at index 1."""
import math

import torch
import torch.nn.functional as F

VGG16 = ((3, 64, False, False), (64, 64, False, True), (64, 128, True, False), (128, 128, False, True),
         (128, 256, True, False), (256, 256, False, False), (256, 256, False, True),
         (256, 512, True, False), (512, 512, False, False), (512, 512, False, True))
SMALL = ((3, 64, False, False), (64, 64, False, True), (64, 128, True, True))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def he_weights(layers, seed):
    """He-normal weights and small nonzero biases from a seed."""
    g = torch.Generator().manual_seed(seed)
    W = [torch.randn(co, ci, 3, 3, generator=g) * math.sqrt(2.0 / (9 * ci)) for ci, co, _, _ in layers]
    B = [0.1 * torch.randn(co, generator=g) for _, co, _, _ in layers]
    return W, B


def images(H, W, seed):
    """gt in [0,1] and img = clamp(gt + 0.1 noise, 0, 1), [3,H,W] float32."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    img = (gt + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return img, gt


def preprocess(x, size, dtype):
    """[B,3,H,W] -> normalised, resized [B,3,size]."""
    mean = torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    return F.interpolate((x.to(dtype) - mean) / std, mode="bilinear", size=tuple(size), align_corners=False)


def forward(W, B, layers, img, gt, size, dtype=torch.float64):
    """The forward of both images.  Returns dict(x, z, a, terms, loss): x the network's input [2,3,size], z / a every layer's
    pre-activation / post-ReLU output [2,C,h,w], terms the l1 term of every tap, loss their sum."""
    x = preprocess(torch.stack([img, gt]), size, dtype)
    h, zs, acts, terms = x, [], [], []
    for (ci, co, pool, tap), w, b in zip(layers, W, B):
        if pool:
            h = F.max_pool2d(h, kernel_size=2, stride=2)
        z = F.conv2d(h, w.to(dtype), b.to(dtype), padding=1)
        h = F.relu(z)
        zs.append(z)
        acts.append(h)
        if tap:
            terms.append(F.l1_loss(h[0:1], h[1:2]))
    return dict(x=x, z=zs, a=acts, terms=terms, loss=sum(terms))


def autograd_gradient(W, B, layers, img, gt, size, dtype=torch.float64):
    """(loss, dLoss/dimg [3,H,W]) through torch's autograd, all in `dtype`."""
    leaf = img.to(dtype).clone().requires_grad_(True)
    r = forward(W, B, layers, leaf, gt.to(dtype), size, dtype)
    (g,) = torch.autograd.grad(r["loss"], leaf)
    return r["loss"].detach(), g


def _window_one_hot(a):
    """[C,h,w] -> bool [C,h,w]: the FIRST maximum of every 2 x 2 window in row-major order (torch's max_pool2d rule)."""
    C, h, w = a.shape
    win = a.view(C, h // 2, 2, w // 2, 2).permute(0, 1, 3, 2, 4).reshape(C, h // 2, w // 2, 4)
    first = torch.zeros_like(win, dtype=torch.bool)
    best = win[..., 0].clone()
    idx = torch.zeros(win.shape[:-1], dtype=torch.long)
    for k in range(1, 4):
        better = win[..., k] > best
        idx[better] = k
        best = torch.where(better, win[..., k], best)
    first.scatter_(-1, idx.unsqueeze(-1), True)
    return first.view(C, h // 2, w // 2, 2, 2).permute(0, 1, 3, 2, 4).reshape(C, h, w)


def pinned_backward(W, layers, acts, image_hw, size, dtype=torch.float64):
    """dLoss/dimg [3,H,W] in `dtype` with every decision read from `acts` (per layer [2,C,h,w]: the rendered image's and the
    target's post-ReLU outputs, e.g. a device's saved activations): the ReLU mask [a > 0], the tap sign sign(a - a_gt) and the
    pool's argmax (first maximum of a's window).  What is left is linear: transposed convolutions, the routing, the resize."""
    L = len(layers)
    g = None        # dLoss/d(a_l) of the rendered image, [C,h,w]
    for l in range(L - 1, -1, -1):
        ci, co, pool, tap = layers[l]
        a, a_gt = acts[l][0].to(dtype), acts[l][1].to(dtype)
        if tap:
            t = torch.sign(a - a_gt) / a.numel()
            g = t if g is None else g + t
        dz = g * (a > 0).to(dtype)
        d_in = F.conv_transpose2d(dz[None], W[l].to(dtype), padding=1)[0]
        if pool:
            prev = acts[l - 1][0].to(dtype)
            d_in = d_in.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * _window_one_hot(prev).to(dtype)
        g = d_in
    # the resize and the normalisation are linear: their transpose through autograd on a dummy leaf
    leaf = torch.zeros(1, 3, *image_hw, dtype=dtype, requires_grad=True)
    (d_img,) = torch.autograd.grad(preprocess(leaf, size, dtype), leaf, g[None])
    return d_img[0]


def decisions_clear(r, layers, margin):
    """Whether the forward `r` (of `forward`) keeps every decision the gradient depends on at least `margin` x its layer's RMS
    pre-activation away from its threshold: a ReLU pre-activation of the rendered image from 0, a tap difference (where either
    side is live) from 0, the top two of a live pool window (of the rendered image) from each other."""
    for l, (ci, co, pool, tap) in enumerate(layers):
        z, a = r["z"][l], r["a"][l]
        tol = margin * float(z.pow(2).mean().sqrt())
        if float(z[0].abs().min()) < tol:
            return False
        if tap:
            live = (a[0] > 0) | (a[1] > 0)
            if bool(live.any()) and float((a[0] - a[1]).abs()[live].min()) < tol:
                return False
        if l + 1 < len(layers) and layers[l + 1][2]:
            C, h, w = a[0].shape
            win = a[0].view(C, h // 2, 2, w // 2, 2).permute(0, 1, 3, 2, 4).reshape(C, h // 2, w // 2, 4)
            top = win.topk(2, dim=-1).values
            live = top[..., 0] > 0
            if bool(live.any()) and float((top[..., 0] - top[..., 1])[live].min()) < tol:
                return False
    return True


def nchw(saved):
    """A device's saved activation [2,h,w,C] (NHWC) as a CPU [2,C,h,w] tensor."""
    return saved.detach().cpu().permute(0, 3, 1, 2).contiguous()
