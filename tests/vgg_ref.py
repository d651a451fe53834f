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
# no pool, 512 wide: at sizes around 32 x 32 its GEMMs take every plan of the split over the taps (1, 3 and 9 planes)
WIDE = ((3, 64, False, False), (64, 512, False, True), (512, 512, False, False), (512, 512, False, True))
# VGG16's flags with every width 64: the stack the recorded run of the reference's own module uses (tests/golden/make_reference_runs.py)
NARROW = tuple((3 if i == 0 else 64, 64, pool, tap) for i, (_, _, pool, tap) in enumerate(VGG16))
# widths whose c_out / 64 is odd: three, five and seven 64-column GEMM tiles, and as many values per lane in the LPIPS tap kernel
ODD = ((3, 64, False, False), (64, 192, False, True), (192, 320, True, True), (320, 448, False, True))
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


def patchwork(H, W, seed):
    """`images` with three quadrants overwritten by what real frames have and noise has not — flat regions: top-left both images
    1.0 (the background the target shares), top-right two different constant colours, bottom-left the rendered image constant
    over a noisy target.  Inside a flat region every unit of a layer sees the same numbers, so rendered and target are EQUAL where
    both are flat and alike (tap differences of exactly 0 on live units) and every pool window is a four-way tie.  Only for
    resizes that keep a flat region bit-flat: the identity and an exact halving (0.5 v + 0.5 v)."""
    img, gt = images(H, W, seed)
    h, w = H // 2, W // 2
    img[:, :h, :w], gt[:, :h, :w] = 1.0, 1.0
    img[:, :h, w:], gt[:, :h, w:] = torch.tensor([0.8, 0.6, 0.4]).view(3, 1, 1), torch.tensor([0.7, 0.65, 0.3]).view(3, 1, 1)
    img[:, h:, :w] = 0.5
    return img, gt


def preprocess(x, size, dtype):
    """[B,3,H,W] -> normalised, resized [B,3,size].  The statistics are float32 numbers in every dtype: the reference keeps them
    in float32 buffers that take the image's dtype afterwards (and the kernel takes them as float)."""
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
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


def _windows(a):
    """[C,h,w] -> [C,h/2,w/2,4]: every 2 x 2 window's values in row-major order."""
    C, h, w = a.shape
    return a.reshape(C, h // 2, 2, w // 2, 2).permute(0, 1, 3, 2, 4).reshape(C, h // 2, w // 2, 4)


def _window_one_hot(a, last=False):
    """[C,h,w] -> bool [C,h,w]: the FIRST maximum of every 2 x 2 window in row-major order (torch's max_pool2d rule).  `last`:
    the LAST maximum instead — the wrong rule, for tests that show their inputs tell the two apart."""
    C, h, w = a.shape
    win = _windows(a)
    first = torch.zeros_like(win, dtype=torch.bool)
    best = win[..., 0].clone()
    idx = torch.zeros(win.shape[:-1], dtype=torch.long)
    for k in range(1, 4):
        better = (win[..., k] >= best) if last else (win[..., k] > best)
        idx[better] = k
        best = torch.where(better, win[..., k], best)
    first.scatter_(-1, idx.unsqueeze(-1), True)
    return first.view(C, h // 2, w // 2, 2, 2).permute(0, 1, 3, 2, 4).reshape(C, h, w)


def sign_plus_at_zero(d):
    """The wrong tap sign: +1 at a difference of 0 (torch.sign, and the l1 term's gradient, give 0 there)."""
    return torch.where(d >= 0, torch.ones_like(d), -torch.ones_like(d))


def pinned_backward(W, layers, acts, image_hw, size, dtype=torch.float64, one_hot=_window_one_hot, sign=torch.sign):
    """dLoss/dimg [3,H,W] in `dtype` with every decision read from `acts` (per layer [2,C,h,w]: the rendered image's and the
    target's post-ReLU outputs, e.g. a device's saved activations): the ReLU mask [a > 0], the tap sign sign(a - a_gt) and the
    pool's argmax (first maximum of a's window).  What is left is linear: transposed convolutions, the routing, the resize.
    `one_hot` / `sign`: the two rules at a tie, replaceable by their opposites to show that an input tells them apart."""
    L = len(layers)
    g = None        # dLoss/d(a_l) of the rendered image, [C,h,w]
    for l in range(L - 1, -1, -1):
        ci, co, pool, tap = layers[l]
        a, a_gt = acts[l][0].to(dtype), acts[l][1].to(dtype)
        if tap:
            t = sign(a - a_gt) / a.numel()
            g = t if g is None else g + t
        dz = g * (a > 0).to(dtype)
        d_in = F.conv_transpose2d(dz[None], W[l].to(dtype), padding=1)[0]
        if pool:
            prev = acts[l - 1][0].to(dtype)
            d_in = d_in.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * one_hot(prev).to(dtype)
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


def live_ties(acts, layers):
    """(live tied pool windows, live zero tap differences) of `acts` (per layer [2,C,h,w], as `forward` returns and a device
    saves): windows of the rendered image that a pool reads whose top two values are equal and above 0, and units of a tapped
    layer whose rendered value is above 0 and equal to the target's.  At these the gradient is decided by a rule, not by a number:
    the first maximum takes the window's gradient, and sign(0) = 0."""
    ties = zeros = 0
    for l, (ci, co, pool, tap) in enumerate(layers):
        a = acts[l]
        if tap:
            zeros += int(((a[0] > 0) & (a[0] == a[1])).sum())
        if l + 1 < len(layers) and layers[l + 1][2]:
            top = _windows(a[0]).topk(2, dim=-1).values
            ties += int(((top[..., 0] > 0) & (top[..., 0] == top[..., 1])).sum())
    return ties, zeros


def receptive_margin(layers):
    """How many pixels of the network's input the receptive field of a unit of the deepest layer spans beyond its first: a unit
    at stride s covers [i s - lo, i s + hi]; a 3 x 3 convolution adds s on either side, a 2 x 2 / 2 pool in front of it adds s
    on the far side and doubles s.  A pixel whose distance to the far edge of a region is MORE than lo + hi lies only in
    receptive fields that are inside the region."""
    s, lo, hi = 1, 0, 0
    for ci, co, pool, tap in layers:
        if pool:
            hi, s = hi + s, 2 * s
        lo, hi = lo + s, hi + s
    return lo + hi


def nchw(saved):
    """A device's saved activation [2,h,w,C] (NHWC) as a CPU [2,C,h,w] tensor."""
    return saved.detach().cpu().permute(0, 3, 1, 2).contiguous()
