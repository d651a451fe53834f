"""A torch restatement of the LPIPS term as include/fr_rasterizer.h defines it (lpips.LPIPS(net='vgg'), normalize=True: unit-
normalised VGG taps, learnt per-channel weights, the spatial mean, the sum over the taps), from stock ops and parametrised by
dtype, layer list and size; the tap's closed-form gradient seed; and a PINNED backward as tests/vgg_ref.py has one — ReLU masks
and pool argmaxes read from handed-in activations, the tap seed by the closed form at those activations.  Everything on the CPU.

The dead-pixel rule is part of the restatement: a pixel whose feature vector is all zero has the unit vector 0, contributes
sum_c w_c b^_c^2, and takes a gradient of exactly 0 (stock autograd: NaN).  `tap_term` is written so that autograd through it
obeys the rule too (the square root never sees a 0); `tap_term_stock` is the formula as the `lpips` package writes it.

Weights, images, `nchw` and the pool's one-hot come from tests/vgg_ref.py."""
import torch
import torch.nn.functional as F

from tests import vgg_ref

EPS = 1e-10
# vgg16.features[:30]: vgg_ref.VGG16 and block 5, taps at relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
LPIPS13 = vgg_ref.VGG16 + ((512, 512, True, False), (512, 512, False, False), (512, 512, False, True))
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)


def lin_weights(layers, seed, signed=False):
    """Per tap a [c_out] vector: uniform in [0, 2 / c_out) (LPIPS's learnt weights are non-negative), or, `signed`, normal / c_out."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(co, generator=g) if signed else 2.0 * torch.rand(co, generator=g)) / co for _, co, _, tap in layers if tap]


def _unit(a, dtype):
    """(a^, r, n, live) of a [C,h,w] feature: n = |a| per pixel (1 where dead, so that nothing divides by or roots a 0),
    r = 1 / (n + eps) or 0 where dead, a^ = a r."""
    s = a.pow(2).sum(0)
    live = s > 0
    n = torch.where(live, s, torch.ones_like(s)).sqrt()
    r = torch.where(live, 1.0 / (n + torch.tensor(EPS, dtype=dtype)), torch.zeros_like(n))
    return a * r, r, n, live


def tap_term(a, b, w, dtype=torch.float64):
    """(1 / (h w)) sum_p sum_c w_c (a^_c - b^_c)^2 with the dead-pixel rule."""
    a, b, w = a.to(dtype), b.to(dtype), w.to(dtype)
    ah, bh = _unit(a, dtype)[0], _unit(b, dtype)[0]
    return (w.view(-1, 1, 1) * (ah - bh).pow(2)).sum() / (a.shape[1] * a.shape[2])


def tap_term_stock(a, b, w):
    """The term as the package computes it (no rule: NaN gradients at a dead pixel).  a, b: [C,h,w] or [C,n] (chosen pixels),
    summed, NOT divided by the pixel count."""
    ah = a / (a.pow(2).sum(0, keepdim=True).sqrt() + EPS)
    bh = b / (b.pow(2).sum(0, keepdim=True).sqrt() + EPS)
    return (w.view(-1, *([1] * (a.dim() - 1))) * (ah - bh).pow(2)).sum()


def tap_seed(a, b, w, dtype=torch.float64):
    """dterm/da [C,h,w] by the closed form: r g_c - a^_c T / n with g_c = 2 w_c (a^_c - b^_c) / (h w), T = sum_c g_c a^_c;
    exactly 0 at a dead pixel."""
    a, b, w = a.to(dtype), b.to(dtype), w.to(dtype)
    ah, r, n, live = _unit(a, dtype)
    bh = _unit(b, dtype)[0]
    g = 2.0 * w.view(-1, 1, 1) * (ah - bh) / (a.shape[1] * a.shape[2])
    T = (g * ah).sum(0)
    return torch.where(live, r * g - ah * (T / n), torch.zeros_like(a))


def forward(W, B, lin, layers, img, gt, size, dtype=torch.float64):
    """vgg_ref.forward's dict (x, z, a) with the LPIPS terms and their sum."""
    r = vgg_ref.forward(W, B, layers, img, gt, size, dtype)
    taps = [l for l, y in enumerate(layers) if y[3]]
    terms = [tap_term(r["a"][l][0], r["a"][l][1], w, dtype) for l, w in zip(taps, lin)]
    return dict(x=r["x"], z=r["z"], a=r["a"], terms=terms, loss=sum(terms))


def autograd_gradient(W, B, lin, layers, img, gt, size, dtype=torch.float64):
    leaf = img.to(dtype).clone().requires_grad_(True)
    r = forward(W, B, lin, layers, leaf, gt.to(dtype), size, dtype)
    (g,) = torch.autograd.grad(r["loss"], leaf)
    return r["loss"].detach(), g


def pinned_backward(W, lin, layers, acts, image_hw, size, dtype=torch.float64):
    """dLoss/dimg [3,H,W] in `dtype` with the ReLU masks and pool argmaxes read from `acts` (per layer [2,C,h,w]) and the tap
    seeds by the closed form at `acts`.  What is left is linear."""
    L = len(layers)
    lin_of = dict(zip([l for l, y in enumerate(layers) if y[3]], lin))
    g = None
    for l in range(L - 1, -1, -1):
        ci, co, pool, tap = layers[l]
        a, a_gt = acts[l][0].to(dtype), acts[l][1].to(dtype)
        if tap:
            t = tap_seed(a, a_gt, lin_of[l], dtype)
            g = t if g is None else g + t
        dz = g * (a > 0).to(dtype)
        d_in = F.conv_transpose2d(dz[None], W[l].to(dtype), padding=1)[0]
        if pool:
            prev = acts[l - 1][0].to(dtype)
            d_in = d_in.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * vgg_ref._window_one_hot(prev).to(dtype)
        g = d_in
    leaf = torch.zeros(1, 3, *image_hw, dtype=dtype, requires_grad=True)
    (d_img,) = torch.autograd.grad(vgg_ref.preprocess(leaf, size, dtype), leaf, g[None])
    return d_img[0]


def decisions_clear(r, layers, margin):
    """vgg_ref.decisions_clear without the tap-sign decision (LPIPS has none): every ReLU pre-activation of the rendered image
    and the top two of its live pool windows are `margin` x the layer's RMS pre-activation clear."""
    for l, (ci, co, pool, tap) in enumerate(layers):
        z, a = r["z"][l], r["a"][l]
        tol = margin * float(z.pow(2).mean().sqrt())
        if float(z[0].abs().min()) < tol:
            return False
        if l + 1 < len(layers) and layers[l + 1][2]:
            top = vgg_ref._windows(a[0]).topk(2, dim=-1).values
            live = top[..., 0] > 0
            if bool(live.any()) and float((top[..., 0] - top[..., 1])[live].min()) < tol:
                return False
    return True


def dead_pixel_case():
    """(W, B, lin, img, gt) on vgg_ref.SMALL whose rendered image has dead pixels at both taps and whose target has none:
    non-negative first-layer weights without bias and negative later biases make a black patch of the rendered image a patch
    of all-zero feature vectors."""
    W, B = vgg_ref.he_weights(vgg_ref.SMALL, seed=14)
    W = [W[0].abs(), W[1], W[2]]
    B = [torch.zeros_like(B[0]), -B[1].abs(), -B[2].abs()]
    img, gt = vgg_ref.images(24, 24, seed=24024)
    img = img.clone()
    img[:, :12, :12] = 0.0
    return W, B, lin_weights(vgg_ref.SMALL, seed=5), img, gt


def dead_target_case():
    """`dead_pixel_case` with black patches in the TARGET too: its bottom-right 12 x 12 (over live rendered pixels: target-only
    dead, where the target takes no gradient and stock autograd is finite) and its top-left 6 x 6 (inside the rendered image's
    black patch: both dead, contribution and scalars exactly 0)."""
    W, B, lin, img, gt = dead_pixel_case()
    gt = gt.clone()
    gt[:, 12:, 12:] = 0.0
    gt[:, :6, :6] = 0.0
    return W, B, lin, img, gt


def dead_classes(acts, layers):
    """Per tap bool masks [h,w] (both dead, rendered only, target only) of `acts` (per layer [2,C,h,w])."""
    out = []
    for l, y in enumerate(layers):
        if y[3]:
            da, db = acts[l][0].pow(2).sum(0) == 0, acts[l][1].pow(2).sum(0) == 0
            out.append((da & db, da & ~db, ~da & db))
    return out


def dead_pixels(acts, layers):
    """Per tap (dead rendered pixels, dead target pixels) of `acts` (per layer [2,C,h,w])."""
    return [(int((acts[l][0].pow(2).sum(0) == 0).sum()), int((acts[l][1].pow(2).sum(0) == 0).sum()))
            for l, y in enumerate(layers) if y[3]]
