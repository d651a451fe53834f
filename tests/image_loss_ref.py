"""A torch restatement of the L1 + D-SSIM image loss, written from its formulas (not from the library's code):

    window  w = g g^T rounded to float32, g = the 11 taps exp(-(i - 5)^2 / (2 x 1.5^2)) rounded to float32, divided by their
            float32 sum
    conv    = correlation with w per channel, zero padding 5
    mu1 = conv(x), mu2 = conv(y), s11 = conv(x x) - mu1^2, s22 = conv(y y) - mu2^2, s12 = conv(x y) - mu1 mu2
    S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),  C1 = 1e-4, C2 = 9e-4
    d_ssim = 1 - mean(S),  l1 = mean |x - y|,  loss = rgb_weight l1 + dssim_weight d_ssim

evaluated in float64 (the reference of the tests) or in float32 (the yardstick for what float32 arithmetic reaches on the
same inputs), the gradients with respect to x from autograd.  CPU only; results are cached per input.
`d_ssim_of` is pinned to recorded runs of the reference's own `d_ssim` (tools/loss_utils/dssim.py) by
tests/test_reference_runs_host.py (tests/golden/reference_image_terms.npz, cases `dssim_*` and `ga`)."""
import functools
from math import exp

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
TILE = 32            # the kernels' output tile (fateavatar_amd/csrc/fr_ssim.hip): the test shapes straddle it
SHAPES = [(3, 1, 1), (3, 7, 5), (3, 11, 11), (3, TILE, TILE), (3, TILE + 1, TILE - 1), (3, 33, 47), (3, 64, 80), (3, 128, 128),
          (1, 33, 47)]
KINDS = ("noise", "smooth", "near")
WEIGHTS = [(0.8, 0.2), (0.0, 1.0), (1.0, 0.0)]
# the issue's bounds: each loss scalar, the gradient's rel-L2, every gradient entry relative to max |g64|
LOSS_ATOL, GRAD_REL_L2, GRAD_ENTRY = 1e-5, 1e-4, 1e-4


def window_taps() -> torch.Tensor:
    """The eleven float32 taps, in the arithmetic of the original `gaussian(11, 1.5)`: float32 roundings of the doubles,
    float32 sum, float32 division."""
    g = torch.tensor([exp(-(i - 5) ** 2 / float(2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    return g / g.sum()


def d_ssim_of(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """1 - mean SSIM map of [C,H,W] images in their own dtype (differentiable)."""
    C = x.shape[0]
    g = window_taps()
    # the 121 products are rounded to float32 BEFORE the window takes the images' dtype (`create_window` multiplies the taps in
    # float32, `d_ssim` casts the result): in float64 the float64 products of the taps are another window, 2e-6 of d_ssim away
    # from the recorded run (tests/golden/reference_image_terms.npz, tests/test_reference_runs_host.py)
    w = (g[:, None] * g[None, :]).to(x.dtype).expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], w, padding=5, groups=C)[0]  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s11, s22, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    S = (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return 1 - S.mean()


def terms(x: torch.Tensor, y: torch.Tensor, dtype=torch.float64):
    """(l1, d_ssim, d l1 / dx, d d_ssim / dx) of float32 [C,H,W] CPU images, evaluated in `dtype`."""
    xx = x.detach().cpu().to(dtype).clone().requires_grad_()
    yy = y.detach().cpu().to(dtype)
    l1 = (xx - yy).abs().mean()
    (g1,) = torch.autograd.grad(l1, xx)
    ds = d_ssim_of(xx, yy)
    (gs,) = torch.autograd.grad(ds, xx)
    return l1.detach(), ds.detach(), g1, gs


def combine(t, weights):
    """(loss3, grad) for (rgb_weight, dssim_weight) from `terms`' output.  A D-SSIM weight of 0 asks for no D-SSIM at all: the
    interface defines the third loss word as 0 then (the SSIM work is skipped)."""
    l1, ds, g1, gs = t
    if weights[1] == 0:
        ds = torch.zeros_like(ds)
    return torch.stack([weights[0] * l1 + weights[1] * ds, l1, ds]), weights[0] * g1 + weights[1] * gs


def make_inputs(shape, kind: str, seed: int = 0):
    """(x, y) float32 CPU [C,H,W]: `noise` uniform against uniform; `smooth` 3 x 3-box-smoothed uniform against the same;
    `near` a smoothed target and the target + 0.02 N(0, 1) — where training lives and where s = E - mu^2 cancels most."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * sum(shape) + len(kind) + shape[1])
    rand = lambda: torch.rand(shape, generator=gen)  # noqa: E731
    smooth = lambda t: F.avg_pool2d(t[None], 3, stride=1, padding=1)[0]  # noqa: E731
    if kind == "noise":
        return rand(), rand()
    if kind == "smooth":
        return smooth(rand()), smooth(rand())
    if kind == "near":
        y = smooth(rand())
        return y + 0.02 * torch.randn(shape, generator=gen), y
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case(shape, kind: str):
    """The inputs of a test case with their float64 terms and the float32 twin's, computed once."""
    x, y = make_inputs(shape, kind)
    return x, y, terms(x, y, torch.float64), terms(x, y, torch.float32)


def errors(loss3, grad, want3, want_grad):
    """(max |loss - want| over the three scalars, gradient rel-L2, max entry error / max |want|) in float64."""
    loss3, grad = loss3.detach().cpu().double(), grad.detach().cpu().double()
    dl = float((loss3 - want3.double()).abs().max())
    gmax = float(want_grad.abs().max())
    diff = grad - want_grad.double()
    return dl, float(diff.norm() / want_grad.double().norm().clamp_min(1e-300)), float(diff.abs().max()) / max(gmax, 1e-300)
