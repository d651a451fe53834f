"""FateAvatar's VGG perceptual term on the fused path: a frozen stack of 3 x 3 convolutions run on the rendered image and on
its target, the mean absolute difference of chosen layer outputs, and the gradient to the rendered image — one call, no
autograd graph, no vendor-library convolutions, the same bits on every launch and graph replay.

reference:
  * `VGGPerceptualLoss` (tools/loss_utils/vgg_feature.py:7-47): (x - mean) / std with the ImageNet statistics, bilinear resize
    to 224^2, torchvision's `vgg16.features[:23]` in four blocks, `l1_loss` of the four block outputs (relu1_2, relu2_2,
    relu3_3, relu4_3) — `VggFeatures.vgg16()` is that stack
  * its weight in the objective: 0.1 (config/fateavatar.yaml:13-25, train/loss.py:123-199) — `Perceptual(features, weight=0.1)`
What is fused: fr_vgg_loss_grad (csrc/fr_vgg.hip) — every convolution an implicit GEMM on the exact-f32 MFMA over NHWC
activations, the data gradient the same GEMM over a second packing of the weights.  The weights are the CALLER's (pretrained
weights are not shipped): `VggFeatures.from_state_dict` reads torchvision's keys.  They are frozen and packed once, here, with
torch permutes; the packings are documented in include/fr_rasterizer.h.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class ConvLayer(NamedTuple):
    """conv3x3(c_in -> c_out, padding 1) + bias + ReLU.  `pool_before`: a 2 x 2 / 2 max-pool on its input; `tap_after`: its
    output is a feature the loss compares."""
    c_in: int
    c_out: int
    pool_before: bool = False
    tap_after: bool = False


# vgg16.features[:23]: ten convolutions, three pools, taps at relu1_2, relu2_2, relu3_3, relu4_3
VGG16_LAYERS = (ConvLayer(3, 64), ConvLayer(64, 64, tap_after=True),
                ConvLayer(64, 128, pool_before=True), ConvLayer(128, 128, tap_after=True),
                ConvLayer(128, 256, pool_before=True), ConvLayer(256, 256), ConvLayer(256, 256, tap_after=True),
                ConvLayer(256, 512, pool_before=True), ConvLayer(512, 512), ConvLayer(512, 512, tap_after=True))


# lpips.LPIPS(net='vgg')'s trunk, vgg16.features[:30]: thirteen convolutions, four pools, taps at relu1_2, relu2_2, relu3_3,
# relu4_3 and relu5_3
LPIPS_VGG16_LAYERS = VGG16_LAYERS + (ConvLayer(512, 512, pool_before=True), ConvLayer(512, 512), ConvLayer(512, 512, tap_after=True))
# lpips' ScalingLayer: (x - shift) / scale on an input in [-1, 1]; `normalize=True` maps [0, 1] there first (2 x - 1)
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
LPIPS_MAX_TAP_WIDTH = 512       # a tapped layer's c_out: eight values a lane (include/fr_rasterizer.h)


def lpips_mean_std(normalize: bool = True):
    """(mean, std) with which `(x - mean) / std` is LPIPS's input layer: for `normalize=True` (images in [0, 1], the
    reference's calls) (2 x - 1 - shift) / scale = (x - (1 + shift) / 2) / (scale / 2), which is the ImageNet statistics;
    for `normalize=False` (images in [-1, 1]) shift and scale themselves."""
    if normalize:
        return tuple((1.0 + s) / 2.0 for s in LPIPS_SHIFT), tuple(s / 2.0 for s in LPIPS_SCALE)
    return LPIPS_SHIFT, LPIPS_SCALE


def as_layers(layers) -> Tuple[ConvLayer, ...]:
    """ConvLayer records from records or plain (c_in, c_out[, pool_before[, tap_after]]) tuples."""
    return tuple(ConvLayer(int(y[0]), int(y[1]), bool(y[2]) if len(y) > 2 else False, bool(y[3]) if len(y) > 3 else False) for y in layers)


def check_layers(layers: Sequence[ConvLayer], size: Tuple[int, int]) -> None:
    """The limits of the kernels (include/fr_rasterizer.h), checked on the host before anything touches the device."""
    layers = as_layers(layers)
    if not 1 <= len(layers) <= _lib.FR_VGG_MAX_LAYERS:
        raise ValueError(f"VggFeatures: 1 .. {_lib.FR_VGG_MAX_LAYERS} layers, not {len(layers)}")
    sh, sw = int(size[0]), int(size[1])
    if not (1 <= sh <= 32767 and 1 <= sw <= 32767):
        raise ValueError(f"VggFeatures: size {size} outside 1 .. 32767")
    pools = 0
    for i, y in enumerate(layers):
        want = 3 if i == 0 else int(layers[i - 1].c_out)
        if int(y.c_in) != want:
            raise ValueError(f"VggFeatures: layer {i} has c_in = {y.c_in}, its input has {want} channels")
        if i > 0 and y.c_in % 32:
            raise ValueError(f"VggFeatures: layer {i}: c_in = {y.c_in} is not a multiple of 32")
        if y.c_out < 64 or y.c_out % 64:
            raise ValueError(f"VggFeatures: layer {i}: c_out = {y.c_out} is not a multiple of 64")
        if i == 0 and y.pool_before:
            raise ValueError("VggFeatures: layer 0 takes no pool")
        pools += 1 if y.pool_before else 0
        if sh % (1 << pools) or sw % (1 << pools):
            raise ValueError(f"VggFeatures: size {(sh, sw)} is not divisible by 2^{pools} (the pools up to layer {i})")
    if not layers[-1].tap_after:
        raise ValueError("VggFeatures: the last layer must be a tap (nothing else reaches it)")


def torchvision_indices(layers: Sequence[ConvLayer]) -> List[int]:
    """The index of every layer's Conv2d inside a torchvision-style `features` Sequential (conv, ReLU, and a MaxPool2d where
    `pool_before` says): 0, 2, 5, 7, 10, 12, 14, 17, 19, 21 for VGG16_LAYERS."""
    out, i = [], 0
    for y in as_layers(layers):
        i += 1 if y.pool_before else 0
        out.append(i)
        i += 2
    return out


def pack_forward(weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """A Conv2d's `weight` [c_out,c_in,3,3] and `bias` as the forward GEMM's operand: [9 c_in][c_out] with row
    (3 ky + kx) c_in + ci, then the bias — flat."""
    co, ci = weight.shape[:2]
    return torch.cat([weight.permute(2, 3, 1, 0).reshape(9 * ci * co), bias.reshape(co)])


def pack_backward(weight: torch.Tensor) -> torch.Tensor:
    """The data gradient's operand: taps flipped, c_in / c_out exchanged — [9 c_out][c_in] with row (3 ky + kx) c_out + co
    holding weight[co, ci, 2 - ky, 2 - kx] — flat."""
    co, ci = weight.shape[:2]
    return weight.flip(2, 3).permute(2, 3, 0, 1).reshape(9 * co * ci)


class VggFeatures:
    """A frozen conv stack and its packed weights.  `layers`: ConvLayer records; `weights` / `biases`: per layer a Conv2d's
    [c_out,c_in,3,3] and [c_out] (default: He-normal weights and zero biases from torch's generator — a stand-in: the
    perceptual term means something with pretrained weights only, which are the caller's to supply); `size`: what both images
    are resized to; `mean` / `std`: the per-channel normalisation."""

    def __init__(self, layers: Sequence[ConvLayer] = VGG16_LAYERS, weights: Optional[Sequence[torch.Tensor]] = None,
                 biases: Optional[Sequence[torch.Tensor]] = None, size: Tuple[int, int] = (224, 224),
                 mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD, device=None):
        self.layers = as_layers(layers)
        self.size = (int(size[0]), int(size[1]))
        check_layers(self.layers, self.size)
        if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
            raise ValueError("VggFeatures: mean and std are three numbers each, std nonzero")
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if (weights is None) != (biases is None):
            raise ValueError("VggFeatures: give both `weights` and `biases`, or neither")
        if weights is None:
            weights = [torch.randn(y.c_out, y.c_in, 3, 3) * math.sqrt(2.0 / (9 * y.c_in)) for y in self.layers]
            biases = [torch.zeros(y.c_out) for y in self.layers]
        if len(weights) != len(self.layers) or len(biases) != len(self.layers):
            raise ValueError(f"VggFeatures: {len(self.layers)} layers, {len(weights)} weights and {len(biases)} biases")
        for i, (y, w, b) in enumerate(zip(self.layers, weights, biases)):
            if tuple(w.shape) != (y.c_out, y.c_in, 3, 3) or tuple(b.shape) != (y.c_out,):
                raise ValueError(f"VggFeatures: layer {i}'s weight is {tuple(w.shape)} and its bias {tuple(b.shape)}, not "
                                 f"{(y.c_out, y.c_in, 3, 3)} and {(y.c_out,)}")
        dev = torch.device(device) if device is not None else weights[0].device
        self.device = dev
        self.weights = [w.detach().to(dev, torch.float32).contiguous() for w in weights]
        self.biases = [b.detach().to(dev, torch.float32).contiguous() for b in biases]
        self.packed_fwd = torch.cat([pack_forward(w, b) for w, b in zip(self.weights, self.biases)]).contiguous()
        self.packed_bwd = torch.cat([pack_backward(w) for w in self.weights]).contiguous()
        self.taps = [i for i, y in enumerate(self.layers) if y.tap_after]

    @classmethod
    def vgg16(cls, **kw) -> "VggFeatures":
        """The reference's stack: vgg16.features[:23] with its four taps."""
        return cls(VGG16_LAYERS, **kw)

    def extents(self) -> List[Tuple[int, int]]:
        """(h, w) of every layer's output."""
        out, (h, w) = [], self.size
        for y in self.layers:
            if y.pool_before:
                h, w = h // 2, w // 2
            out.append((h, w))
        return out

    def _names(self, prefix: str = "") -> List[str]:
        return [f"{prefix}features.{i}" for i in torchvision_indices(self.layers)]

    @torch.no_grad()
    def state_dict(self, prefix: str = "") -> dict:
        """torchvision's naming: features.{i}.weight / .bias with i the Conv2d's place in the Sequential."""
        sd = {}
        for n, w, b in zip(self._names(prefix), self.weights, self.biases):
            sd[n + ".weight"], sd[n + ".bias"] = w.clone(), b.clone()
        return sd

    @classmethod
    def from_state_dict(cls, sd: dict, prefix: str = "", layers: Sequence[ConvLayer] = VGG16_LAYERS, **kw) -> "VggFeatures":
        """From a torchvision-style state dict (`vgg16().state_dict()`: features.{0,2,5,7,10,12,14,17,19,21}.{weight,bias} for
        the default layers; later entries and the classifier are ignored)."""
        weights, biases = [], []
        for i in torchvision_indices(layers):
            for key, into in ((f"{prefix}features.{i}.weight", weights), (f"{prefix}features.{i}.bias", biases)):
                if key not in sd:
                    raise KeyError(f"VggFeatures: the state lacks {key}")
                into.append(sd[key])
        return cls(layers, weights, biases, **kw)

    def describe(self, H: int, W: int, image=None, target=None, tile: int = _lib.FR_VGG_TILE_AUTO) -> _lib.fr_vgg:
        d = _lib.fr_vgg()
        d.n_layers, d.H, d.W, d.size_h, d.size_w, d.tile = len(self.layers), int(H), int(W), self.size[0], self.size[1], int(tile)
        for c in range(3):
            d.mean[c], d.std[c] = self.mean[c], self.std[c]
        for i, y in enumerate(self.layers):
            d.layers[i] = _lib.fr_vgg_layer(y.c_in, y.c_out, int(y.pool_before), int(y.tap_after))
        d.weights_fwd, d.weights_bwd = self.packed_fwd.data_ptr(), self.packed_bwd.data_ptr()
        d.image = None if image is None else image.data_ptr()
        d.target = None if target is None else target.data_ptr()
        return d


class Perceptual:
    """The perceptual term of one training loop: `features` on a device, the term's `weight` in the objective, and the
    workspace (allocated HERE, outside any capture; one per object: calls that may overlap use different objects)."""

    _NAME, _BYTES, _ENTRY = "Perceptual", "fr_vgg_workspace_bytes", "fr_vgg_loss_grad"

    def __init__(self, features: VggFeatures, weight: float = 0.1):
        if not isinstance(features, VggFeatures):
            raise TypeError(f"{self._NAME}: `features` must be a VggFeatures")
        if features.device.type != "cuda":
            raise RuntimeError(f"{self._NAME} needs device tensors (there is no CPU path): VggFeatures(..., device=)")
        self.features, self.weight = features, float(weight)
        self.tile = _lib.FR_VGG_TILE_AUTO
        self.n_terms = len(features.taps)
        need = int(getattr(_lib.lib(), self._BYTES)(C.byref(features.describe(1, 1))))
        if need == 0:
            raise RuntimeError(f"{self._NAME}: the library refuses the layer table ({self._BYTES} returned 0)")
        # zeroed: the head of the workspace (counters and partials of the terms' sums) must be, and every call leaves it so
        self._workspace = torch.zeros(need, dtype=torch.uint8, device=features.device)

    def _check_image(self, t: torch.Tensor, what: str, shape=None):
        dev = self.features.device
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != 3 or not t.is_contiguous() or t.device != dev or \
                (shape is not None and tuple(t.shape) != tuple(shape)) or t.shape[1] * t.shape[2] == 0:
            raise ValueError(f"{self._NAME}: {what} must be a contiguous float32 [3,H,W] tensor on {dev}"
                             + (f" of shape {tuple(shape)}" if shape is not None else ""))

    @torch.no_grad()
    def loss_and_grad(self, img: torch.Tensor, gt: torch.Tensor, loss_out: Optional[torch.Tensor] = None, grad_out=None,
                      accumulate: bool = False, weight: Optional[float] = None):
        """(losses [1 + T], gradient).  losses[0]: the unweighted sum of the T tap terms, losses[1:] the terms.  The gradient
        buffer receives `weight` (default: the object's) x dLoss/dimg — stored, or with `accumulate` ADDED to what `grad_out`
        holds (a step adds it to its L1 gradient without another launch).  `grad_out=False`: forward only, no gradient.
        `loss_out` / `grad_out`: the buffers of a captured step."""
        img = img.detach()
        self._check_image(img, "img")
        self._check_image(gt, "gt", img.shape)
        dev = self.features.device
        loss = loss_out if loss_out is not None else torch.empty(1 + self.n_terms, dtype=torch.float32, device=dev)
        if loss.dtype != torch.float32 or loss.numel() != 1 + self.n_terms or not loss.is_contiguous() or loss.device != dev:
            raise ValueError(f"{self._NAME}: loss_out must be a contiguous float32 [{1 + self.n_terms}] tensor on {dev}")
        grad = None
        if grad_out is not False:
            if grad_out is None:
                if accumulate:
                    raise ValueError(f"{self._NAME}: `accumulate` needs the `grad_out` to add to")
                grad_out = torch.empty_like(img)
            self._check_image(grad_out, "grad_out", img.shape)
            grad = grad_out
        d = self.features.describe(img.shape[1], img.shape[2], img, gt, self.tile)
        _lib.launch(self._ENTRY, dev, C.byref(d), *self._term_args(), C.c_float(self.weight if weight is None else float(weight)),
                    int(bool(accumulate)), loss.data_ptr(), None if grad is None else grad.data_ptr(), self._workspace.data_ptr())
        return loss, grad

    def _term_args(self) -> tuple:
        """What the entry point takes between the descriptor and the weight."""
        return ()

    def _view(self, offset: int, shape) -> torch.Tensor:
        n = 4 * math.prod(shape)
        return self._workspace[offset:offset + n].view(torch.float32).view(*shape)

    def saved_input(self) -> torch.Tensor:
        """The normalised, resized images of the last call, [2, size_h, size_w, 3] (0: the image, 1: the target): a view."""
        return self._view(_r256(_lib.FR_VGG_REDUCE_BYTES), (2, self.features.size[0], self.features.size[1], 3))

    def saved_activations(self) -> List[torch.Tensor]:
        """Every layer's post-ReLU output of the last call, [2, h_l, w_l, c_out_l] (NHWC; 0: the image, 1: the target): views
        into the workspace, where the backward reads its masks, argmaxes and signs."""
        f = self.features
        o = _r256(_lib.FR_VGG_REDUCE_BYTES) + _r256(2 * f.size[0] * f.size[1] * 3 * 4)
        out = []
        for y, (h, w) in zip(f.layers, f.extents()):
            out.append(self._view(o, (2, h, w, y.c_out)))
            o += _r256(2 * h * w * y.c_out * 4)
        return out

    def __call__(self, img: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        return vgg_perceptual_loss(img, gt, self)


# Where the `lpips` package keeps a tap's learnt weights in its state dict: `lin{k}.model.1.weight`, [1,C,1,1] (model.0 is a
# Dropout).  Written from memory of the package: it is not installed where this was written and the reference does not vendor
# it, so the names could not be checked against it.  They live in this one table.
LPIPS_LIN_KEYS = tuple(f"lin{k}.model.1.weight" for k in range(5))


class Lpips(Perceptual):
    """The LPIPS term of one training loop (or the metric): `features` — the trunk, by default to be built with
    `Lpips.trunk()` — the taps' learnt `lin` weights (per tap a [c_out] tensor; default: uniform 1 / c_out, a stand-in as the
    trunk's default weights are) and the term's `weight` in the objective (FlashAvatar 0.05, SplattingAvatar 0.01).  The
    calls, buffers and saved-state views are `Perceptual`'s; `loss_and_grad(..., grad_out=False)` is the metric.
    A pixel whose feature vector is all zero contributes with a zero unit vector and takes a gradient of exactly 0, where stock
    autograd gives NaN (include/fr_rasterizer.h)."""
    _NAME, _BYTES, _ENTRY = "Lpips", "fr_lpips_workspace_bytes", "fr_lpips_loss_grad"

    def __init__(self, features: VggFeatures, lin: Optional[Sequence[torch.Tensor]] = None, weight: float = 0.05):
        if isinstance(features, VggFeatures):
            for i in features.taps:
                if features.layers[i].c_out > LPIPS_MAX_TAP_WIDTH:
                    raise ValueError(f"Lpips: layer {i} is a tap of {features.layers[i].c_out} channels, more than {LPIPS_MAX_TAP_WIDTH}")
        super().__init__(features, weight)
        widths = [features.layers[i].c_out for i in features.taps]
        if lin is None:
            lin = [torch.full((c,), 1.0 / c) for c in widths]
        if len(lin) != len(widths) or any(w.numel() != c for w, c in zip(lin, widths)):
            raise ValueError(f"Lpips: `lin` is one vector per tap, of {widths} elements")
        self.lin = [w.detach().reshape(-1).to(features.device, torch.float32).contiguous() for w in lin]
        self.packed_lin = torch.cat(self.lin).contiguous()

    def _term_args(self) -> tuple:
        return (self.packed_lin.data_ptr(),)

    @staticmethod
    def trunk(size: Tuple[int, int], normalize: bool = True, **kw) -> VggFeatures:
        """The 13-layer trunk at `size` (LPIPS does not resize: the frame's (H, W)) with LPIPS's input statistics."""
        mean, std = lpips_mean_std(normalize)
        return VggFeatures(LPIPS_VGG16_LAYERS, size=size, mean=mean, std=std, **kw)

    def saved_pixel_scalars(self) -> List[torch.Tensor]:
        """Per tap [h, w, 3]: (1 / (n_a + 1e-10), 1 / (n_b + 1e-10), T / n_a) of the last call, all 0 at a dead pixel: views."""
        f = self.features
        o, out = workspace_bytes(f), []
        for i, (h, w) in enumerate(f.extents()):
            if f.layers[i].tap_after:
                out.append(self._view(o, (h, w, 3)))
                o += _r256(h * w * 3 * 4)
        return out

    def lin_state_dict(self) -> dict:
        return {LPIPS_LIN_KEYS[k]: w.clone().view(1, -1, 1, 1) for k, w in enumerate(self.lin)}

    @classmethod
    def from_state_dicts(cls, trunk_sd: dict, lin_sd: dict, size: Tuple[int, int], weight: float = 0.05, normalize: bool = True,
                         prefix: str = "", device=None) -> "Lpips":
        """From torchvision's `vgg16().state_dict()` (features.{0,2,..,28}.{weight,bias}) and the `lpips` package's state
        (LPIPS_LIN_KEYS).  `size`: the frames' (H, W)."""
        mean, std = lpips_mean_std(normalize)
        f = VggFeatures.from_state_dict(trunk_sd, prefix, LPIPS_VGG16_LAYERS, size=size, mean=mean, std=std, device=device)
        lin = []
        for k, key in enumerate(LPIPS_LIN_KEYS):
            if key not in lin_sd:
                raise KeyError(f"Lpips: the state lacks {key}")
            c = LPIPS_VGG16_LAYERS[f.taps[k]].c_out
            if tuple(lin_sd[key].shape) != (1, c, 1, 1):
                raise ValueError(f"Lpips: {key} is {tuple(lin_sd[key].shape)}, not {(1, c, 1, 1)}")
            lin.append(lin_sd[key].reshape(c))
        return cls(f, lin, weight)

    def __call__(self, img: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        return lpips_loss(img, gt, self)


def lpips_workspace_bytes(features: VggFeatures) -> int:
    """include/fr_rasterizer.h's formula of fr_lpips_workspace_bytes, restated."""
    total, seed_max = workspace_bytes(features), 0
    for i, (y, (h, w)) in enumerate(zip(features.layers, features.extents())):
        if y.tap_after:
            total += _r256(h * w * 3 * 4)
            if i + 1 < len(features.layers):
                seed_max = max(seed_max, h * w * y.c_out)
    return total + _r256(seed_max * 4)


def _r256(v: int) -> int:
    return (int(v) + 255) // 256 * 256


def workspace_bytes(features: VggFeatures) -> int:
    """include/fr_rasterizer.h's formula of fr_vgg_workspace_bytes, restated."""
    sh, sw = features.size
    total = _r256(_lib.FR_VGG_REDUCE_BYTES) + _r256(2 * sh * sw * 3 * 4)
    pool_max = grad_max = split_max = 0
    for i, (y, (h, w)) in enumerate(zip(features.layers, features.extents())):
        total += _r256(2 * h * w * y.c_out * 4)
        grad_max = max(grad_max, h * w * y.c_out)
        if y.pool_before:
            pool_max = max(pool_max, h * w * y.c_in)
        if i > 0:
            for M, N in ((2 * h * w, y.c_out), (h * w, y.c_in)):
                s = gemm_splits(M, N)
                split_max = max(split_max, s * M * N if s > 1 else 0)
    return total + _r256(2 * pool_max * 4) + 2 * _r256(grad_max * 4) + _r256(pool_max * 4) + _r256(split_max * 4)


def gemm_splits(M: int, N: int) -> int:
    """Into how many groups of taps the kernels split a GEMM of M rows and N columns (include/fr_rasterizer.h)."""
    tiles = -(-M // 64) * -(-N // 64)
    return 1 if tiles >= 256 else (3 if 3 * tiles >= 256 else 9)


class _VggPerceptual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt, perceptual):
        x = img.detach()
        x = x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()
        y = gt if gt.dtype == torch.float32 and gt.is_contiguous() else gt.float().contiguous()
        loss, grad = perceptual.loss_and_grad(x, y, grad_out=None if ctx.needs_input_grad[0] else False, weight=1.0)
        if grad is not None:
            ctx.save_for_backward(grad)
        ctx.in_dtype = img.dtype
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return (grad * grad_output).to(ctx.in_dtype), None, None


def vgg_perceptual_loss(img: torch.Tensor, gt: torch.Tensor, perceptual: Perceptual) -> torch.Tensor:
    """The UNWEIGHTED perceptual loss (the sum of the tap terms) as a 0-dim tensor, differentiable with respect to `img`: the
    fused kernels compute the gradient in the forward, the backward scales it by the incoming one.  The reference's objective
    adds `0.1 * vgg_perceptual_loss(...)`.  The target takes no gradient: `gt.requires_grad` raises."""
    if gt.requires_grad:
        raise RuntimeError("vgg_perceptual_loss: the target takes no gradient; detach it")
    return _VggPerceptual.apply(img, gt, perceptual)


def lpips_loss(img: torch.Tensor, gt: torch.Tensor, lpips: Lpips) -> torch.Tensor:
    """The UNWEIGHTED LPIPS distance of two [3,H,W] images in [0,1] as a 0-dim tensor, differentiable with respect to `img`
    (as vgg_perceptual_loss is).  The objectives add `lpips.weight * lpips_loss(...)`."""
    if not isinstance(lpips, Lpips):
        raise TypeError("lpips_loss: `lpips` must be an Lpips")
    if gt.requires_grad:
        raise RuntimeError("lpips_loss: the target takes no gradient; detach it")
    return _VggPerceptual.apply(img, gt, lpips)


__all__ = ["LPIPS_LIN_KEYS", "LPIPS_SCALE", "LPIPS_SHIFT", "LPIPS_VGG16_LAYERS", "Lpips", "lpips_loss", "lpips_mean_std", "lpips_workspace_bytes", "ConvLayer", "as_layers", "IMAGENET_MEAN", "IMAGENET_STD", "Perceptual", "VGG16_LAYERS", "VggFeatures", "check_layers", "gemm_splits", "pack_backward",
           "pack_forward", "torchvision_indices", "vgg_perceptual_loss", "workspace_bytes"]
