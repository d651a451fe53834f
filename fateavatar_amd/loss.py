"""Image loss of the optimisation step.

reference: `nn.L1Loss(reduction='mean')` on the rendered image (model/loss.py:92) followed by `loss.backward()` — eight
launch-bound PyTorch kernels between the rasterizer's forward and its backward.  `l1_loss_and_grad` produces the loss
and the gradient autograd would hand to the rasterizer (`sign(img - gt) / n`, for a unit upstream gradient) in one
launch of the HIP library (`fr_l1_loss_grad`, include/fr_rasterizer.h); the caller continues with
`render.backward(grad)`.  `image_loss_and_grad` is the same for the weighted L1 + D-SSIM objective of GaussianAvatars and
3DGS (train/loss.py:351-365, tools/loss_utils/dssim.py:28-56) in two launches (`fr_image_loss_grad`), and `d_ssim` the
reference's function as an autograd op on those kernels.  `huber_loss_and_grad` is FlashAvatar's Huber term with its optional
mouth-mask term (train/loss.py:217-221, :231-239) in one launch (`fr_huber_loss_grad`).  `pixel_loss_and_grad` is
SplattingAvatar's L1 + MSE image term (train/loss.py:279-283, :288-304) in one launch (`fr_pixel_loss_grad`) and
`scale_term_and_grad` its scale term (:307-315) in two (`fr_scale_term`).  `scale_ratio_term_and_grad` is FateAvatar's scale-ratio
term (:144-151) in one launch (`fr_scale_ratio_term`) and `scale_ratio_loss` the same expression as an autograd op.
`rot_term_and_grad` is neural baking's rotation term (UVDecoderLoss, :612-617) in one launch (`fr_rot_term`) and `rot_loss` the
same as an autograd op.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from .workspace import StreamWorkspace

# one workspace per op and (device, stream): workspace.py says why
_l1_ws = StreamWorkspace("l1_workspace", lambda: _lib.lib().fr_l1_workspace_bytes(), "image's")
_huber_ws = StreamWorkspace("huber_workspace", lambda: _lib.lib().fr_huber_workspace_bytes(), "image's")
_pixel_ws = StreamWorkspace("pixel_loss_workspace", lambda: _lib.lib().fr_pixel_loss_workspace_bytes(), "image's")
_scale_ws = StreamWorkspace("scale_term_workspace", lambda: _lib.lib().fr_scale_term_workspace_bytes(), "parameters'")
_ratio_ws = StreamWorkspace("scale_ratio_workspace", lambda: _lib.lib().fr_scale_ratio_workspace_bytes(), "parameters'")
_rot_ws = StreamWorkspace("rot_term_workspace", lambda: _lib.lib().fr_rot_term_workspace_bytes(), "rotations'")
_reg_ws = StreamWorkspace("regulariser_workspace", lambda: _lib.lib().fr_regularise_workspace_bytes(), "parameters'")
_mesh_ws = StreamWorkspace("mesh_terms_workspace", lambda: _lib.lib().fr_mesh_terms_workspace_bytes(), "vertices'")


# ---- what the wrappers below ask of their arguments, said once; `who`: the wrapper's name, for the message
def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _image_pair(img: torch.Tensor, gt: torch.Tensor, who: str):
    """The image (detached) and its target as contiguous float32, and their device."""
    if not (img.is_cuda and gt.is_cuda):
        raise RuntimeError(f"{who} needs device tensors (there is no CPU path)")
    if img.shape != gt.shape:
        raise RuntimeError(f"{who}: shapes differ: {tuple(img.shape)} vs {tuple(gt.shape)}")
    return _f32c(img.detach()), _f32c(gt), img.device


def _outputs(img: torch.Tensor, k: int, grad_out, loss_out, who: str):
    """The gradient buffer (None for `grad_out=False`) and the k-word loss tensor of an image term on the prepared `img`: the
    caller's, checked, or fresh ones.  (k = 1 is `l1_loss_and_grad`, whose contract is older and asks less.)"""
    dev = img.device
    grad = None if grad_out is False else (grad_out if grad_out is not None else torch.empty_like(img))
    loss = loss_out if loss_out is not None else torch.empty(() if k == 1 else (k,), dtype=torch.float32, device=dev)
    bad = (grad is not None and (grad.shape != img.shape or grad.dtype != torch.float32 or not grad.is_contiguous())) or loss.numel() != k
    if k == 1:
        what = ""
    else:
        bad = bad or (grad is not None and grad.device != dev) or loss.dtype != torch.float32 or loss.device != dev or not loss.is_contiguous()
        what = f" (gradient of the image's shape, {k}-element loss, float32, contiguous)"
    if bad:
        raise RuntimeError(f"{who}: bad output buffers{what}")
    return grad, loss


def _check_rows3(who: str, dev: torch.device, rows: int, tensors, what: str) -> None:
    """Every tensor (None: skipped) is contiguous float32 [rows,3] on `dev`."""
    for t in tensors:
        if t is not None and (t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (rows, 3)):
            raise RuntimeError(f"{who}: contiguous float32 {what}")


def _out_words(who: str, out: Optional[torch.Tensor], k: int, dev: torch.device, whose: str, fresh=torch.empty) -> torch.Tensor:
    """The k-word loss tensor of a term: the caller's `out`, checked, or a fresh one."""
    loss = out if out is not None else fresh((k,), dtype=torch.float32, device=dev)
    if loss.device != dev or loss.dtype != torch.float32 or loss.numel() != k or not loss.is_contiguous():
        raise RuntimeError(f"{who}: `out` is a contiguous {k}-element float32 tensor on the {whose} device")
    return loss


def _ptrs(tensors):
    """The tensors' addresses as a C pointer array (None: NULL)."""
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _image_lists(who: str, imgs, gts, loss_outs, grad_outs, workspaces):
    """The lists of a batched image term: 1 .. FR_MAX_BATCH images with one of everything each, on a device.  Returns the
    detached images, every tensor the kernel walks (images, targets, the gradient buffers that are not None) and the device."""
    K = len(imgs)
    if not (1 <= K <= _lib.FR_MAX_BATCH and len(gts) == len(loss_outs) == len(grad_outs) == len(workspaces) == K):
        raise RuntimeError(f"{who}: 1 .. {_lib.FR_MAX_BATCH} images, one gt / loss / grad / workspace each")
    imgs = [i.detach() for i in imgs]
    tensors = list(imgs) + list(gts) + [g for g in grad_outs if g is not None]
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who} needs device tensors (there is no CPU path)")
    return imgs, tensors, imgs[0].device


def l1_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `l1_loss_and_grad(..., workspace=)`: for callers that launch from several streams or
    graphs at once and want to own the scratch explicitly."""
    return _l1_ws.fresh(dev)


def l1_loss_and_grad(img: torch.Tensor, gt: torch.Tensor, loss_out: Optional[torch.Tensor] = None,
                     grad_out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """mean |img - gt| (0-dim device tensor) and its gradient with respect to `img`.  `loss_out` / `grad_out`: write into
    these tensors instead of fresh ones (buffers of a captured step).  `workspace`: scratch from `l1_workspace()`; by
    default one is kept per (device, current stream) — launches that may overlap must not share one."""
    who = "l1_loss_and_grad"
    img, gt, dev = _image_pair(img, gt, who)
    grad, loss = _outputs(img, 1, grad_out, loss_out, who)
    ws = _l1_ws.resolve(dev, workspace, who)
    _lib.launch("fr_l1_loss_grad", dev, img.numel(), img.data_ptr(), gt.data_ptr(), grad.data_ptr(), loss.data_ptr(), ws.data_ptr())
    return loss, grad


def l1_loss_and_grad_batch(imgs, gts, loss_outs, grad_outs, workspaces):
    """`l1_loss_and_grad` for the images of the 1 .. 4 frames of a batch in ONE launch (`fr_l1_loss_grad_batch`): lists of
    equally-sized contiguous float32 device tensors; every image has its own loss scalar, gradient buffer and workspace
    (`l1_workspace()`).  Returns (loss_outs, grad_outs)."""
    who = "l1_loss_and_grad_batch"
    imgs, tensors, dev = _image_lists(who, imgs, gts, loss_outs, grad_outs, workspaces)
    n = imgs[0].numel()
    for t in tensors:
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise RuntimeError(f"{who}: contiguous float32 tensors of one device and one size")
    need = _lib.lib().fr_l1_workspace_bytes()
    for w, l in zip(workspaces, loss_outs):
        if not (w.is_cuda and w.device == dev and w.dtype == torch.uint8 and w.numel() >= need) or l.numel() != 1:
            raise RuntimeError(f"{who}: workspaces from l1_workspace(), one-element loss tensors")
    _lib.launch("fr_l1_loss_grad_batch", dev, len(imgs), n, _ptrs(imgs), _ptrs(gts), _ptrs(grad_outs), _ptrs(loss_outs), _ptrs(workspaces))
    return loss_outs, grad_outs


# ---- FlashAvatar's Huber image term (FlashAvatarLoss, train/loss.py:217-221, :231-239): ONE launch (`fr_huber_loss_grad`) gives the
# three loss words and the gradient autograd would hand to the rasterizer
class HuberLoss(NamedTuple):
    """The Huber term's threshold and the weight of its mouth-mask term: the reference has 0.1 and 40 (train/loss.py:231-239)."""
    alpha: float = 0.1
    mask_weight: float = 40.0


REFERENCE_HUBER_LOSS = HuberLoss(0.1, 40.0)

def huber_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `huber_loss_and_grad(..., workspace=)`."""
    return _huber_ws.fresh(dev)


def huber_loss_and_grad(img: torch.Tensor, gt: torch.Tensor, terms=REFERENCE_HUBER_LOSS, mask: Optional[torch.Tensor] = None,
                        loss_out: Optional[torch.Tensor] = None, grad_out: Optional[torch.Tensor] = None,
                        workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """FlashAvatar's image term of `img` against `gt` ([C,H,W] or [1,C,H,W]) in ONE launch: returns the 3-element device tensor
    (huber + terms.mask_weight * mouth, huber, mouth) and the gradient of its first word with respect to `img`, of `img`'s
    shape.  huber = mean h(img - gt) with h(x) = 0.5 x^2 below |x| = terms.alpha and alpha (|x| - alpha / 2) from there on;
    mouth = mean h(mask * (img - gt)) for a `mask` [1,H,W] or [H,W] with values in [0,1], broadcast over the channels (None: no
    mouth term, the word is 0).  `loss_out` / `grad_out`: write into these tensors instead of fresh ones (buffers of a captured
    step).  `workspace`: scratch from `huber_workspace()`; by default one is kept per (device, current stream) — launches that
    may overlap must not share one.  The losses without the gradient: `grad_out=False`.  There is no CPU path."""
    who = "huber_loss_and_grad"
    img, gt, dev = _image_pair(img, gt, who)
    Cn, H, W = _chw(img, who)
    alpha, mask_weight = float(terms[0]), float(terms[1])
    if not alpha > 0.0:
        raise ValueError(f"{who}: alpha must be > 0")
    if mask is not None:
        if not mask.is_cuda or mask.device != dev or mask.numel() != H * W or tuple(mask.shape[-2:]) != (H, W):
            raise RuntimeError(f"{who}: the mask is [1,{H},{W}] or [{H},{W}] on the image's device")
        mask = _f32c(mask.detach())
    grad, loss = _outputs(img, 3, grad_out, loss_out, who)
    ws = _huber_ws.resolve(dev, workspace, who)
    cfg = _lib.fr_huber_config(alpha, mask_weight)
    _lib.launch("fr_huber_loss_grad", dev, C.byref(cfg), Cn, H, W, img.data_ptr(), gt.data_ptr(),
                mask.data_ptr() if mask is not None else None, grad.data_ptr() if grad is not None else None, loss.data_ptr(),
                ws.data_ptr())
    return loss, grad


# ---- SplattingAvatar's image term (SplattingAvatarLoss, train/loss.py:279-283, :288-304): ONE launch (`fr_pixel_loss_grad`) gives the
# three loss words and the gradient autograd would hand to the rasterizer
class PixelLoss(NamedTuple):
    """Weights of SplattingAvatar's image term: loss = rgb_weight * L1 + mse_weight * MSE (config/splattingavatar.yaml:13-20 has
    1.0 and 10.0)."""
    rgb_weight: float = 1.0
    mse_weight: float = 10.0


def pixel_loss_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `pixel_loss_and_grad(..., workspace=)`."""
    return _pixel_ws.fresh(dev)


def pixel_loss_and_grad(img: torch.Tensor, gt: torch.Tensor, weights=PixelLoss(), loss_out: Optional[torch.Tensor] = None,
                        grad_out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """SplattingAvatar's image term of `img` against `gt` ([C,H,W] or [1,C,H,W]) in ONE launch: `weights` = (rgb_weight,
    mse_weight), e.g. a `PixelLoss`; returns the 3-element device tensor (rgb_weight * l1 + mse_weight * mse, l1, mse) — the last
    two unweighted means over all C H W values — and the gradient of its first word with respect to `img`, of `img`'s shape:
    rgb_weight * sign(img - gt) / n + mse_weight * 2 (img - gt) / n.  The l1 word is `l1_loss_and_grad`'s loss, bit for bit.
    `loss_out` / `grad_out`: write into these tensors instead of fresh ones (buffers of a captured step).  `workspace`: scratch
    from `pixel_loss_workspace()`; by default one is kept per (device, current stream) — launches that may overlap must not
    share one.  The losses without the gradient: `grad_out=False`.  There is no CPU path."""
    who = "pixel_loss_and_grad"
    img, gt, dev = _image_pair(img, gt, who)
    Cn, H, W = _chw(img, who)
    cfg = _lib.fr_pixel_loss_config(float(weights[0]), float(weights[1]))
    grad, loss = _outputs(img, 3, grad_out, loss_out, who)
    ws = _pixel_ws.resolve(dev, workspace, who)
    _lib.launch("fr_pixel_loss_grad", dev, C.byref(cfg), Cn, H, W, img.data_ptr(), gt.data_ptr(),
                grad.data_ptr() if grad is not None else None, loss.data_ptr(), ws.data_ptr())
    return loss, grad


# ---- SplattingAvatar's scale term (SplattingAvatarLoss, train/loss.py:307-315): two launches (`fr_scale_term`) give the unweighted
# loss with the number of selected rows and add the weighted gradient into dL/d_scaling
class ScaleTerm(NamedTuple):
    """SplattingAvatar's scale term: its weight and the two gates of its row selection (config/splattingavatar.yaml:13-20 has
    scale_loss 1.0, scale_threshold 10.0, max_scaling 0.008)."""
    weight: float = 1.0
    scale_threshold: float = 10.0
    max_scaling: float = 0.008


def scale_term_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `scale_term_and_grad(..., workspace=)`."""
    return _scale_ws.fresh(dev)


def scale_term_and_grad(scaling: torch.Tensor, d_scaling: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
                        terms=ScaleTerm(), workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SplattingAvatar's scale term (train/loss.py:307-315) on the raw `_scaling` [P,3] (`fr_scale_term`): with scale =
    exp(scaling), a row is selected if its largest component is > terms.max_scaling and more than terms.scale_threshold times
    its smallest; returns `out` = (mean of the largest component over the selected rows — 0 if there is none —, the number
    of selected rows), UNWEIGHTED, a 2-element device tensor, and ADDS terms.weight * d scale_loss / d _scaling into `d_scaling`
    ([P,3] gradient buffer: one entry per selected row, its largest component's; None, or a weight of 0: no gradient traffic).
    A row with a NaN is not selected.  `workspace`: scratch from `scale_term_workspace()`; by default one is kept per (device,
    current stream) — launches that may overlap must not share one.  There is no CPU path."""
    if not scaling.is_cuda:
        raise RuntimeError("scale_term_and_grad needs device tensors (there is no CPU path)")
    dev = scaling.device
    P = int(scaling.shape[0])
    scaling = scaling.detach()
    _check_rows3("scale_term_and_grad", dev, P, (scaling, d_scaling), "[P,3] tensors of one device")
    loss = _out_words("scale_term_and_grad", out, 2, dev, "parameters'", fresh=torch.zeros)   # (P == 0 launches nothing)
    ws = _scale_ws.resolve(dev, workspace, "scale_term_and_grad")
    cfg = _lib.fr_scale_term_config(float(terms[0]), float(terms[1]), float(terms[2]))
    _lib.launch("fr_scale_term", dev, C.byref(cfg), P, scaling.data_ptr() if P else None,
                d_scaling.data_ptr() if d_scaling is not None and P else None, loss.data_ptr(), ws.data_ptr())
    return loss


# ---- FateAvatar's scale-ratio term (FateAvatarLoss, train/loss.py:144-151): ONE launch (`fr_scale_ratio_term`) gives the unweighted
# loss with the number of rows over the threshold and adds the weighted gradient into dL/d_scaling
class ScaleRatioTerm(NamedTuple):
    """FateAvatar's scale term: its weight and the ratio a row's largest scale may have to its smallest before the term acts
    (config/fateavatar.yaml:13-25 has scale_loss 0.1, scale_threshold 9.0)."""
    weight: float = 0.1
    scale_threshold: float = 9.0


def scale_ratio_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `scale_ratio_term_and_grad(..., workspace=)`."""
    return _ratio_ws.fresh(dev)


def scale_ratio_term_and_grad(scaling: torch.Tensor, d_scaling: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
                              terms=ScaleRatioTerm(), workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FateAvatar's scale term (train/loss.py:144-151) on the raw `_scaling` [P,3] in ONE launch (`fr_scale_ratio_term`): with
    scale = exp(scaling) and ratio = scale.max(-1) / scale.min(-1), returns `out` = (mean over all P rows of relu(ratio -
    terms.scale_threshold), the number of rows over the threshold), UNWEIGHTED, a 2-element device tensor, and ADDS terms.weight *
    d scale_loss / d _scaling into `d_scaling` ([P,3] gradient buffer: +weight / P * ratio on a row's largest component, the
    same subtracted from its smallest, the first of equal components; None, or a weight of 0: no gradient traffic).  A row
    whose ratio is not finite (a NaN, an overflowing exp, a smallest scale that underflows to 0) adds nothing anywhere.
    `workspace`: scratch from `scale_ratio_workspace()`; by default one is kept per (device, current stream) — launches that
    may overlap must not share one.  There is no CPU path."""
    if not scaling.is_cuda:
        raise RuntimeError("scale_ratio_term_and_grad needs device tensors (there is no CPU path)")
    dev = scaling.device
    P = int(scaling.shape[0])
    scaling = scaling.detach()
    _check_rows3("scale_ratio_term_and_grad", dev, P, (scaling, d_scaling), "[P,3] tensors of one device")
    loss = _out_words("scale_ratio_term_and_grad", out, 2, dev, "parameters'", fresh=torch.zeros)   # (P == 0 launches nothing)
    ws = _ratio_ws.resolve(dev, workspace, "scale_ratio_term_and_grad")
    cfg = _lib.fr_scale_ratio_config(float(terms[0]), float(terms[1]))
    _lib.launch("fr_scale_ratio_term", dev, C.byref(cfg), P, scaling.data_ptr() if P else None,
                d_scaling.data_ptr() if d_scaling is not None and P else None, loss.data_ptr(), ws.data_ptr())
    return loss


class _ScaleRatio(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, scale_threshold):
        s = _f32c(scaling.detach())
        grad = torch.zeros_like(s) if ctx.needs_input_grad[0] else None     # None: the loss only
        loss = scale_ratio_term_and_grad(s, grad, terms=ScaleRatioTerm(1.0, scale_threshold))
        if grad is not None:
            ctx.save_for_backward(grad)
        ctx.in_dtype = scaling.dtype
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return (grad * grad_output).to(ctx.in_dtype), None


def scale_ratio_loss(scaling: torch.Tensor, scale_threshold: float = 9.0) -> torch.Tensor:
    """FateAvatar's scale expression — also `UVDecoderLoss`'s scale term on a baked avatar's decoded log-scales
    (train/loss.py:597-604) — as a 0-dim tensor, UNWEIGHTED: relu(exp(scaling).max(-1) / exp(scaling).min(-1) -
    scale_threshold).mean(), differentiable with respect to `scaling` [P,3] (the fused kernel's gradient with weight 1, scaled
    by the incoming one), with `scale_ratio_term_and_grad`'s rules for ties and non-finite rows."""
    if scaling.dim() != 2 or scaling.shape[-1] != 3:
        raise RuntimeError(f"scale_ratio_loss: log-scales are [P,3], got {tuple(scaling.shape)}")
    return _ScaleRatio.apply(scaling, float(scale_threshold))


# ---- the baking objective's rotation term (UVDecoderLoss, train/loss.py:612-617): ONE launch (`fr_rot_term`) gives the
# unweighted loss and adds the weighted gradient into dL/d(decoded rotation)
def rot_term_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `rot_term_and_grad(..., workspace=)`."""
    return _rot_ws.fresh(dev)


def rot_term_and_grad(rotation: torch.Tensor, d_rotation: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
                      weight: float = 0.1, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Neural baking's rot_loss (train/loss.py:612-617) on the decoded rotation rows [N,4] in ONE launch (`fr_rot_term`): with
    raw = quaternion_to_axis_angle(rotation) (pytorch3d 0.7.7's formula; element 0 of a row is taken for the real part, as
    the reference runs it on its shuffled rows), returns `out` = mean(raw[:,0]^2) + mean(raw[:,2]^2), UNWEIGHTED, a 1-element
    device tensor, and ADDS weight * d rot_loss / d rotation into `d_rotation` ([N,4] gradient buffer; None, or a weight of 0:
    no gradient traffic).  A row whose vector part is 0 passes no gradient through the norm (autograd's rule).  `workspace`:
    scratch from `rot_term_workspace()`; by default one is kept per (device, current stream) — launches that may overlap must
    not share one.  There is no CPU path."""
    who = "rot_term_and_grad"
    if not rotation.is_cuda:
        raise RuntimeError(f"{who} needs device tensors (there is no CPU path)")
    dev, N = rotation.device, int(rotation.shape[0])
    rotation = rotation.detach()
    for t in (rotation, d_rotation):
        if t is not None and (t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (N, 4)):
            raise RuntimeError(f"{who}: contiguous float32 [N,4] tensors of one device")
    loss = _out_words(who, out, 1, dev, "rotations'", fresh=torch.zeros)   # (N == 0 launches nothing)
    ws = _rot_ws.resolve(dev, workspace, who)
    _lib.launch("fr_rot_term", dev, float(weight), N, rotation.data_ptr() if N else None,
                d_rotation.data_ptr() if d_rotation is not None and N else None, loss.data_ptr(), ws.data_ptr())
    return loss


class _RotLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rotation):
        r = _f32c(rotation.detach())
        grad = torch.zeros_like(r) if ctx.needs_input_grad[0] else None     # None: the loss only
        loss = rot_term_and_grad(r, grad, weight=1.0)
        if grad is not None:
            ctx.save_for_backward(grad)
        ctx.in_dtype = rotation.dtype
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return (grad * grad_output).to(ctx.in_dtype)


def rot_loss(rotation: torch.Tensor) -> torch.Tensor:
    """`rot_term_and_grad`'s expression as a 0-dim tensor, UNWEIGHTED, differentiable with respect to `rotation` [N,4] (the
    fused kernel's gradient with weight 1, scaled by the incoming one)."""
    if rotation.dim() != 2 or rotation.shape[-1] != 4:
        raise RuntimeError(f"rot_loss: rotations are [N,4], got {tuple(rotation.shape)}")
    return _RotLoss.apply(rotation)


def regulariser_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `gaussian_regularisers(..., workspace=)`."""
    return _reg_ws.fresh(dev)


def gaussian_regularisers(scaling: torch.Tensor, xyz: torch.Tensor, d_scaling: Optional[torch.Tensor],
                          d_xyz: Optional[torch.Tensor], out: Optional[torch.Tensor] = None, weights=(1.0, 0.01),
                          thresholds=(0.6, 1.0), workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GaussianAvatars' scale and xyz regularisers (train/loss.py:367-379) on the raw `_scaling` / `_xyz` [P,3] in ONE launch
    (`fr_gaussian_regularise`): returns `out` = (scale_loss, xyz_loss), UNWEIGHTED, a 2-element device tensor, and ADDS
    `weights[0] * d scale_loss / d _scaling` into `d_scaling` and `weights[1] * d xyz_loss / d _xyz` into `d_xyz` ([P,3]
    gradient buffers; None: that gradient is not wanted; a weight of 0 leaves its buffer untouched).  `thresholds`:
    (threshold_scale, threshold_xyz).  `workspace`: scratch from `regulariser_workspace()`; by default one is kept per
    (device, current stream) — launches that may overlap must not share one.  There is no CPU path."""
    if not (scaling.is_cuda and xyz.is_cuda):
        raise RuntimeError("gaussian_regularisers needs device tensors (there is no CPU path)")
    dev = scaling.device
    P = int(scaling.shape[0])
    scaling, xyz = scaling.detach(), xyz.detach()
    _check_rows3("gaussian_regularisers", dev, P, (scaling, xyz, d_scaling, d_xyz), "[P,3] tensors of one device")
    loss = _out_words("gaussian_regularisers", out, 2, dev, "parameters'")
    ws = _reg_ws.resolve(dev, workspace, "gaussian_regularisers")
    cfg = _lib.fr_regularise_config(float(weights[0]), float(weights[1]), float(thresholds[0]), float(thresholds[1]))
    _lib.launch("fr_gaussian_regularise", dev, C.byref(cfg), P, scaling.data_ptr(), xyz.data_ptr(),
                d_scaling.data_ptr() if d_scaling is not None else None, d_xyz.data_ptr() if d_xyz is not None else None,
                loss.data_ptr(), ws.data_ptr())
    return loss


# ---- FateAvatar's mesh terms (FateAvatarLoss, train/loss.py:112-121, :166-180, :192-197): ONE launch (`fr_mesh_terms`) gives
# both unweighted losses and adds their weighted gradient into dL/dposed_verts
class MeshTerms(NamedTuple):
    """Weights of FateAvatar's two mesh terms: config/fateavatar.yaml:23 has laplacian_loss 100000.0, flame_loss 0."""
    laplacian_weight: float = 1e5
    flame_weight: float = 0.0


REFERENCE_MESH_TERMS = MeshTerms()

def mesh_terms_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `mesh_terms_and_grad(..., workspace=)`."""
    return _mesh_ws.fresh(dev)


def mesh_terms_and_grad(verts: torch.Tensor, verts_orig: torch.Tensor, lap, terms=REFERENCE_MESH_TERMS,
                        d_verts: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                        workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FateAvatar's Laplacian-smoothing and FLAME-distance terms of the mesh `verts` [V,3] against `verts_orig` [V,3] in ONE
    launch (`fr_mesh_terms`): returns `out` = (laplacian_loss, flame_loss), UNWEIGHTED, a 2-element device tensor, and ADDS
    terms.laplacian_weight * d laplacian_loss / d verts + terms.flame_weight * d flame_loss / d verts into `d_verts` [V,3]
    (None: losses only; a weight of 0 skips its term, both 0 leave the buffer untouched).  `lap`: the mesh's
    `binding.mesh_laplacian(faces, V)` on the vertices' device.  `workspace`: scratch from `mesh_terms_workspace()`; by
    default one is kept per (device, current stream) — launches that may overlap must not share one.  There is no CPU path."""
    if not (verts.is_cuda and verts_orig.is_cuda):
        raise RuntimeError("mesh_terms_and_grad needs device tensors (there is no CPU path)")
    dev = verts.device
    V = int(lap.V)
    verts, verts_orig = verts.detach(), verts_orig.detach()
    _check_rows3("mesh_terms_and_grad", dev, V, (verts, verts_orig, d_verts), "[V,3] tensors of one device, V that of the Laplacian")
    for t, n in ((lap.row_ptr, V + 1), (lap.col, None)):
        if t.device != dev or t.dtype != torch.int32 or not t.is_contiguous() or t.dim() != 1 or (n is not None and t.numel() != n):
            raise RuntimeError("mesh_terms_and_grad: `lap` is a binding.mesh_laplacian() on the vertices' device")
    loss = _out_words("mesh_terms_and_grad", out, 2, dev, "vertices'")
    ws = _mesh_ws.resolve(dev, workspace, "mesh_terms_and_grad")
    cfg = _lib.fr_mesh_terms_config(float(terms[0]), float(terms[1]))
    # (a mesh without edges has an empty `col` nobody reads; the entry point refuses NULL, and an empty tensor has no address)
    col = lap.col if lap.col.numel() else lap.row_ptr
    nz = lambda t: t.data_ptr() if t.numel() else ws.data_ptr()   # noqa: E731  (V == 0: nothing is launched)
    _lib.launch("fr_mesh_terms", dev, C.byref(cfg), V, nz(verts), nz(verts_orig), lap.row_ptr.data_ptr(), col.data_ptr(),
                d_verts.data_ptr() if d_verts is not None else None, loss.data_ptr(), ws.data_ptr())
    return loss


class _LaplacianSmoothing(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, verts_orig, lap):
        shape = verts.shape
        v = verts.detach().float().reshape(-1, 3).contiguous()
        o = verts_orig.detach().float().reshape(-1, 3).contiguous()
        grad = torch.zeros_like(v) if ctx.needs_input_grad[0] else None     # None: the loss only
        loss = mesh_terms_and_grad(v, o, lap, MeshTerms(1.0, 0.0), d_verts=grad)
        if grad is not None:
            ctx.save_for_backward(grad.view(shape))
        ctx.in_dtype = verts.dtype
        return loss[0].clone()

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return (grad * grad_output).to(ctx.in_dtype), None, None


def laplacian_smoothing_loss(verts_orig: torch.Tensor, verts: torch.Tensor, lap) -> torch.Tensor:
    """`FateAvatarLoss.get_laplacian_smoothing_loss(verts_orig, verts)` (train/loss.py:166-180), the reference's argument
    order, with the mesh's `binding.mesh_laplacian` where the reference builds the dense matrix: ((L verts - L verts_orig)^2)
    .sum(-1, keepdim=True).mean() as a 0-dim tensor, differentiable with respect to `verts` (the fused kernel's gradient,
    scaled by the incoming one).  [V,3] or [1,V,3].  `verts_orig` takes no gradient (the reference detaches it)."""
    for t in (verts, verts_orig):
        if not (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)) or t.shape[-1] != 3:
            raise RuntimeError(f"laplacian_smoothing_loss: vertices are [V,3] or [1,V,3], got {tuple(t.shape)}")
    return _LaplacianSmoothing.apply(verts, verts_orig.detach(), lap)


_copy_calls = {}   # (dst ptr, src ptr, floats) per pair -> the prepared argument arrays of fr_multi_copy


def multi_copy(pairs) -> None:
    """`dst.copy_(src)` for up to twelve (dst, src) pairs of contiguous float32 device tensors in ONE launch
    (`fr_multi_copy`): the per-frame inputs of a captured step (of every frame of a batch).  A step calls this with the
    same few sets of tensors over and over (its static buffers, the frames of a resident sequence): the ctypes argument
    arrays of a set are made once and looked up by the tensors' addresses afterwards — this call is on the host's critical
    path of a 130 us step."""
    pairs = [(d, s) for d, s in pairs if d.numel()]
    if not pairs:
        return
    if len(pairs) > 12:
        raise RuntimeError("multi_copy: at most twelve pairs")
    dev = pairs[0][0].device
    f32 = torch.float32
    for d, s in pairs:
        if not (d.is_cuda and s.is_cuda and d.device == dev and s.device == dev):
            raise RuntimeError("multi_copy needs tensors of one device")
        if d.dtype is not f32 or s.dtype is not f32 or not d.is_contiguous() or not s.is_contiguous() or d.numel() != s.numel():
            raise RuntimeError("multi_copy: contiguous float32 tensors of equal size")
    key = tuple((d.data_ptr(), s.data_ptr(), d.numel()) for d, s in pairs)
    call = _copy_calls.get(key)
    if call is None:
        n = len(pairs)
        call = (n, (C.c_void_p * n)(*[d.data_ptr() for d, _ in pairs]), (C.c_void_p * n)(*[s.data_ptr() for _, s in pairs]),
                (C.c_uint64 * n)(*[d.numel() for d, _ in pairs]))
        if len(_copy_calls) > 4096:     # (addresses are only a key while their tensors live: bounded, rebuilt on demand)
            _copy_calls.clear()
        _copy_calls[key] = call
    n, dst, src, cnt = call
    # (not `_lib.launch`: the raw handle of the device's current stream without building a torch.cuda.Stream object, and no
    # device guard where the device is current: 5 us of a host path that has to stay under the step's 130 us)
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    stream = raw(dev.index) if raw is not None else torch.cuda.current_stream(dev).cuda_stream
    if torch.cuda.current_device() == dev.index:
        rc = _lib.lib().fr_multi_copy(n, dst, src, cnt, stream)
    else:
        with torch.cuda.device(dev):
            rc = _lib.lib().fr_multi_copy(n, dst, src, cnt, stream)
    _lib.check(rc, "fr_multi_copy")


def scaled_sum(dst: torch.Tensor, srcs, scale: float) -> torch.Tensor:
    """dst = scale * sum(srcs) for 1 .. 4 contiguous float32 device tensors of dst's size, in ONE pass (`fr_scaled_sum`):
    the mean of the gradient buffers of the views a rank rendered in flight together."""
    srcs = list(srcs)
    if not 1 <= len(srcs) <= _lib.FR_ADAM_MAX_GRADS:
        raise RuntimeError(f"scaled_sum: 1..{_lib.FR_ADAM_MAX_GRADS} sources")
    dev = dst.device
    for t in [dst] + srcs:
        if not t.is_cuda or t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != dst.numel():
            raise RuntimeError("scaled_sum: contiguous float32 tensors of one device and one size")
    _lib.launch("fr_scaled_sum", dev, len(srcs), _ptrs(srcs), dst.data_ptr(), dst.numel(), float(scale))
    return dst


# ---- L1 + D-SSIM (GaussianAvatarsLoss, train/loss.py:351-365; d_ssim of tools/loss_utils/dssim.py:28-56): two launches of
# the HIP library (`fr_image_loss_grad`) give the three loss scalars and the gradient autograd would hand to the rasterizer
class ImageLoss(NamedTuple):
    """Weights of the image term: loss = rgb_weight * L1 + dssim_weight * d_ssim (config/gaussianavatars.yaml:16-20 has
    0.8 and 0.2, the original 3DGS mix)."""
    rgb_weight: float
    dssim_weight: float


def _image_bytes(C: int, H: int, W: int) -> int:
    if min(int(C), int(H), int(W)) < 1:
        raise RuntimeError("image_loss_workspace: C, H, W >= 1")
    return _lib.lib().fr_image_loss_workspace_bytes(int(C), int(H), int(W))


# (its size depends on the image: the stream's own is grown to the largest shape asked for — one buffer per stream, not one per
# shape: the maps take 12 bytes per pixel and channel)
_image_ws = StreamWorkspace("image_loss_workspace", _image_bytes, "images'", first="the first call for this image size",
                            maker_args="device, C, H, W")
_image_workspace = _image_ws.kept   # (device index, stream handle) -> workspace of fr_image_loss_grad


def ssim_window() -> torch.Tensor:
    """The eleven 1-D taps of d_ssim's window, `gaussian(11, 1.5)` of dssim.py:18-20 in its float32 arithmetic (CPU tensor)."""
    out = (C.c_float * 11)()
    _lib.lib().fr_ssim_window(out)
    return torch.tensor(list(out), dtype=torch.float32)


def image_loss_workspace(dev: torch.device, C: int, H: int, W: int) -> torch.Tensor:
    """A fresh zeroed workspace for `image_loss_and_grad(..., workspace=)` on [C,H,W] images."""
    _image_bytes(C, H, W)   # (the shape is refused before the device)
    return _image_ws.fresh(dev, C, H, W)


def _chw(t: torch.Tensor, what: str):
    if t.dim() == 4 and t.shape[0] == 1:
        return tuple(t.shape[1:])
    if t.dim() != 3:
        raise RuntimeError(f"{what}: images are [C,H,W] or [1,C,H,W], got {tuple(t.shape)}")
    return tuple(t.shape)


def image_loss_and_grad_batch(imgs, gts, weights, loss_outs, grad_outs, workspaces):
    """`image_loss_and_grad` for the images of the 1 .. 4 frames of a batch in ONE launch pair (`fr_image_loss_grad`): lists of
    equally-shaped contiguous float32 device tensors; every image has its own 3-element loss tensor, gradient buffer (an
    entry may be None: losses only) and workspace (`image_loss_workspace()`).  Returns (loss_outs, grad_outs)."""
    who = "image_loss_and_grad_batch"
    imgs, tensors, dev = _image_lists(who, imgs, gts, loss_outs, grad_outs, workspaces)
    shape = _chw(imgs[0], who)
    for t in tensors:
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or _chw(t, who) != shape:
            raise RuntimeError(f"{who}: contiguous float32 tensors of one device and one shape")
    need = _lib.lib().fr_image_loss_workspace_bytes(*shape)
    for w, l in zip(workspaces, loss_outs):
        if not (w.is_cuda and w.device == dev and w.dtype == torch.uint8 and w.numel() >= need):
            raise RuntimeError(f"{who}: workspace must come from image_loss_workspace() for this image shape "
                               f"on the images' device ({need} bytes)")
        if not (l.is_cuda and l.device == dev and l.dtype == torch.float32 and l.numel() == 3 and l.is_contiguous()):
            raise RuntimeError(f"{who}: contiguous 3-element float32 loss tensors on the images' device")
    cfg = _lib.fr_image_loss_config(float(weights[0]), float(weights[1]))
    _lib.launch("fr_image_loss_grad", dev, C.byref(cfg), len(imgs), shape[0], shape[1], shape[2], _ptrs(imgs), _ptrs(gts),
                _ptrs(grad_outs), _ptrs(loss_outs), _ptrs(workspaces))
    return loss_outs, grad_outs


def image_loss_and_grad(img: torch.Tensor, gt: torch.Tensor, weights, loss_out: Optional[torch.Tensor] = None,
                        grad_out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`weights` = (rgb_weight, dssim_weight), e.g. an `ImageLoss`: returns the 3-element device tensor
    (rgb_weight * l1 + dssim_weight * d_ssim, l1, d_ssim) — the last two unweighted — and the gradient of the first with
    respect to `img`, of `img`'s shape.  `img`, `gt`: [C,H,W] or [1,C,H,W].  `loss_out` / `grad_out`: write into these
    tensors instead of fresh ones (buffers of a captured step).  `workspace`: scratch from `image_loss_workspace()`; by
    default one is kept per (device, current stream) — launches that may overlap must not share one.  The losses without the
    gradient: `image_loss_and_grad_batch` with a None gradient entry."""
    img, gt, dev = _image_pair(img, gt, "image_loss_and_grad")
    shape = _chw(img, "image_loss_and_grad")
    grad, loss = _outputs(img, 3, grad_out, loss_out, "image_loss_and_grad")
    # (a caller's workspace is checked by image_loss_and_grad_batch, which names the bytes this shape takes)
    ws = workspace if workspace is not None else _image_ws.resolve(dev, None, "image_loss_and_grad", need=shape)
    image_loss_and_grad_batch([img], [gt], weights, [loss], [grad], [ws])
    return loss, grad


class _DSsim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        x, y, _ = _image_pair(img1, img2, "d_ssim")
        grad = torch.empty_like(x) if ctx.needs_input_grad[0] else None     # None: losses only, pass 2 is not launched
        loss = torch.empty(3, dtype=torch.float32, device=x.device)
        image_loss_and_grad_batch([x], [y], (0.0, 1.0), [loss], [grad], [_image_ws.resolve(x.device, None, "d_ssim", need=_chw(x, "d_ssim"))])
        if grad is not None:
            ctx.save_for_backward(grad.view(img1.shape))
        ctx.in_dtype = img1.dtype
        return loss[2].clone()

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return (grad * grad_output).to(ctx.in_dtype), None


def d_ssim(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """`d_ssim` of the reference (tools/loss_utils/dssim.py:28-56; window 11, averaged): 1 - mean SSIM map as a 0-dim tensor,
    differentiable with respect to `img1` (the fused kernels' gradient, scaled by the incoming one).  The target takes no
    gradient: `img2.requires_grad` raises."""
    if img2.requires_grad:
        raise RuntimeError("d_ssim: the target (img2) takes no gradient; detach it")
    return _DSsim.apply(img1, img2)
