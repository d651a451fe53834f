"""FlashAvatar's deformation MLP on the fused path: the embedding of the canonical points and the ReLU network that turns
(embedded point, this frame's condition) into the ten raw deformation outputs of every Gaussian.

reference:
  * `Embedder` (model/baseline/flashavatar.py:396-430): [x, sin(x 2^0), cos(x 2^0), sin(x 2^1), cos(x 2^1), ...], each a block of
    the point's three coordinates — `embed_points`
  * `MLP` (:434-464): `fcs` = Linear(in, 256) + (hidden_layers - 1) x Linear(256, 256), ReLU after each, then `output_linear`
    Linear(256, out) — `DeformMLP`; the network is fed cat([embedded canonical points, cond.repeat(N, 1)]) (:238-240) with
    cond = [expression, jaw pose, eyes pose] and its output goes through tanh (:243), which stays with the binding
  * its optimizer: Adam(deformNet.parameters(), lr=deformer_lr) (train/optim.py:55-59) — `FlashStep(deformer=...)`
What is fused: fr_mlp_forward / fr_mlp_backward (csrc/fr_mlp.hip) — every product an exact-f32 MFMA GEMM, the condition half of
the first layer folded into its bias instead of being repeated per point, weight gradients summed in fixed chunks (the same
bits on every launch).  The weights live in ONE flat buffer in nn.Linear's own layout, so that one FusedAdam launch updates
them and a reference checkpoint's `deformNet.*` entries copy in and out as they are.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

WIDTH = _lib.FR_MLP_WIDTH
PREFIX = "deformNet."      # the network's name inside the reference model's state_dict


def embed_points(points: torch.Tensor, n_freqs: int = 8) -> torch.Tensor:
    """`Embedder(N_freqs=n_freqs)(points)` (:396-430) for points [N,3]: [N, 3 (1 + 2 n_freqs)] in the reference's column order —
    x, then for every frequency 2^0 .. 2^(n_freqs-1) sin(x f) and cos(x f).  Plain torch: it runs once, at construction."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("embed_points: points must be [N,3]")
    if int(n_freqs) < 0:
        raise ValueError("embed_points: n_freqs >= 0")
    cols = [points]
    if n_freqs > 0:
        for freq in 2.0 ** torch.linspace(0.0, n_freqs - 1, steps=int(n_freqs)):   # (log sampling, as the reference's)
            cols += [torch.sin(points * freq), torch.cos(points * freq)]
    return torch.cat(cols, dim=1)


def layer_shapes(in_dim: int, layers: int, out_dim: int):
    """[(out, in)] of the network's layers in order, the output layer last."""
    return [(WIDTH, in_dim)] + [(WIDTH, WIDTH)] * (layers - 1) + [(out_dim, WIDTH)]


def check_shape(point_dim: int, cond_dim: int, layers: int, out_dim: int, width: int = WIDTH) -> None:
    """The limits of the kernels (include/fr_rasterizer.h), checked on the host before anything touches the device."""
    if int(width) != WIDTH:
        raise ValueError(f"DeformMLP: hidden width {width} is not built (the kernels' width is {WIDTH}, a compile-time constant)")
    if not 1 <= int(layers) <= _lib.FR_MLP_MAX_LAYERS:
        raise ValueError(f"DeformMLP: 1 .. {_lib.FR_MLP_MAX_LAYERS} hidden layers, not {layers}")
    if int(point_dim) < 1 or int(cond_dim) < 0 or int(point_dim) + int(cond_dim) > WIDTH:
        raise ValueError(f"DeformMLP: point features >= 1, cond_dim >= 0 and their sum <= {WIDTH} "
                         f"(got {point_dim} + {cond_dim})")
    if not 1 <= int(out_dim) <= _lib.FR_MLP_MAX_OUT:
        raise ValueError(f"DeformMLP: 1 .. {_lib.FR_MLP_MAX_OUT} output columns, not {out_dim}")


class _MLPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, cond, mlp):
        out = torch.empty((mlp.N, mlp.out_dim), dtype=torch.float32, device=flat.device)
        cond = cond.detach().contiguous()
        mlp.forward_into(cond, out)
        ctx.mlp, ctx.cond = mlp, cond
        return out

    @staticmethod
    def backward(ctx, g):
        mlp = ctx.mlp
        d_cond = torch.zeros_like(ctx.cond)
        mlp.backward_from(g.contiguous(), ctx.cond, d_cond)
        return mlp.flat_grad.clone(), d_cond, None


class DeformMLP:
    """The deformation network over N fixed points.  `point_features` [N,De]: the per-point half of every input row (the
    embedded canonical points, `embed_points`), a constant: it gets no gradient.  `cond_dim`: the length of the frame's
    condition vector.  `flat` (a leaf that requires grad) holds every layer's weight [out,in] then bias [out] in nn.Linear's
    layout, `flat_grad` the same layout of gradients — what the kernels OVERWRITE on every backward; `weight(i)` / `bias(i)`
    (and `grad_weight` / `grad_bias`) are views of layer i, the output layer being layer `layers`.  Initialised as nn.Linear
    does, drawing from torch's generator in the order the reference's `MLP.__init__` does."""

    def __init__(self, point_features: torch.Tensor, cond_dim: int, layers: int = 6, out_dim: int = 10, width: int = WIDTH):
        if point_features.dim() != 2:
            raise ValueError("DeformMLP: point_features must be [N,De]")
        check_shape(point_features.shape[1], cond_dim, layers, out_dim, width)
        if point_features.dtype != torch.float32:
            raise TypeError("DeformMLP: point_features must be float32")
        if point_features.requires_grad:
            raise ValueError("DeformMLP: point_features is a constant of the network (a registered buffer in the reference); "
                             "a tensor that requires grad would get none")
        self.point_features = point_features.detach().contiguous()
        self.N, self.point_dim = int(point_features.shape[0]), int(point_features.shape[1])
        self.cond_dim, self.layers, self.out_dim = int(cond_dim), int(layers), int(out_dim)
        self.in_dim = self.point_dim + self.cond_dim
        self.shapes = layer_shapes(self.in_dim, self.layers, self.out_dim)
        dev = self.point_features.device
        mods = [torch.nn.Linear(i, o) for o, i in self.shapes]      # (nn.Linear's default initialisation, in MLP.__init__'s order)
        flat = torch.cat([t.detach().reshape(-1) for m in mods for t in (m.weight, m.bias)])
        self.flat = flat.to(dev).contiguous().requires_grad_(True)
        self.flat_grad = torch.zeros_like(self.flat, requires_grad=False)
        self._offsets, o = [], 0
        for out, inn in self.shapes:
            self._offsets.append(o)
            o += out * inn + out
        assert o == self.flat.numel()
        self._workspace = None

    # ---- per-layer views
    def _view(self, buf, i, bias):
        out, inn = self.shapes[i]
        o = self._offsets[i]
        return buf[o + out * inn:o + out * inn + out] if bias else buf[o:o + out * inn].view(out, inn)

    def weight(self, i: int) -> torch.Tensor:
        return self._view(self.flat.detach(), i, False)

    def bias(self, i: int) -> torch.Tensor:
        return self._view(self.flat.detach(), i, True)

    def grad_weight(self, i: int) -> torch.Tensor:
        return self._view(self.flat_grad, i, False)

    def grad_bias(self, i: int) -> torch.Tensor:
        return self._view(self.flat_grad, i, True)

    def parameters(self):
        return [self.flat]

    # ---- the reference's names: fcs.{i}.weight / .bias, output_linear.weight / .bias (inside the model: deformNet. + these)
    def _names(self, prefix=""):
        return [f"{prefix}fcs.{i}" for i in range(self.layers)] + [f"{prefix}output_linear"]

    @torch.no_grad()
    def state_dict(self, prefix: str = "") -> dict:
        sd = {}
        for i, n in enumerate(self._names(prefix)):
            sd[n + ".weight"], sd[n + ".bias"] = self.weight(i).clone(), self.bias(i).clone()
        return sd

    def check_state_dict(self, sd: dict, prefix: str = "") -> None:
        """Raises unless `sd` holds every layer under `prefix` with this network's shapes (nothing is changed)."""
        for i, n in enumerate(self._names(prefix)):
            out, inn = self.shapes[i]
            for key, shape in ((n + ".weight", (out, inn)), (n + ".bias", (out,))):
                if key not in sd:
                    raise KeyError(f"DeformMLP: the state lacks {key}")
                if tuple(sd[key].shape) != shape:
                    raise ValueError(f"DeformMLP: {key} is {tuple(sd[key].shape)}, this network's is {shape}")

    @torch.no_grad()
    def load_state_dict(self, sd: dict, prefix: str = "") -> None:
        """The values are copied IN PLACE (the buffers keep their addresses: a captured step stays valid)."""
        if prefix == "" and any(k.startswith(PREFIX) for k in sd):
            prefix = PREFIX
        self.check_state_dict(sd, prefix)
        for i, n in enumerate(self._names(prefix)):
            self.weight(i).copy_(sd[n + ".weight"])
            self.bias(i).copy_(sd[n + ".bias"])

    @classmethod
    def from_torch(cls, module: torch.nn.Module, point_features: torch.Tensor, cond_dim: int) -> "DeformMLP":
        """From a network of the reference's `MLP` layout (`fcs`: a ModuleList of Linear, `output_linear`), same weights."""
        fcs, last = list(module.fcs), module.output_linear
        for fc in fcs:
            check_shape(point_features.shape[-1], cond_dim, len(fcs), last.out_features, fc.out_features)
        if fcs and fcs[0].in_features != int(point_features.shape[-1]) + int(cond_dim):
            raise ValueError(f"DeformMLP.from_torch: the module's input is {fcs[0].in_features} wide, point_features + cond_dim "
                             f"is {int(point_features.shape[-1]) + int(cond_dim)}")
        rng = torch.get_rng_state()
        mlp = cls(point_features, cond_dim, layers=len(fcs), out_dim=last.out_features)
        torch.set_rng_state(rng)       # (the throw-away initialisation leaves the caller's generator where it was)
        mlp.load_state_dict(module.state_dict())
        return mlp

    # ---- the two entry points
    def _desc(self, cond: torch.Tensor) -> _lib.fr_mlp:
        dev = self.flat.device
        if not self.flat.is_cuda:
            raise RuntimeError("DeformMLP needs device tensors (there is no CPU path)")
        if cond.dtype != torch.float32:
            raise TypeError("DeformMLP: cond must be float32")
        if tuple(cond.shape) != (self.cond_dim,) or cond.device != dev or not cond.is_contiguous():
            raise ValueError(f"DeformMLP: cond must be a contiguous [{self.cond_dim}] tensor on {dev}")
        if self._workspace is None:
            need = _lib.lib().fr_mlp_workspace_bytes(self.N, self.layers)
            self._workspace = torch.empty(max(int(need), 1), dtype=torch.uint8, device=dev)
        return _lib.fr_mlp(self.N, self.layers, self.point_dim, self.cond_dim, self.out_dim, self.point_features.data_ptr(),
                           cond.data_ptr() if self.cond_dim else None, self.flat.data_ptr())

    def _check_rows(self, t: torch.Tensor, what: str) -> None:
        if t.dtype != torch.float32 or tuple(t.shape) != (self.N, self.out_dim) or not t.is_contiguous() or t.device != self.flat.device:
            raise ValueError(f"DeformMLP: {what} must be a contiguous float32 [{self.N},{self.out_dim}] tensor on {self.flat.device}")

    @torch.no_grad()
    def forward_into(self, cond: torch.Tensor, out: torch.Tensor) -> None:
        """The raw outputs of every point for `cond` [Dc], written into `out` [N,out_dim]; the activations the backward needs
        stay in the network's workspace until the next forward."""
        d = self._desc(cond)
        self._check_rows(out, "out")
        _lib.launch("fr_mlp_forward", self.flat.device, C.byref(d), out.data_ptr(), self._workspace.data_ptr())

    @torch.no_grad()
    def backward_from(self, d_out: torch.Tensor, cond: torch.Tensor, d_cond: Optional[torch.Tensor] = None) -> None:
        """After `forward_into(cond, ..)`: OVERWRITES `flat_grad` with dLoss/d(weights) and, if given, `d_cond` [Dc] with
        dLoss/d(cond), for `d_out` = dLoss/d(out)."""
        d = self._desc(cond)
        self._check_rows(d_out, "d_out")
        if d_cond is not None and (d_cond.dtype != torch.float32 or tuple(d_cond.shape) != (self.cond_dim,) or not d_cond.is_contiguous()
                                   or d_cond.device != self.flat.device):
            raise ValueError(f"DeformMLP: d_cond must be a contiguous float32 [{self.cond_dim}] tensor on {self.flat.device}")
        _lib.launch("fr_mlp_backward", self.flat.device, C.byref(d), d_out.data_ptr(), self.flat_grad.data_ptr(),
                    d_cond.data_ptr() if d_cond is not None and self.cond_dim else None, self._workspace.data_ptr())

    def saved_activation(self, layer: int) -> torch.Tensor:
        """Hidden layer `layer`'s post-ReLU activations [N,256] as the last forward left them in the workspace (a view: the
        backward's masks are its signs)."""
        if self._workspace is None or not 0 <= int(layer) < self.layers:
            raise ValueError("DeformMLP.saved_activation: no forward has run, or no such hidden layer")
        stride = (self.N * WIDTH * 4 + 255) // 256 * 256
        return self._workspace[int(layer) * stride:int(layer) * stride + self.N * WIDTH * 4].view(torch.float32).view(self.N, WIDTH)

    def forward(self, cond: torch.Tensor) -> torch.Tensor:
        """The raw outputs [N,out_dim] as an autograd op: differentiable with respect to the weights (`flat.grad` gets a copy
        of `flat_grad`) and `cond`.  For callers that keep their own loop; FlashStep(deformer=...) calls the entry points
        itself, inside its captured step."""
        return _MLPFunction.apply(self.flat, cond, self)

    __call__ = forward


__all__ = ["DeformMLP", "PREFIX", "WIDTH", "check_shape", "embed_points", "layer_shapes"]
