"""FLAME with FateAvatar's personalised deltas on the fused path: the mesh under the Gaussians, posed by two launches per
direction (csrc/fr_flame.hip) instead of FLAME's eager PyTorch forward, run twice, and its autograd backward.

reference:
  * `FLAME.forward_with_delta_blendshape` / `FLAME.forward` (flame/FLAME.py:131-204) over `lbs()` (flame/lbs.py:24-101) with a
    batch of one: betas = (zeros [n_shape], expression[:n_exp]), the learnt `delta_shapedirs` [V,3,L], `delta_posedirs` [36,3V]
    and `delta_vertex` [V,3] added to `shapedirs`, `posedirs` and `v_template` (model/fateavatar.py:87-94,212-223)
  * their optimizer — the `bs` group of train/optim.py:27-33 with config/fateavatar.yaml:40-41: Adam at 1e-5, 1e-5 and 1e-4
The shape columns of `shapedirs + delta_shapedirs` are multiplied by exact zeros, so the gradient of `delta_shapedirs[:, :, :n_shape]`
is exactly 0 and torch's Adam (no weight decay) leaves those columns bit-for-bit where they are (tests/test_flame_host.py pins
both).  The trained state is therefore the expression slice `delta_exp` [V,3,n_exp] alone; the shape columns are kept as they
were loaded and put back into the reference's [V,3,L] layout only in `state_dict()`.
`FlameMesh` holds the trained state in ONE flat buffer (`delta_exp`, `delta_posedirs`, `delta_vertex`, in the order of the
optimizer's groups) with a flat gradient the kernels OVERWRITE, like `mlp.DeformMLP`: one FusedAdam launch with three (count,
rate) segments updates it (`AvatarStep(flame=...)`).  `mesh(expression, pose)` is the autograd op for callers that keep their
own loop — the tracking optimisation of expression and pose that every model's trainer runs (train/base.py:76-113).
Inputs are assumed finite: the kernels make no promise about NaN / Inf coefficients.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

MAX_E = _lib.FR_FLAME_MAX_E
JOINTS = _lib.FR_FLAME_JOINTS
POSE_FEATURES = _lib.FR_FLAME_POSE_FEATURES
PREFIX = "flame."          # FLAME's buffers inside the reference model's state_dict
DELTA_KEYS = ("delta_shapedirs", "delta_posedirs", "delta_vertex")
# config/fateavatar.yaml:40-41 (delta_shapedirs_lr, delta_posedirs_lr) and train/optim.py:30 (delta_vertex)
REFERENCE_FLAME_LRS = dict(delta_shapedirs=1e-5, delta_posedirs=1e-5, delta_vertex=1e-4)


class FlameFrame(NamedTuple):
    """What a frame brings for the mesh: `expression` [n_exp] and `pose` [15] (axis-angle of the five joints)."""
    expression: torch.Tensor
    pose: torch.Tensor


class _MeshFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, expression, pose, fm):
        dev = flat.device
        expression, pose = expression.detach().contiguous(), pose.detach().contiguous()
        verts = torch.empty((fm.V, 3), dtype=torch.float32, device=dev)
        phi = torch.empty(POSE_FEATURES, dtype=torch.float32, device=dev)
        A = torch.empty((JOINTS, 4, 4), dtype=torch.float32, device=dev)
        fm.forward_into(expression, pose, verts, pose_feature=phi, transforms=A)
        ctx.fm, ctx.expression, ctx.pose = fm, expression, pose
        ctx.mark_non_differentiable(phi, A)
        return verts, phi, A

    @staticmethod
    def backward(ctx, g, _g_phi, _g_A):
        fm = ctx.fm
        # (the state the backward reads is the LAST forward's: one frame at a time through one FlameMesh)
        fm.forward_into(ctx.expression, ctx.pose, fm._scratch_verts())
        d_e, d_p = torch.empty_like(ctx.expression), torch.empty_like(ctx.pose)
        fm.backward_from(g.contiguous(), ctx.expression, ctx.pose, d_e, d_p)
        return fm.flat_grad.clone(), d_e, d_p, None


class FlameMesh:
    """FLAME's buffers (constants) and the three learnt deltas (one flat leaf).  `flat` holds `delta_exp` [V,3,n_exp], then
    `delta_posedirs` [36,3V], then `delta_vertex` [V,3], all zero at construction as in the reference
    (model/fateavatar.py:87-94); `flat_grad` has the same layout and is what every backward OVERWRITES.  `delta_exp`,
    `delta_posedirs`, `delta_vertex` (and `grad_*`) are views.  Lives on the device of `v_template` (or `device`); the two entry
    points need a HIP device, everything else works on the CPU."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, n_shape: int, n_exp: int, device=None):
        t = lambda x: torch.as_tensor(x).detach()  # noqa: E731
        v_template, shapedirs, posedirs, J_regressor, lbs_weights = (t(x) for x in (v_template, shapedirs, posedirs, J_regressor,
                                                                                     lbs_weights))
        dev = torch.device(device) if device is not None else v_template.device
        n_shape, n_exp = int(n_shape), int(n_exp)
        if n_shape < 0 or not 1 <= n_exp <= MAX_E:
            raise ValueError(f"FlameMesh: n_shape >= 0 and 1 <= n_exp <= {MAX_E} (the kernels' limit), not {n_shape} and {n_exp}")
        if v_template.dim() != 2 or v_template.shape[1] != 3:
            raise ValueError("FlameMesh: v_template must be [V,3]")
        V, L = int(v_template.shape[0]), n_shape + n_exp
        if 108 * V >= 2 ** 31:
            raise ValueError("FlameMesh: too many vertices (36 x 3V must stay below 2^31)")
        for name, x, shape in (("shapedirs", shapedirs, (V, 3, L)), ("posedirs", posedirs, (POSE_FEATURES, 3 * V)),
                               ("J_regressor", J_regressor, (JOINTS, V)), ("lbs_weights", lbs_weights, (V, JOINTS))):
            if tuple(x.shape) != shape:
                raise ValueError(f"FlameMesh: {name} is {tuple(x.shape)}, expected {shape} (V = {V}, n_shape + n_exp = {L})")
        par = [int(p) for p in np.asarray(t(parents).cpu()).reshape(-1)]
        if len(par) != JOINTS:
            raise ValueError(f"FlameMesh: parents must name {JOINTS} joints")
        if any(not 0 <= par[i] < i for i in range(1, JOINTS)):
            raise ValueError(f"FlameMesh: parents[i] must lie in 0 .. i - 1 for every joint after the root, got {par}")
        f32 = lambda x: x.to(dev, torch.float32).contiguous()  # noqa: E731
        self.V, self.n_shape, self.n_exp = V, n_shape, n_exp
        self.v_template, self.shapedirs, self.posedirs = f32(v_template), f32(shapedirs), f32(posedirs)
        self.J_regressor, self.lbs_weights = f32(J_regressor), f32(lbs_weights)
        self.parents = torch.tensor([-1] + par[1:], dtype=torch.int32, device=dev)
        # the shape columns of delta_shapedirs: never trained (their gradient is exactly 0), kept as loaded
        self.delta_shape_columns = torch.zeros((V, 3, n_shape), dtype=torch.float32, device=dev)
        self.counts = (V * 3 * n_exp, POSE_FEATURES * 3 * V, 3 * V)
        self.flat = torch.zeros(sum(self.counts), dtype=torch.float32, device=dev).requires_grad_(True)
        self.flat_grad = torch.zeros_like(self.flat, requires_grad=False)
        self._workspace = self._scratch = None

    # ---- views of the flat buffers
    def _views(self, buf):
        a, b, _ = self.counts
        return (buf[:a].view(self.V, 3, self.n_exp), buf[a:a + b].view(POSE_FEATURES, 3 * self.V), buf[a + b:].view(self.V, 3))

    delta_exp = property(lambda self: self._views(self.flat.detach())[0])
    delta_posedirs = property(lambda self: self._views(self.flat.detach())[1])
    delta_vertex = property(lambda self: self._views(self.flat.detach())[2])
    grad_delta_exp = property(lambda self: self._views(self.flat_grad)[0])
    grad_delta_posedirs = property(lambda self: self._views(self.flat_grad)[1])
    grad_delta_vertex = property(lambda self: self._views(self.flat_grad)[2])

    @property
    def device(self):
        return self.flat.device

    def parameters(self):
        return [self.flat]

    def adam_segments(self, lrs: Optional[dict] = None):
        """The `bs` optimizer's groups (train/optim.py:27-33) as runs of the flat buffer."""
        lr = dict(REFERENCE_FLAME_LRS, **(lrs or {}))
        unknown = set(lr) - set(REFERENCE_FLAME_LRS)
        if unknown or any(not float(v) > 0.0 for v in lr.values()):
            raise ValueError(f"FlameMesh: learning rates are positive numbers under {sorted(REFERENCE_FLAME_LRS)}")
        return [(n, float(lr[k])) for n, k in zip(self.counts, DELTA_KEYS)]

    # ---- the reference's names and shapes: delta_shapedirs [V,3,L], delta_posedirs [36,3V], delta_vertex [V,3]
    @torch.no_grad()
    def state_dict(self) -> dict:
        return {"delta_shapedirs": torch.cat([self.delta_shape_columns, self.delta_exp], dim=2),
                "delta_posedirs": self.delta_posedirs.clone(), "delta_vertex": self.delta_vertex.clone()}

    def check_state_dict(self, sd: dict) -> None:
        """Raises unless `sd` holds the three deltas with this mesh's shapes (nothing is changed)."""
        V, L = self.V, self.n_shape + self.n_exp
        for key, shape in zip(DELTA_KEYS, ((V, 3, L), (POSE_FEATURES, 3 * V), (V, 3))):
            if key not in sd:
                raise KeyError(f"FlameMesh: the state lacks {key}")
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"FlameMesh: {key} is {tuple(sd[key].shape)}, this mesh's is {shape}")

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """The values are copied IN PLACE (the buffers keep their addresses: a captured step stays valid)."""
        self.check_state_dict(sd)
        ds = sd["delta_shapedirs"].to(self.device, torch.float32)
        self.delta_shape_columns.copy_(ds[:, :, :self.n_shape])
        self.delta_exp.copy_(ds[:, :, self.n_shape:])
        self.delta_posedirs.copy_(sd["delta_posedirs"])
        self.delta_vertex.copy_(sd["delta_vertex"])

    @classmethod
    def from_state_dict(cls, model_sd: dict, n_exp: int, n_shape: Optional[int] = None, device=None) -> "FlameMesh":
        """From a reference checkpoint's `model` entry: FLAME's registered buffers `flame.v_template`, `flame.shapedirs`,
        `flame.posedirs`, `flame.J_regressor`, `flame.parents`, `flame.lbs_weights` (flame/FLAME.py:94-115) — a checkpoint
        stands in for the licensed generic_model.pkl.  `n_exp` (and `n_shape`, default: the remaining columns) are the model
        configuration's, which the buffers do not carry.  The three `delta_*` entries are loaded if the dict has them."""
        need = ["v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights"]
        missing = [PREFIX + k for k in need if PREFIX + k not in model_sd]
        if missing:
            raise KeyError(f"FlameMesh.from_state_dict: the state lacks {missing}")
        b = {k: model_sd[PREFIX + k] for k in need}
        L = int(b["shapedirs"].shape[-1])
        n_shape = L - int(n_exp) if n_shape is None else int(n_shape)
        fm = cls(b["v_template"], b["shapedirs"], b["posedirs"], b["J_regressor"], b["parents"], b["lbs_weights"], n_shape, n_exp,
                 device=device)
        if all(k in model_sd for k in DELTA_KEYS):
            fm.load_state_dict(model_sd)
        return fm

    # ---- the two entry points
    def _ensure_workspace(self) -> None:
        """The kernels' workspace (zeroed once) — allocated here, outside any stream capture."""
        if self._workspace is None:
            if not self.flat.is_cuda:
                raise RuntimeError("FlameMesh needs device tensors to run (there is no CPU path)")
            need = int(_lib.lib().fr_flame_workspace_bytes(self.V, self.n_exp))
            self._workspace = torch.zeros(max(need, 16), dtype=torch.uint8, device=self.device)

    def _scratch_verts(self) -> torch.Tensor:
        if self._scratch is None:
            self._scratch = torch.empty((self.V, 3), dtype=torch.float32, device=self.device)
        return self._scratch

    def workspace_zeroed_part(self) -> torch.Tensor:
        """The part of the workspace every call leaves zeroed (counters and partials), as bytes."""
        self._ensure_workspace()
        return self._workspace[:int(_lib.lib().fr_flame_workspace_zeroed_bytes())]

    def _check(self, t: Optional[torch.Tensor], shape, what: str, optional: bool = False) -> Optional[int]:
        if t is None:
            if optional:
                return None
            raise ValueError(f"FlameMesh: {what} is required")
        if t.dtype != torch.float32:
            raise TypeError(f"FlameMesh: {what} must be float32")
        if tuple(t.shape) != tuple(shape) or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"FlameMesh: {what} must be a contiguous {list(shape)} tensor on {self.device}")
        return t.data_ptr()

    def _desc(self, expression: torch.Tensor, pose: torch.Tensor, deltas: bool = True) -> _lib.fr_flame:
        self._ensure_workspace()
        e, p = self._check(expression, (self.n_exp,), "expression"), self._check(pose, (3 * JOINTS,), "pose")
        dE, dP, dV = self.delta_exp, self.delta_posedirs, self.delta_vertex
        return _lib.fr_flame(self.V, self.n_shape, self.n_exp, self.parents.data_ptr(), self.v_template.data_ptr(),
                             self.shapedirs.data_ptr(), self.posedirs.data_ptr(), self.J_regressor.data_ptr(),
                             self.lbs_weights.data_ptr(), dE.data_ptr() if deltas else None, dP.data_ptr() if deltas else None,
                             dV.data_ptr() if deltas else None, e, p)

    @torch.no_grad()
    def forward_into(self, expression: torch.Tensor, pose: torch.Tensor, verts: torch.Tensor, verts_orig: Optional[torch.Tensor] = None,
                     pose_feature: Optional[torch.Tensor] = None, transforms: Optional[torch.Tensor] = None) -> None:
        """The posed mesh for `expression` [n_exp] and `pose` [15], written into `verts` [V,3]; `verts_orig` [V,3] (optional): the
        mesh WITHOUT the deltas (the reference's second FLAME forward); `pose_feature` [36] and `transforms` [5,4,4] (optional):
        what `lbs()` returns next to the vertices.  What the backward needs stays in the workspace until the next forward."""
        d = self._desc(expression, pose)
        V = self.V
        args = (self._check(verts, (V, 3), "verts"), self._check(verts_orig, (V, 3), "verts_orig", True),
                self._check(pose_feature, (POSE_FEATURES,), "pose_feature", True),
                self._check(transforms, (JOINTS, 4, 4), "transforms", True))
        if V == 0:
            return
        _lib.launch("fr_flame_forward", self.device, C.byref(d), *args, self._workspace.data_ptr())

    @torch.no_grad()
    def backward_from(self, g_verts: torch.Tensor, expression: torch.Tensor, pose: torch.Tensor,
                      d_expression: Optional[torch.Tensor] = None, d_pose: Optional[torch.Tensor] = None, deltas: bool = True) -> None:
        """After `forward_into(expression, pose, ..)`: OVERWRITES `flat_grad` (unless `deltas` is False) with dLoss/d(deltas)
        and, if given, `d_expression` [n_exp] and `d_pose` [15], for `g_verts` [V,3] = dLoss/dverts."""
        d = self._desc(expression, pose)
        g = self._check(g_verts, (self.V, 3), "g_verts")
        de = self._check(d_expression, (self.n_exp,), "d_expression", True)
        dp = self._check(d_pose, (3 * JOINTS,), "d_pose", True)
        if self.V == 0:
            for t in (d_expression, d_pose):
                if t is not None:
                    t.zero_()
            return
        gE, gP, gV = self.grad_delta_exp, self.grad_delta_posedirs, self.grad_delta_vertex
        _lib.launch("fr_flame_backward", self.device, C.byref(d), g, gE.data_ptr() if deltas else None,
                    gP.data_ptr() if deltas else None, gV.data_ptr() if deltas else None, de, dp, self._workspace.data_ptr())

    def mesh(self, expression: torch.Tensor, pose: torch.Tensor):
        """`(verts [V,3], pose_feature [36], transforms [5,4,4])` as an autograd op: `verts` is differentiable with respect to
        `expression`, `pose` and the deltas (`flat.grad` gets a copy of `flat_grad`); the other two are returned as lbs()
        returns them and carry no gradient.  For callers that keep their own loop — any model's tracking optimisation;
        AvatarStep(flame=...) calls the entry points itself, inside its captured step."""
        return _MeshFunction.apply(self.flat, expression, pose, self)

    __call__ = mesh


def synthetic_flame(template_verts, seed: int = 0, n_shape: int = 10, n_exp: int = 50, device=None, amplitude: float = 0.004) -> FlameMesh:
    """A FLAME-shaped model over `template_verts` [V,3] for the tools and the tests (the licensed model is not redistributable):
    every table is a smooth function of the vertex, as tools/train_synthetic.py's tables for MonoGaussianAvatar are — shape and
    expression directions and pose correctives are low-frequency sine fields of `amplitude` metres, the five joints (root, neck,
    jaw, two eyes; parents -1, 0, 1, 1, 1) sit at fixed places of the bounding box, a joint's regressor row is a normalised
    Gaussian bump around it and the skinning weights are a softmax of the squared distances to the joints."""
    v = torch.as_tensor(np.asarray(template_verts, dtype=np.float64))
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError("synthetic_flame: template_verts must be [V,3] with V >= 1")
    V, L = int(v.shape[0]), int(n_shape) + int(n_exp)
    g = torch.Generator().manual_seed(int(seed))
    lo, hi = v.min(0).values, v.max(0).values
    size = (hi - lo).clamp_min(1e-6)
    u = (v - lo) / size                                                     # the vertex in the unit box
    rnd = lambda *s: torch.rand(s, generator=g, dtype=torch.float64)  # noqa: E731
    # directions: amplitude * decay_l * sin(2 pi (f_l . u) + phase_lk)
    freq, phase = rnd(L, 3) * 2.0 + 0.25, rnd(L, 3) * 6.283185307179586
    decay = 1.0 / (1.0 + 0.05 * torch.arange(L, dtype=torch.float64))
    S = amplitude * decay[None, None, :] * torch.sin(6.283185307179586 * (u @ freq.T)[:, None, :] + phase.T[None, :, :])
    fp, pp = rnd(POSE_FEATURES, 3) * 1.5 + 0.25, rnd(POSE_FEATURES, 3) * 6.283185307179586
    P = 0.5 * amplitude * torch.sin(6.283185307179586 * (u @ fp.T).T[:, :, None] + pp[:, None, :])      # [36,V,3]
    at = torch.tensor([[0.5, 0.1, 0.4], [0.5, 0.3, 0.45], [0.5, 0.35, 0.7], [0.35, 0.65, 0.85], [0.65, 0.65, 0.85]], dtype=torch.float64)
    joints = lo + at * size
    d2 = ((v[:, None, :] - joints[None, :, :]) / size.max()).pow(2).sum(-1)                                # [V,5]
    Jr = torch.exp(-d2 / (2 * 0.15 ** 2)).T
    Jr = Jr / Jr.sum(1, keepdim=True).clamp_min(1e-300)
    W = torch.softmax(-d2 / (2 * 0.2 ** 2), dim=1)
    return FlameMesh(v.float(), S.float(), P.reshape(POSE_FEATURES, 3 * V).float(), Jr.float(), [-1, 0, 1, 1, 1], W.float(),
                     n_shape, n_exp, device=device)


__all__ = ["DELTA_KEYS", "FlameFrame", "FlameMesh", "JOINTS", "MAX_E", "POSE_FEATURES", "PREFIX", "REFERENCE_FLAME_LRS", "synthetic_flame"]
