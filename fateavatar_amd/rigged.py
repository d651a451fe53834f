"""GaussianAvatars — the reference's headline baseline — on the fused path: Gaussians rigged to the triangles of the posed
mesh, SH degree 3, one optimisation step per call.

reference:
  * parameters — `_register_init_gaussian` (model/baseline/gaussianavatars.py:97-120): ONE Gaussian per face
    (`binding = arange(F)`, :52-60), local position 0, log-scale 0, identity rotation, opacity 0.1, a random colour / 255 in
    the DC term, `max_sh_degree` 3 (config/gaussianavatars.yaml:23) with `active_sh_degree` 0 (:45-46)
  * their Adam groups — `_xyz, _opacity, _features_dc, _features_rest, _rotation, _scaling` in that order
    (train/optim.py:73-80) with the rates of config/gaussianavatars.yaml:26-31, `_features_rest` at feature_dc_lr / 20
  * a frame — gaussianavatars.py:144-171: every Gaussian is carried by its face's local frame (`binding.
    bind_gaussians_face_local`), then render() with the ACTIVE SH degree (:157)
  * `_update_sh_degree` (:497-499)
What is fused: the binding runs inside the rasterizer's per-Gaussian kernels (bound.render_bound_batch with a
FaceLocalBinding; `fold_binding=False` keeps the stand-alone op as the A/B), activations and densification statistics run
inside the rasterizer kernels, one L1 launch, one Adam launch over the flat buffer, the whole step ONE HIP graph.
Not here: the clone / split densification with `binding_counter` and its guarded prune, the scale / xyz
regularisers and the D-SSIM term, the position learning-rate schedule, a multi-lane batch step, data-parallel runs, FLAME.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .binding import bind_gaussians_face_local
from .bound import FaceLocalBinding, render_bound_batch
from .loss import l1_loss_and_grad, l1_workspace
from .model import TorchCamera
from .optim import FusedAdam
from .rasterizer import GradOut
from .render import render
from .train import TrainStep

# config/gaussianavatars.yaml:26-31 (group names of train/optim.py:73-80; position_lr_init: the schedule is out of scope)
RIGGED_LRS = dict(xyz=0.005, opacity=0.05, feature_dc=0.0025, feature_rest=0.0025 / 20, rotation=0.001, scaling=0.017)


class RiggedGaussians(torch.nn.Module):
    """The face-bound Gaussian parameters of GaussianAvatars in ONE flat buffer, in the order of the optimizer groups
    (train/optim.py:73-80).  `binding` [P] is the face of every Gaussian (gaussianavatars.py:52-60)."""
    max_sh_degree = 3        # config/gaussianavatars.yaml:23
    FIELDS = (("_xyz", 3), ("_opacity", 1), ("_features_dc", 3), ("_features_rest", 45), ("_rotation", 4), ("_scaling", 3))
    SHAPES = {"_xyz": (3,), "_opacity": (1,), "_features_dc": (1, 3), "_features_rest": (15, 3), "_rotation": (4,),
              "_scaling": (3,)}
    fused_activations = True

    def __init__(self, binding, device, rng: Optional[np.random.Generator] = None):
        """_register_init_gaussian (gaussianavatars.py:97-120) for the Gaussians bound to the faces `binding` [P]."""
        super().__init__()
        self.binding = torch.as_tensor(np.asarray(binding), dtype=torch.int32, device=device).contiguous()
        P = int(self.binding.shape[0])
        rng = rng or np.random.default_rng(0)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
        dc = torch.from_numpy((rng.random((P, 3)) / 255.0).astype(np.float32)).to(device).reshape(P, 1, 3)   # :101-104
        rot = z(P, 4)
        rot[:, 0] = 1
        op = torch.full((P, 1), float(np.log(0.1 / 0.9)), dtype=torch.float32, device=device)   # inverse_sigmoid(0.1)
        self.active_sh_degree = 0
        self._bind([z(P, 3), op, dc, z(P, 15, 3), rot, z(P, 3)])

    @classmethod
    def one_per_face(cls, n_faces: int, device, rng: Optional[np.random.Generator] = None) -> "RiggedGaussians":
        """The reference's initial binding: Gaussian i on face i (gaussianavatars.py:52-60)."""
        return cls(np.arange(int(n_faces), dtype=np.int32), device, rng)

    @property
    def P(self) -> int:
        return int(self.binding.shape[0])

    def widths(self):
        return [w for _, w in self.FIELDS]

    def _bind(self, raw):
        P, dev = raw[0].shape[0], raw[0].device
        sizes = [P * w for _, w in self.FIELDS]
        self.flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        # (gradient buffer + the step's overflow word behind it: model.FlatGaussians._bind)
        self._grad_store = torch.zeros(sum(sizes) + 4, dtype=torch.float32, device=dev)
        self.flat_grad = self._grad_store[:sum(sizes)]
        self.overflow_word = self._grad_store[sum(sizes):sum(sizes) + 1]
        off = 0
        for (name, w), n, r in zip(self.FIELDS, sizes, raw):
            shp = (P,) + self.SHAPES[name]
            self.flat[off:off + n].copy_(r.detach().reshape(-1))
            p = torch.nn.Parameter(self.flat[off:off + n].view(shp))
            p._fr_grad_out = GradOut(self.flat_grad[off:off + n].view(shp))   # (see AvatarGaussians._bind)
            setattr(self, name, p)
            off += n

    @property
    def get_features(self) -> torch.Tensor:
        """[P,16,3]: GaussianModel.get_features (volume_rendering/gaussian_model.py:119-122)."""
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    def begin_step(self):
        for name, _ in self.FIELDS:
            getattr(self, name).grad = None

    def collect_grads(self) -> torch.Tensor:
        """Every parameter's gradient in the flat gradient buffer (most are written there by the kernels already; the two
        halves of the SH block come back from autograd's split of the concatenation)."""
        off = 0
        for name, w in self.FIELDS:
            n = self.P * w
            g, view = getattr(self, name).grad, self.flat_grad[off:off + n]
            if g is None:
                view.zero_()
            elif g.data_ptr() != view.data_ptr() or not g.is_contiguous():
                view.view(g.shape).copy_(g)
            off += n
        return self.flat_grad


class _RiggedFrame:
    """What render() / render_bound_batch() read of a Gaussian holder for one frame.  `max_sh_degree` is the degree the frame
    is rendered with: the reference hands render() a GaussianModel(sh_degree=active_sh_degree), gaussianavatars.py:157."""
    fused_activations = True

    def __init__(self, pc: RiggedGaussians, stats, bound=None):
        self.max_sh_degree = self.active_sh_degree = int(pc.active_sh_degree)
        self._opacity, self.get_features = pc._opacity, pc.get_features
        if bound is None:     # raw parameters: the rasterizer evaluates the binding itself
            self._xyz, self._rotation, self._scaling = pc._xyz, pc._rotation, pc._scaling
        else:                 # the stand-alone op's outputs
            self.get_xyz, self._rotation, self._scaling = bound
        self.fused_densification_stats = stats


class RiggedStep(TrainStep):
    """One optimisation step of GaussianAvatars per call: `step(camera, posed_verts, gt_image)` —
    bind in the frame -> render -> L1 -> backward -> densification statistics -> Adam."""

    def __init__(self, pc: RiggedGaussians, faces: torch.Tensor, camera: TorchCamera, bg: torch.Tensor, verts: torch.Tensor,
                 lrs: Optional[dict] = None, use_graph: bool = True, fold_binding: bool = True):
        """`verts` [V,3]: any pose of the mesh (sizes the step's static vertex buffer and is its first content).
        `fold_binding` (default): the binding is evaluated inside the rasterizer's per-Gaussian kernels (fr_aux::binding with
        FR_BIND_FACE_LOCAL) — no binding launches.  False: the stand-alone `bind_gaussians_face_local` op in front of
        render() (same results; the A/B and the op's own user)."""
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise RuntimeError("RiggedStep: data-parallel runs are not built (DESIGN.md)")
        self.pc, self.bg = pc, bg
        self.fold_binding = bool(fold_binding)
        self.dev = pc.flat.device
        self.world, self.exchange, self.exchange_in_graph = 1, False, False
        self.lr = dict(RIGGED_LRS, **(lrs or {}))
        self.faces = faces.to(self.dev, torch.int32).contiguous()
        self._make_adam()
        self.xyz_gradient_accum = torch.zeros((pc.P, 1), device=self.dev)
        self.denom = torch.zeros((pc.P, 1), device=self.dev)
        self.cam = camera
        self.verts = verts.to(self.dev, torch.float32).clone().contiguous()   # static input of the captured step
        self.gt = torch.zeros((3, camera.image_height, camera.image_width), device=self.dev)
        self.loss = torch.zeros((), device=self.dev)
        self._dimage = torch.zeros_like(self.gt)   # dL/dimage of the step
        self._l1_ws = l1_workspace(self.dev)
        self.out = None
        self.use_graph = bool(use_graph)
        self._graph, self._eager_steps, self.overflows = None, 0, 0
        self.host_steps = 0      # (TrainStep.skipped_steps)

    def adam_segments(self):
        """The optimizer groups (train/optim.py:73-80 with config/gaussianavatars.yaml:26-31) as runs of the flat buffer."""
        lr, P = self.lr, self.pc.P
        return [(P * 3, lr["xyz"]), (P * 1, lr["opacity"]), (P * 3, lr["feature_dc"]), (P * 45, lr["feature_rest"]),
                (P * 4, lr["rotation"]), (P * 3, lr["scaling"])]

    def _make_adam(self):
        pc = self.pc
        self.adam = FusedAdam(pc.flat, pc.flat_grad, self.adam_segments())
        self.adam.set_skip_words([pc.overflow_word])

    def _forward_backward(self):
        pc = self.pc
        pc.begin_step()                                             # zero_grad(set_to_none=True)
        stats = (self.xyz_gradient_accum, self.denom, pc.overflow_word)
        if self.fold_binding:
            from . import rasterizer
            out = render_bound_batch([self.cam], [_RiggedFrame(pc, stats)], [self.verts], FaceLocalBinding(self.faces, pc.binding),
                                     self.bg, slots=[rasterizer._slot])[0]
        else:
            bound = bind_gaussians_face_local(self.verts, self.faces, pc.binding, pc._xyz, pc._rotation, pc._scaling)
            out = render(self.cam, _RiggedFrame(pc, stats, bound), self.bg)
        _, g = l1_loss_and_grad(out["render"], self.gt, loss_out=self.loss, grad_out=self._dimage, workspace=self._l1_ws)   # see TrainStep
        out["render"].backward(g)
        pc.collect_grads()                                          # (the SH halves: see RiggedGaussians.collect_grads)
        self.out = {"render": out["render"].detach(), "radii": out["radii"], "visibility_filter": out["visibility_filter"]}

    def step(self, camera: TorchCamera, posed_verts: torch.Tensor, gt_image: torch.Tensor) -> torch.Tensor:
        self._extra_inputs = [(self.verts, posed_verts)]
        return super().step(camera, gt_image)

    def _load_inputs(self, camera, gt_image, extra=()):
        super()._load_inputs(camera, gt_image, extra=self._extra_inputs)

    def update_sh_degree(self) -> int:
        """_update_sh_degree (gaussianavatars.py:497-499).  The degree is a launch argument of the captured kernels: the step
        is captured again on its next call.  Returns the active degree."""
        pc = self.pc
        if pc.active_sh_degree < pc.max_sh_degree:
            pc.active_sh_degree += 1
            self._graph = None
        return pc.active_sh_degree

    # ---- the maintenance of TrainStep moves rows of a FlatGaussians; the rigged set's own (clone / split with
    #      binding_counter, guarded prune) is not built
    def _no_maintenance(self, *a, **k):
        raise NotImplementedError("RiggedStep: GaussianAvatars' densification / prune / opacity reset are not built (DESIGN.md)")

    prune_low_opacity = densify_by_gradient = reset_opacity = _no_maintenance

    # ---- checkpoints: 'model' holds what GaussianAvatars.state_dict() holds of the Gaussians (the six parameters and the
    #      `binding` buffer); 'optimizer', 'densification' and 'active_sh_degree' are what a seamless resume needs on top
    GAUSSIAN_ATTRIBUTES = ["_xyz", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "binding"]

    def state_dict(self) -> dict:
        pc = self.pc
        model = {name: getattr(pc, name).detach().clone() for name, _ in pc.FIELDS}
        model["binding"] = pc.binding.clone()
        return {"global_step": self.adam.step_count, "model": model, "active_sh_degree": int(pc.active_sh_degree),
                "optimizer": {"exp_avg": self.adam.exp_avg.clone(), "exp_avg_sq": self.adam.exp_avg_sq.clone(),
                              "state": self.adam.state_words()},
                "densification": {"xyz_gradient_accum": self.xyz_gradient_accum.clone(), "denom": self.denom.clone()}}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> list:
        """Restores the Gaussians (any row count), the optimizer state and the statistics; returns the keys of sd['model'] it
        did not use."""
        model = dict(sd["model"])
        missing = [k for k in self.GAUSSIAN_ATTRIBUTES if k not in model]
        if missing:
            raise KeyError(f"checkpoint lacks Gaussian attributes {missing}")
        g = {k: model.pop(k) for k in self.GAUSSIAN_ATTRIBUTES}
        pc = self.pc
        pc.binding = g["binding"].to(self.dev, torch.int32).contiguous()
        P = int(pc.binding.shape[0])
        pc._bind([g[name].to(self.dev, torch.float32).reshape((P,) + pc.SHAPES[name]) for name, _ in pc.FIELDS])
        pc.active_sh_degree = int(sd.get("active_sh_degree", pc.active_sh_degree))
        self._make_adam()                                  # fresh (zero) moments over the new buffers
        self._graph, self._eager_steps = None, 0           # buffers moved: the captured step is stale
        self.xyz_gradient_accum = torch.zeros((P, 1), device=self.dev)
        self.denom = torch.zeros((P, 1), device=self.dev)
        opt, dens = sd.get("optimizer"), sd.get("densification")
        if opt is not None:
            self.adam.exp_avg.copy_(opt["exp_avg"])
            self.adam.exp_avg_sq.copy_(opt["exp_avg_sq"])
            self.adam.load_state_words(opt["state"])
        self.host_steps = self.adam.step_count
        if dens is not None:
            self.xyz_gradient_accum.copy_(dens["xyz_gradient_accum"])
            self.denom.copy_(dens["denom"])
        return sorted(model.keys())
