"""FlashAvatar — the reference's MLP-deformed baseline — on the fused path: Gaussians sit at fixed barycentric points of the
posed mesh and a deformation MLP moves, turns and stretches them per frame; SH degree 0, one optimisation step per call.

reference:
  * parameters — `_register_init_gaussian` (model/baseline/flashavatar.py:196-219): one Gaussian per covered texel of the
    template's UV layout at `tex_size` 128 (config/flashavatar.yaml:20; `uniform_sampling_barycoords(..., strict=False)`, :159-164),
    DC inverse_sigmoid(0.5) = 0, rest 0 (`max_sh_degree` 3, :72), log of the mean nearest-neighbour distance of the sampled
    canonical points on all axes, identity rotation, opacity 0.1
  * their Adam groups — `_opacity, _features_dc, _features_rest, _rotation, _scaling` in that order (train/optim.py:45-51) with
    the rates of config/flashavatar.yaml:22-25, `_features_rest` at feature_dc_lr / 20; the deformation MLP has an Adam of its
    own (deformer_lr 1e-4, :55-59)
  * a frame — `forward` :242-276: t = tanh(MLP(embedded canonical point, condition)), position = barycentric point + t[0:3],
    rotation = quatProduct_batch(_rotation, (exp(t[3]), t[4:7])), scaling = _scaling * exp(t[7:10]), rendered with
    GaussianModel(sh_degree=0)
  * the loss — FlashAvatarLoss (train/loss.py:203-255): Huber with alpha 0.1, plus 40 x the same on the mouth region if the
    frame brings a mouth mask, plus 0.05 x LPIPS once `cur_step > 15000` (config/flashavatar.yaml:16):
    `FlashStep(lpips=Lpips(..., weight=REFERENCE_LPIPS_WEIGHT), lpips_start=REFERENCE_LPIPS_START)`, opt-in; the term's weights
    are the caller's to load (`perceptual.Lpips.from_state_dicts`), none are shipped
What is fused: the binding runs inside the rasterizer's per-Gaussian kernels (bound.render_bound_batch with a DeformBinding;
`fold_binding=False` keeps the stand-alone op `binding.bind_gaussians_deform` as the A/B), activations and densification
statistics run inside the rasterizer kernels, one Huber launch, one Adam launch over the flat buffer, the whole step ONE HIP
graph.  By default the MLP stays the caller's stock PyTorch, as FLAME does: the step takes this frame's `deform` [N,10] as one
more static input and hands back `d_deform`, the caller goes on with `deform.backward(step.d_deform)` and its own optimizer.
With `FlashStep(deformer=DeformMLP(...))` the network is part of the captured step (mlp.py, csrc/fr_mlp.hip): the step takes the
frame's condition vector instead, runs the MLP's forward into its `deform` buffer and its backward from `d_deform`, and a
second FusedAdam launch updates the network's flat buffer — still ONE graph, nothing eager between replays.

The reference renders SH degree 0 (:256), so `_features_rest` is never read and only ever gets a zero gradient.  The frame hands
the rasterizer `_features_dc` alone (M = 1), as AvatarGaussians' frames do: the image is the same; `_features_rest` keeps its
place in the flat buffer, its rate and its checkpoint key, and stays exactly 0.

NOT here:
  * density control (the reference has none for this model) and data-parallel runs of the step
  * batch steps (several frames per update)
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .binding import bind_gaussians_deform
from .bound import DeformBinding, render_bound_batch
from .flat import FlatParams
from .loss import REFERENCE_HUBER_LOSS, HuberLoss, huber_loss_and_grad, huber_workspace
from .mlp import PREFIX as DEFORM_PREFIX, DeformMLP
from .model import TorchCamera
from .optim import FusedAdam
from .render import render
from .train import BoundStep

# config/flashavatar.yaml:22-25 (group names of train/optim.py:45-51)
FLASH_LRS = dict(opacity=0.05, feature_dc=0.0025, feature_rest=0.0025 / 20, rotation=0.001, scaling=0.005)
DEFORM_COLS = 10     # position 3, rotation 4, scale 3 (:247-254)
REFERENCE_LPIPS_WEIGHT, REFERENCE_LPIPS_START = 0.05, 15_000     # config/flashavatar.yaml:16, train/loss.py:203-255


class FlashGaussians(FlatParams):
    """FlashAvatar's Gaussian parameters in ONE flat buffer, in the order of the optimizer groups (train/optim.py:45-51).
    `face_index` [P] / `bary_coords` [P,3] are every Gaussian's fixed place on the mesh (:159-164)."""
    FIELDS = (("_opacity", 1), ("_features_dc", 3), ("_features_rest", 45), ("_rotation", 4), ("_scaling", 3))
    SHAPES = {"_opacity": (1,), "_features_dc": (1, 3), "_features_rest": (15, 3), "_rotation": (4,), "_scaling": (3,)}
    ROW_BUFFERS = (("face_index", torch.int32, "new_face_index"), ("bary_coords", torch.float32, "new_bary"))
    max_sh_degree = 3        # :72
    fused_activations = True

    def __init__(self, face_index, bary_coords, scale_init: float, device):
        """_register_init_gaussian (:196-219): DC inverse_sigmoid(0.5) = 0, rest 0, log-scale `scale_init` on all axes, identity
        rotation, opacity inverse_sigmoid(0.1)."""
        super().__init__()
        self.face_index = torch.as_tensor(np.asarray(face_index)).to(device, torch.int32).contiguous()
        self.bary_coords = torch.as_tensor(np.asarray(bary_coords)).to(device, torch.float32).contiguous()
        P = int(self.face_index.shape[0])
        if self.bary_coords.shape != (P, 3):
            raise ValueError("FlashGaussians: face_index [P], bary_coords [P,3]")
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
        rot = z(P, 4)
        rot[:, 0] = 1
        op = torch.full((P, 1), float(np.log(0.1 / 0.9)), dtype=torch.float32, device=device)
        self.active_sh_degree = 0
        self._bind([op, z(P, 1, 3), z(P, 15, 3), rot, torch.full((P, 3), float(scale_init), dtype=torch.float32, device=device)])

    @classmethod
    def from_template(cls, device, uv_resolution: int = 128) -> "FlashGaussians":
        """`_register_template_mesh` + `_register_init_gaussian` (:150-219) on the head template: one Gaussian per texel centre the
        template's UV layout covers at `uv_resolution` x `uv_resolution`, in row-major texel order, NOT padded (`strict=False`,
        :159-164: the row count is what the layout covers); scale_init = the reference's knn estimate on the sampled canonical
        points (:98, :366-377)."""
        from . import mesh_sampling, scenes
        from .knn import init_scale_by_knn
        verts, faces, _ = scenes.head_geometry()
        uv = scenes.head_uv()
        if uv is None:
            raise RuntimeError("the head template's UV layout is not in fateavatar_amd/data/head_template_geom.npz")
        fi, bc = mesh_sampling.uniform_sampling_barycoords(int(uv_resolution) * int(uv_resolution), uv[0], uv[1], strict=False)
        pts = (verts[faces[fi]] * bc[:, :, None]).sum(1).astype(np.float32)      # reweight_verts_by_barycoords
        return cls(fi, bc, float(init_scale_by_knn(torch.from_numpy(pts).to(device))[2]), device)

    def canonical_points(self, canonical_verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
        """`verts_sampling` (:187-192): the Gaussians' barycentric points on the canonical mesh [P,3] — what the reference embeds
        for its deformation MLP."""
        tri = canonical_verts.detach().to(self.flat.device, torch.float32)[faces.to(self.flat.device).long()[self.face_index.long()]]
        return (tri * self.bary_coords.unsqueeze(-1)).sum(1)


class _FlashFrame:
    """What render() / render_bound_batch() read of a Gaussian holder for one frame: SH degree 0 from `_features_dc` alone."""
    fused_activations = True
    max_sh_degree = active_sh_degree = 0

    def __init__(self, pc: FlashGaussians, stats, deform=None, bound=None):
        self._opacity, self.get_features = pc._opacity, pc._features_dc
        if bound is None:     # raw parameters: the rasterizer evaluates the binding itself
            self._deform, self._rotation, self._scaling = deform, pc._rotation, pc._scaling
        else:                 # the stand-alone op's outputs
            self.get_xyz, self._rotation, self._scaling = bound
        self.fused_densification_stats = stats


class FlashStep(BoundStep):
    """One optimisation step of FlashAvatar's Gaussians per call: `step(camera, posed_verts, deform, gt_image, mouth_mask=None)` —
    bind in the frame -> render -> Huber -> backward -> densification statistics -> Adam.  The optimizer groups are those of
    train/optim.py:45-51 with config/flashavatar.yaml:22-25."""
    LRS = FLASH_LRS
    LR_KEYS = {"_opacity": "opacity", "_features_dc": "feature_dc", "_features_rest": "feature_rest", "_rotation": "rotation",
               "_scaling": "scaling"}

    def __init__(self, pc: FlashGaussians, faces: torch.Tensor, camera: TorchCamera, bg: torch.Tensor, verts: torch.Tensor,
                 lrs: Optional[dict] = None, use_graph: bool = True, fold_binding: bool = True,
                 huber: HuberLoss = REFERENCE_HUBER_LOSS, mouth_mask: bool = False, vertex_grad: bool = False,
                 deformer: Optional[DeformMLP] = None, deformer_lr: float = 1e-4, lpips=None,
                 lpips_start: int = REFERENCE_LPIPS_START):
        """`verts` [V,3]: any pose of the mesh (sizes the step's static vertex buffer and is its first content).
        `fold_binding` (default): the binding is evaluated inside the rasterizer's per-Gaussian kernels (fr_aux::binding with
        FR_BIND_DEFORM).  False: the stand-alone `bind_gaussians_deform` op in front of render() (same results; the A/B and the
        op's own user).  `huber`: the image term's (alpha, mask_weight).  `mouth_mask`: whether every frame brings a mouth mask
        [1,H,W] — fixed here because the mask's term is part of the captured step: with True `step()` requires one, with False
        it refuses one.  `vertex_grad`: `d_verts` [V,3] holds every step's dLoss/dposed_verts (BoundStep; the reference's
        tracking optimisation, train/base.py:76-113, reaches the FLAME coefficients through it).
        After every `step()`, `d_deform` [N,10] holds THIS step's dLoss/d(deform), with the lifetime and the zeroing rules of
        `d_verts`; `loss_terms` holds (huber + mask_weight x mouth, huber, mouth) and `loss` is its first word.
        `deformer`: a `mlp.DeformMLP` over the holder's P points makes the network part of the step:
        `step(camera, posed_verts, cond, gt_image, mouth_mask=None)` then takes the frame's condition [Dc] where it took
        `deform`, and the captured body is MLP forward -> frame -> MLP backward -> the Gaussians' Adam -> an Adam of the
        network's flat buffer at `deformer_lr` (train/optim.py:55-59), skipped by the same overflow word.  `d_cond` [Dc] holds
        THIS step's dLoss/d(cond) (the reference's tracking optimisation of expression and pose), with the lifetime rules of
        `d_verts`.  None (default): the MLP is the caller's, nothing here changes.
        `lpips`: a `perceptual.Lpips` adds the LPIPS term from step `lpips_start` + 1 on (the reference multiplies it by 0 until
        `cur_step > 15000`; here it is not launched before): ONE call behind the Huber launch adds weight x its gradient to the
        step's image-gradient buffer, in front of the rasterizer's backward.  `lpips_loss` [1 + T] holds the step's UNWEIGHTED
        terms and stays zero until then; `loss` and `loss_terms` keep their meaning.  The step's number is `schedule_steps`, a
        host count of the schedule's own: step() calls, and after `load_state_dict` the checkpoint's `global_step` — as the
        reference's loader restores it (train/loader.py:102) and applies `cur_step > 15000` to it (train/loss.py:250) — so a
        checkpoint in the reference's own layout (`global_step` and `model`, no `optimizer` entry) resumes the SCHEDULE where
        it was although the optimizer starts fresh (`host_steps`, `adam.step_count` and `skipped_steps` keep their meaning and
        restart at 0 there).  No device word is read.  At a crossing — the start, or a checkpoint from the other side of it —
        the captured graph is dropped ONCE (`lpips_switches` counts it) and the step re-captured with or without the launch in
        it, as after an overflow.  None (default): not one launch changes."""
        self._init_lpips(lpips, pc)
        if int(lpips_start) < 0:
            raise ValueError("FlashStep: lpips_start is a step count, >= 0")
        self.lpips_start, self._lpips_on, self.lpips_switches, self.captures = int(lpips_start), False, 0, 0
        self.schedule_steps = 0
        if deformer is not None:
            if not isinstance(deformer, DeformMLP):
                raise TypeError("FlashStep: `deformer` must be a mlp.DeformMLP")
            if deformer.N != pc.P or deformer.out_dim != DEFORM_COLS:
                raise ValueError(f"FlashStep: the deformer maps {deformer.N} points to {deformer.out_dim} columns, the step needs "
                                 f"[{pc.P},{DEFORM_COLS}]")
            if deformer.flat.device != pc.flat.device:
                raise ValueError("FlashStep: the deformer and the Gaussians live on different devices")
            if not float(deformer_lr) > 0.0:
                raise ValueError("FlashStep: deformer_lr must be positive")
        self.deformer, self.deformer_lr, self.deformer_adam = deformer, float(deformer_lr), None
        if int(pc.face_index.shape[0]) and (int(pc.face_index.min()) < 0 or int(pc.face_index.max()) >= int(faces.shape[0])):
            raise ValueError("FlashStep: `face_index` names a face the mesh does not have")
        self.huber = HuberLoss(*[float(x) for x in huber])
        super().__init__(pc, faces, camera, bg, verts, lrs, use_graph, fold_binding, data_parallel=False, vertex_grad=vertex_grad)
        self.loss_terms = torch.zeros(3, device=self.dev)
        self.loss = self.loss_terms[0]
        self._huber_ws = huber_workspace(self.dev)
        # static inputs of the captured step, next to verts / gt / the camera
        self.deform = torch.zeros((pc.P, DEFORM_COLS), device=self.dev)
        self.mask = torch.zeros((1, camera.image_height, camera.image_width), device=self.dev) if mouth_mask else None
        self.d_deform = None
        # with a deformer: the frame's condition, one more static input, and its gradient
        self.cond = self.d_cond = None
        if deformer is not None:
            self.cond = torch.zeros(deformer.cond_dim, device=self.dev)
            self.d_cond = torch.zeros(deformer.cond_dim, device=self.dev)

    def _make_adam(self):
        """The Gaussians' optimizer and, with a deformer, a FRESH one over its flat buffer; both skip on the holder's present
        overflow word."""
        super()._make_adam()
        if self.deformer is not None:
            d = self.deformer
            self.deformer_adam = FusedAdam(d.flat.detach(), d.flat_grad, [(d.flat.numel(), self.deformer_lr)])
            self.deformer_adam.set_skip_words([self.pc.overflow_word])

    def _buffers_moved(self, old_index, old_rows, *, stats):
        super()._buffers_moved(old_index, old_rows, stats=stats)
        if self.deformer is not None:
            if self.deformer.N != self.pc.P:
                raise ValueError(f"FlashStep: the deformer is built over {self.deformer.N} points, the Gaussians now have {self.pc.P}")
            self.deformer_adam.set_skip_words([self.pc.overflow_word])   # (a remapped optimizer: the word may have moved)
        if getattr(self, "deform", None) is not None and self.deform.shape[0] != self.pc.P:   # (a checkpoint with another row count)
            self.deform = torch.zeros((self.pc.P, DEFORM_COLS), device=self.dev)
            self.d_deform = None

    def _forward_backward(self):
        pc = self.pc
        pc.begin_step()                                             # zero_grad(set_to_none=True)
        stats = (self.xyz_gradient_accum, self.denom, pc.overflow_word)
        verts = self._vertex_leaf(self.verts)
        if self.deformer is not None:
            self.deformer.forward_into(self.cond, self.deform)
        deform = self.deform.detach().requires_grad_(True)         # a leaf over the static buffer (no copy), as `_vertex_leaf`
        if self.fold_binding:
            from . import rasterizer
            out = render_bound_batch([self.cam], [_FlashFrame(pc, stats, deform=deform)], [verts],
                                     DeformBinding(self.faces, pc.face_index, pc.bary_coords), self.bg, slots=[rasterizer._slot])[0]
        else:
            bound = bind_gaussians_deform(verts, self.faces, pc.face_index, pc.bary_coords, deform, pc._rotation, pc._scaling)
            out = render(self.cam, _FlashFrame(pc, stats, bound=bound), self.bg)
        _, g = huber_loss_and_grad(out["render"], self.gt, self.huber, mask=self.mask, loss_out=self.loss_terms,
                                   grad_out=self._dimage, workspace=self._huber_ws)
        if self._lpips_on:
            self._add_lpips(out["render"], g)
        out["render"].backward(g)
        self._keep_vertex_grad(verts)
        self.d_deform = deform.grad      # (inside a captured step: graph-owned storage, the same on every replay)
        if self.deformer is not None:
            self.deformer.backward_from(self.d_deform, self.cond, self.d_cond)
        self.out = self._kept(out)

    def _body(self):
        super()._body()
        if self.deformer is not None:
            self.deformer_adam.step()

    def _capture(self):
        self.captures += 1
        super()._capture()

    def step(self, camera: TorchCamera, posed_verts: torch.Tensor, deform: torch.Tensor, gt_image: torch.Tensor,
             mouth_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`deform` [N,10]: the deformation MLP's RAW outputs for this frame (only the values are loaded: it usually hangs on
        the MLP's autograd graph) — or, for a step built with a `deformer`, the frame's condition vector [Dc].  `mouth_mask`
        [1,H,W] or [H,W]: required if the step was built with `mouth_mask=True`, refused otherwise."""
        if (mouth_mask is None) != (self.mask is None):
            raise ValueError("FlashStep.step: `mouth_mask` goes with FlashStep(mouth_mask=True) (required with it, refused without)")
        if self.deformer is not None:
            if tuple(deform.shape) != tuple(self.cond.shape):
                raise ValueError(f"FlashStep.step: a step with a deformer takes the frame's condition [{self.cond.shape[0]}] "
                                 f"where it took `deform`, not a tensor of shape {tuple(deform.shape)}")
            extra = [(self.cond, deform.detach())]
        elif tuple(deform.shape) != tuple(self.deform.shape):
            raise ValueError(f"FlashStep.step: deform must be [{self.pc.P},{DEFORM_COLS}]")
        else:
            extra = [(self.deform, deform.detach())]
        if mouth_mask is not None:
            extra.append((self.mask, mouth_mask.detach().reshape(self.mask.shape)))
        self.schedule_steps += 1
        on = self.lpips is not None and self.schedule_steps > self.lpips_start
        if on != self._lpips_on:       # the schedule's crossing: the captured step does not hold the launch (or holds it: a restored count)
            self._lpips_on, self._graph, self._eager_steps = on, None, 0
            self.lpips_switches += 1
            if not on:
                self.lpips_loss.zero_()
        return super().step(camera, posed_verts.detach(), gt_image, extra)

    # ---- FlashAvatar has no density control, and the step no data-parallel form
    def densify_by_gradient(self, *a, **k):
        raise NotImplementedError("FlashStep: FlashAvatar's point set is fixed (no density control in the reference)")

    def prune_low_opacity(self, *a, **k):
        raise NotImplementedError("FlashStep: FlashAvatar's point set is fixed (no density control in the reference)")

    def reduce_densification_stats(self, *a, **k):
        raise NotImplementedError("FlashStep: data-parallel runs are not built (DESIGN.md)")

    # ---- checkpoints: 'model' holds the five parameters under the reference's names and the two binding buffers
    #      (deserialize_checkpoints_flashavatar, train/deserialize.py:44-53: model.load_state_dict of exactly these, next to
    #      the deformation MLP's and FLAME's entries, which are returned as ignored keys)
    GAUSSIAN_ATTRIBUTES = ["_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "face_index", "bary_coords"]
    RESUME_REMAPPED = False     # resumes FRESH

    # with a deformer the checkpoint's 'model' also carries the network under the reference's `deformNet.*` names, and
    # `deformer_optimizer` (an addition, like `optimizer`) its Adam state
    def _save_extras(self, sd: dict) -> None:
        if self.deformer is not None:
            sd["model"].update(self.deformer.state_dict(DEFORM_PREFIX))
            a = self.deformer_adam
            sd["deformer_optimizer"] = {"exp_avg": a.exp_avg.clone(), "exp_avg_sq": a.exp_avg_sq.clone(), "state": a.state_words()}

    def _load_extras(self, sd: dict, g: dict) -> None:
        if self.deformer is not None:
            self.deformer.check_state_dict(sd["model"], DEFORM_PREFIX)
            if int(g["_opacity"].shape[0]) != self.deformer.N:
                raise ValueError(f"FlashStep: the checkpoint holds {int(g['_opacity'].shape[0])} Gaussians, the deformer is built "
                                 f"over {self.deformer.N} points")

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> list:
        """BoundStep.load_state_dict; with a deformer the `deformNet.*` entries are LOADED (in place) instead of being returned
        as ignored, and `deformer_optimizer`, if the checkpoint has one, restores the network's Adam (else it starts fresh).
        The LPIPS schedule goes on at the checkpoint's `global_step` (train/loader.py:102), with or without an `optimizer` entry."""
        ignored = super().load_state_dict(sd)
        self.schedule_steps = int(sd["global_step"]) if "global_step" in sd else self.host_steps
        if self.deformer is None:
            return ignored
        self.deformer.load_state_dict(sd["model"], DEFORM_PREFIX)
        opt = sd.get("deformer_optimizer")
        if opt is not None:
            self.deformer_adam.exp_avg.copy_(opt["exp_avg"])
            self.deformer_adam.exp_avg_sq.copy_(opt["exp_avg_sq"])
            self.deformer_adam.load_state_words(opt["state"])
        mine = set(self.deformer.state_dict(DEFORM_PREFIX))
        return [k for k in ignored if k not in mine]


__all__ = ["DEFORM_COLS", "FLASH_LRS", "FlashGaussians", "FlashStep", "REFERENCE_LPIPS_START", "REFERENCE_LPIPS_WEIGHT"]
