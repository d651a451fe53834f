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
  * the image term — `GaussianAvatarsLoss` (train/loss.py:351-365): rgb_weight x L1 + dssim_weight x d_ssim with the weights of
    config/gaussianavatars.yaml:16-20: `RiggedStep(image_loss=REFERENCE_IMAGE_LOSS)`, two launches in the L1 launch's place
    (`loss.image_loss_and_grad`)
  * the scale / xyz regularisers — `GaussianAvatarsLoss.accumulate_gradients` (train/loss.py:367-379) with the weights and
    thresholds of config/gaussianavatars.yaml: `RiggedStep(regularisers=...)`, one more launch inside the captured step
    (`loss.gaussian_regularisers`) that adds their gradients in front of Adam
  * density control — `_densify_and_prune`, `_clone_densify`, `_split_densify`, `_prune` with `binding_counter`,
    `_reset_opacity` (gaussianavatars.py:278-495): `RiggedStep.densify_and_prune / prune / prune_low_opacity /
    reset_opacity`, torch index surgery between steps
Not here: the position learning-rate schedule, `max_radii2D` (see `densify_and_prune`), a multi-lane batch step, data-parallel runs, FLAME.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from .binding import bind_gaussians_face_local
from .bound import FaceLocalBinding, render_bound_batch
from .flat import FlatParams
from .loss import ImageLoss, gaussian_regularisers, regulariser_workspace
from .model import TorchCamera
from .render import render
from .gs_utils import build_rotation
from .train import CloneSplitStep

# config/gaussianavatars.yaml:26-31 (group names of train/optim.py:73-80; position_lr_init: the schedule is out of scope)
RIGGED_LRS = dict(xyz=0.005, opacity=0.05, feature_dc=0.0025, feature_rest=0.0025 / 20, rotation=0.001, scaling=0.017)


class Regularisers(NamedTuple):
    """The scale / xyz regularisers of GaussianAvatarsLoss (train/loss.py:367-379)."""
    scale_weight: float
    xyz_weight: float
    threshold_scale: float
    threshold_xyz: float


# the reference's values (config/gaussianavatars.yaml:13-20)
REFERENCE_REGULARISERS = Regularisers(scale_weight=1.0, xyz_weight=0.01, threshold_scale=0.6, threshold_xyz=1.0)
# rgb_weight, dssim_weight of the image term (config/gaussianavatars.yaml:16-20)
REFERENCE_IMAGE_LOSS = ImageLoss(rgb_weight=0.8, dssim_weight=0.2)


class RiggedGaussians(FlatParams):
    """The face-bound Gaussian parameters of GaussianAvatars in ONE flat buffer, in the order of the optimizer groups
    (train/optim.py:73-80).  `binding` [P] is the face of every Gaussian (gaussianavatars.py:52-60)."""
    max_sh_degree = 3        # config/gaussianavatars.yaml:23
    FIELDS = (("_xyz", 3), ("_opacity", 1), ("_features_dc", 3), ("_features_rest", 45), ("_rotation", 4), ("_scaling", 3))
    SHAPES = {"_xyz": (3,), "_opacity": (1,), "_features_dc": (1, 3), "_features_rest": (15, 3), "_rotation": (4,),
              "_scaling": (3,)}
    ROW_BUFFERS = (("binding", torch.int32, "new_binding"),)
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
    def get_features(self) -> torch.Tensor:
        """[P,16,3]: GaussianModel.get_features (volume_rendering/gaussian_model.py:119-122)."""
        return torch.cat((self._features_dc, self._features_rest), dim=1)


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


class RiggedStep(CloneSplitStep):
    """One optimisation step of GaussianAvatars per call: `step(camera, posed_verts, gt_image)` —
    bind in the frame -> render -> L1 -> backward -> densification statistics -> Adam.  The optimizer groups are those of
    train/optim.py:73-80 with config/gaussianavatars.yaml:26-31."""
    LRS = RIGGED_LRS
    LR_KEYS = {"_xyz": "xyz", "_opacity": "opacity", "_features_dc": "feature_dc", "_features_rest": "feature_rest",
               "_rotation": "rotation", "_scaling": "scaling"}

    def __init__(self, pc: RiggedGaussians, faces: torch.Tensor, camera: TorchCamera, bg: torch.Tensor, verts: torch.Tensor,
                 lrs: Optional[dict] = None, use_graph: bool = True, fold_binding: bool = True,
                 regularisers: Optional[Regularisers] = None, image_loss: Optional[ImageLoss] = None, vertex_grad: bool = False):
        """`verts` [V,3]: any pose of the mesh (sizes the step's static vertex buffer and is its first content).
        `fold_binding` (default): the binding is evaluated inside the rasterizer's per-Gaussian kernels (fr_aux::binding with
        FR_BIND_FACE_LOCAL) — no binding launches.  False: the stand-alone `bind_gaussians_face_local` op in front of
        render() (same results; the A/B and the op's own user).
        `regularisers`: a `Regularisers` (REFERENCE_REGULARISERS holds the reference's values) adds the scale / xyz terms of
        train/loss.py:367-379 to every step — one launch between the backward and Adam; `reg_loss` then holds the step's
        unweighted (scale_loss, xyz_loss).  None (default): no such launch, `reg_loss` is None.
        `image_loss`: an `ImageLoss` (REFERENCE_IMAGE_LOSS holds the reference's 0.8 / 0.2) makes the image term
        rgb_weight x L1 + dssim_weight x d_ssim (train/loss.py:351-365) — two launches where the L1 launch is; `loss_terms`
        then holds the step's (weighted image loss, l1, d_ssim) and `loss` is its first word.  None (default): the image
        term is L1 with weight 1, `loss_terms` is None.
        `vertex_grad`: `d_verts` [V,3] holds every step's dLoss/dposed_verts (BoundStep)."""
        super().__init__(pc, faces, camera, bg, verts, lrs, use_graph, fold_binding, image_loss, data_parallel=False,
                         vertex_grad=vertex_grad)
        self.regularisers = None if regularisers is None else Regularisers(*[float(x) for x in regularisers])
        # the reference's out['scale_loss'] / out['xyz_loss'] of the step (unweighted), written by the regulariser launch
        self.reg_loss = None if regularisers is None else torch.zeros(2, device=self.dev)
        self._reg_ws = None if regularisers is None else regulariser_workspace(self.dev)
        self.n_faces = int(self.faces.shape[0])
        self._check_binding(pc.binding)
        self._count_binding()

    def _check_binding(self, binding: torch.Tensor) -> None:
        """Refuses a `binding` out of the mesh's range (reads device state: the constructor and load_state_dict only)."""
        if binding.numel() and (int(binding.min()) < 0 or int(binding.max()) >= self.n_faces):
            raise ValueError("RiggedStep: `binding` names a face the mesh does not have")

    def _count_binding(self) -> None:
        """binding_counter [F] int32: Gaussians per face (gaussianavatars.py:66-69)."""
        self.binding_counter = torch.bincount(self.pc.binding.long(), minlength=self.n_faces).to(torch.int32)

    def _buffers_moved(self, old_index, old_rows, *, stats):
        """... and the rows with them: binding_counter is counted again — THE place that keeps it equal to bincount(binding)
        (the reference adds to it in clone and split, :313-315, :374-377, and subtracts in _prune)."""
        super()._buffers_moved(old_index, old_rows, stats=stats)
        self._count_binding()

    def _forward_backward(self):
        pc = self.pc
        pc.begin_step()                                             # zero_grad(set_to_none=True)
        stats = (self.xyz_gradient_accum, self.denom, pc.overflow_word)
        verts = self._vertex_leaf(self.verts)
        if self.fold_binding:
            from . import rasterizer
            out = render_bound_batch([self.cam], [_RiggedFrame(pc, stats)], [verts], FaceLocalBinding(self.faces, pc.binding),
                                     self.bg, slots=[rasterizer._slot])[0]
        else:
            bound = bind_gaussians_face_local(verts, self.faces, pc.binding, pc._xyz, pc._rotation, pc._scaling)
            out = render(self.cam, _RiggedFrame(pc, stats, bound), self.bg)
        out["render"].backward(self._image_loss_and_grad(out["render"]))   # see TrainStep
        self._keep_vertex_grad(verts)
        pc.collect_grads()                                          # (the SH halves: see FlatParams.collect_grads)
        if self.regularisers is not None:
            # train/loss.py:367-379: weight x the two regularisers' gradients are ADDED to the image term's, in front of Adam.
            # A replay that overflowed its binning capacity back-propagated zeros and its Adam launch skips the step (the
            # overflow word): what this launch added to the zeroed gradient is then never applied — harmless.
            r = self.regularisers
            gaussian_regularisers(pc._scaling, pc._xyz, pc.grad_view("_scaling"), pc.grad_view("_xyz"), out=self.reg_loss,
                                  weights=(r.scale_weight, r.xyz_weight), thresholds=(r.threshold_scale, r.threshold_xyz),
                                  workspace=self._reg_ws)
        self.out = self._kept(out)

    def update_sh_degree(self) -> int:
        """_update_sh_degree (gaussianavatars.py:497-499).  The degree is a launch argument of the captured kernels: the step
        is captured again on its next call.  Returns the active degree."""
        pc = self.pc
        if pc.active_sh_degree < pc.max_sh_degree:
            pc.active_sh_degree += 1
            self._graph = None
        return pc.active_sh_degree

    # ---- GaussianAvatars' density control (gaussianavatars.py:278-495): CloneSplitStep's, with the binding_counter guard
    def _prune_guard(self, mask: torch.Tensor) -> torch.Tensor:
        """If a face would lose ALL of its Gaussians none of its marked ones is removed (binding_counter guard,
        gaussianavatars.py:420-424); otherwise all of them are."""
        b = self.pc.binding.long()
        marked = torch.bincount(b[mask], minlength=self.n_faces).to(torch.int32)
        return mask & ((self.binding_counter - marked) > 0)[b]

    def _split_children(self, rows, sel, samples, N):
        """Children at R(_rotation) . sample + _xyz on the parent's face, everything else repeated (:353-416)."""
        i_xyz, i_rot = self._field_index("_xyz"), self._field_index("_rotation")
        rows[i_xyz] = torch.bmm(build_rotation(rows[i_rot]), samples.unsqueeze(-1)).squeeze(-1) + rows[i_xyz]
        return rows, dict(new_binding=self.pc.binding[sel].repeat(N))

    def densify_and_prune(self, max_grad: float = 1e-4, min_opacity: float = 0.005, extent: float = 2.0,
                          max_screen_size=None, generator: Optional[torch.Generator] = None):
        """_densify_and_prune with _clone_densify and _split_densify (gaussianavatars.py:278-416): CloneSplitStep's, which
        states the rule — grads :281-282, clone :297-351 (on the same face), split :353-416 (`_split_children`; the selected
        originals go through the guarded prune), final prune :287-293.  Returns (cloned, split, pruned) row counts."""
        return super().densify_and_prune(max_grad, min_opacity, extent, max_screen_size, generator)

    def densify_by_gradient(self, *a, **k):
        raise NotImplementedError("RiggedStep: the rigged set densifies with densify_and_prune() (GaussianAvatars' clone / split)")

    # ---- checkpoints: 'model' holds what GaussianAvatars.state_dict() holds of the Gaussians (the six parameters and the
    #      `binding` buffer); 'optimizer', 'densification' and 'active_sh_degree' are what a seamless resume needs on top
    GAUSSIAN_ATTRIBUTES = ["_xyz", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "binding"]
    RESUME_REMAPPED = False     # resumes FRESH

    def _save_extras(self, sd: dict) -> None:
        sd["active_sh_degree"] = int(self.pc.active_sh_degree)

    def _load_extras(self, sd: dict, g: dict) -> None:
        self._check_binding(g["binding"])
        self.pc.active_sh_degree = int(sd.get("active_sh_degree", self.pc.active_sh_degree))   # (the recount: _buffers_moved)
