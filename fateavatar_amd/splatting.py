"""SplattingAvatar — the reference's Phong-surface baseline — on the fused path: Gaussians embedded in the posed mesh by
(face, barycentrics, offset along the interpolated normal), SH degree 0, one optimisation step per call.

reference:
  * parameters — `_register_init_gaussian` (model/baseline/splattingavatar.py:147-183): `num_init_samples` (10 000,
    config/splattingavatar.yaml:23) points sampled on the canonical mesh by `sample_bary_on_triangles` (:725-736), `_uvd` 0,
    colour RGB2SH(0.5), log sqrt of the mean squared distance to the 3 nearest samples (distCUDA2, clamped at 1e-7), identity
    rotation, opacity 0.1, `max_sh_degree` 0 (:217: `_features_rest` is [N,0,3])
  * their Adam groups — `_uvd, _opacity, _features_dc, _features_rest, _rotation, _scaling` in that order (train/optim.py:106-117)
    with the rates of config/splattingavatar.yaml:26-30, `_features_rest` at feature_dc_lr / 20
  * a frame — `forward` :203-246: the per-frame mesh pass (vertex normals, per-vertex quaternions, face area ratios:
    `binding.phong_frame`), every Gaussian placed on the Phong surface (`binding.bind_gaussians_phong`), then render()
What is fused: the mesh pass is one launch, the per-Gaussian binding runs inside the rasterizer's per-Gaussian kernels
(bound.render_bound_batch with a PhongBinding; `fold_binding=False` keeps the stand-alone op as the A/B), activations and
densification statistics run inside the rasterizer kernels, one L1 launch, one Adam launch over the flat buffer, the whole
step — mesh pass included — ONE HIP graph.

  * the objective — `SplattingAvatarLoss.accumulate_gradients` (train/loss.py:288-323) with config/splattingavatar.yaml:13-20:
    1.0 x L1 + 10.0 x MSE + 1.0 x the scale term + 0.01 x LPIPS.  `SplattingStep(image_loss=REFERENCE_IMAGE_LOSS)`:
    one launch in the L1 launch's place (`loss.pixel_loss_and_grad`); `SplattingStep(scale_term=REFERENCE_SCALE_TERM)`: two more
    launches inside the captured step (`loss.scale_term_and_grad`) that add the term's gradient in front of Adam;
    `SplattingStep(lpips=Lpips(..., weight=REFERENCE_LPIPS_WEIGHT))`: one call behind the image-loss launch (csrc/fr_vgg.hip's
    fr_lpips_loss_grad) that adds the term's gradient to the image gradient.  All are opt-in: the default step optimises L1
    alone.  The LPIPS term's weights (torchvision's VGG-16 and the `lpips` package's linear layers) are the caller's to load
    (`perceptual.Lpips.from_state_dicts`); none are shipped

  * density control and the triangle walk — `_densify_and_prune`, `_clone_densify`, `_split_densify`, `_prune`,
    `_walking_on_triangles`, `_reset_opacity` (:386-715): `SplattingStep.densify_and_prune / prune / prune_low_opacity /
    walk_on_triangles / reset_opacity`, between step() calls.  The reference's schedule (config/splattingavatar.yaml:35-44,
    train/iteration.py:271-298) densifies every 100 steps from 600, resets opacity every 3 500 and walks every 100.  What the
    reference keeps on the CPU for this (submodules/simple_phongsurf: the C++ walk, and `update_corres_spt`'s ~100 x 40 small
    launches and four blocking copies per densification) is two HIP kernels here (`phongsurf.PhongSurface`): the walk moves
    the embedding in place, so the captured step survives it.  With the reference's forward, which reads `_uvd[..., -1:]`
    alone, the `u, v` columns of `_uvd` only ever hold zeros and the walk leaves every interior Gaussian where it is — exactly
    as in the reference.

NOT here:
  * camera gradients for this step (render through a model.PoseCamera), and FLAME itself: `SplattingStep(mesh_grad=True)` hands
    dLoss/dposed_verts back (`d_verts`), the mesh's own parameters and their optimizer stay the caller's torch
  * data-parallel runs of the step (`reduce_densification_stats`)
  * `max_radii2D` (see `densify_and_prune`)
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .binding import PhongCanonical, PhongGradBuffers, bind_gaussians_phong, phong_canonical, phong_frame
from .bound import PhongBinding, PosedPhongBinding, render_bound_batch
from .flat import FlatParams
from .gs_utils import RGB2SH, build_rotation
from .loss import PixelLoss, ScaleTerm, scale_term_and_grad, scale_term_workspace
from .model import TorchCamera
from .phongsurf import PhongSurface, triwalk
from .render import render
from .train import CloneSplitStep

# config/splattingavatar.yaml:26-30 (group names of train/optim.py:106-117)
SPLATTING_LRS = dict(uvd=0.00016, opacity=0.05, feature_dc=0.0025, feature_rest=0.0025 / 20, rotation=0.001, scaling=0.005)
NUM_INIT_SAMPLES = 10_000   # config/splattingavatar.yaml:23
# config/splattingavatar.yaml:13-20 (SplattingAvatarLoss.Params, train/loss.py:261-268)
REFERENCE_IMAGE_LOSS = PixelLoss(rgb_weight=1.0, mse_weight=10.0)
REFERENCE_SCALE_TERM = ScaleTerm(weight=1.0, scale_threshold=10.0, max_scaling=0.008)
REFERENCE_LPIPS_WEIGHT = 0.01


def sample_bary_on_triangles(num_faces: int, num_samples: int, generator: Optional[torch.Generator] = None):
    """sample_bary_on_triangles (model/baseline/splattingavatar.py:725-736) with a seeded generator: (face of every sample
    [n] int64, barycentrics [n,3] — u uniform, v uniform in the rest, w the remainder, then shuffled per row).  Faces are drawn
    uniformly, not by area, as in the reference."""
    bary = torch.zeros(num_samples, 3)
    bary[:, 0] = torch.rand(num_samples, generator=generator)
    bary[:, 1] = torch.rand(num_samples, generator=generator) * (1.0 - bary[:, 0])
    bary[:, 2] = 1.0 - bary[:, 0] - bary[:, 1]
    fidxs = torch.randint(0, num_faces, size=(num_samples,), generator=generator)
    indices = torch.argsort(torch.rand(num_samples, 3, generator=generator), dim=-1)
    return fidxs, torch.gather(bary, dim=-1, index=indices)


class SplattingGaussians(FlatParams):
    """SplattingAvatar's Gaussian parameters in ONE flat buffer, in the order of the optimizer groups (train/optim.py:106-117).
    `face_index` [P] / `bary_coords` [P,3] are every Gaussian's embedding (`sample_fidxs`, `sample_bary`): moved in place by
    `SplattingStep.walk_on_triangles`, rebuilt with the rows by the density control."""
    max_sh_degree = 0        # :217
    FIELDS = (("_uvd", 3), ("_opacity", 1), ("_features_dc", 3), ("_features_rest", 0), ("_rotation", 4), ("_scaling", 3))
    SHAPES = {"_uvd": (3,), "_opacity": (1,), "_features_dc": (1, 3), "_features_rest": (0, 3), "_rotation": (4,),
              "_scaling": (3,)}
    ROW_BUFFERS = (("face_index", torch.int32, "new_face_index"), ("bary_coords", torch.float32, "new_bary"))
    fused_activations = True

    def __init__(self, face_index, bary_coords, log_scale, device):
        """_register_init_gaussian (:147-183) for Gaussians embedded at (`face_index` [P], `bary_coords` [P,3]); `log_scale`:
        the initial `_scaling` value(s), a float or [P] (`log(sqrt(distCUDA2))` of the sampled points: `SplattingGaussians.sample`)."""
        super().__init__()
        self.face_index = torch.as_tensor(face_index).to(device, torch.int32).contiguous()
        self.bary_coords = torch.as_tensor(bary_coords).to(device, torch.float32).contiguous()
        P = int(self.face_index.shape[0])
        if self.bary_coords.shape != (P, 3):
            raise ValueError("SplattingGaussians: face_index [P], bary_coords [P,3]")
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
        dc = torch.full((P, 1, 3), float(RGB2SH(0.5)), dtype=torch.float32, device=device)          # :151-158
        rot = z(P, 4)
        rot[:, 0] = 1
        op = torch.full((P, 1), float(np.log(0.1 / 0.9)), dtype=torch.float32, device=device)       # inverse_sigmoid(0.1)
        scl = torch.as_tensor(log_scale, dtype=torch.float32).to(device).reshape(-1, 1).expand(P, 3)   # :164
        self.active_sh_degree = 0
        self._bind([z(P, 3), op, dc, z(P, 0, 3), rot, scl.contiguous()])

    @classmethod
    def sample(cls, cano_verts: torch.Tensor, faces: torch.Tensor, num_samples: int = NUM_INIT_SAMPLES,
               generator: Optional[torch.Generator] = None) -> "SplattingGaussians":
        """`_sample_initial_points` + `_register_init_gaussian` (:128-183) on the canonical mesh (device tensors): the samples
        of `sample_bary_on_triangles`, scales from this project's `distCUDA2` of the sampled points."""
        from .knn import distCUDA2
        dev = cano_verts.device
        fidxs, bary = sample_bary_on_triangles(int(faces.shape[0]), int(num_samples), generator)
        tri = cano_verts.detach().float()[faces.long()][fidxs.to(dev)]
        points = torch.einsum("nij,ni->nj", tri, bary.to(dev)).contiguous()                         # :136
        dist2 = torch.clamp_min(distCUDA2(points), 0.0000001)                                       # :163
        return cls(fidxs, bary, torch.log(torch.sqrt(dist2)), dev)

    @property
    def get_features(self) -> torch.Tensor:
        """[P,1,3]: GaussianModel.get_features (volume_rendering/gaussian_model.py:119-122) at SH degree 0."""
        return torch.cat((self._features_dc, self._features_rest), dim=1)


class _SplattingFrame:
    """What render() / render_bound_batch() read of a Gaussian holder for one frame."""
    fused_activations = True
    max_sh_degree = active_sh_degree = 0

    def __init__(self, pc: SplattingGaussians, stats, bound=None):
        self._opacity, self.get_features = pc._opacity, pc.get_features
        if bound is None:     # raw parameters: the rasterizer evaluates the binding itself
            self._uvd, self._rotation, self._scaling = pc._uvd, pc._rotation, pc._scaling
        else:                 # the stand-alone op's outputs
            self.get_xyz, self._rotation, self._scaling = bound
        self.fused_densification_stats = stats


class SplattingStep(CloneSplitStep):
    """One optimisation step of SplattingAvatar per call: `step(camera, posed_verts, gt_image)` —
    mesh pass -> bind in the frame -> render -> L1 -> backward -> densification statistics -> Adam.  The optimizer groups are
    those of train/optim.py:106-117 with config/splattingavatar.yaml:26-30 (`_features_rest` is empty at SH degree 0: its
    group keeps its place and rate)."""
    LRS = SPLATTING_LRS
    VERTEX_GRAD = False
    VERTEX_GRAD_MISSING = ("the Phong-surface binding has no vertex gradient under this name (fr_backward refuses "
                           "fr_aux::d_verts in that mode); its vertex gradient is two calls of its own behind the frame: "
                           "ask for it with `mesh_grad=True`")
    LR_KEYS = {"_uvd": "uvd", "_opacity": "opacity", "_features_dc": "feature_dc", "_features_rest": "feature_rest",
               "_rotation": "rotation", "_scaling": "scaling"}

    def __init__(self, pc: SplattingGaussians, canonical: PhongCanonical, camera: TorchCamera, bg: torch.Tensor, verts: torch.Tensor,
                 lrs: Optional[dict] = None, use_graph: bool = True, fold_binding: bool = True, vertex_grad: bool = False,
                 mesh_grad: bool = False, image_loss=None, scale_term: Optional[ScaleTerm] = None, lpips=None):
        """`canonical`: `binding.phong_canonical(cano_verts, faces)`; `verts` [V,3]: any pose of the mesh (sizes the step's
        static vertex buffer and is its first content).  `fold_binding` (default): the per-Gaussian binding is evaluated
        inside the rasterizer's per-Gaussian kernels (fr_aux::binding with FR_BIND_PHONG).  False: the stand-alone
        `bind_gaussians_phong` op in front of render() (same results; the A/B and the op's own user).
        `mesh_grad`: after every `step()`, `d_verts` [V,3] holds THIS step's dLoss/dposed_verts — through the barycentric
        point, the vertex normals, the per-vertex quaternions and the face area ratios, as the reference's autograd forms it
        (splattingavatar.py:203-246) — like `AvatarStep(vertex_grad=True)`: the caller goes on with
        `posed_verts.backward(step.d_verts)` into whatever made the mesh.  One preallocated buffer (`PhongGradBuffers`, per
        mesh, not per Gaussian: density control leaves it alone); its zeroing, the per-Gaussian scatter and the mesh pass's
        backward are launches of the step, inside its captured graph.  Parameters and moments are what they are without it.
        `vertex_grad=True` raises: that name stays the refusal it was; the gradient is asked for as `mesh_grad`.
        `image_loss`: a `PixelLoss` (REFERENCE_IMAGE_LOSS holds the reference's 1.0 / 10.0) makes the image term
        rgb_weight x L1 + mse_weight x MSE (train/loss.py:288-304) — one launch where the L1 launch is; `loss_terms` then holds
        the step's (weighted image loss, l1, mse) and `loss` is its first word.  (An `ImageLoss` gives L1 + D-SSIM, as in every
        step.)  None (default): the image term is L1 with weight 1, `loss_terms` is None.
        `scale_term`: a `ScaleTerm` (REFERENCE_SCALE_TERM holds the reference's values) adds the scale term of
        train/loss.py:307-315 to every step — two launches between the backward and Adam; `reg_loss` then holds the step's
        unweighted scale_loss and the number of rows it selected.  None (default): no such launch, `reg_loss` is None.
        `lpips`: a `perceptual.Lpips` (the reference's weight: REFERENCE_LPIPS_WEIGHT) adds the LPIPS term of
        train/loss.py:259-323 to every step: ONE call behind the image-loss launch adds weight x its gradient to the step's
        image-gradient buffer, in front of the rasterizer's backward; `lpips_loss` [1 + T] then holds the step's UNWEIGHTED
        terms (their sum first); `loss` and `loss_terms` keep their meaning.  None (default): not one launch changes."""
        self._init_lpips(lpips, pc)
        if scale_term is not None and not isinstance(scale_term, ScaleTerm):
            raise TypeError(f"SplattingStep: `scale_term` is a ScaleTerm or None, not {type(scale_term).__name__}")
        self.mesh_grad = bool(mesh_grad)
        self.canonical = PhongCanonical(*[t.to(pc.flat.device).contiguous() for t in canonical])
        if pc.P and (int(pc.face_index.min()) < 0 or int(pc.face_index.max()) >= int(self.canonical.faces.shape[0])):
            raise ValueError("SplattingStep: `face_index` names a face the mesh does not have")
        super().__init__(pc, self.canonical.faces, camera, bg, verts, lrs, use_graph, fold_binding, image_loss, data_parallel=False,
                         vertex_grad=vertex_grad)
        self.scale_term = None if scale_term is None else ScaleTerm(*[float(x) for x in scale_term])
        # the reference's out['scale_loss'] of the step (unweighted) and the rows it averaged over, written by the term's launch;
        # the scratch is the step's own and its size does not depend on P: density control leaves both alone
        self.reg_loss = None if scale_term is None else torch.zeros(2, device=self.dev)
        self._scale_ws = None if scale_term is None else scale_term_workspace(self.dev)
        if self.mesh_grad:
            self._mesh_buffers = PhongGradBuffers(self.verts.shape[0], self.faces.shape[0], self.dev, zeroed=True)
            self.d_verts = self._mesh_buffers.d_verts

    def step(self, camera: TorchCamera, posed_verts: torch.Tensor, gt_image: torch.Tensor, _extra=()) -> torch.Tensor:
        if self.mesh_grad:
            posed_verts = posed_verts.detach()     # (as BoundStep.step with vertex_grad: only the values are loaded)
        return super().step(camera, posed_verts, gt_image, _extra)

    def _forward_backward(self):
        pc = self.pc
        pc.begin_step()                                             # zero_grad(set_to_none=True)
        stats = (self.xyz_gradient_accum, self.denom, pc.overflow_word)
        verts, binding = self.verts, PhongBinding
        if self.mesh_grad:     # a leaf over the static buffer's storage (no copy) that carries the step's gradient buffers
            verts, binding = self.verts.detach().requires_grad_(True), PosedPhongBinding
            verts._fr_phong_grad = self._mesh_buffers
        if self.fold_binding:
            from . import rasterizer
            out = render_bound_batch([self.cam], [_SplattingFrame(pc, stats)], [verts],
                                     binding(self.faces, pc.face_index, pc.bary_coords, self.canonical), self.bg,
                                     slots=[rasterizer._slot])[0]
        else:
            frame = phong_frame(self.canonical, verts, differentiable=self.mesh_grad)
            bound = bind_gaussians_phong(verts, self.faces, pc.face_index, pc.bary_coords, frame, pc._uvd, pc._rotation,
                                         pc._scaling)
            out = render(self.cam, _SplattingFrame(pc, stats, bound), self.bg)
        g = self._image_loss_and_grad(out["render"])                       # see TrainStep
        self._add_lpips(out["render"], g)
        out["render"].backward(g)
        if self.mesh_grad and not self.fold_binding:     # (the ops' backward allocates its own: copied into the step's buffer)
            self.d_verts.copy_(verts.grad)
        pc.collect_grads()
        if self.scale_term is not None:
            # train/loss.py:307-315: weight x the scale term's gradient is ADDED to the image term's, in front of Adam.
            # A replay that overflowed its binning capacity back-propagated zeros and its Adam launch skips the step (the
            # overflow word): what this launch added to the zeroed gradient is then never applied — harmless.
            scale_term_and_grad(pc._scaling, pc.grad_view("_scaling"), out=self.reg_loss, terms=self.scale_term,
                                workspace=self._scale_ws)
        self.out = self._kept(out)

    # ---- SplattingAvatar's density control, triangle walk and opacity reset (:386-715): the density control is CloneSplitStep's
    #      with the children re-embedded on the canonical mesh; `reset_opacity` is TrainStep's (:697-715 is the same rule), in place
    @property
    def phongsurf(self) -> PhongSurface:
        """The canonical mesh's Phong surface as the reference constructs it (:122-125: outer_loop 2, inner_loop 50, 'uvd'), with
        the canonical vertex normals `phong_frame(canonical, cano_verts)[0]`.  Made on first use."""
        if getattr(self, "_phongsurf", None) is None:
            c = self.canonical
            self._phongsurf = PhongSurface(c.cano_verts, c.faces, phong_frame(c, c.cano_verts)[0], outer_loop=2, inner_loop=50,
                                           method="uvd")
        return self._phongsurf

    @torch.no_grad()
    def walk_on_triangles(self) -> None:
        """_walking_on_triangles (:668-695): every Gaussian walks over the mesh by `_uvd[:, :2]` (one launch, in place: the
        embedding buffers, the parameters and the moments keep their addresses, so the captured step and the step count are
        kept), then those two columns and the matching columns of both Adam moments are zeroed."""
        pc, surf = self.pc, self.phongsurf
        triwalk(surf.faces_nbr, pc.face_index, pc.bary_coords, pc._uvd.detach(), surf.status, surf.decay)
        pc._uvd.data[:, :2] = 0
        i, P = self._field_index("_uvd"), pc.P
        off = P * sum(pc.widths()[:i])
        for m in (self.adam.exp_avg, self.adam.exp_avg_sq):
            m[off:off + 3 * P].view(P, 3)[:, :2] = 0

    def _split_children(self, rows, sel, samples, N):
        """Children at R(_rotation) . sample + xyz_cano (:473-574).  `xyz_cano` is the reference's MIXTURE (:490-502), kept: the
        barycentric point on the step's CURRENT POSED vertices (the last frame's) plus the CANONICAL interpolated normal times
        `_uvd[:, 2]`.  The children are re-embedded on the canonical mesh by `PhongSurface.update_corres_spt` (:517) starting
        from the parent's face and (u, v): bary = (u, v, 1 - u - v), `_uvd` = (0, 0, the parent's d) — the fitted d is
        discarded, as in the reference —, everything else repeated.  `self.last_fit_iterations` holds the fit's iteration count
        per outer round (empty if nothing was split)."""
        pc = self.pc
        i_uvd, i_rot = self._field_index("_uvd"), self._field_index("_rotation")
        fidx, bary = pc.face_index[sel].repeat(N), pc.bary_coords[sel].repeat(N, 1)
        self.last_fit_iterations = []
        if fidx.numel():
            surf = self.phongsurf
            corners = self.faces.long()[fidx.long()]
            base_xyz = torch.einsum("nij,ni->nj", self.verts[corners], bary)                                   # :490-493
            base_normal = torch.nn.functional.normalize(torch.einsum("nij,ni->nj", surf.N[corners], bary), dim=-1)
            xyz_cano = base_xyz + base_normal * rows[i_uvd][:, 2:]
            new_xyz = torch.bmm(build_rotation(rows[i_rot]), samples.unsqueeze(-1)).squeeze(-1) + xyz_cano
            fidx, uv = surf.update_corres_spt(new_xyz, None, fidx, bary[:, :2].contiguous())                   # :517
            bary = torch.cat([uv, 1.0 - uv[:, 0:1] - uv[:, 1:2]], dim=-1)
            self.last_fit_iterations = surf.fit_iterations()
        rows[i_uvd] = torch.cat([torch.zeros_like(rows[i_uvd][:, :2]), rows[i_uvd][:, 2:]], dim=-1)
        return rows, dict(new_face_index=fidx, new_bary=bary)

    def densify_and_prune(self, max_grad: float = 2e-4, min_opacity: float = 0.005, extent: float = 2.0, max_screen_size=None,
                          generator: Optional[torch.Generator] = None):
        """_densify_and_prune with _clone_densify and _split_densify (:386-574): CloneSplitStep's, which states the rule — grads
        :389-390, clone :407-470 (with their face_index / bary_coords), split :473-574 (`_split_children`), final prune
        :395-404.  Returns (cloned, split, pruned) row counts."""
        return super().densify_and_prune(max_grad, min_opacity, extent, max_screen_size, generator)

    def densify_by_gradient(self, *a, **k):
        raise NotImplementedError("SplattingStep: the set densifies with densify_and_prune() (SplattingAvatar's clone / split)")

    def reduce_densification_stats(self, *a, **k):
        raise NotImplementedError("SplattingStep: data-parallel runs are not built (DESIGN.md)")

    # ---- checkpoints: 'model' holds the six parameters under the reference's names and the embedding buffers
    GAUSSIAN_ATTRIBUTES = ["_uvd", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "sample_fidxs",
                           "sample_bary"]
    ROW_BUFFER_KEYS = {"face_index": "sample_fidxs", "bary_coords": "sample_bary"}
    RESUME_REMAPPED = False     # resumes FRESH


__all__ = ["NUM_INIT_SAMPLES", "REFERENCE_IMAGE_LOSS", "REFERENCE_LPIPS_WEIGHT", "REFERENCE_SCALE_TERM", "SPLATTING_LRS", "SplattingGaussians", "SplattingStep", "phong_canonical", "sample_bary_on_triangles"]
