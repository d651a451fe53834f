"""FateAvatar's own per-frame optimisation loop around the path (BASELINE.json configs[2]).

reference:
  * parameters and their Adam groups — `_opacity, _offset, _features_dc, _rotation, _scaling` in that order
    (train/optim.py:15-21), learning rates of config/fateavatar.yaml:34-39, Adam(eps 1e-8, default betas)
  * a frame — model/fateavatar.py:225-276: the Gaussians are BOUND to the posed mesh (`bind_gaussians`: position =
    barycentric point + normal * shell_len * tanh(offset); rotation = face quaternion (x) rotation; scaling += log of
    the face's scale ratio), rendered with SH degree 0, one L1 term here (train/loss.py:92)
  * the step — train/iteration.py:21-60: zero_grad(set_to_none) -> render -> loss -> backward -> densification
    statistics -> Adam
  * maintenance — train/iteration.py:62-86 with model/fateavatar.py:610-731: `_uv_densify` (multinomial draw by
    accumulated screen-space gradient, NEW barycentrics on the sampled rows' faces, scale * 0.75, zero Adam moments,
    statistics reset), `_prune_low_opacity_points` (statistics kept for the surviving rows), `_reset_opacity`.
What is fused: binding forward / backward are one kernel each, activations and statistics run inside the rasterizer
kernels, Adam is one kernel over the flat buffer, and the whole step replays as ONE HIP graph.  Data-parallel: one frame
per rank, one flat-gradient all-reduce; the random draws of a densification are made on rank 0 from the SUMMED
statistics and broadcast, so every rank appends identical rows.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import dp
from .binding import bind_gaussians, face_scale
from .bound import MeshBinding, render_bound_batch
from .flame import REFERENCE_FLAME_LRS, FlameFrame, FlameMesh
from .flat import FlatParams
from .model import TorchCamera
from .optim import FusedAdam
from .perceptual import Perceptual
from .render import render
from .loss import (MeshTerms, ScaleRatioTerm, l1_loss_and_grad, l1_workspace, mesh_terms_and_grad, mesh_terms_workspace,
                   scale_ratio_term_and_grad, scale_ratio_workspace)
from .train import BoundStep, TrainStep

# config/fateavatar.yaml:34-39 (group names of train/optim.py:15-21)
FATE_LRS = dict(opacity=0.05, offset=0.0016, color=0.0025, rotation=0.001, scaling=0.005)
# config/fateavatar.yaml:41-47
FATE_MAINTAIN = dict(opacity_reset_interval=60000, densify_interval=3000, prune_interval=2000, min_opacity=0.005,
                     increase_num=1000, max_points_num=200000)
# config/fateavatar.yaml:13-25: scale_loss 0.1, scale_threshold 9.0
REFERENCE_SCALE_TERM = ScaleRatioTerm(0.1, 9.0)


class AvatarGaussians(FlatParams):
    """The mesh-bound Gaussian parameters of FateAvatar (model/fateavatar.py:166-190) in ONE flat buffer, in the order
    of the optimizer groups.  `face_index` / `bary_coords` are the binding (model/fateavatar.py:120-164)."""
    FIELDS = (("_opacity", 1), ("_offset", 1), ("_features_dc", 3), ("_rotation", 4), ("_scaling", 3))
    SHAPES = {"_opacity": (1,), "_offset": (1,), "_features_dc": (1, 3), "_rotation": (4,), "_scaling": (3,)}
    ROW_BUFFERS = (("face_index", torch.int32, "new_face_index"), ("bary_coords", torch.float32, "new_bary"))
    max_sh_degree = 0   # model/fateavatar.py:54,244
    fused_activations = True

    def __init__(self, face_index, bary_coords, scale_init: float, device):
        """_register_init_gaussian (model/fateavatar.py:166-190): grey colour (DC = inverse_sigmoid(0.5) = 0), log
        scale_init on all axes, identity rotation, opacity 0.1, zero offset."""
        super().__init__()
        P = int(len(face_index))
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)  # noqa: E731
        rot = z(P, 4)
        rot[:, 0] = 1
        op = torch.full((P, 1), float(np.log(0.1 / 0.9)), dtype=torch.float32, device=device)
        self.face_index = torch.as_tensor(np.asarray(face_index), dtype=torch.int32, device=device).contiguous()
        self.bary_coords = torch.as_tensor(np.asarray(bary_coords), dtype=torch.float32, device=device).contiguous()
        self._bind([op, z(P, 1), z(P, 1, 3), rot, torch.full((P, 3), float(scale_init), dtype=torch.float32, device=device)])

    @classmethod
    def from_template(cls, device, uv_resolution: int = 256, num_points: Optional[int] = None, sampling: str = "uv",
                      rng: Optional[np.random.Generator] = None) -> "AvatarGaussians":
        """The reference's own initialisation on the head template: `_register_template_mesh` + `_register_init_gaussian`
        (model/fateavatar.py:120-190, 597-608).  `sampling="uv"` (the reference): binding points = the texel centres the
        template's UV layout covers at `uv_resolution` x `uv_resolution` (config/fateavatar.yaml:28 `tex_size: 256`), in
        row-major texel order, padded to uv_resolution^2 rows with random points on sampled faces
        (volume_rendering/mesh_sampling.py:86-138); `num_points` (default uv_resolution^2) asks for another row count the way
        the reference's `num_points` argument does (raster side int(sqrt(num_points))).  `sampling="random"`: the
        area-weighted draw the reference keeps commented out (model/fateavatar.py:135-137, mesh_sampling.py:140-169).
        scale_init = the reference's knn estimate on the canonical template points."""
        from . import mesh_sampling, scenes
        from .knn import init_scale_by_knn
        n = int(num_points) if num_points is not None else int(uv_resolution) * int(uv_resolution)
        rng = rng or np.random.default_rng(0)
        verts, faces, _ = scenes.head_geometry()
        if sampling == "uv":
            uv = scenes.head_uv()
            if uv is None:
                raise RuntimeError("the head template's UV layout is not in fateavatar_amd/data/head_template_geom.npz")
            fi, bc = mesh_sampling.uniform_sampling_barycoords(n, uv[0], uv[1], rng=rng)
        elif sampling == "random":
            fi, bc = mesh_sampling.random_sampling_barycoords(n, verts, faces, rng)
        else:
            raise ValueError(f"sampling must be 'uv' or 'random', not {sampling!r}")
        pts = (verts[faces[fi]] * bc[:, :, None]).sum(1).astype(np.float32)      # reweight_verts_by_barycoords
        scale_init = float(init_scale_by_knn(torch.from_numpy(pts).to(device))[2])
        return cls(fi, bc, scale_init, device)

class _BoundFrame:
    """What render() reads of a Gaussian holder (render_3dgs.py:19-63), for one frame's bound values."""
    max_sh_degree = 0
    fused_activations = True

    def __init__(self, xyz, pc: AvatarGaussians, rot, scl, stats):
        self.get_xyz, self._opacity, self._scaling, self._rotation = xyz, pc._opacity, scl, rot
        self.get_features = pc._features_dc            # cat(features_dc, features_rest) with an empty rest (M = 1)
        self.fused_densification_stats = stats


class _RawFrame:
    """What render_bound_batch() reads: the RAW parameters of a frame whose binding the rasterizer evaluates itself.  (Not a
    holder for render(): it has no bound positions.)"""
    max_sh_degree = 0
    fused_activations = True

    def __init__(self, pc: AvatarGaussians, stats):
        self._opacity, self._offset, self._rotation, self._scaling = pc._opacity, pc._offset, pc._rotation, pc._scaling
        self.get_features = pc._features_dc
        self.fused_densification_stats = stats


class AvatarStep(BoundStep):
    """One optimisation step of FateAvatar per call: `step(camera, posed_verts, gt_image)`.  The optimizer groups are those
    of train/optim.py:15-21 with config/fateavatar.yaml:34-39 (the `gs` group).  The other half of the model — the mesh
    under the Gaussians, learnt through FLAME's `delta_shapedirs` / `delta_posedirs` / `delta_vertex`
    (model/fateavatar.py:87-94,212-223, the `bs` group) — stays the caller's, in stock PyTorch, by default: `vertex_grad` /
    `mesh_terms` hand it this step's dLoss/dposed_verts.  With `flame=FlameMesh(...)` the mesh is part of the captured step too
    (flame.py, csrc/fr_flame.hip): `step(camera, FlameFrame(expression, pose), gt_image)`."""
    LRS = FATE_LRS
    LR_KEYS = {"_opacity": "opacity", "_offset": "offset", "_features_dc": "color", "_rotation": "rotation", "_scaling": "scaling"}
    CAMERA_GRAD = True
    K = 1                   # frames per step (AvatarBatchStep: its views_per_step)

    def __init__(self, pc: AvatarGaussians, faces: torch.Tensor, canonical_verts: torch.Tensor, camera: TorchCamera,
                 bg: torch.Tensor, lrs: Optional[dict] = None, shell_len: float = 0.05, resize_scale: bool = True,
                 use_graph: bool = True, fold_binding: bool = True, keep_coherent: bool = False, vertex_grad: bool = False,
                 mesh_terms: Optional[MeshTerms] = None, camera_grad: bool = False, flame: Optional[FlameMesh] = None,
                 flame_lrs: Optional[dict] = None, perceptual: Optional[Perceptual] = None,
                 scale_term: Optional[ScaleRatioTerm] = None):
        """`keep_coherent`: after every `uv_densify` the rows are re-stored in a spatially coherent order (`sort_coherent`):
        the reference appends the new rows at the end (model/fateavatar.py:640-665), so a set that started in UV-raster
        order (mesh_sampling.py:86-138: neighbours in storage are neighbours on the mesh) grows an unordered tail; the
        results do not depend on the order, the rasterizer's speed does.  Off by default: row i then stays
        row i as in the reference.
        `fold_binding` (default): the binding is evaluated inside the rasterizer's per-Gaussian kernels (bound.py,
        fr_aux::binding) — no binding launches, no bound arrays written by one kernel to be read by the next.  False: the
        stand-alone `bind_gaussians` op in front of `render()` (same results; kept as the A/B and as the op's own user).
        `vertex_grad`: `d_verts` [V,3] holds every step's dLoss/dposed_verts (BoundStep).
        `mesh_terms`: a `MeshTerms` (REFERENCE_MESH_TERMS holds the reference's 1e5 / 0) adds FateAvatar's Laplacian-smoothing
        and FLAME-distance terms (train/loss.py:112-121,166-180,192-197) to every step: `step(..., verts_orig=)` takes the
        mesh the posed one is held to (the reference's `verts_orig`: the FLAME mesh without the learnt deltas, same pose) as
        one more static input, and ONE launch behind the rasterizer's backward (`loss.mesh_terms_and_grad`) adds the terms'
        weighted gradient into `d_verts`; `mesh_loss` then holds the step's unweighted (laplacian_loss, flame_loss), `loss`
        stays the image term.  Implies `vertex_grad`.  None (default): no such launch, `mesh_loss` is None.
        `camera_grad`: `d_view` / `d_proj` / `d_campos` hold every step's dLoss/d(camera) (BoundStep): what a per-frame camera
        embedding (the reference's `cam_pose`, train/base.py:123,142) trains on.
        `flame`: a `flame.FlameMesh` over the mesh's V vertices makes FLAME and its three learnt deltas part of the step:
        `step(camera, FlameFrame(expression, pose), gt_image)` then takes the frame's coefficients where it took the posed
        vertices (a vertex tensor or a `verts_orig` argument is refused), and the captured body is FLAME forward (into the
        step's vertex buffer and, with `mesh_terms`, into `verts_orig`: the reference's second, delta-free forward) -> the
        frame -> the mesh terms -> FLAME backward from `d_verts` -> the Gaussians' Adam -> an Adam of the mesh's flat buffer
        with the three groups of train/optim.py:27-33 at `flame_lrs` (default REFERENCE_FLAME_LRS: 1e-5, 1e-5, 1e-4), skipped by
        the same overflow word.  `d_expression` [n_exp] and `d_pose` [15] hold THIS step's dLoss/d(expression, pose) — what the
        reference's tracking optimisation (tracking_lr) trains on — with the lifetime rules of `d_verts`.  Implies
        `vertex_grad`.  None (default): the mesh is the caller's, nothing here changes.
        `perceptual`: a `perceptual.Perceptual` adds FateAvatar's VGG term (train/loss.py:123-199, weight 0.1) to every step:
        ONE call directly behind the L1 launch (csrc/fr_vgg.hip) ADDS weight x its gradient to the L1 gradient in the step's
        image-gradient buffer, before the rasterizer's backward; `perceptual_loss` [1 + T] then holds the step's unweighted
        sum of the tap terms and the terms, `loss` stays the L1 term (the reference's total is
        loss + perceptual.weight * perceptual_loss[0] + ...).  None (default): not one launch changes.
        `scale_term`: a `ScaleRatioTerm` (REFERENCE_SCALE_TERM holds the reference's 0.1 / 9.0) adds FateAvatar's scale term
        (train/loss.py:144-151) on the RAW `_scaling` to every step: ONE launch (`loss.scale_ratio_term_and_grad`) behind the
        frame's backward adds weight x its gradient into the flat gradient buffer, in front of the data-parallel exchange and
        Adam; `reg_loss` [2] then holds the step's unweighted (scale_loss, rows over the threshold), `loss` stays the L1 term.
        The term has no state: checkpoints and density control are what they are without it.  None (default): no such
        launch, `reg_loss` is None."""
        if scale_term is not None and not isinstance(scale_term, ScaleRatioTerm):
            raise TypeError(f"AvatarStep: `scale_term` is a ScaleRatioTerm or None, not {type(scale_term).__name__}")
        self.scale_term = None if scale_term is None else ScaleRatioTerm(*[float(x) for x in scale_term])
        self.keep_coherent = bool(keep_coherent)
        if perceptual is not None:
            if not isinstance(perceptual, Perceptual):
                raise TypeError("AvatarStep: `perceptual` must be a perceptual.Perceptual")
            if perceptual.features.device != pc.flat.device:
                raise ValueError("AvatarStep: the perceptual term and the Gaussians live on different devices")
        self.perceptual = perceptual
        self.mesh_terms = None if mesh_terms is None else MeshTerms(*[float(x) for x in mesh_terms])
        if flame is not None:
            if not isinstance(flame, FlameMesh):
                raise TypeError("AvatarStep: `flame` must be a flame.FlameMesh")
            if flame.V != int(canonical_verts.shape[0]):
                raise ValueError(f"AvatarStep: the FLAME model has {flame.V} vertices, the mesh {int(canonical_verts.shape[0])}")
            if flame.device != pc.flat.device:
                raise ValueError("AvatarStep: the FLAME model and the Gaussians live on different devices")
            if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                raise NotImplementedError("AvatarStep(flame=...): data-parallel runs of the fused mesh are not built (its gradient "
                                          "has no all-reduce): use the caller's FLAME with `vertex_grad`")
            self._flame_segments = flame.adam_segments(flame_lrs)
            flame._ensure_workspace()              # (allocates: outside any capture)
        self.flame, self.flame_adam = flame, None
        super().__init__(pc, faces, camera, bg, canonical_verts, lrs, use_graph, fold_binding,
                         vertex_grad=bool(vertex_grad) or mesh_terms is not None or flame is not None, camera_grad=camera_grad)
        # with a FLAME model: the frame's coefficients, two more static inputs, and their gradients
        self.expression = self.pose = self.d_expression = self.d_pose = None
        if flame is not None:
            self.expression, self.pose = torch.zeros(flame.n_exp, device=self.dev), torch.zeros(15, device=self.dev)
            self.d_expression, self.d_pose = torch.zeros(flame.n_exp, device=self.dev), torch.zeros(15, device=self.dev)
        # (the term's workspace is its own, allocated with it: outside any capture)
        self.perceptual_loss = None if perceptual is None else torch.zeros(1 + perceptual.n_terms, device=self.dev)
        # the reference's out['scale_loss'] of the step (unweighted) and the rows over the threshold, written by the term's
        # launch; the scratch is the step's own and its size does not depend on P: density control leaves both alone
        self.reg_loss = None if self.scale_term is None else torch.zeros(2, device=self.dev)
        self._ratio_ws = None if self.scale_term is None else scale_ratio_workspace(self.dev)
        self.mesh_loss = self.verts_orig = self.laplacian = self._mesh_ws = None
        if self.mesh_terms is not None:
            from .binding import mesh_laplacian
            self.laplacian = mesh_laplacian(self.faces, int(self.verts.shape[0]))
            self.verts_orig = self.verts.clone()       # static input of the captured step
            self.mesh_loss = torch.zeros(2, device=self.dev)
            self._mesh_ws = mesh_terms_workspace(self.dev)
        self.shell_len, self.resize_scale = float(shell_len), bool(resize_scale)
        self.canon_verts = self.verts.clone()
        # compute_face_orientation(canonical verts, return_scale=True)[1] (model/fateavatar.py:84-85)
        self.face_scale_canonical = face_scale(self.canon_verts, self.faces)

    def _make_adam(self):
        """The Gaussians' optimizer; the mesh's is made ONCE (a change of the point set does not touch the mesh: its moments
        and step count go on) and skips on the holder's present overflow word."""
        super()._make_adam()
        if self.flame is not None:
            if self.flame_adam is None:
                self.flame_adam = FusedAdam(self.flame.flat.detach(), self.flame.flat_grad, self._flame_segments)
            self.flame_adam.set_skip_words([self.pc.overflow_word])

    def _buffers_moved(self, old_index, old_rows, *, stats):
        super()._buffers_moved(old_index, old_rows, stats=stats)
        if self.flame is not None:
            self.flame_adam.set_skip_words([self.pc.overflow_word])   # (a remapped optimizer: the word may have moved)

    def _forward_backward(self):
        self._forward_backward_on(self)

    def _body(self):
        super()._body()
        if self.flame is not None:
            self.flame_adam.step()

    def _add_scale_term(self, pc):
        """train/loss.py:144-151: weight x the scale term's gradient is ADDED to the image term's dL/d_scaling in `pc`'s flat
        gradient buffer, ONCE per step, in front of the exchange and Adam.  Adam divides the summed gradient by the step's K
        frames and the ranks: the launch carries K x weight (K = 1 here; exact in float32 for the batch step's K = 2, 4), and
        under data-parallel every rank adds weight x g to identical parameters, so the all-reduced sum is world x weight x g
        and Adam's 1 / world gives weight x g.  A replay that overflowed its binning capacity back-propagated zeros and its
        Adam launch skips the step (the overflow word): what this launch added to the zeroed gradient is never applied."""
        pc.collect_grads()
        t = self.scale_term
        scale_ratio_term_and_grad(pc._scaling, pc.grad_view("_scaling"), out=self.reg_loss,
                                  terms=ScaleRatioTerm(ctypes.c_float(t.weight).value * self.K, t.scale_threshold), workspace=self._ratio_ws)

    def _forward_backward_on(self, L):
        """Bind, render, L1, backward for one frame.  `L` holds what the frame reads and writes — pc, verts, cam, gt, loss,
        _dimage, xyz_gradient_accum, denom, out: this object itself, or one lane of an AvatarBatchStep."""
        pc = L.pc
        pc.begin_step()                                             # zero_grad(set_to_none=True), iteration.py:48-49
        if self.flame is not None:     # model/fateavatar.py:212-223: both FLAME forwards, two launches
            self.flame.forward_into(self.expression, self.pose, L.verts, self.verts_orig)
        verts, cam = self._vertex_leaf(L.verts), self._camera_leaf(L.cam)
        if self.fold_binding:
            from . import rasterizer
            out = render_bound_batch([cam], [_RawFrame(pc, (L.xyz_gradient_accum, L.denom, pc.overflow_word))], [verts], self._binding(pc),
                                     self.bg, slots=[rasterizer._slot])[0]
        else:
            xyz, rot, scl = bind_gaussians(verts, self.faces, pc.face_index, pc.bary_coords, self.face_scale_canonical,
                                           pc._offset, pc._rotation, pc._scaling, self.shell_len, self.resize_scale)
            frame = _BoundFrame(xyz, pc, rot, scl, (L.xyz_gradient_accum, L.denom, pc.overflow_word))
            out = render(cam, frame, self.bg)
        _, g = l1_loss_and_grad(out["render"], L.gt, loss_out=L.loss, grad_out=L._dimage, workspace=L._l1_ws)   # see TrainStep
        if self.perceptual is not None:     # weight x the VGG term's gradient, ADDED to the L1 gradient in place
            self.perceptual.loss_and_grad(out["render"], L.gt, loss_out=self.perceptual_loss, grad_out=g, accumulate=True)
        out["render"].backward(g)
        self._keep_vertex_grad(verts)
        self._keep_camera_grad(cam)
        if self.mesh_terms is not None:
            # train/loss.py:112-121: weight x the mesh terms' gradient is ADDED to the image term's dL/dposed_verts.  A replay
            # that overflowed its binning capacity back-propagated zeros: d_verts then holds the mesh terms alone.
            mesh_terms_and_grad(L.verts, self.verts_orig, self.laplacian, self.mesh_terms, d_verts=self.d_verts, out=self.mesh_loss,
                                workspace=self._mesh_ws)
        if self.flame is not None:     # d_verts -> the deltas' flat gradient, d_expression, d_pose: two launches
            self.flame.backward_from(self.d_verts, self.expression, self.pose, self.d_expression, self.d_pose)
        if self.scale_term is not None and getattr(L, "k", 0) == 0:    # (a batch step's lanes: once per step, in lane 0's body)
            self._add_scale_term(pc)
        L.out = self._kept(out)

    def step(self, camera: TorchCamera, posed_verts, gt_image: torch.Tensor,
             verts_orig: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`verts_orig` [V,3]: the mesh the mesh terms hold `posed_verts` to — required with `mesh_terms`, refused without.
        A step built with `flame` takes a `FlameFrame(expression [n_exp], pose [15])` where it took `posed_verts` and makes
        both meshes itself: a vertex tensor or a `verts_orig` is refused."""
        if self.flame is not None:
            if verts_orig is not None or not isinstance(posed_verts, FlameFrame):
                raise ValueError("AvatarStep.step: a step with a FLAME model takes FlameFrame(expression, pose) where it took the "
                                 "posed vertices, and no `verts_orig` (it makes both meshes itself)")
            e, p = posed_verts
            if tuple(e.shape) != tuple(self.expression.shape) or tuple(p.shape) != (15,):
                raise ValueError(f"AvatarStep.step: FlameFrame(expression [{self.expression.shape[0]}], pose [15]), not "
                                 f"{tuple(e.shape)} and {tuple(p.shape)}")
            # (BoundStep.step would load the vertex buffer: here the kernels write it)
            return TrainStep.step(self, camera, gt_image, [(self.expression, e.detach()), (self.pose, p.detach())])
        if (verts_orig is None) != (self.mesh_terms is None):
            raise ValueError("AvatarStep.step: `verts_orig` goes with `mesh_terms` (required with them, refused without)")
        return super().step(camera, posed_verts, gt_image, () if verts_orig is None else [(self.verts_orig, verts_orig.detach())])

    def _binding(self, pc: AvatarGaussians) -> MeshBinding:
        return MeshBinding(self.faces, pc.face_index, pc.bary_coords, self.face_scale_canonical, self.shell_len, self.resize_scale)

    # ---- maintenance (train/iteration.py:62-86)
    def maintain(self, global_step: int, cfg: Optional[dict] = None) -> dict:
        """The reference's schedule after the optimizer step of `global_step`.  Returns what was done."""
        c = dict(FATE_MAINTAIN, **(cfg or {}))
        did = {}
        if global_step % c["densify_interval"] == 0 and self.pc.P < c["max_points_num"]:
            did["densified"] = self.uv_densify(min(c["max_points_num"] - self.pc.P, c["increase_num"]))
        if global_step % c["prune_interval"] == 0:
            did["pruned"] = self.prune_low_opacity(c["min_opacity"])
        if global_step % c["opacity_reset_interval"] == 0 and global_step != 0:
            self.reset_opacity()
            did["opacity_reset"] = True
        return did

    @torch.no_grad()
    def uv_densify(self, increase_num: int, generator: Optional[torch.Generator] = None) -> int:
        """_uv_densify (model/fateavatar.py:610-672).  The two random draws (multinomial over xyz_gradient_accum, with
        replacement; then uniform barycentrics) are `_draw_by_gradient`'s: made on rank 0 from the statistics summed over all
        ranks and broadcast."""
        idx, uvw, rows = self._draw_by_gradient(increase_num, generator, uniforms=3)
        new_bary = uvw / uvw.sum(dim=-1, keepdim=True)
        # appended rows start with zero Adam moments, the statistics restart from zero (:667-669)
        self._resize(carry_stats=False, new_rows=rows, new_face_index=self.pc.face_index[idx], new_bary=new_bary)
        self.last_densify = (idx, new_bary)
        if self.keep_coherent:
            AvatarStep.sort_coherent(self)     # (a subclass's lanes are rebuilt by its own uv_densify)
        return increase_num

    @torch.no_grad()
    def coherent_order(self, cells: int = 32) -> torch.Tensor:
        """Row indices in a spatially coherent sequence: grid cells (`cells` per axis, x fastest) of the Gaussians' points
        on the CANONICAL mesh (barycentric points: the posed offsets are small against a cell) — scenes.spatial_order on
        the device, deterministic (stable sort), so identical on every rank of a data-parallel run."""
        pc = self.pc
        tri = self.canon_verts[self.faces.long()[pc.face_index.long()]]                 # [P,3,3]
        pts = (tri * pc.bary_coords.unsqueeze(-1)).sum(1).double()
        lo, hi = pts.min(0).values, pts.max(0).values
        c = ((pts - lo) / (hi - lo).clamp_min(1e-12) * cells).long().clamp_(max=cells - 1)
        return torch.argsort((c[:, 2] * cells + c[:, 1]) * cells + c[:, 0], stable=True)

    @torch.no_grad()
    def sort_coherent(self, cells: int = 32) -> torch.Tensor:
        """Re-store the Gaussians (parameters, binding, Adam moments, densification statistics) in `coherent_order`.
        Returns the order applied (old row of every new row)."""
        order = self.coherent_order(cells)
        self._resize(carry_stats=True, order=order)
        return order

    @torch.no_grad()
    def prune_low_opacity(self, min_opacity: float = 0.005) -> int:
        """_prune_low_opacity_points (model/fateavatar.py:674-711): the statistics of the surviving rows are kept."""
        old_rows = self.pc.P
        self._resize(carry_stats=True, keep_mask=~(torch.sigmoid(self.pc._opacity) < min_opacity).reshape(-1))
        return old_rows - self.pc.P

    # ---- checkpoints in the reference's layout (Trainer.save_checkpoint, train/trainer.py:396-435: a dict with 'epoch',
    #      'global_step' and 'model' = model.state_dict(), which for FateAvatar holds the six Gaussian parameters and the
    #      two binding buffers next to the FLAME / blendshape entries)
    GAUSSIAN_ATTRIBUTES = ['_offset', '_features_dc', '_features_rest', '_scaling', '_rotation', '_opacity', 'face_index',
                           'bary_coords']   # train/deserialize.py:10-12
    RESUME_REMAPPED = True      # a checkpoint without an `optimizer` entry goes on from this step's count with zero moments

    # with a FLAME model the checkpoint's 'model' also carries delta_shapedirs [V,3,L], delta_posedirs [36,3V] and
    # delta_vertex [V,3] under the reference's names (model/fateavatar.py:87-94), and `flame_optimizer` (an addition, like
    # `optimizer`) their Adam state
    def _save_extras(self, sd: dict) -> None:
        sd["model"]["_features_rest"] = torch.zeros((self.pc.P, 0, 3), device=self.dev)   # max_sh_degree 0: empty (fateavatar.py:172-183)
        if self.flame is not None:
            sd["model"].update(self.flame.state_dict())
            a = self.flame_adam
            sd["flame_optimizer"] = {"exp_avg": a.exp_avg.clone(), "exp_avg_sq": a.exp_avg_sq.clone(), "state": a.state_words()}

    def _load_extras(self, sd: dict, g: dict) -> None:
        if int(g["_features_rest"].shape[1]) != 0:
            raise ValueError("FateAvatar renders SH degree 0: _features_rest must be empty")
        if self.flame is not None:
            self.flame.check_state_dict(sd["model"])

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> list:
        """BoundStep.load_state_dict; with a FLAME model the three `delta_*` entries are LOADED (in place) instead of being
        returned as ignored, and `flame_optimizer`, if the checkpoint has one, restores their Adam (else it goes on as it is)."""
        ignored = super().load_state_dict(sd)
        if self.flame is None:
            return ignored
        self.flame.load_state_dict(sd["model"])
        opt = sd.get("flame_optimizer")
        if opt is not None:
            self.flame_adam.exp_avg.copy_(opt["exp_avg"])
            self.flame_adam.exp_avg_sq.copy_(opt["exp_avg_sq"])
            self.flame_adam.load_state_words(opt["state"])
        return [k for k in ignored if k not in ("delta_shapedirs", "delta_posedirs", "delta_vertex")]


class _Lane:
    """One view of a batch: everything its frame reads and writes next to the shared parameters."""


class AvatarBatchStep(AvatarStep):
    """K frames per optimisation step, IN FLIGHT TOGETHER: `step(cameras, posed_verts, gt_images)` with K of each.

    reference: the model renders the frames of a batch one after the other with shared Gaussians
    (`for bs_ in range(bs)`, model/fateavatar.py:251-276) and the loss is the mean over the batch (train/loss.py:92-105).
    Here every frame of the batch is a LANE — its own leaves over the shared parameter storage with its own gradient
    buffer (AvatarGaussians.lane), static inputs, densification statistics, stream, fr_handle slot and captured graph
    (bind -> render -> L1 -> backward) — and the lanes run concurrently: one frame's kernels leave most of the chip idle
    (DESIGN.md §4).  One fused Adam then steps on the SUM of the lanes' gradients (fr_adam_step_multi; grad_scale
    = 1 / (K x ranks) makes it the batch mean)."""

    def __init__(self, pc: AvatarGaussians, faces, canonical_verts, camera: TorchCamera, bg, views_per_step: int = 3,
                 chain: bool = True, **kw):
        """`chain` (default): the K frames go through ONE launch chain on ONE stream instead of K lanes on K streams — bind x K,
        `render_batch` (fr_forward_batch: every rasterizer kernel launched once for the K views), L1 x K, one batched
        backward (fr_backward_batch), bind backward x K, Adam: the whole step one captured graph, no stream or
        hardware-queue arrangement and no cross-stream events (10.0 k against 8.2 k frames/s at K = 4, 100 k Gaussians,
        512^2).  `chain=False` keeps the lanes: a stream, a handle and a captured graph per frame."""
        from . import _lib
        if not 1 <= int(views_per_step) <= _lib.FR_ADAM_MAX_GRADS:
            raise ValueError(f"views_per_step must be 1..{_lib.FR_ADAM_MAX_GRADS}")
        if kw.get("camera_grad"):
            raise NotImplementedError("AvatarBatchStep: `camera_grad` is not built for the batch step: use AvatarStep")
        if kw.get("flame") is not None:
            raise NotImplementedError("AvatarBatchStep: `flame` is not built for the batch step (one FLAME state per step, like "
                                      "`vertex_grad`): use AvatarStep")
        if kw.get("perceptual") is not None:
            raise NotImplementedError("AvatarBatchStep: `perceptual` is not built for the batch step (one workspace per lane): "
                                      "use AvatarStep")
        if kw.get("vertex_grad") or kw.get("mesh_terms") is not None:
            raise NotImplementedError("AvatarBatchStep: `vertex_grad` / `mesh_terms` are not built for the batch step (two step "
                                      "bodies, and its twelve multi_copy segments are used up at K = 4): use AvatarStep")
        self.K = int(views_per_step)
        self.chain = bool(chain)
        self._chain_graph = None
        super().__init__(pc, faces, canonical_verts, camera, bg, **kw)
        self._build_lanes()

    def _make_adam(self):
        super()._make_adam()
        self.adam.set_grad_scale(1.0 / (self.world * self.K))

    def _build_lanes(self):
        from .streams import concurrent_streams
        # (streams that land on one hardware queue are serialised: pick lanes' streams that overlap with each other and
        # with the caller's — fateavatar_amd/streams.py)
        # (the launch chain runs on the caller's stream: no lane streams, no probing)
        streams = ([None] * self.K if self.chain else
                   concurrent_streams(self.K, self.dev, also_with=[torch.cuda.current_stream(self.dev)]))
        self.lanes = []
        for k in range(self.K):
            L = _Lane()
            L.k = k
            if k == 0:     # lane 0 IS this object's own frame state
                L.pc, L.cam, L.verts, L.gt, L.loss, L._dimage = self.pc, self.cam, self.verts, self.gt, self.loss, self._dimage
                L.xyz_gradient_accum, L.denom, L._l1_ws = self.xyz_gradient_accum, self.denom, self._l1_ws
            else:
                L.pc, L.cam, L.verts = self.pc.lane(), self.cam.clone(), self.verts.clone()
                L.gt, L.loss, L._dimage = torch.zeros_like(self.gt), torch.zeros_like(self.loss), torch.zeros_like(self._dimage)
                L.xyz_gradient_accum, L.denom = torch.zeros_like(self.xyz_gradient_accum), torch.zeros_like(self.denom)
                L._l1_ws = l1_workspace(self.dev)   # (the lanes' loss kernels overlap: one scratch each, loss.py)
            L.out, L.graph = None, None
            L.stream, L.done = streams[k], torch.cuda.Event()
            self.lanes.append(L)
        self._eager_steps = 0
        self._chain_graph = None           # (captured over the old lanes' buffers)
        self._ready = torch.cuda.Event()
        # one overflowed view skips the whole step (its zero gradient would otherwise be averaged in)
        self.adam.set_skip_words([L.pc.overflow_word for L in self.lanes])

    # ---- the step
    def _capture_lanes(self):
        from . import rasterizer
        for L in self.lanes:
            with rasterizer.handle_slot(L.k), rasterizer.no_wait():
                acc, den = L.xyz_gradient_accum.clone(), L.denom.clone()
                L.stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(L.stream):
                    self._forward_backward_on(L)          # warms the allocator pools of the capture path: not a step
                torch.cuda.synchronize()
                L.xyz_gradient_accum.copy_(acc)
                L.denom.copy_(den)
                L.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(L.graph, stream=L.stream, capture_error_mode="thread_local"):
                    self._forward_backward_on(L)
                torch.cuda.synchronize()

    def _drop_graphs(self):
        for L in self.lanes:
            L.graph = None
        self._chain_graph = None
        self._eager_steps = 0

    # ---- the step as one launch chain
    def _chain_body(self):
        from .render import render_batch
        frames = []
        for L in self.lanes:
            L.pc.begin_step()
            if self.fold_binding:
                frames.append(_RawFrame(L.pc, (L.xyz_gradient_accum, L.denom, L.pc.overflow_word)))
                continue
            xyz, rot, scl = bind_gaussians(L.verts, self.faces, L.pc.face_index, L.pc.bary_coords, self.face_scale_canonical,
                                           L.pc._offset, L.pc._rotation, L.pc._scaling, self.shell_len, self.resize_scale)
            frames.append(_BoundFrame(xyz, L.pc, rot, scl, (L.xyz_gradient_accum, L.denom, L.pc.overflow_word)))
        if self.fold_binding:
            outs = render_bound_batch([L.cam for L in self.lanes], frames, [L.verts for L in self.lanes], self._binding(self.pc),
                                      self.bg, slots=[L.k for L in self.lanes])
        else:
            outs = render_batch([L.cam for L in self.lanes], frames, self.bg, slots=[L.k for L in self.lanes])
        from .loss import l1_loss_and_grad_batch
        images = [out["render"] for out in outs]
        _, grads = l1_loss_and_grad_batch(images, [L.gt for L in self.lanes], [L.loss for L in self.lanes],
                                          [L._dimage for L in self.lanes], [L._l1_ws for L in self.lanes])
        for L, out in zip(self.lanes, outs):
            L.out = self._kept(out)
        torch.autograd.backward(images, grad_tensors=grads)
        if self.scale_term is not None:            # once per step, into lane 0's gradient: K x weight (_add_scale_term)
            self._add_scale_term(self.lanes[0].pc)
        if self.exchange:                          # sum of the local lanes, then the sum over the ranks; Adam scales
            flat = [L.pc.exchange_buffer() for L in self.lanes]   # (gradients + overflow words: the words add up too)
            for g in flat[1:]:
                flat[0].add_(g)
            if self.exchange_in_graph or not torch.cuda.is_current_stream_capturing():
                dp.allreduce_sum_(flat[0])
            self.adam.step()
        else:
            self.adam.step([L.pc.collect_grads() for L in self.lanes])

    def _capture_chain(self):
        from . import rasterizer
        with rasterizer.no_wait():
            stats = [(L.xyz_gradient_accum.clone(), L.denom.clone()) for L in self.lanes]
            side = torch.cuda.Stream(device=self.dev)
            side.wait_stream(torch.cuda.current_stream(self.dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                self._chain_body()
            torch.cuda.synchronize()
            for L, (acc, den) in zip(self.lanes, stats):   # (capturing does not execute: nothing to put back, but keep the
                L.xyz_gradient_accum.copy_(acc)            # statistics exactly as they were)
                L.denom.copy_(den)
        self._chain_graph = g

    def step(self, cameras, posed_verts, gt_images):
        """One optimisation step on K frames.  Returns the K (device) loss scalars of the step."""
        from . import rasterizer
        from .loss import multi_copy
        if not (len(cameras) == len(posed_verts) == len(gt_images) == self.K):
            raise ValueError(f"AvatarBatchStep.step needs {self.K} cameras, vertex sets and images")
        self.host_steps += 1
        main = torch.cuda.current_stream(self.dev)
        pairs = []
        for L, cam, verts, gt in zip(self.lanes, cameras, posed_verts, gt_images):
            pairs += [(L.verts, verts), (L.gt, gt)]
            if cam is not L.cam:
                L.cam.check_same_intrinsics(cam)
                pairs.append((L.cam._packed, cam._packed))
        try:
            multi_copy(pairs)                      # the inputs of all K frames: one launch
        except RuntimeError:                       # (host tensors, other dtypes, more than twelve pairs: plain copies)
            for d, s in pairs:
                d.copy_(s, non_blocking=True)
        if self.chain:
            return self._step_chain()
        captured = self.lanes[0].graph is not None
        if self.use_graph and not captured and self._eager_steps >= 2:
            self._capture_lanes()
            captured = True
        self._steps_since_poll = getattr(self, "_steps_since_poll", 0) + 1
        if captured and self._steps_since_poll >= 8:
            # a replayed frame that overflowed its binning capacity (pinned counts, no synchronisation): back to eager
            self._steps_since_poll = 0
            for L in self.lanes:
                with rasterizer.handle_slot(L.k):
                    if rasterizer.check_async_overflow(self.dev.index or 0):
                        self.overflows += 1
                        self._drop_graphs()
                        captured = False
                        break
        self._ready.record(main)                   # inputs loaded; the previous step's Adam has been enqueued before it
        for L in self.lanes:
            with torch.cuda.stream(L.stream):
                L.stream.wait_event(self._ready)
                if captured:
                    L.graph.replay()
                else:
                    with rasterizer.handle_slot(L.k):
                        self._forward_backward_on(L)
                        L.pc.collect_grads()
                L.done.record(L.stream)
        if not captured:
            self._eager_steps += 1
        for L in self.lanes:
            main.wait_event(L.done)
        grads = [L.pc.flat_grad for L in self.lanes]
        if self.exchange:                          # sum of the local lanes, then the sum over the ranks; Adam scales
            grads = [L.pc._grad_store for L in self.lanes]        # (gradients + overflow words: the words add up too)
            for g in grads[1:]:
                grads[0].add_(g)
            dp.allreduce_sum_(grads[0])
            self.adam.step()
        else:
            self.adam.step(grads)
        self.out = self.lanes[0].out
        return tuple(L.loss for L in self.lanes)

    def _step_chain(self):
        from . import rasterizer
        captured = self._chain_graph is not None
        # (a gloo exchange cannot be captured: such steps stay eager)
        if self.use_graph and not captured and self._eager_steps >= 2 and (not self.exchange or self.exchange_in_graph):
            self._capture_chain()
            captured = True
        # Every step polls the lanes' pinned count slots (a host read, no synchronisation): the counts are those of the
        # most recent replay that has FINISHED, so an overflow inside the captured chain is seen one or two steps late.
        # Those replays back-propagated zeros for the overflowed view — and their Adam launch SKIPPED the step on the device
        # (the view's overflow word, FusedAdam.set_skip_words): nothing moved on a partly zero gradient.  They are counted
        # and named — `overflow_steps` — and the chain is captured again with the raised capacity.
        self._step_no = getattr(self, "_step_no", 0) + 1
        if captured:
            for L in self.lanes:
                with rasterizer.handle_slot(L.k):
                    if rasterizer.check_async_overflow(self.dev.index or 0):
                        self.overflows += 1
                        self.overflow_steps = getattr(self, "overflow_steps", []) + [self._step_no - 1]
                        import warnings   # (every occurrence: each one is a step whose view contributed a zero gradient)
                        warnings.warn(f"AvatarBatchStep: the binning capacity overflowed inside the captured chain around step "
                                      f"{self._step_no - 1} (view {L.k}, occurrence {self.overflows}); that view back-propagated zeros and "
                                      "the optimizer skipped the affected step(s) on every rank; the chain is captured again with a "
                                      "larger capacity")
                        self._drop_graphs()
                        captured = False
                        break
        if captured:
            self._chain_graph.replay()
        else:
            self._chain_body()
            self._eager_steps += 1
        self.out = self.lanes[0].out
        return tuple(L.loss for L in self.lanes)

    def check(self) -> None:
        from . import rasterizer
        for L in self.lanes:
            with rasterizer.handle_slot(L.k):
                if (L.graph is not None or self._chain_graph is not None) and rasterizer.check_async_overflow(self.dev.index or 0):
                    raise RuntimeError("binning capacity overflowed inside a captured frame; re-create the step")

    # ---- maintenance: the lanes' statistics are folded into this object's before anything reads them, and the lanes are
    #      rebuilt whenever the point set (and with it every buffer) changes
    @torch.no_grad()
    def _fold_stats(self):
        for L in self.lanes[1:]:
            self.xyz_gradient_accum.add_(L.xyz_gradient_accum)
            self.denom.add_(L.denom)
            L.xyz_gradient_accum.zero_()
            L.denom.zero_()

    def reduce_densification_stats(self):
        self._fold_stats()
        return super().reduce_densification_stats()

    def _maintenance(self, op, *args, fold: bool = True, rebuild: bool = True):
        """One of AvatarStep's maintenance calls on the batch: wait for the lanes, fold their statistics (`fold`), run it,
        rebuild the lanes over the new buffers (`rebuild`)."""
        torch.cuda.synchronize()
        if fold:
            self._fold_stats()
        out = op(*args)
        if rebuild:
            self._build_lanes()
        return out

    def uv_densify(self, increase_num: int, generator=None) -> int:
        return self._maintenance(super().uv_densify, increase_num, generator, fold=False)   # (folds in reduce_densification_stats)

    def prune_low_opacity(self, min_opacity: float = 0.005) -> int:
        return self._maintenance(super().prune_low_opacity, min_opacity)

    def reset_opacity(self) -> None:
        # in place: the lanes' leaves see it (shared storage), their graphs stay valid
        self._maintenance(super().reset_opacity, fold=False, rebuild=False)

    def sort_coherent(self, cells: int = 32):
        return self._maintenance(super().sort_coherent, cells)

    def load_state_dict(self, sd: dict) -> list:
        return self._maintenance(super().load_state_dict, sd, fold=False)               # (the checkpoint brings the statistics)
