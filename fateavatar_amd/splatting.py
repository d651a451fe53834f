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
  * its MSE / scale / LPIPS loss terms (config/splattingavatar.yaml:13-20): the image term is L1 (`rgb_loss` 1.0)
  * gradients to the posed vertices (the reference's tracking / deformer rates): the mesh pass is not differentiable
  * data-parallel runs of the step (`reduce_densification_stats`)
  * `max_radii2D` (see `densify_and_prune`)
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .binding import PhongCanonical, bind_gaussians_phong, phong_canonical, phong_frame
from .bound import PhongBinding, render_bound_batch
from .flat import FlatParams
from .gs_utils import RGB2SH
from .model import TorchCamera
from .phongsurf import PhongSurface, triwalk
from .render import render
from .rigged import build_rotation
from .train import BoundStep

# config/splattingavatar.yaml:26-30 (group names of train/optim.py:106-117)
PERCENT_DENSE = 0.01        # splattingavatar.py: percent_dense
SPLATTING_LRS = dict(uvd=0.00016, opacity=0.05, feature_dc=0.0025, feature_rest=0.0025 / 20, rotation=0.001, scaling=0.005)
NUM_INIT_SAMPLES = 10_000   # config/splattingavatar.yaml:23


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


class SplattingStep(BoundStep):
    """One optimisation step of SplattingAvatar per call: `step(camera, posed_verts, gt_image)` —
    mesh pass -> bind in the frame -> render -> L1 -> backward -> densification statistics -> Adam.  The optimizer groups are
    those of train/optim.py:106-117 with config/splattingavatar.yaml:26-30 (`_features_rest` is empty at SH degree 0: its
    group keeps its place and rate)."""
    LRS = SPLATTING_LRS
    LR_KEYS = {"_uvd": "uvd", "_opacity": "opacity", "_features_dc": "feature_dc", "_features_rest": "feature_rest",
               "_rotation": "rotation", "_scaling": "scaling"}

    def __init__(self, pc: SplattingGaussians, canonical: PhongCanonical, camera: TorchCamera, bg: torch.Tensor, verts: torch.Tensor,
                 lrs: Optional[dict] = None, use_graph: bool = True, fold_binding: bool = True):
        """`canonical`: `binding.phong_canonical(cano_verts, faces)`; `verts` [V,3]: any pose of the mesh (sizes the step's
        static vertex buffer and is its first content).  `fold_binding` (default): the per-Gaussian binding is evaluated
        inside the rasterizer's per-Gaussian kernels (fr_aux::binding with FR_BIND_PHONG).  False: the stand-alone
        `bind_gaussians_phong` op in front of render() (same results; the A/B and the op's own user)."""
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise RuntimeError("SplattingStep: data-parallel runs are not built (DESIGN.md)")
        self.canonical = PhongCanonical(*[t.to(pc.flat.device).contiguous() for t in canonical])
        if pc.P and (int(pc.face_index.min()) < 0 or int(pc.face_index.max()) >= int(self.canonical.faces.shape[0])):
            raise ValueError("SplattingStep: `face_index` names a face the mesh does not have")
        super().__init__(pc, self.canonical.faces, camera, bg, verts, lrs, use_graph, fold_binding, data_parallel=False)

    def _forward_backward(self):
        pc = self.pc
        pc.begin_step()                                             # zero_grad(set_to_none=True)
        stats = (self.xyz_gradient_accum, self.denom, pc.overflow_word)
        if self.fold_binding:
            from . import rasterizer
            out = render_bound_batch([self.cam], [_SplattingFrame(pc, stats)], [self.verts],
                                     PhongBinding(self.faces, pc.face_index, pc.bary_coords, self.canonical), self.bg,
                                     slots=[rasterizer._slot])[0]
        else:
            frame = phong_frame(self.canonical, self.verts)
            bound = bind_gaussians_phong(self.verts, self.faces, pc.face_index, pc.bary_coords, frame, pc._uvd, pc._rotation,
                                         pc._scaling)
            out = render(self.cam, _SplattingFrame(pc, stats, bound), self.bg)
        out["render"].backward(self._image_loss_and_grad(out["render"]))   # see TrainStep
        pc.collect_grads()
        self.out = self._kept(out)

    # ---- SplattingAvatar's density control, triangle walk and opacity reset (:386-715), with RiggedStep's conventions: torch
    #      index surgery under no_grad between step() calls, optimizer state through FusedAdam.remap_rows, the graph dropped
    #      when the buffers move; `reset_opacity` is TrainStep's (:697-715 is the same rule), in place
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

    @torch.no_grad()
    def _append(self, rows, face_index, bary) -> int:
        """Appends `rows` (FIELDS order) embedded at (`face_index`, `bary`) with zero moments; the statistics restart from zero
        whether or not anything was appended (_densification_postfix always runs, :577-603)."""
        n = int(face_index.numel())
        if n == 0:
            self.xyz_gradient_accum.zero_()
            self.denom.zero_()
            return 0
        pc = self.pc
        old_rows = pc.P
        old_index = pc.resize(new_rows=rows, new_face_index=face_index, new_bary=bary)
        self._buffers_moved(old_index, old_rows, stats=None)
        return n

    @torch.no_grad()
    def prune(self, mask: torch.Tensor) -> int:
        """_prune (:606-665): removes the Gaussians marked in `mask` [P]; the surviving rows keep their statistics and moments.
        Returns the number of Gaussians removed."""
        pc = self.pc
        mask = mask.to(self.dev).bool().reshape(-1)
        if mask.numel() != pc.P:
            raise ValueError("prune: mask must have one entry per Gaussian")
        n = int(mask.sum())
        if n == 0:
            return 0
        keep = ~mask
        stats = (self.xyz_gradient_accum[keep].contiguous(), self.denom[keep].contiguous())
        old_rows = pc.P
        old_index = pc.resize(keep_mask=keep)
        self._buffers_moved(old_index, old_rows, stats=stats)
        return n

    @torch.no_grad()
    def prune_low_opacity(self, min_opacity: float = 0.005) -> int:
        """`prune` with the opacity mask of _densify_and_prune (:395-397)."""
        return self.prune((torch.sigmoid(self.pc._opacity) < min_opacity).reshape(-1))

    @torch.no_grad()
    def densify_and_prune(self, max_grad: float = 2e-4, min_opacity: float = 0.005, extent: float = 2.0, max_screen_size=None,
                          generator: Optional[torch.Generator] = None):
        """_densify_and_prune with _clone_densify and _split_densify (:386-574); call it between step() calls.  Returns (cloned,
        split, pruned) row counts.
          * grads = xyz_gradient_accum / denom, NaN -> 0 (:389-390)
          * clone (:407-470): rows with grads >= max_grad and max exp(_scaling) <= percent_dense * extent are appended as they
            are, with their face_index / bary_coords
          * split (:473-574), over the set after the clone (the clones' padded gradient is 0), N = 2: rows with grads >= max_grad
            and max exp(_scaling) > percent_dense * extent get two children at R(_rotation) . sample + xyz_cano, sample ~
            N(0, exp(_scaling)) — ONE torch.normal call of shape [2 n, 3], made on the generator's device.  `xyz_cano` is the
            reference's MIXTURE (:490-502), kept: the barycentric point on the step's CURRENT POSED vertices (the last frame's)
            plus the CANONICAL interpolated normal times `_uvd[:, 2]`.  The children are re-embedded on the canonical mesh by
            `PhongSurface.update_corres_spt` (:517) starting from the parent's face and (u, v): bary = (u, v, 1 - u - v),
            `_uvd` = (0, 0, the parent's d) — the fitted d is discarded, as in the reference —, _scaling = log(exp(_scaling) /
            (0.8 N)), everything else repeated; the selected originals are then removed
          * appended rows start with zero Adam moments, the step count is kept; the statistics restart from zero after the
            clone and after the split, even when nothing was selected
          * final prune (:395-404): sigmoid(_opacity) < min_opacity, and with a truthy `max_screen_size` also max exp(_scaling) >
            0.1 * extent.  The reference also ORs in `max_radii2D > max_screen_size`; that test can never fire there
            (_densification_postfix zeroes max_radii2D in clone and in split immediately before it), so max_radii2D is not
            tracked here.
        `self.last_fit_iterations` holds the fit's iteration count per outer round (empty if nothing was split)."""
        pc = self.pc
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        grads = torch.norm(grads, dim=-1)
        fields = lambda sel: [getattr(pc, name).detach()[sel] for name, _ in pc.FIELDS]  # noqa: E731
        largest = lambda: torch.exp(pc._scaling.detach()).max(dim=1).values  # noqa: E731
        # ---- clone
        sel = (grads >= max_grad) & (largest() <= PERCENT_DENSE * extent)
        n_clone = self._append(fields(sel), pc.face_index[sel], pc.bary_coords[sel])
        # ---- split
        N = 2
        padded = torch.zeros(pc.P, device=self.dev)
        padded[:grads.shape[0]] = grads
        sel = (padded >= max_grad) & (largest() > PERCENT_DENSE * extent)
        n_split = int(sel.sum())
        self.last_fit_iterations = []
        rows = [r.repeat((N,) + (1,) * (r.dim() - 1)) for r in fields(sel)]
        i_uvd, i_rot, i_scl = (self._field_index(n) for n in ("_uvd", "_rotation", "_scaling"))
        stds = torch.exp(rows[i_scl])                           # exp(_scaling)[sel].repeat(N, 1)
        gdev = generator.device if generator is not None else self.dev
        samples = torch.normal(mean=torch.zeros((stds.shape[0], 3), device=gdev), std=stds.to(gdev), generator=generator).to(self.dev)
        fidx, bary = pc.face_index[sel].repeat(N), pc.bary_coords[sel].repeat(N, 1)
        if n_split:
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
        rows[i_scl] = torch.log(stds / (0.8 * N))
        self._append(rows, fidx, bary)
        if n_split:
            self.prune(torch.cat([sel, torch.zeros(N * n_split, dtype=torch.bool, device=self.dev)]))
        # ---- prune
        mask = (torch.sigmoid(pc._opacity.detach()) < min_opacity).reshape(-1)
        if max_screen_size:
            mask |= torch.exp(pc._scaling.detach()).max(dim=1).values > 0.1 * extent
        return n_clone, n_split, self.prune(mask)

    def densify_by_gradient(self, *a, **k):
        raise NotImplementedError("SplattingStep: the set densifies with densify_and_prune() (SplattingAvatar's clone / split)")

    def reduce_densification_stats(self, *a, **k):
        raise NotImplementedError("SplattingStep: data-parallel runs are not built (DESIGN.md)")

    # ---- checkpoints: 'model' holds the six parameters under the reference's names and the embedding buffers
    GAUSSIAN_ATTRIBUTES = ["_uvd", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "sample_fidxs",
                           "sample_bary"]

    def state_dict(self) -> dict:
        pc = self.pc
        model = {name: getattr(pc, name).detach().clone() for name, _ in pc.FIELDS}
        model["sample_fidxs"], model["sample_bary"] = pc.face_index.clone(), pc.bary_coords.clone()
        return {"global_step": self.adam.step_count, "model": model, **self._training_state()}

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
        pc.face_index = g["sample_fidxs"].to(self.dev, torch.int32).contiguous()
        pc.bary_coords = g["sample_bary"].to(self.dev, torch.float32).contiguous()
        P = int(pc.face_index.shape[0])
        pc._bind([g[name].to(self.dev, torch.float32).reshape((P,) + pc.SHAPES[name]) for name, _ in pc.FIELDS])
        # FRESH, not remapped: a checkpoint without an `optimizer` entry starts the optimizer over, step count 0
        self._buffers_moved(None, None, stats=None)
        self._load_training_state(sd)
        return sorted(model.keys())


__all__ = ["NUM_INIT_SAMPLES", "SPLATTING_LRS", "SplattingGaussians", "SplattingStep", "phong_canonical", "sample_bary_on_triangles"]
