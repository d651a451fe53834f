"""The per-frame optimisation step around the path.

reference loop: `iteration_step_fateavatar`, train/iteration.py:21-89 —
    zero_grad(set_to_none) -> render -> L1(mean) -> backward -> _add_densification_stats -> Adam.step()
with the Adam groups of train/optim.py:11-37 and the learning rates of config/fateavatar.yaml:34-39
(generic-3DGS variant for the positions).  Densify / prune / opacity reset are
reference model surgery outside the path and are not reproduced.

What is fused here compared with the reference: the activations and the densification statistics run inside
the rasterizer kernels (FR_FLAG_RAW_ACTIVATIONS, fr_aux), Adam is one kernel over the flat parameter buffer
(fr_adam_step), and the whole step — about 20 kernel launches instead of about 90 — is replayed as ONE HIP graph.
Data-parallel (one frame per rank): the flat gradient is summed over ranks with one RCCL
all-reduce between the backward and the Adam kernel (which applies 1/world); the densification statistics are
plain sums over frames, so every rank accumulates its own and `reduce_densification_stats()` adds them up
when they are needed.
"""
from __future__ import annotations

import copy
from typing import Optional

import torch

from . import dp
from .loss import (ImageLoss, PixelLoss, image_loss_and_grad, image_loss_workspace, l1_loss_and_grad, l1_workspace, multi_copy,
                   pixel_loss_and_grad, pixel_loss_workspace)
from .model import FlatGaussians, TorchCamera
from .optim import FusedAdam
from .render import render

# config/fateavatar.yaml:34-39 (+ the generic 3DGS position rate; FateAvatar optimises a mesh offset instead)
DEFAULT_LRS = dict(xyz=1.6e-4, feature_dc=2.5e-3, feature_rest=2.5e-3 / 20, opacity=0.05, scaling=5e-3, rotation=1e-3)
PERCENT_DENSE = 0.01     # clone / split threshold as a share of the scene extent (gaussianavatars.py:47, splattingavatar.py)


class TrainStep:
    def __init__(self, pc: FlatGaussians, camera: TorchCamera, bg: torch.Tensor, lrs: Optional[dict] = None,
                 use_graph: bool = True, image_loss: Optional[ImageLoss] = None):
        """`image_loss`: an `ImageLoss(rgb_weight, dssim_weight)` makes the image term rgb_weight x L1 + dssim_weight x d_ssim
        (the original 3DGS objective is ImageLoss(0.8, 0.2)): two launches of `loss.image_loss_and_grad` where the L1 launch
        is; `loss_terms` then holds the step's (weighted total, l1, d_ssim) and `loss` is its first word.  A
        `PixelLoss(rgb_weight, mse_weight)` makes it rgb_weight x L1 + mse_weight x MSE (SplattingAvatar's image term): ONE launch
        of `loss.pixel_loss_and_grad` where the L1 launch is; `loss_terms` then holds (weighted total, l1, mse).  None (default):
        the plain L1 step, `loss_terms` is None."""
        if not pc.fused_activations:
            raise ValueError("TrainStep drives the fused path: build FlatGaussians(..., fused_activations=True)")
        self.pc, self.bg = pc, bg
        self.dev = pc.flat.device
        self._init_exchange()
        if use_graph and self.exchange and not self.exchange_in_graph:
            import warnings
            warnings.warn(f"TrainStep: the {torch.distributed.get_backend()} exchange cannot be captured; the all-reduce and Adam "
                          "run eagerly behind the captured frame")
        self.lr = dict(DEFAULT_LRS, **(lrs or {}))
        self._make_adam()
        self._init_step_state(camera, use_graph, image_loss)

    def _init_exchange(self, data_parallel: bool = True):
        self.world = torch.distributed.get_world_size() if data_parallel and torch.distributed.is_initialized() else 1
        # RCCL ("nccl") collectives can be captured into a HIP graph: the whole step — render, backward, all-reduce of
        # the flat gradient buffer, Adam — is then ONE replay, with no host work between the backward and the update.
        # (gloo cannot be captured: the CPU tests keep the eager exchange.)
        self.exchange = data_parallel and torch.distributed.is_initialized() and (self.world > 1 or dp.group_of_one())
        self.exchange_in_graph = self.exchange and torch.distributed.get_backend() == "nccl"

    def adam_segments(self):
        """The optimizer groups (train/optim.py:11-37) as runs of the flat buffer; the SH block is one run, DC at
        feature_dc, the rest at feature_rest (FusedAdam's 5-tuple form)."""
        lr, P, M = self.lr, self.pc.P, self.pc.M
        return [(P * 3, lr["xyz"]), (P * M * 3, lr["feature_dc"], M * 3, 3, lr["feature_rest"]),
                (P, lr["opacity"]), (P * 3, lr["scaling"]), (P * 4, lr["rotation"])]

    def _make_adam(self):
        """A FRESH optimizer over the holder's present buffers: zero moments, step count 0."""
        pc = self.pc
        self.adam = FusedAdam(pc.flat, pc.flat_grad, self.adam_segments(), grad_scale=1.0 / self.world)
        # a replayed frame that overflowed its binning capacity back-propagates zeros: the rasterizer's backward says so in
        # the word behind the gradient buffer (summed over ranks by the same all-reduce) and the update skips that step
        self.adam.set_skip_words([pc.overflow_word])

    def _init_step_state(self, camera: TorchCamera, use_graph: bool, image_loss: Optional[ImageLoss] = None):
        """Everything the captured step reads and writes besides the parameters, and the bookkeeping of the capture."""
        self._set_stats(None)
        # static inputs of the captured step
        self.cam = camera
        self.gt = torch.zeros((3, camera.image_height, camera.image_width), device=self.dev)
        self.loss = torch.zeros((), device=self.dev)
        self._dimage = torch.zeros_like(self.gt)   # dL/dimage of the step
        self._l1_ws = l1_workspace(self.dev)       # scratch of this step's loss kernel (not shared with launches that may overlap)
        self._init_image_loss(image_loss)
        self.out = None
        self.use_graph = bool(use_graph)
        self._graph = None       # render .. backward (.. Adam when world == 1)
        self._eager_steps = 0
        self.overflows = 0       # replayed frames that overflowed the captured binning capacity (see _poll_overflow)
        self.host_steps = 0      # step() calls; the device's own count of APPLIED updates is adam.step_count (skipped_steps)

    STATS_ON_HOLDER = True       # render() reads the statistics' buffers from the holder (a bound frame carries its own)

    def _set_stats(self, stats):
        """The _add_densification_stats accumulators (model/fateavatar.py:186-188,734-737), updated by the backward kernel:
        `stats` = the (xyz_gradient_accum, denom) to go on with, or None: they restart from zero."""
        if stats is None:
            stats = (torch.zeros((self.pc.P, 1), device=self.dev), torch.zeros((self.pc.P, 1), device=self.dev))
        self.xyz_gradient_accum, self.denom = stats
        if self.STATS_ON_HOLDER:
            self.pc.fused_densification_stats = (self.xyz_gradient_accum, self.denom, self.pc.overflow_word)

    def _init_image_loss(self, image_loss):
        """The buffers of the step's L1 + D-SSIM (an `ImageLoss`) or L1 + MSE (a `PixelLoss`) image term (after self.gt /
        self.loss exist): `loss` becomes a view of loss_terms[0]."""
        if image_loss is not None and not isinstance(image_loss, (ImageLoss, PixelLoss)):
            raise TypeError(f"{type(self).__name__}: `image_loss` is an ImageLoss (L1 + D-SSIM), a PixelLoss (L1 + MSE) or None, "
                            f"not {type(image_loss).__name__}")
        self.image_loss = None if image_loss is None else type(image_loss)(*[float(x) for x in image_loss])
        self.loss_terms, self._image_ws = None, None
        if self.image_loss is not None:
            self.loss_terms = torch.zeros(3, device=self.dev)
            self.loss = self.loss_terms[0]
            self._image_ws = pixel_loss_workspace(self.dev) if isinstance(self.image_loss, PixelLoss) else \
                image_loss_workspace(self.dev, *self.gt.shape)

    def _image_loss_and_grad(self, image: torch.Tensor) -> torch.Tensor:
        """dL/dimage of the step's image term, written into the step's buffers with the loss."""
        if self.image_loss is None:
            # nn.L1Loss(reduction='mean') (loss.py:92) + loss.backward(): the loss and the gradient autograd would hand to the
            # rasterizer in one launch, written straight into the step's buffers
            _, g = l1_loss_and_grad(image, self.gt, loss_out=self.loss, grad_out=self._dimage, workspace=self._l1_ws)
        elif isinstance(self.image_loss, PixelLoss):
            _, g = pixel_loss_and_grad(image, self.gt, self.image_loss, loss_out=self.loss_terms, grad_out=self._dimage,
                                       workspace=self._image_ws)
        else:
            _, g = image_loss_and_grad(image, self.gt, self.image_loss, loss_out=self.loss_terms, grad_out=self._dimage,
                                       workspace=self._image_ws)
        return g

    # -- the step body: everything between zero_grad and the gradient exchange
    def _forward_backward(self):
        self.pc.begin_step()                                   # zero_grad(set_to_none=True), iteration.py:48-49
        out = render(self.cam, self.pc, self.bg)               # activations + rasterizer (fused)
        # the image term and its gradient (_image_loss_and_grad), then the rasterizer backward (stats fused)
        out["render"].backward(self._image_loss_and_grad(out["render"]))
        self.out = self._kept(out)

    @staticmethod
    def _kept(out: dict) -> dict:
        """The step's outputs WITHOUT their autograd graph: a graph kept alive across steps keeps its AccumulateGrad nodes
        (and the stream they were created on) alive, which breaks a later stream capture."""
        return {"render": out["render"].detach(), "radii": out["radii"], "visibility_filter": out["visibility_filter"]}

    def _exchange_and_update(self):
        dp.allreduce_sum_(self.pc.exchange_buffer())  # gradients + overflow word; Adam applies grad_scale = 1 / world
        self.adam.step()

    def _body(self):
        self._forward_backward()
        if not self.exchange:
            self.adam.step()
        elif self.exchange_in_graph:
            self._exchange_and_update()

    def _capture(self):
        from . import rasterizer
        # nothing in the captured frame may wait on the host: FR_FLAG_NO_WAIT, scoped to the capture (a replay does not
        # go through rasterize_gaussians at all), so that other renders of the process keep their overflow handling
        with rasterizer.no_wait():
            # one frame on a side stream warms the allocator pools of the capture path; it is not a step (no Adam), so
            # the statistics it accumulated are put back
            acc, den = self.xyz_gradient_accum.clone(), self.denom.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._forward_backward()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.xyz_gradient_accum.copy_(acc)
            self.denom.copy_(den)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):  # thread_local: an RCCL watchdog thread may exist
                self._body()
            torch.cuda.synchronize()
        self._graph = g

    def step(self, camera: TorchCamera, gt_image: torch.Tensor, _extra=()) -> torch.Tensor:
        """One optimisation step on this rank's frame.  Returns the (device) loss scalar of the step.  (`_extra`: further
        (static buffer, value) pairs a subclass loads with the frame's inputs.)"""
        self.host_steps += 1
        self._load_inputs(camera, gt_image, _extra)
        if self.use_graph and self._graph is None and self._eager_steps >= 2:
            self._capture()
        if self._graph is not None:
            self._poll_overflow()     # may drop the graph
        if self._graph is not None:
            self._graph.replay()
        else:
            self._body()              # eager: first steps size the binning capacity (high-water mark)
            self._eager_steps += 1
        if self.exchange and not self.exchange_in_graph:
            self._exchange_and_update()
        return self.loss

    def _load_inputs(self, camera: TorchCamera, gt_image: torch.Tensor, extra=()) -> None:
        """The frame's inputs go into the buffers the step was captured with — camera block, target image and whatever
        a subclass adds — in one launch when they are device tensors already."""
        pairs = list(extra)
        if camera is not self.cam:
            self.cam.check_same_intrinsics(camera)
            pairs.append((self.cam._packed, camera._packed))
        pairs.append((self.gt, gt_image))
        if all(s.is_cuda and s.dtype == torch.float32 and s.is_contiguous() and s.shape == d.shape for d, s in pairs):
            multi_copy(pairs)
        else:
            for d, s in pairs:
                d.copy_(s, non_blocking=True)

    @property
    def skipped_steps(self) -> int:
        """Steps whose update the device skipped because a captured frame overflowed its binning capacity (the overflow word,
        FusedAdam.set_skip_words): step() calls minus applied Adam updates.  The host-side schedules (learning-rate decay,
        densify / prune / reset intervals) advance with step() calls; a caller that wants the lost iterations back re-runs this
        many.  Reads device state: synchronises."""
        return self.host_steps - self.adam.step_count

    def _poll_overflow(self):
        """The sort kernel of every frame writes its counts to pinned host memory; reading them costs nothing and
        needs no synchronisation (they belong to the most recent frame that has got that far).  A replayed frame that
        overflowed the capacity the graph was captured with produced no image and no gradients — and its Adam launch did
        nothing (the overflow word the backward sets, FusedAdam.set_skip_words): raise the capacity, drop the graph (the
        next steps run eagerly with the overflow check, then re-capture) and count the event."""
        from . import rasterizer
        if rasterizer.check_async_overflow(self.dev.index or 0):
            self.overflows += 1
            self._graph, self._eager_steps = None, 0
            # every occurrence warns.  The replays since the overflow SKIPPED their update on the device: the Adam step count
            # (`self.adam.step_count`, device state) stays behind the host's iteration counters by the number of skipped steps —
            # the `skipped_steps` property is that difference, for callers whose schedules should re-run the lost iterations
            import warnings
            warnings.warn(f"{type(self).__name__}: the binning capacity overflowed inside the captured step (occurrence "
                          f"{self.overflows}); the affected replays back-propagated zeros and their optimizer launch skipped the "
                          "step (overflow word; `skipped_steps` counts them), the step runs eagerly and is captured again")

    # -- Gaussian maintenance (reference: train/iteration.py:62-86 -> model/fateavatar.py:610-731), generic-3DGS flavour:
    #    the FateAvatar versions additionally carry the mesh binding (face index, barycentrics) of every row
    @torch.no_grad()
    def _buffers_moved(self, old_index, old_rows, *, stats):
        """After the holder rebuilt its buffers (resize, _bind): re-attach the optimizer, point the update at the new
        overflow word and drop the captured step.  `old_index`: the row map the moments follow (FusedAdam.remap_rows: rows
        mapped to -1 start with zero moments, the step count is KEPT) — or None for a FRESH optimizer (`_make_adam`: zero
        moments, step count 0).  `stats`: see `_set_stats` — the caller says whether the statistics restart or are carried."""
        pc = self.pc
        if old_index is None:
            self._make_adam()
        else:
            self.adam.remap_rows(pc.flat, pc.flat_grad, old_index, pc.widths(), old_rows)
            self.adam.set_skip_words([pc.overflow_word])
        self._set_stats(stats)
        self._graph, self._eager_steps = None, 0   # buffers moved: the captured step is stale

    @torch.no_grad()
    def _resize(self, *, carry_stats: bool, **resize_kw) -> torch.Tensor:
        """THE way a step changes its point set between step() calls: `pc.resize(**resize_kw)`, then `_buffers_moved` along
        the row map it returned — the moments follow their rows, appended rows start with zero moments, the step count is
        kept, the captured step is dropped.  `carry_stats`: the statistics follow their rows too (a prune, a re-ordering;
        no caller appends and carries, so a map with appended rows is refused); False: they restart from zero, as after
        every change of the point set in model/fateavatar.py:667-672.  Returns the row map."""
        pc = self.pc
        old_rows = pc.P
        old_index = pc.resize(**resize_kw)
        stats = None
        if carry_stats:
            if bool((old_index < 0).any()):
                raise ValueError("_resize: appended rows have no statistics to carry")
            stats = (self.xyz_gradient_accum[old_index].contiguous(), self.denom[old_index].contiguous())
        self._buffers_moved(old_index, old_rows, stats=stats)
        return old_index

    @torch.no_grad()
    def prune_low_opacity(self, min_opacity: float = 0.005) -> int:
        """_prune_low_opacity_points (model/fateavatar.py:674-711); generic 3DGS: the statistics restart from zero after a change
        of the point set (:667-672).  Returns the number of Gaussians removed."""
        old_rows = self.pc.P
        self._resize(carry_stats=False, keep_mask=~(torch.sigmoid(self.pc._opacity) < min_opacity).reshape(-1))
        return old_rows - self.pc.P

    @torch.no_grad()
    def _draw_by_gradient(self, increase_num: int, generator: Optional[torch.Generator], uniforms: int = 0):
        """The draw of _uv_densify (model/fateavatar.py:610-624): `increase_num` rows with probability proportional to
        xyz_gradient_accum (multinomial, with replacement), then `uniforms` uniform numbers per drawn row.  Data-parallel: the
        statistics are per-view sums (model/fateavatar.py:734-737), so both draws are made on rank 0 (`generator`: rank 0's
        only) from the sum over all ranks and broadcast — every replica appends the same rows.  Returns (the row indices,
        the uniforms [increase_num, uniforms], the drawn rows' values in FIELDS order with their scale multiplied by 0.75)."""
        pc = self.pc
        acc, _ = self.reduce_densification_stats()
        w = acc.reshape(-1)
        idx = torch.zeros(increase_num, dtype=torch.int64, device=self.dev)
        u = torch.zeros((increase_num, uniforms), dtype=torch.float32, device=self.dev)
        if float(w.sum()) <= 0:       # (the summed statistics are identical on every rank: all of them raise, none is left
            raise RuntimeError("no densification statistics accumulated yet")   # waiting in the broadcast below)
        if not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0:
            idx = torch.multinomial(w, increase_num, replacement=True, generator=generator)
            if uniforms:
                u = torch.rand((increase_num, uniforms), device=self.dev, generator=generator)
        dp.broadcast_(idx)
        if uniforms:
            dp.broadcast_(u)
        rows = [getattr(pc, name).detach()[idx].clone() for name, _ in pc.FIELDS]
        i = self._field_index("_scaling")
        rows[i] = torch.log(torch.exp(rows[i]) * 0.75)          # new_scaling (:624)
        return idx, u, rows

    @torch.no_grad()
    def densify_by_gradient(self, increase_num: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """The sampling and cloning rule of _uv_densify (model/fateavatar.py:610-672) without the mesh re-binding
        (`_draw_by_gradient`); appended rows start with zero Adam moments.  Returns the sampled row indices."""
        idx, _, rows = self._draw_by_gradient(increase_num, generator)
        self._resize(carry_stats=False, new_rows=rows)
        return idx

    @torch.no_grad()
    def reset_opacity(self) -> None:
        """_reset_opacity (model/fateavatar.py:713-731): opacity <- min(opacity, 0.01), its Adam moments <- 0."""
        pc = self.pc
        cur = torch.sigmoid(pc._opacity)
        new = torch.minimum(cur, torch.full_like(cur, 0.01))
        pc._opacity.data.copy_(torch.log(new / (1 - new)))
        # in place: the captured graph keeps pointing at the same parameter and moment buffers
        self.adam.zero_field_moments(pc.widths(), pc.P, fields=(self._field_index("_opacity"),))

    def _field_index(self, name: str) -> int:
        return [n for n, _ in self.pc.FIELDS].index(name)

    # -- checkpoint / resume (reference layout: Trainer.save_checkpoint, train/trainer.py:396-435 — a dict with
    #    'global_step' and 'model' = the Gaussian parameters under the GaussianModel names and shapes; the reference
    #    does not save optimizer state, `optimizer` and `densification` here are additions a resume needs)
    @torch.no_grad()
    def state_dict(self) -> dict:
        pc = self.pc
        f = pc._features.detach()
        model = {"_xyz": pc._xyz.detach().clone(), "_features_dc": f[:, :1, :].clone(), "_features_rest": f[:, 1:, :].clone(),
                 "_opacity": pc._opacity.detach().clone(), "_scaling": pc._scaling.detach().clone(),
                 "_rotation": pc._rotation.detach().clone()}
        return {"global_step": self.adam.step_count, "model": model, **self._training_state()}

    def _training_state(self) -> dict:
        """The `optimizer` and `densification` entries of a checkpoint."""
        return {"optimizer": {"exp_avg": self.adam.exp_avg.clone(), "exp_avg_sq": self.adam.exp_avg_sq.clone(),
                              "state": self.adam.state_words()},
                "densification": {"xyz_gradient_accum": self.xyz_gradient_accum.clone(), "denom": self.denom.clone()}}

    @torch.no_grad()
    def _load_training_state(self, sd: dict) -> None:
        """Restores what `_training_state` wrote, after `_buffers_moved(.., stats=None)` re-attached the optimizer: an entry
        the checkpoint lacks leaves what that call made (zero moments and zero statistics; the step count as it chose)."""
        opt, dens = sd.get("optimizer"), sd.get("densification")
        if opt is not None:
            self.adam.exp_avg.copy_(opt["exp_avg"])
            self.adam.exp_avg_sq.copy_(opt["exp_avg_sq"])
            self.adam.load_state_words(opt["state"])
        self.host_steps = self.adam.step_count          # (skipped_steps counts from the restored state on)
        if dens is not None:
            self.xyz_gradient_accum.copy_(dens["xyz_gradient_accum"])
            self.denom.copy_(dens["denom"])

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        pc, m = self.pc, sd["model"]
        rows = [m["_xyz"], torch.cat([m["_features_dc"], m["_features_rest"]], dim=1), m["_opacity"], m["_scaling"],
                m["_rotation"]]
        if int(rows[1].shape[1]) != pc.M:
            raise ValueError("checkpoint holds a different number of SH coefficients")
        old_rows = pc.P
        pc._bind([r.to(self.dev, torch.float32) for r in rows])
        # REMAPPED, not fresh: a checkpoint without an `optimizer` entry goes on from this step's count with zero moments
        self._buffers_moved(torch.full((pc.P,), -1, dtype=torch.int64, device=self.dev), old_rows, stats=None)
        self._load_training_state(sd)

    def check(self) -> None:
        """After synchronising: raise if a captured (no-wait) frame overflowed its binning capacity."""
        from . import rasterizer
        if self._graph is not None and rasterizer.check_async_overflow(self.dev.index or 0):
            raise RuntimeError("binning capacity overflowed inside the captured step; re-create the TrainStep")

    def reduce_densification_stats(self):
        """(xyz_gradient_accum, denom) summed over all ranks (they are sums over the frames each rank has seen)."""
        acc, den = self.xyz_gradient_accum.clone(), self.denom.clone()
        if self.world > 1:
            dp.allreduce_sum_(acc)
            dp.allreduce_sum_(den)
        return acc, den


class BoundStep(TrainStep):
    """What the steps of the mesh-bound models share on top of TrainStep: `step(camera, posed_verts, gt_image)` — the posed
    vertices are one more static input of the captured step —, the choice between the binding folded into the rasterizer's
    per-Gaussian kernels and the stand-alone binding op, one Adam group per field of the holder, and the checkpoint pair.  A
    subclass names its rates (`LRS`, `LR_KEYS`) and its checkpoint layout (`GAUSSIAN_ATTRIBUTES`, `ROW_BUFFER_KEYS`,
    `RESUME_REMAPPED`) and writes `_forward_backward`."""
    LRS: dict = {}            # the model's learning rates by the reference's group names
    LR_KEYS: dict = {}        # field of the holder -> its key in LRS
    STATS_ON_HOLDER = False   # every frame carries the statistics' buffers itself
    GAUSSIAN_ATTRIBUTES: list = []   # what a checkpoint's 'model' must hold of the Gaussians
    ROW_BUFFER_KEYS: dict = {}       # row buffer of the holder -> its name in 'model' (default: the attribute's own)
    RESUME_REMAPPED = False          # load_state_dict without an `optimizer` entry: the step count goes on, or (False) restarts
    VERTEX_GRAD = True               # the model's binding has a gradient to the posed vertices (`vertex_grad=True`) ...
    VERTEX_GRAD_MISSING = ""         # ... or why it has none
    CAMERA_GRAD = False              # the step keeps the frame's camera gradients (`camera_grad=True`): AvatarStep

    def __init__(self, pc, faces: torch.Tensor, camera: TorchCamera, bg: torch.Tensor, verts: torch.Tensor,
                 lrs: Optional[dict] = None, use_graph: bool = True, fold_binding: bool = True,
                 image_loss: Optional[ImageLoss] = None, data_parallel: bool = True, vertex_grad: bool = False,
                 camera_grad: bool = False):
        """`verts` [V,3]: any pose of the mesh (sizes the step's static vertex buffer and is its first content).
        `vertex_grad`: after every `step()`, `d_verts` [V,3] holds THIS step's dLoss/dposed_verts (the binding's backward
        scatters it; zeroed by the step itself, never accumulated over steps; one storage across the replays of a captured
        step, like `out`) — the caller goes on with `posed_verts.backward(step.d_verts)` into whatever made the mesh (FLAME
        and its blendshape deltas: stock PyTorch) and its own optimizer.  It is this rank's frame's gradient: the caller's
        mesh parameters need their own all-reduce.  A replay that overflowed its binning capacity back-propagated zeros.
        False (default): no such buffer, `d_verts` is None and the kernels are handed no vertex-gradient array.
        `camera_grad`: after every `step()`, `d_view` [4,4], `d_proj` [4,4] and `d_campos` [3] hold THIS step's dLoss/d(the
        camera's world_view_transform, full_proj_transform, camera_center) — what the reference's `cam_pose` tracking embedding
        (train/base.py:123,142) needs and its rasterizer does not return; the caller chains them through its own camera
        construction (`model.PoseCamera`: `wvt.backward(step.d_view)` ...) into its own optimizer.  Like `d_verts`: this step's,
        this rank's, one storage across the replays of a captured step, zeros after a replay that overflowed.  False
        (default): no such buffers, no extra launch."""
        if camera_grad and not self.CAMERA_GRAD:
            raise NotImplementedError(f"{type(self).__name__}(camera_grad=True): camera gradients are built for AvatarStep only "
                                      "(render through a model.PoseCamera for any other model)")
        self.camera_grad, self.d_view, self.d_proj, self.d_campos = bool(camera_grad), None, None, None
        if vertex_grad and not self.VERTEX_GRAD:
            raise NotImplementedError(f"{type(self).__name__}(vertex_grad=True): {self.VERTEX_GRAD_MISSING}")
        self.vertex_grad, self.d_verts = bool(vertex_grad), None
        if not data_parallel and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise RuntimeError(f"{type(self).__name__}: data-parallel runs are not built (DESIGN.md)")
        self.pc, self.bg = pc, bg
        self.fold_binding = bool(fold_binding)
        self.dev = pc.flat.device
        self._init_exchange(data_parallel)
        self.lr = dict(self.LRS, **(lrs or {}))
        self.faces = faces.to(self.dev, torch.int32).contiguous()
        self._make_adam()
        self.verts = verts.detach().to(self.dev, torch.float32).clone().contiguous()   # static input of the captured step
        self._init_step_state(camera, use_graph, image_loss)

    # -- the LPIPS term of the objectives that carry one (FlashStep, SplattingStep): `lpips=` of their constructors
    lpips = lpips_loss = None

    def _init_lpips(self, lpips, pc) -> None:
        """The checks of AvatarStep's `perceptual=` for `lpips=` (before anything is built); None: nothing changes."""
        if lpips is not None:
            from .perceptual import Lpips
            if not isinstance(lpips, Lpips):
                raise TypeError(f"{type(self).__name__}: `lpips` must be a perceptual.Lpips")
            if lpips.features.device != pc.flat.device:
                raise ValueError(f"{type(self).__name__}: the LPIPS term and the Gaussians live on different devices")
            # [1 + T]: the step's UNWEIGHTED terms (the objective adds lpips.weight x lpips_loss[0]); `loss` / `loss_terms` keep
            # their meaning
            self.lpips_loss = torch.zeros(1 + lpips.n_terms, device=pc.flat.device)
        self.lpips = lpips

    def _add_lpips(self, image: torch.Tensor, g: torch.Tensor) -> None:
        """ONE call behind the step's image-loss launch (csrc/fr_vgg.hip) ADDS weight x the term's gradient to the image
        gradient `g` in place, in front of the rasterizer's backward."""
        if self.lpips is not None:
            self.lpips.loss_and_grad(image, self.gt, loss_out=self.lpips_loss, grad_out=g, accumulate=True)

    def adam_segments(self):
        """The optimizer groups (train/optim.py, one per parameter in the holder's order) as runs of the flat buffer; an
        empty field keeps its place and rate."""
        P = self.pc.P
        return [(P * w, self.lr[self.LR_KEYS[name]]) for name, w in self.pc.FIELDS]

    def step(self, camera: TorchCamera, posed_verts: torch.Tensor, gt_image: torch.Tensor, _extra=()) -> torch.Tensor:
        if self.vertex_grad:
            posed_verts = posed_verts.detach()     # (the caller's mesh usually hangs on its autograd graph: only the values are loaded)
        return super().step(camera, gt_image, [(self.verts, posed_verts), *_extra])

    def _vertex_leaf(self, verts: torch.Tensor) -> torch.Tensor:
        """What a frame hands its binding as the posed mesh: the static buffer `verts` itself, or with `vertex_grad` a leaf
        over the same storage (no copy), whose gradient `_keep_vertex_grad` picks up after the backward."""
        return verts.detach().requires_grad_(True) if self.vertex_grad else verts

    def _keep_vertex_grad(self, leaf: torch.Tensor) -> None:
        """After the frame's backward: `d_verts` = the leaf's gradient — the buffer the binding's backward zeroed and
        scattered into (inside a captured step: graph-owned storage, the same on every replay)."""
        if self.vertex_grad:
            self.d_verts = leaf.grad

    def _camera_leaf(self, cam):
        """What a frame is rendered through: the static camera `cam` itself, or with `camera_grad` a camera whose three tensors
        are leaves over the same storage (no copy), whose gradients `_keep_camera_grad` picks up after the backward."""
        if not self.camera_grad:
            return cam
        leaf = copy.copy(cam)
        for n in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(leaf, n, getattr(cam, n).detach().requires_grad_(True))
        return leaf

    def _keep_camera_grad(self, leaf) -> None:
        if self.camera_grad:
            self.d_view, self.d_proj, self.d_campos = (leaf.world_view_transform.grad, leaf.full_proj_transform.grad,
                                                       leaf.camera_center.grad)

    # ---- checkpoints in the reference's layout (Trainer.save_checkpoint, train/trainer.py:396-435: a dict with 'global_step'
    #      and 'model' = model.state_dict(), which holds the Gaussian parameters and the binding buffers under the model's
    #      own names next to whatever else the model owns); 'optimizer' and 'densification' are additions a seamless
    #      resume needs, the reference saves neither
    def _save_extras(self, sd: dict) -> None:
        """What the model's checkpoint holds beyond the holder's fields and row buffers: written into `sd`."""

    def _load_extras(self, sd: dict, g: dict) -> None:
        """The model's own checks and entries; `g` = the popped Gaussian attributes.  Runs before anything is changed."""

    @torch.no_grad()
    def state_dict(self) -> dict:
        pc = self.pc
        model = {name: getattr(pc, name).detach().clone() for name, _ in pc.FIELDS}
        model.update({self.ROW_BUFFER_KEYS.get(attr, attr): getattr(pc, attr).clone() for attr, _, _ in pc.ROW_BUFFERS})
        sd = {"global_step": self.adam.step_count, "model": model}
        self._save_extras(sd)
        return {**sd, **self._training_state()}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> list:
        """deserialize_checkpoints_fateavatar (train/deserialize.py:7-40): the Gaussian attributes are POPPED from
        sd['model'] (their row count differs from the freshly built model's), re-attached as parameters / buffers — any row
        count —, and the per-point statistics restart from zero unless the checkpoint brings them; whatever else 'model'
        holds (FLAME, blendshape deltas: outside this path) is returned as the list of ignored keys.  A checkpoint written by
        the reference itself loads the same way."""
        model = dict(sd["model"])
        missing = [k for k in self.GAUSSIAN_ATTRIBUTES if k not in model]
        if missing:
            raise KeyError(f"checkpoint lacks Gaussian attributes {missing}")
        g = {k: model.pop(k) for k in self.GAUSSIAN_ATTRIBUTES}
        self._load_extras(sd, g)
        pc = self.pc
        old_rows, P = pc.P, int(g[pc.FIELDS[0][0]].shape[0])
        for attr, dtype, _ in pc.ROW_BUFFERS:
            setattr(pc, attr, g[self.ROW_BUFFER_KEYS.get(attr, attr)].to(self.dev, dtype).contiguous())
        pc._bind([g[name].to(self.dev, torch.float32).reshape((P,) + pc.SHAPES[name]) for name, _ in pc.FIELDS])
        if self.RESUME_REMAPPED:   # a checkpoint without an `optimizer` entry goes on from this step's count with zero moments
            self._buffers_moved(torch.full((P,), -1, dtype=torch.int64, device=self.dev), old_rows, stats=None)
        else:                      # ... or starts the optimizer over: FRESH, step count 0
            self._buffers_moved(None, None, stats=None)
        self._load_training_state(sd)
        return sorted(model.keys())


class CloneSplitStep(BoundStep):
    """The density control the 3DGS-style bound models share — GaussianAvatars' and SplattingAvatar's `_densify_and_prune`,
    `_clone_densify`, `_split_densify`, `_prune` (model/baseline/gaussianavatars.py:278-475, splattingavatar.py:386-665) — with
    TrainStep's conventions (`_resize`): torch index surgery under no_grad between step() calls, the moments follow their rows,
    the graph is dropped when the buffers move, host_steps is untouched.  A model says where a split child goes
    (`_split_children`) and which marked rows a prune may not take (`_prune_guard`)."""

    def _split_children(self, rows, sel, samples, N):
        """`rows`: the selected parents' values (FIELDS order) repeated N times, `sel` [P] bool: the parents, `samples` [N n, 3]
        ~ N(0, exp(_scaling)).  Returns (the children's rows — their `_scaling` is set by the caller —, their row buffers under
        resize()'s keywords)."""
        raise NotImplementedError

    def _prune_guard(self, mask: torch.Tensor) -> torch.Tensor:
        """The rows of `mask` a prune may remove: all of them, unless the model says otherwise."""
        return mask

    @torch.no_grad()
    def _append(self, rows, **row_buffers) -> int:
        """Appends `rows` (FIELDS order) with their row buffers and zero moments; the statistics restart from zero whether or
        not anything was appended (_densification_postfix always runs, gaussianavatars.py:462-475, splattingavatar.py:577-603)."""
        n = int(rows[0].shape[0])
        if n == 0:
            self.xyz_gradient_accum.zero_()
            self.denom.zero_()
            return 0
        self._resize(carry_stats=False, new_rows=rows, **row_buffers)
        return n

    @torch.no_grad()
    def prune(self, mask: torch.Tensor) -> int:
        """_prune (gaussianavatars.py:418-460, splattingavatar.py:606-665): removes the Gaussians marked in `mask` [P] that
        `_prune_guard` lets go; the surviving rows keep their statistics (:455-456) and moments.  Returns the number of
        Gaussians removed."""
        mask = mask.to(self.dev).bool().reshape(-1)
        if mask.numel() != self.pc.P:
            raise ValueError("prune: mask must have one entry per Gaussian")
        mask = self._prune_guard(mask)
        n = int(mask.sum())
        if n:
            self._resize(carry_stats=True, keep_mask=~mask)
        return n

    @torch.no_grad()
    def prune_low_opacity(self, min_opacity: float = 0.005) -> int:
        """`prune` with the opacity mask of _densify_and_prune (gaussianavatars.py:287, splattingavatar.py:395-397)."""
        return self.prune((torch.sigmoid(self.pc._opacity) < min_opacity).reshape(-1))

    @torch.no_grad()
    def densify_and_prune(self, max_grad: float, min_opacity: float = 0.005, extent: float = 2.0, max_screen_size=None,
                          generator: Optional[torch.Generator] = None):
        """_densify_and_prune with _clone_densify and _split_densify; call it between step() calls.  Returns (cloned, split,
        pruned) row counts.
          * grads = xyz_gradient_accum / denom, NaN -> 0
          * clone: rows with grads >= max_grad and max exp(_scaling) <= percent_dense * extent are appended as they are, with
            their row buffers
          * split, over the set after the clone (the clones' padded gradient is 0), N = 2: rows with grads >= max_grad and max
            exp(_scaling) > percent_dense * extent get two children placed by `_split_children` from sample ~ N(0,
            exp(_scaling)) — ONE torch.normal(mean=zeros, std=stds, generator=generator) call of shape [2 n, 3], made on the
            generator's device, also when nothing is selected — with _scaling = log(exp(_scaling) / (0.8 N)); the selected
            originals are then removed through `prune`
          * appended rows start with zero Adam moments, the step count is kept; the statistics restart from zero after the
            clone and after the split, even when nothing was selected (and then nothing is resized: the captured step stays)
          * final prune: sigmoid(_opacity) < min_opacity, and with a truthy `max_screen_size` also max exp(_scaling) >
            0.1 * extent.  The reference also ORs in `max_radii2D > max_screen_size`; that test can never fire there
            (_densification_postfix zeroes max_radii2D in clone and in split immediately before it), so max_radii2D is not
            tracked here.
        The reference calls this between backward() and optimizer.step(), where the new Parameters have no gradients; that
        ordering is not copied."""
        pc = self.pc
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        grads = torch.norm(grads, dim=-1)
        fields = lambda sel: [getattr(pc, name).detach()[sel] for name, _ in pc.FIELDS]  # noqa: E731
        largest = lambda: torch.exp(pc._scaling.detach()).max(dim=1).values  # noqa: E731
        # ---- clone
        sel = (grads >= max_grad) & (largest() <= PERCENT_DENSE * extent)
        n_clone = self._append(fields(sel), **{key: getattr(pc, attr)[sel] for attr, _, key in pc.ROW_BUFFERS})
        # ---- split
        N = 2
        padded = torch.zeros(pc.P, device=self.dev)
        padded[:grads.shape[0]] = grads
        sel = (padded >= max_grad) & (largest() > PERCENT_DENSE * extent)
        n_split = int(sel.sum())
        rows = [r.repeat((N,) + (1,) * (r.dim() - 1)) for r in fields(sel)]
        stds = torch.exp(rows[self._field_index("_scaling")])   # exp(_scaling)[sel].repeat(N, 1)
        gdev = generator.device if generator is not None else self.dev
        samples = torch.normal(mean=torch.zeros((stds.shape[0], 3), device=gdev), std=stds.to(gdev), generator=generator).to(self.dev)
        rows, row_buffers = self._split_children(rows, sel, samples, N)
        rows[self._field_index("_scaling")] = torch.log(stds / (0.8 * N))
        self._append(rows, **row_buffers)
        if n_split:
            self.prune(torch.cat([sel, torch.zeros(N * n_split, dtype=torch.bool, device=self.dev)]))
        # ---- prune
        mask = (torch.sigmoid(pc._opacity.detach()) < min_opacity).reshape(-1)
        if max_screen_size:
            mask |= torch.exp(pc._scaling.detach()).max(dim=1).values > 0.1 * extent
        return n_clone, n_split, self.prune(mask)
