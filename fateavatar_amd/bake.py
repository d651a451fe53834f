"""Neural baking: FateAvatar's second stage — a trained avatar turned into UV attribute maps — as one captured step.

reference: train_neural_baking.py, `UVBaker.bake_step` (train/baker.py:363-393), `UVDecoder.forward`
(model/uv_decoder.py:387-542) and `UVDecoderLoss` (train/loss.py:522-677): per frame the decoder's [1,11,H,W] output is
sliced, activated (a dozen element-wise launches for the rotation alone), looked up with five grid_sample launches, bound,
rendered, and held to the frame by L1 (+ VGG) with the rot_loss (weight 0.1, train_neural_baking.py:34) and the scale-ratio
term on the DECODED rows; autograd scatters every point's gradient back into the maps with float atomics and
torch.optim.Adam(lr 1e-3) steps `decoder.parameters()` — nothing else (train/baker.py:97-105).

`BakeStep` is that step with the replay rules of the other steps.  Its captured body:
    decode (`fr_bake_decode`: one launch, the rotation activation inside it) -> the frame's attribute selection
    (`BakedAvatar._frame`: looked-up where baked, the prior elsewhere, the looked-up opacity always) -> `render_bound_batch`
    -> L1 (+ the perceptual term's call) -> the rasterizer's backward -> the rot and scale-ratio terms on the decoded rows
    (`fr_rot_term`, `fr_scale_ratio_term`: the reference takes them whether or not the attribute is baked, so a non-baked
    scaling / rotation slice still gets the terms' gradient) -> decode backward (`fr_bake_decode_backward`: one walk per
    texel, every texel stored) -> Adam over the texture (feature-map mode).
The Gaussians, FLAME and the mesh have no trainable state in this stage, so there is no Gaussian Adam, no density control
and no mesh term: the reference's Laplacian term reaches no parameter here, and leaving it out changes no gradient.  Its
`reg_loss` (train/loss.py:654-675) is not built: the decoded arrays have P + 65 536 rows and the priors P, so its MSE cannot
broadcast — dead code behind a default weight of 0.  One view per step; FLAME is the caller's (the step takes posed vertices).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from .baked import ATTRIBUTES, BakedAvatar
from .binding import face_scale
from .bound import render_bound_batch
from .loss import (ScaleRatioTerm, l1_loss_and_grad, l1_workspace, rot_term_and_grad, rot_term_workspace, scale_ratio_term_and_grad,
                   scale_ratio_workspace)
from .model import TorchCamera
from .optim import FusedAdam
from .perceptual import Perceptual
from .texture import TEXTURE_CHANNELS, _check_decoder_output, decode_backward_into
from .train import TrainStep


class RotTerm(NamedTuple):
    """Neural baking's rotation term: its weight (train_neural_baking.py:34, --rot_weight)."""
    weight: float = 0.1


REFERENCE_ROT_TERM = RotTerm(0.1)
BAKE_LR = 1e-3                     # train/baker.py:97-105
N_CHANNELS = sum(c for _, c in TEXTURE_CHANNELS)
_VALUE_WIDTHS = {"color": 3, "opacity": 1, "scaling": 3, "rotation": 4, "offset": 1}


class BakeStep:
    """One neural-baking step per call (the module docstring has its body).

    `texture="feature_map"` (`FeatureMap`, model/unet/arch.py:70-80): the step OWNS the decoder's one parameter,
    `optim_texture` [1,11,H,W] (uniform(-1, 1) from `generator`), and a `FusedAdam` over it at `lr`:
    `step(camera, posed_verts, gt_image)`.
    `texture=None` (a caller's U-Net or decode_only decoder): `step(camera, posed_verts, gt_image, tex_out)` loads the
    caller's decoder output [1,11,H,W] (values only) into a static input and leaves `d_tex_out` [1,11,H,W] = THIS step's
    dLoss/d(tex_out) for `tex_out.backward(step.d_tex_out)` and the caller's own optimizer — one storage across the steps,
    every texel rewritten by every step, never accumulated; after a replay that overflowed its binning capacity it holds the
    decoded-row terms' gradient alone (the frame back-propagated zeros).
    After every step: `loss` (the L1 term), `rot_loss` [1] and `reg_loss` [2] (scale_loss, rows over the threshold) —
    UNWEIGHTED, None without their term —, `perceptual_loss` as in AvatarStep, `out` (render, radii, visibility_filter).  The
    reference's total is loss + rot_term.weight * rot_loss[0] + scale_term.weight * reg_loss[0] (+ the perceptual term).
    A frame that overflowed its binning capacity inside a captured replay makes Adam skip the step (the overflow word), as
    in every other step.  Data-parallel runs are not built."""

    # the replay rules are TrainStep's own functions: they read nothing of a Gaussian holder
    _kept = staticmethod(TrainStep._kept)
    _load_inputs = TrainStep._load_inputs
    _capture = TrainStep._capture
    _poll_overflow = TrainStep._poll_overflow
    _replay_or_run = TrainStep.step
    check = TrainStep.check
    exchange = exchange_in_graph = False
    world = 1

    def __init__(self, baked: BakedAvatar, faces: torch.Tensor, canonical_verts: torch.Tensor, camera: TorchCamera, bg: torch.Tensor,
                 *, bake_attribute=ATTRIBUTES, shell_len: float = 0.05, resize_scale: bool = True, texture: Optional[str] = None,
                 lr: float = BAKE_LR, rot_term: Optional[RotTerm] = REFERENCE_ROT_TERM, scale_term: Optional[ScaleRatioTerm] = None,
                 perceptual: Optional[Perceptual] = None, use_graph: bool = True, generator: Optional[torch.Generator] = None):
        if not isinstance(baked, BakedAvatar):
            raise TypeError("BakeStep: `baked` is a baked.BakedAvatar")
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError("BakeStep: data-parallel runs are not built (the texture's gradient has no all-reduce)")
        if texture not in (None, "feature_map"):
            raise ValueError(f"BakeStep: `texture` is None (the caller's decoder) or 'feature_map', not {texture!r}")
        if rot_term is not None and not isinstance(rot_term, RotTerm):
            raise TypeError(f"BakeStep: `rot_term` is a RotTerm or None, not {type(rot_term).__name__}")
        if scale_term is not None and not isinstance(scale_term, ScaleRatioTerm):
            raise TypeError(f"BakeStep: `scale_term` is a ScaleRatioTerm or None, not {type(scale_term).__name__}")
        self.baked, self.bg = baked, bg
        self.dev = dev = baked.plan.device
        if perceptual is not None:
            if not isinstance(perceptual, Perceptual):
                raise TypeError("BakeStep: `perceptual` must be a perceptual.Perceptual")
            if perceptual.features.device != dev:
                raise ValueError("BakeStep: the perceptual term and the avatar live on different devices")
        self.perceptual = perceptual
        self.bake_attribute = tuple(bake_attribute)
        unknown = [a for a in self.bake_attribute if a not in ATTRIBUTES]
        if unknown:
            raise RuntimeError(f"BakeStep: unknown attributes {unknown}; known: {ATTRIBUTES}")
        if baked.N != baked.P and any(a not in self.bake_attribute for a in ("color", "scaling", "rotation", "offset")):
            raise RuntimeError(f"BakeStep: the binding was extended to {baked.N} points but the priors have {baked.P} rows: bake "
                               "every attribute")
        self.rot_term = None if rot_term is None else RotTerm(float(rot_term.weight))
        self.scale_term = None if scale_term is None else ScaleRatioTerm(*[float(x) for x in scale_term])
        self.faces = faces.to(dev, torch.int32).contiguous()
        canon = canonical_verts.detach().to(dev, torch.float32).contiguous()
        # compute_face_orientation(canonical verts, return_scale=True)[1] (model/fateavatar.py:84-85)
        self.binding = baked.mesh_binding(self.faces, face_scale(canon, self.faces), float(shell_len), bool(resize_scale))
        baked.plan.csr()                                   # (sorts and synchronises: here, outside any capture)
        N, H, W = baked.N, baked.plan.H, baked.plan.W
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        # static inputs of the captured step
        self.cam, self.verts = camera, canon.clone()
        self.gt = z(3, camera.image_height, camera.image_width)
        self.feature_map = texture == "feature_map"
        if self.feature_map:
            cpu = torch.empty((1, N_CHANNELS, H, W), dtype=torch.float32).uniform_(-1, 1, generator=generator)
            self.optim_texture = self.tex_out = cpu.to(dev)
        else:
            self.optim_texture, self.tex_out = None, z(1, N_CHANNELS, H, W)
        # what the step writes
        self.d_tex_out = z(1, N_CHANNELS, H, W)
        self.values = {name: z(N, w) for name, w in _VALUE_WIDTHS.items()}       # the decoded rows
        self._d_zero = {"scaling": z(N, 3), "rotation": z(N, 4)}                 # the terms' target where the frame left no gradient
        self.loss, self._dimage, self._l1_ws = z(), torch.zeros_like(self.gt), l1_workspace(dev)
        self.rot_loss = None if self.rot_term is None else z(1)
        self._rot_ws = None if self.rot_term is None else rot_term_workspace(dev)
        self.reg_loss = None if self.scale_term is None else z(2)
        self._ratio_ws = None if self.scale_term is None else scale_ratio_workspace(dev)
        self.perceptual_loss = None if perceptual is None else z(1 + perceptual.n_terms)
        # the frame's side outputs: the overflow word Adam skips on (the statistics are nobody's: no density control here)
        self.xyz_gradient_accum, self.denom, self.overflow_word = z(N, 1), z(N, 1), z(1)
        self.adam = None
        if self.feature_map:
            self.adam = FusedAdam(self.optim_texture.view(-1), self.d_tex_out.view(-1), [(self.optim_texture.numel(), float(lr))])
            self.adam.set_skip_words([self.overflow_word])
        self.out = None
        self.use_graph = bool(use_graph)
        self._graph, self._eager_steps, self.overflows, self.host_steps = None, 0, 0, 0

    # ---- the step body
    def _forward_backward(self):
        from . import rasterizer
        baked, plan, tex = self.baked, self.baked.plan, self.tex_out
        vals = self.values
        _lib.launch("fr_bake_decode", self.dev, plan.N, plan.uv.data_ptr(), plan.H, plan.W, tex.data_ptr(), baked.mean_scaling,
                    baked.max_scaling, *[vals[name].data_ptr() for name, _ in TEXTURE_CHANNELS])
        # leaves over the decoded rows' storage (no copy): the frame's backward leaves their gradients
        leaves = {name: v.detach().requires_grad_(True) for name, v in vals.items()}
        frame = baked._frame(leaves, self.bake_attribute)
        frame.fused_densification_stats = (self.xyz_gradient_accum, self.denom, self.overflow_word)
        out = render_bound_batch([self.cam], [frame], [self.verts], self.binding, self.bg, slots=[rasterizer._slot])[0]
        _, g = l1_loss_and_grad(out["render"], self.gt, loss_out=self.loss, grad_out=self._dimage, workspace=self._l1_ws)
        if self.perceptual is not None:     # weight x the VGG term's gradient, ADDED to the L1 gradient in place
            self.perceptual.loss_and_grad(out["render"], self.gt, loss_out=self.perceptual_loss, grad_out=g, accumulate=True)
        out["render"].backward(g)
        d = {name: leaf.grad for name, leaf in leaves.items()}
        # train/loss.py:597-604, :612-617: weight x the terms' gradient ADDED to the image term's, on the decoded rows
        for name, term in (("rotation", self.rot_term), ("scaling", self.scale_term)):
            if term is not None and d[name] is None:           # (not baked: the frame read the prior)
                d[name] = self._d_zero[name].zero_()
        if self.rot_term is not None:
            rot_term_and_grad(vals["rotation"], d["rotation"], out=self.rot_loss, weight=self.rot_term.weight, workspace=self._rot_ws)
        if self.scale_term is not None:                        # 'scale' = exp(decode_scaling) (uv_decoder.py:515)
            scale_ratio_term_and_grad(vals["scaling"], d["scaling"], out=self.reg_loss, terms=self.scale_term, workspace=self._ratio_ws)
        decode_backward_into(plan, tex, baked.mean_scaling, baked.max_scaling, [d[name] for name, _ in TEXTURE_CHANNELS],
                             self.d_tex_out)
        self.out = self._kept(out)

    def _body(self):
        self._forward_backward()
        if self.adam is not None:
            self.adam.step()

    def step(self, camera: TorchCamera, posed_verts: torch.Tensor, gt_image: torch.Tensor,
             tex_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One step on one frame.  `tex_out` [1,11,H,W]: the caller's decoder output — required with `texture=None`, refused
        in feature-map mode.  Returns the (device) L1 loss scalar of the step."""
        if (tex_out is None) != self.feature_map:
            raise ValueError("BakeStep.step: `tex_out` goes with BakeStep(texture=None) (required with it, refused in feature-map mode)")
        extra = [(self.verts, posed_verts.detach())]
        if tex_out is not None:
            _check_decoder_output(tex_out, self.baked.plan, "BakeStep.step")
            extra.append((self.tex_out, tex_out.detach().reshape(self.tex_out.shape)))
        return self._replay_or_run(camera, gt_image, extra)

    @property
    def skipped_steps(self) -> int:
        """Feature-map mode: step() calls minus applied Adam updates (TrainStep.skipped_steps).  Synchronises."""
        if self.adam is None:
            raise RuntimeError("BakeStep(texture=None) has no optimizer: the decoder is the caller's")
        return self.host_steps - self.adam.step_count

    def texture_dict(self) -> dict:
        """The raw slices {name: [1,C,H,W]} of the step's present decoder output (views, detached): what `BakedAvatar.render`
        / `export` and the reference's `texture_dump` (train/baker.py:406-414) take; colour is NOT activated in it (the
        reference activates it outside, train/baker.py:630)."""
        out, off = {}, 0
        for name, c in TEXTURE_CHANNELS:
            out[name] = self.tex_out.detach()[:, off:off + c]
            off += c
        return out

    # ---- checkpoints: the reference's layout (Trainer.save_checkpoint: 'global_step' and 'model' = model.state_dict(), in which
    #      FeatureMap's parameter is 'decoder.optim_texture' [1,11,H,W]); 'optimizer' is an addition a seamless resume needs
    @torch.no_grad()
    def state_dict(self) -> dict:
        if self.adam is None:
            raise RuntimeError("BakeStep(texture=None) owns no parameter: the decoder and its checkpoint are the caller's")
        a = self.adam
        return {"global_step": a.step_count, "model": {"decoder.optim_texture": self.optim_texture.clone()},
                "optimizer": {"exp_avg": a.exp_avg.clone(), "exp_avg_sq": a.exp_avg_sq.clone(), "state": a.state_words()}}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> list:
        """Loads `decoder.optim_texture` IN PLACE (the captured step stays valid) and, if the checkpoint has one, the
        optimizer's state (else it goes on as it is); returns the keys of 'model' it ignored (a checkpoint of the reference
        also holds the avatar's)."""
        if self.adam is None:
            raise RuntimeError("BakeStep(texture=None) owns no parameter: the decoder and its checkpoint are the caller's")
        model = dict(sd["model"])
        if "decoder.optim_texture" not in model:
            raise KeyError("checkpoint lacks 'decoder.optim_texture'")
        t = model.pop("decoder.optim_texture")
        if tuple(t.shape) != tuple(self.optim_texture.shape):
            raise ValueError(f"checkpoint's texture is {tuple(t.shape)}, the step's {tuple(self.optim_texture.shape)}")
        self.optim_texture.copy_(t.to(self.dev, torch.float32))
        opt = sd.get("optimizer")
        if opt is not None:
            self.adam.exp_avg.copy_(opt["exp_avg"])
            self.adam.exp_avg_sq.copy_(opt["exp_avg_sq"])
            self.adam.load_state_words(opt["state"])
        self.host_steps = self.adam.step_count
        return sorted(model.keys())
