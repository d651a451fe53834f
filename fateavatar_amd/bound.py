"""Frames rendered STRAIGHT FROM THEIR MESH BINDING: `bind_gaussians` + `render` as one differentiable op per batch of
views, with the binding evaluated inside the rasterizer's per-Gaussian kernels (include/fr_rasterizer.h, fr_aux::binding).

reference: model/fateavatar.py:225-276 — per frame the Gaussians are bound to the posed mesh (about forty PyTorch
kernels and their autograd twins, :225-258), assigned to gaussian._xyz / _rotation / _scaling, and rendered
(volume_rendering/render_3dgs.py:7-81).  `binding.bind_gaussians` makes the binding one kernel per direction;
here it is no kernel at all: the preprocess kernel computes a Gaussian's bound position / rotation / log-scale in front of
its own work (and stores them for the backward), and the per-Gaussian backward kernel carries its gradients on through
the binding to offset / rotation / scaling (and the posed vertices).  Same expressions from one header
(csrc/fr_bind_math.hpp), so the results are those of `bind_gaussians` followed by `render_batch`, bit for bit in the
forward and to atomic-summation order in the backward.

The same holds for GaussianAvatars' face-local binding (model/baseline/gaussianavatars.py:144-171,
`binding.bind_gaussians_face_local`): hand `render_bound_batch` a `FaceLocalBinding` instead of a `MeshBinding`.

And for SplattingAvatar's Phong-surface binding (model/baseline/splattingavatar.py:203-246, `binding.bind_gaussians_phong`):
hand it a `PhongBinding`.  That mode's per-frame mesh pass (`binding.phong_frame`, one launch per view) runs in front of
the launch chain; the per-Gaussian part is folded like the other two.

And for FlashAvatar's MLP-deformed binding (model/baseline/flashavatar.py:242-276, `binding.bind_gaussians_deform`): hand it a
`DeformBinding`; the holders carry the MLP's outputs for their view as `_deform` [N,10].
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from .binding import (DEFORM, FACE_LOCAL, PHONG, SHELL, PhongCanonical, PhongGradBuffers, _check_shapes, _chk, _chk_phong_frame,
                      _describe, _grad_buffer, _no_vertex_gradient, phong_frame, phong_frame_backward, phong_scatter_frame_grads)
from .rasterizer import (_GRAD_NAMES, _any_grad, _backward_args, _camera_grads, _camera_inputs_of, _forward_args, _forward_batch,
                         _FrameGrads, _per_view_outputs, _pick_forward_only, _SavedFrame, rasterize_gaussians_backward_batch)
from .render import _result, _screenspace_points, _settings


# Every binding class names its mode's record (`mode`, binding.BindMode) and has two methods: `describe_args()`, what
# `binding._describe` takes behind the per-Gaussian parameters (nothing it does not read), and `per_view(posed_verts)`,
# render_bound_batch's preparation: (the checked binding of every view, the vertices the views are rendered from).
class MeshBinding(NamedTuple):
    """What does not change from frame to frame: model/fateavatar.py:120-164 (face_index, bary_coords), :84-85
    (face_scale_canonical), the mesh topology and the two configuration values of :256-258."""
    faces: torch.Tensor                   # [F,3] int32
    face_index: torch.Tensor              # [N]   int32
    bary_coords: torch.Tensor             # [N,3]
    face_scale_canonical: Optional[torch.Tensor]   # [F,1] (`binding.face_scale` of the canonical mesh), None without resize_scale
    shell_len: float
    resize_scale: bool = True

    mode = SHELL

    def describe_args(self):
        return self.bary_coords, self.face_scale_canonical, self.shell_len, self.resize_scale

    def per_view(self, posed_verts):
        mb = MeshBinding(_chk(self.faces, torch.int32, "faces"), _chk(self.face_index, torch.int32, "face_index"),
                         _chk(self.bary_coords, torch.float32, "bary_coords"),
                         _chk(self.face_scale_canonical, torch.float32, "face_scale_canonical")
                         if self.face_scale_canonical is not None else None, float(self.shell_len), bool(self.resize_scale))
        return [mb] * len(posed_verts), posed_verts


class FaceLocalBinding(NamedTuple):
    """GaussianAvatars' binding (model/baseline/gaussianavatars.py:52-60,144-171): the mesh topology and the face of every
    Gaussian.  The per-Gaussian position in that face's frame is a parameter (the holder's `_xyz`), not part of this."""
    faces: torch.Tensor                   # [F,3] int32
    face_index: torch.Tensor              # [N]   int32 (the reference's `binding`)

    mode = FACE_LOCAL

    def describe_args(self):
        return ()

    def per_view(self, posed_verts):
        mb = FaceLocalBinding(_chk(self.faces, torch.int32, "faces"), _chk(self.face_index, torch.int32, "face_index"))
        return [mb] * len(posed_verts), posed_verts


class _PhongView(NamedTuple):
    """A PhongBinding of ONE view: with the outputs of that view's mesh pass in the canonical data's place."""
    faces: torch.Tensor
    face_index: torch.Tensor
    bary_coords: torch.Tensor
    frame: tuple                          # (vert_normals [V,3], vert_quats [V,4], face_ratio [F])

    mode = PHONG

    def describe_args(self):
        return self.bary_coords, None, 0.0, False, self.frame


class PhongBinding(NamedTuple):
    """SplattingAvatar's binding (model/baseline/splattingavatar.py:128-145, :224-246): the mesh topology, every Gaussian's
    face and barycentrics, and the once-per-mesh data of `binding.phong_canonical`.  The per-Gaussian `_uvd` is a parameter of
    the holder, not part of this."""
    faces: torch.Tensor                   # [F,3] int32
    face_index: torch.Tensor              # [N]   int32 (the reference's `sample_fidxs`)
    bary_coords: torch.Tensor             # [N,3]       (`sample_bary`)
    canonical: PhongCanonical

    mode = PHONG

    def per_view(self, posed_verts):
        """One `binding.phong_frame` per distinct posed mesh, in front of the frame's launch chain; the vertices detached."""
        faces, fidx = _chk(self.faces, torch.int32, "faces"), _chk(self.face_index, torch.int32, "face_index")
        bary = _chk(self.bary_coords, torch.float32, "bary_coords")
        V, frames, mbs = self.canonical.cano_verts.shape[0], {}, []
        for verts in posed_verts:
            _no_vertex_gradient(verts, "render_bound_batch")
            if id(verts) not in frames:   # (views of one pose share its mesh pass)
                frames[id(verts)] = _chk_phong_frame(phong_frame(self.canonical, verts), V, faces.shape[0], "render_bound_batch")
            mbs.append(_PhongView(faces, fidx, bary, frames[id(verts)]))
        return mbs, [v.detach() for v in posed_verts]


class _PosedPhongView(NamedTuple):
    """A PosedPhongBinding of ONE view: `_PhongView` and what the vertex gradient needs — the canonical data, which of the
    batch's distinct posed meshes the view is rendered from, and that mesh's preallocated buffers (or None)."""
    faces: torch.Tensor
    face_index: torch.Tensor
    bary_coords: torch.Tensor
    frame: tuple
    canonical: PhongCanonical
    group: int
    buffers: Optional[PhongGradBuffers]

    mode = PHONG
    # what the frame's backward stores on top of the parameters' gradients: the gradients of the bound values
    bound_grads = ("dL_dmeans3D", "dL_drotations", "dL_dscales")

    def describe_args(self):
        return self.bary_coords, None, 0.0, False, self.frame


class PosedPhongBinding(NamedTuple):
    """`PhongBinding` whose posed vertices take a gradient: `render_bound_batch` returns dLoss/dposed_verts per view for it
    (the reference's autograd through splattingavatar.py:203-246).  The frame is `PhongBinding`'s, bit for bit — image, bound
    values and every parameter gradient; its backward also stores the gradients of the bound values, and behind the frame's
    launch chain `fr_bind_backward_phong_frame` scatters them per view and `fr_phong_frame_backward` runs once per distinct
    posed mesh: views that share a mesh (the same tensor object) share one mesh pass forward, and their gradients are summed
    into that mesh's one d_verts.  A mesh tensor may carry `_fr_phong_grad`, a `binding.PhongGradBuffers`: its gradient is then
    formed in those preallocated buffers (zeroed by the backward itself)."""
    faces: torch.Tensor                   # [F,3] int32
    face_index: torch.Tensor              # [N]   int32
    bary_coords: torch.Tensor             # [N,3]
    canonical: PhongCanonical

    mode = PHONG

    def per_view(self, posed_verts):
        faces, fidx = _chk(self.faces, torch.int32, "faces"), _chk(self.face_index, torch.int32, "face_index")
        bary = _chk(self.bary_coords, torch.float32, "bary_coords")
        V, frames, mbs = self.canonical.cano_verts.shape[0], {}, []
        for verts in posed_verts:
            if id(verts) not in frames:   # (views of one pose share its mesh pass, forward and backward)
                frame = _chk_phong_frame(phong_frame(self.canonical, verts), V, faces.shape[0], "render_bound_batch")
                frames[id(verts)] = (frame, len(frames))
            frame, group = frames[id(verts)]
            mbs.append(_PosedPhongView(faces, fidx, bary, frame, self.canonical, group, getattr(verts, "_fr_phong_grad", None)))
        return mbs, list(posed_verts)


class DeformBinding(NamedTuple):
    """FlashAvatar's binding (model/baseline/flashavatar.py:159-164, :262-274): the mesh topology and every Gaussian's face and
    barycentrics.  The ten outputs of the deformation MLP are per frame: the holder's `_deform` [N,10], not part of this."""
    faces: torch.Tensor                   # [F,3] int32
    face_index: torch.Tensor              # [N]   int32
    bary_coords: torch.Tensor             # [N,3]

    mode = DEFORM

    def describe_args(self):
        return (self.bary_coords,)

    def per_view(self, posed_verts):
        mb = DeformBinding(_chk(self.faces, torch.int32, "faces"), _chk(self.face_index, torch.int32, "face_index"),
                           _chk(self.bary_coords, torch.float32, "bary_coords"))
        return [mb] * len(posed_verts), posed_verts


class _RasterizeBoundBatch(torch.autograd.Function):
    """Tensor arguments per view: (verts, own, rotation, scaling, means2D, sh, opacities) — the RAW parameters, as render()
    hands them over with `fused_activations`; `own` is the binding's own per-Gaussian parameter (offset [N,1], the local
    position [N,3], uvd [N,3], the MLP's outputs [N,10]: `BindMode.attr` of the holder); then — optionally — per view its settings'
    (viewmatrix, projmatrix, campos), which then receive gradients (`rasterizer._camera_inputs`).  Outputs per view: those of
    `_SavedFrame`."""
    PER_VIEW = 7

    @staticmethod
    def forward(ctx, settings, bindings, slots, forward_only, depth_alpha, *tensors):
        K, n = len(settings), _RasterizeBoundBatch.PER_VIEW
        assert len(tensors) in (n * K, (n + 3) * K) and len(bindings) == K
        ctx.bindings, ctx.slots, ctx.own_shapes, ctx.camera = bindings, slots, [], len(tensors) == (n + 3) * K
        empty = torch.Tensor([])
        views, viss, descs, bound, checked = [], [], [], [], []
        for k, (rs, mb) in enumerate(zip(settings, bindings)):
            verts, own, rotation, scaling, means2D, sh, opacities = tensors[n * k:n * k + n]
            ctx.own_shapes.append(tuple(own.shape))
            verts, own = _chk(verts, torch.float32, "verts"), _chk(own, torch.float32, mb.mode.own)
            rotation, scaling = _chk(rotation, torch.float32, "rotation"), _chk(scaling, torch.float32, "scaling")
            checked.append((verts, own, rotation, scaling))   # (what the descriptor points at: alive until the launch, saved for the backward)
            N, dev = mb.face_index.shape[0], verts.device
            args = (mb.mode, verts, mb.faces, mb.face_index, own, rotation, scaling, *mb.describe_args())
            _check_shapes("render_bound_batch", mb.mode.frame_shapes, *args)
            descs.append(_describe(*args))
            # the bound values: written by the preprocess kernel, read again by the backward
            xyz = torch.empty((N, 3), dtype=torch.float32, device=dev)
            rot = torch.empty((N, 4), dtype=torch.float32, device=dev)
            scl = torch.empty((N, 3), dtype=torch.float32, device=dev)
            bound.append((xyz, rot, scl))
            views.append(_forward_args(rs, xyz, means2D, sh, empty, opacities, scl, rot, empty))
            viss.append(torch.empty((N,), dtype=torch.bool, device=dev))
        res = _forward_batch(views, slots, True, viss, descs, forward_only, depth_alpha)
        frames = []
        for k, rs in enumerate(settings):
            verts, own, rotation, scaling, means2D, sh, opacities = tensors[n * k:n * k + n]
            grads = _FrameGrads({"dL_dsh": sh if sh.numel() else None, "dL_dopacity": opacities, "d_own": own,
                                 "d_rotation": rotation, "d_scaling": scaling}, sh, bound=True)
            frames.append(_SavedFrame(rs, res[k], viss[k], means2D, grads, (*checked[k], sh, *bound[k])))
            res[k].radii._fr_bound = bound[k]           # (xyz, rotation, scaling) as bind_gaussians returns them
        return _SavedFrame.save(ctx, frames)

    @staticmethod
    def backward(ctx, *grad_outs):
        K, n = len(ctx.frames), _RasterizeBoundBatch.PER_VIEW
        if not _any_grad(grad_outs):
            return (None,) * (5 + (n + 3 if ctx.camera else n) * K)
        empty = torch.Tensor([])
        views, outs, descs, bgrads, planes, wants, posed = [], [], [], [], [], [], {}
        for k, (f, saved, fw, g, pl) in enumerate(_SavedFrame.load(ctx, grad_outs)):
            (verts, own, rotation, scaling, sh, xyz, rot, scl), mb = saved, ctx.bindings[k]
            dev, N = verts.device, xyz.shape[0]
            views.append(_backward_args(f.rs, (empty, xyz, scl, rot, empty, sh), fw, g))
            planes.append(pl)
            claimed = f.grads.claim(accumulate=False)[0]
            outs.append({m: b for m, b in claimed.items() if m.startswith("dL_")})
            need_v, need_o, need_r, need_s = ctx.needs_input_grad[5 + n * k:5 + n * k + 4]   # (after the 5 non-tensor arguments)
            want = f.grads.want
            if need_v and isinstance(mb, _PosedPhongView):
                # (the kernel is handed no d_verts in this mode: it stores the bound values' gradients, and the two calls
                # of the Phong vertex gradient follow the launch chain below)
                posed[k], need_v, want = (verts, own, rotation, scaling), False, want | set(mb.bound_grads)
            wants.append(want)
            descs.append(_describe(mb.mode, verts, mb.faces, mb.face_index, own, rotation, scaling, *mb.describe_args()))
            # (the own parameter's gradient goes to the kernel under the name its mode has in fr_aux)
            bgrads.append({"d_verts": torch.zeros_like(verts) if need_v else None,
                           mb.mode.grad: _grad_buffer(need_o, claimed.get("d_own"), mb.mode.grad_shape(N), dev),
                           "d_rotation": _grad_buffer(need_r, claimed.get("d_rotation"), (N, 4), dev),
                           "d_scaling": _grad_buffer(need_s, claimed.get("d_scaling"), (N, 3), dev)})
        res = rasterize_gaussians_backward_batch(views, slots=ctx.slots, raw=True, wants=wants,
                                                 outs=outs, stats=[f.stats for f in ctx.frames], bindings=descs, bind_grads=bgrads,
                                                 planes=planes if ctx.frames[0].has_planes else None, camera=ctx.camera)
        if posed:
            _phong_vertex_grads(ctx.bindings, posed, res, bgrads)
        flat = [None, None, None, None, None]
        for grads, b, mb, own_shape in zip(res, bgrads, ctx.bindings, ctx.own_shapes):
            g = dict(zip(_GRAD_NAMES, grads))   # (the eight per-Gaussian arrays; camera gradients, if any, come behind them)
            d_own = b[mb.mode.grad]
            d_own = d_own.view(own_shape) if d_own is not None else None
            # (fresh view objects: AccumulateGrad adopts a gradient without a copy only if nobody else references it)
            fresh = lambda t: t.view(t.shape) if t is not None else None  # noqa: E731
            flat += [b["d_verts"], d_own, fresh(b["d_rotation"]), fresh(b["d_scaling"]), g["dL_dmeans2D"], g["dL_dsh"], g["dL_dopacity"]]
        if ctx.camera:
            flat += [t for f, grads in zip(ctx.frames, res) for t in _camera_grads(f.rs, grads)]
        return tuple(flat)


def _phong_vertex_grads(bindings, posed, res, bgrads):
    """dLoss/dposed_verts of the views `posed` (view -> its checked verts, uvd, rotation, scaling) of a PosedPhongBinding, from
    the gradients of the bound values their frame's backward stored in `res`: one scatter launch per view into its mesh's four
    arrays, then the mesh pass's backward once per distinct mesh.  The mesh's d_verts becomes the gradient of the FIRST view
    rendered from it (`bgrads[k]["d_verts"]`); autograd adds nothing for the others."""
    meshes = {}
    for k, (verts, own, rotation, scaling) in posed.items():
        mb = bindings[k]
        if mb.group not in meshes:
            buf = mb.buffers
            if buf is None:
                buf = PhongGradBuffers(verts.shape[0], mb.faces.shape[0], verts.device, zeroed=True)
            else:
                buf.check(verts.shape[0], mb.faces.shape[0], verts.device)
                buf.zero_()
            meshes[mb.group] = (buf, verts, mb.canonical)
            bgrads[k]["d_verts"] = buf.d_verts
        buf = meshes[mb.group][0]
        g = dict(zip(_GRAD_NAMES, res[k]))
        phong_scatter_frame_grads(verts, mb.faces, mb.face_index, mb.bary_coords, mb.frame, own, rotation, scaling,
                                  g["dL_dmeans3D"], g["dL_drotations"], g["dL_dscales"], buf.d_verts, buf.d_vert_normals,
                                  buf.d_vert_quats, buf.d_face_ratio)
    for buf, verts, canonical in meshes.values():
        phong_frame_backward(canonical, verts, buf.d_vert_normals, buf.d_vert_quats, buf.d_face_ratio, buf.d_verts, buf.workspace)


def render_bound_batch(viewpoint_cameras, pcs, posed_verts, binding, bg_colors, scaling_modifier=1.0, slots=None,
                       depth_alpha=False):
    """`bind_gaussians` + `render_batch` for K views in one launch chain without binding kernels.

    `pcs`: per view (or one for all) a holder with the raw parameters `_opacity` [N,1], `_offset` [N,1], `_rotation` [N,4],
    `_scaling` [N,3], the features `get_features` [N,M,3], `max_sh_degree` — and optionally `fused_densification_stats`;
    `posed_verts`: per view the posed mesh [V,3].  Returns the list of render() dicts; `out["bound"]` holds the
    (xyz, rotation, scaling) the reference assigns to the Gaussians before render() (model/fateavatar.py:256-258) as plain
    kernel OUTPUTS, DETACHED from autograd: gradients reach offset / rotation / scaling / verts through the image only.  A
    regulariser on the bound values themselves needs the differentiable stand-alone op (`binding.bind_gaussians`, what
    `AvatarStep(fold_binding=False)` renders through).  `depth_alpha=True` (extension): "depth" and "alpha" as in render().

    `binding`: a `MeshBinding`, a `PhongBinding` (SplattingAvatar, model/baseline/splattingavatar.py:203-246; stand-alone op
    `binding.bind_gaussians_phong`; the holders carry `_uvd` [N,3] where FateAvatar's carry `_offset`, the posed vertices get no
    gradient, and every view's mesh pass `binding.phong_frame` is launched here, in front of the frame's launch chain), a
    `PosedPhongBinding` (the same frame, and dLoss/dposed_verts behind it: the class's docstring), or a
    `FaceLocalBinding` (GaussianAvatars, model/baseline/gaussianavatars.py:144-171;
    stand-alone op `binding.bind_gaussians_face_local`).  The holders then carry the local position `_xyz` [N,3] where
    FateAvatar's carry `_offset`, and the frame is rendered with their `active_sh_degree` (the reference hands render() a
    GaussianModel(sh_degree=active_sh_degree), :157) from `get_features` [N,M,3], M >= (active_sh_degree + 1)^2.
    Or a `DeformBinding` (FlashAvatar, model/baseline/flashavatar.py:242-276; stand-alone op `binding.bind_gaussians_deform`): the
    holders carry `_deform` [N,10], the RAW outputs of the caller's deformation MLP for THEIR view (every view has its own
    expression, so one holder per view), which takes a gradient like a parameter; the posed vertices get one too."""
    K = len(viewpoint_cameras)
    if not 1 <= K <= _lib.FR_MAX_BATCH:
        raise RuntimeError(f"render_bound_batch: 1 .. {_lib.FR_MAX_BATCH} views")
    if not isinstance(pcs, (list, tuple)):
        pcs = [pcs] * K
    mode = binding.mode
    for pc in pcs:
        if getattr(pc, mode.attr, None) is None:
            raise RuntimeError(f"render_bound_batch: {mode.holder}; {type(pc).__name__} has none")
    if isinstance(bg_colors, torch.Tensor):
        bg_colors = [bg_colors] * K
    if isinstance(posed_verts, torch.Tensor):
        posed_verts = [posed_verts] * K
    mbs, posed_verts = binding.per_view(posed_verts)
    settings, tensors, points = [], [], []
    for cam, pc, bg, verts in zip(viewpoint_cameras, pcs, bg_colors, posed_verts):
        sp = _screenspace_points(pc._scaling, pc)
        rs = _settings(cam, pc, bg, scaling_modifier)
        if mode.active_sh:
            rs = rs._replace(sh_degree=int(getattr(pc, "active_sh_degree", pc.max_sh_degree)))
        settings.append(rs)
        tensors += [verts, getattr(pc, mode.attr), pc._rotation, pc._scaling, sp, pc.get_features, pc._opacity]
        points.append(sp)
    tensors += _camera_inputs_of(settings)
    res = _RasterizeBoundBatch.apply(settings, mbs, list(range(K)) if slots is None else list(slots),
                                     _pick_forward_only(tensors), bool(depth_alpha), *tensors)
    out = []
    for r, sp in zip(_per_view_outputs(res, K), points):
        o = _result(r, sp)
        o["bound"] = tuple(t.detach() for t in o["radii"]._fr_bound)
        out.append(o)
    return out
