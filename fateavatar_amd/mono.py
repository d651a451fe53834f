"""MonoGaussianAvatar — the reference's point-based baseline — on the fused path: a cloud of free points, each with its own
learned expression basis, pose-corrective basis and skinning weights, moved by FLAME's linear blend skinning and splatted with
colours the networks predict.  It is not a mesh binding (there are no faces), so it has no `fr_binding` mode: three calls of
their own, `fateavatar_amd/csrc/fr_point_lbs.hip`.

reference (model/baseline/monogaussianavatar.py, flame/FLAME.py, flame/lbs.py, train/loss.py):
  * the deformation — `FLAME.forward_pts` (flame/FLAME.py:207-237) over flame/lbs.py:103-188, called per point under
    vmap(jacfwd(...)) (:345-359) with the expression vector, the pose feature and the [J,4,4] transforms expanded to one copy per
    point (:180-186) and a batched torch.inverse (flame/lbs.py:174): `deform_points`, one launch per direction, and with
    `frame_grad=True` one more that sums the gradients to the FRAME's pose state over the points
    (`fr_point_lbs_backward_pose`): what the reference's tracking optimisation of `expression` and `flame_pose`
    (train/base.py:113-156, :198-228) receives through the caller's FLAME
  * the nearest FLAME vertex of every canonical point — pytorch3d's knn_points(p, verts, K=1) (train/loss.py:231-233):
    `nearest_vertex`
  * the three blendshape terms — get_gt_blendshape / get_lbs_loss (train/loss.py:418-445, :472-515), three [N, .] gathers and
    three MSELoss graphs: `lbs_terms_and_grad`, one launch that also adds the weighted gradients onto the backward's
  * the attribute arithmetic between the two MLPs (:196-206) and `scales + radius` (:417): `splat_attributes`, plain torch
  * the frame (:380-428): `render_points`, the rasterizer with `colors_precomp`
  * the point cloud and its schedule (PointCloud :524-565, `_register_points` :132-148, `_upsample_points` :430-467): `MonoPoints`
The MLPs (geometry, deformer, rendering and Gaussian networks) and FLAME stay the caller's stock PyTorch, as in flash.py.

NOT here: the canonical pose state's gradient (a constant buffer in the reference), camera-pose gradients, the VGG
term, a captured whole step, data-parallel runs.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import _lib
from .binding import _grad_buffer
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, GradOut
from .workspace import StreamWorkspace

POSE_FEATURES = _lib.FR_LBS_POSE_FEATURES


class PoseState(NamedTuple):
    """One pose of FLAME as `deform_points` reads it: the expression coefficients, the pose-corrective feature
    (the flattened rotation matrices of the four non-root joints minus the identity) and the bone transforms.  PRECONDITION:
    every bone matrix has the last row (0, 0, 0, 1); with a ghost bone the caller puts the identity in front (:174-176)."""
    betas: torch.Tensor           # [E]
    pose_feature: torch.Tensor    # [36]
    transforms: torch.Tensor      # [J,4,4] (or [J,16], row-major)


def _f32(t, name, who):
    """Type and dtype first, shapes next, the device last: the errors a caller can make without a device read the same there."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{who}: {name} must be a tensor")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{who}: {name} must be float32, not {t.dtype}")
    return t.contiguous()


def _one_device(who, *tensors):
    dev = tensors[0].device
    if not all(t.is_cuda and t.device == dev for t in tensors):
        raise RuntimeError(f"{who}: all tensors must be on one HIP device (there is no CPU path)")
    return dev


def _no_pose_gradient(state, which):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in state):
        why = "it is a constant buffer in the reference" if which == "canonical" else \
            "the frame's state gets one only from deform_points(..., frame_grad=True)"
        raise RuntimeError(f"deform_points: the {which} pose state requires grad, and the pose states get no gradient here ({why}); "
                           "hand it detached tensors")


_pose_ws = StreamWorkspace("pose_workspace", lambda: _lib.lib().fr_point_lbs_pose_workspace_bytes(), "points'",
                           first="first call with frame_grad=True")
_terms_ws = StreamWorkspace("lbs_terms_workspace", lambda: _lib.lib().fr_lbs_terms_workspace_bytes(), "predictions'")


def pose_workspace(dev) -> torch.Tensor:
    """A fresh zeroed workspace for `deform_points(..., frame_grad=True, workspace=)`."""
    return _pose_ws.fresh(dev)


def _pose(state, E, J, which):
    b, f, A = (_f32(t.detach(), f"{which}.{n}", "deform_points") for t, n in zip(state, PoseState._fields))
    if b.shape != (E,) or f.shape != (POSE_FEATURES,) or A.numel() != J * 16 or A.shape[0] != J:
        raise RuntimeError(f"deform_points: the {which} pose state is betas [{E}], pose_feature [{POSE_FEATURES}], transforms "
                           f"[{J},4,4]")
    return b, f, A


def _describe(points, S, P, w, canonical, frame):
    d = _lib.fr_point_lbs()
    d.N, d.E, d.J = points.shape[0], S.shape[2], w.shape[1]
    d.points, d.shapedirs, d.posedirs, d.weights = points.data_ptr(), S.data_ptr(), P.data_ptr(), w.data_ptr()
    for dst, src in ((d.canonical, canonical), (d.frame, frame)):
        dst.betas, dst.pose_feature, dst.transforms = (t.data_ptr() for t in src)
    return d


class _Deform(torch.autograd.Function):
    """fr_point_lbs_forward / fr_point_lbs_backward, and fr_point_lbs_backward_pose where the frame's state asks for it."""

    @staticmethod
    def forward(ctx, workspace, points, shapedirs, posedirs, weights, *pose):
        who = "deform_points"
        points, S, P, w = (_f32(t, n, who) for t, n in zip((points, shapedirs, posedirs, weights),
                                                            ("points", "shapedirs", "posedirs", "lbs_weights")))
        N = points.shape[0]
        if points.dim() != 2 or points.shape[1] != 3 or S.dim() != 3 or S.shape[:2] != (N, 3) or P.shape != (N, POSE_FEATURES, 3) \
                or w.dim() != 2 or w.shape[0] != N:
            raise RuntimeError(f"{who}: points [N,3], shapedirs [N,3,E], posedirs [N,{POSE_FEATURES},3], lbs_weights [N,J]")
        E, J = int(S.shape[2]), int(w.shape[1])
        if not (1 <= E <= _lib.FR_LBS_MAX_E and 1 <= J <= _lib.FR_LBS_MAX_J):
            raise RuntimeError(f"{who}: E in 1 .. {_lib.FR_LBS_MAX_E} and J in 1 .. {_lib.FR_LBS_MAX_J}, not E = {E}, J = {J}")
        canonical, frame = _pose(pose[:3], E, J, "canonical"), _pose(pose[3:], E, J, "frame")
        dev = _one_device(who, points, S, P, w, *canonical, *frame)
        # (the workspace is settled here, where the caller called, not on the backward's thread)
        ctx.workspace = _pose_ws.resolve(dev, workspace, "deform_points") if any(ctx.needs_input_grad[8:11]) else None
        ctx.frame_shapes = tuple(tuple(t.shape) for t in pose[3:])
        xyz = torch.empty((N, 3), dtype=torch.float32, device=dev)
        d = _describe(points, S, P, w, canonical, frame)
        _lib.launch("fr_point_lbs_forward", dev, C.byref(d), xyz.data_ptr())
        ctx.save_for_backward(points, S, P, w, *canonical, *frame)
        ctx.grad_slots = tuple(GradOut.of(t) for t in (points, shapedirs, posedirs, weights))
        return xyz

    @staticmethod
    def backward(ctx, g_xyz):
        points, S, P, w, *pose = ctx.saved_tensors
        dev = points.device
        g_xyz = g_xyz.contiguous().float()
        outs = []
        for need, slot, like in zip(ctx.needs_input_grad[1:5], ctx.grad_slots, (points, S, P, w)):
            claimed = slot.claim()[0] if need and slot is not None else None
            outs.append(_grad_buffer(need, claimed, tuple(like.shape), dev))
        p = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        d = _describe(points, S, P, w, pose[:3], pose[3:])
        _lib.launch("fr_point_lbs_backward", dev, C.byref(d), g_xyz.data_ptr() if g_xyz.numel() else None, *[p(t) for t in outs])
        frame = [None, None, None]
        if ctx.workspace is not None:
            make = torch.empty if points.shape[0] else torch.zeros      # (N == 0 launches nothing: sums over no points)
            frame = [make(shape, dtype=torch.float32, device=dev) if need else None
                     for need, shape in zip(ctx.needs_input_grad[8:11], ctx.frame_shapes)]
            _lib.launch("fr_point_lbs_backward_pose", dev, C.byref(d), g_xyz.data_ptr() if g_xyz.numel() else None,
                        *[t.data_ptr() if t is not None else None for t in frame], ctx.workspace.data_ptr())
        return (None, *outs, None, None, None, *frame)


def deform_points(points, shapedirs, posedirs, lbs_weights, canonical: PoseState, frame: PoseState, *, frame_grad: bool = False,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`FLAME.forward_pts` (flame/FLAME.py:207-237) for N points in one launch: points [N,3] (canonical), shapedirs [N,3,E],
    posedirs [N,36,3], lbs_weights [N,J] (the deformer's outputs for the points), and the canonical and the frame's `PoseState`.
    Per point, with h = (p, 1):
        T_c = sum_j w_j A^c_j,  z = T_c^-1 h,  x = z[:3] - S beta_c - P^T phi_c + S beta + P^T phi,  xyz = (sum_j w_j A_j (x, 1))[:3]
    Returns xyz [N,3].  Differentiable w.r.t. the first four arguments (`GradOut` slots on them are honoured); a pose state that
    requires grad is refused, unless `frame_grad=True`: then the FRAME's betas, pose_feature and transforms may require grad, and
    the backward makes one more launch (only if one of them does) that sums, with g = dL/dxyz, T = sum_j w_j A_j, d_x = T[:3,:3]^T g,
        d_betas[l] = sum_n sum_k S_n[k,l] d_x_n[k],  d_pose_feature[i] = sum_n sum_k P_n[i,k] d_x_n[k],
        d_transforms[j,r,c] = sum_n w_nj g_n[r] (x_n, 1)[c]   (rows 0 .. 2; the bones' constant last rows get 0)
    in the inputs' shapes (N == 0: zeros): what a trainer's `expression` / `flame_pose` receive through its own FLAME.  The four
    per-point gradients keep their bits either way.  The canonical state is refused in both modes (a constant buffer in the
    reference).  `workspace`: that launch's scratch from `pose_workspace()`; by default one is kept per (device, current
    stream) — launches that may overlap must not share one.  The weights are taken as given (they need not sum to 1).  There is
    no CPU path."""
    for state in (canonical, frame):
        if not isinstance(state, (tuple, list)) or len(state) != 3:
            raise RuntimeError("deform_points: a pose state is (betas, pose_feature, transforms)")
    _no_pose_gradient(canonical, "canonical")
    if not frame_grad:
        _no_pose_gradient(frame, "frame")
    if workspace is not None and not isinstance(workspace, torch.Tensor):
        raise RuntimeError("deform_points: workspace must come from pose_workspace() on the points' device")
    return _Deform.apply(workspace, points, shapedirs, posedirs, lbs_weights, *canonical, *frame)


def nearest_vertex(points: torch.Tensor, verts: torch.Tensor):
    """pytorch3d's `knn_points(points, verts, K=1)` (train/loss.py:231-233): (index int32 [N], dist2 float32 [N]) of the vertex
    nearest to every point, brute force against at most 8192 vertices (FLAME has 5023).  The squared distance is
    (dx*dx + dy*dy) + dz*dz in float32; ties go to the lowest index.  Not differentiable."""
    points, verts = _f32(points.detach(), "points", "nearest_vertex"), _f32(verts.detach(), "verts", "nearest_vertex")
    if points.dim() != 2 or points.shape[1] != 3 or verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError("nearest_vertex: points [N,3], verts [V,3]")
    N, V = int(points.shape[0]), int(verts.shape[0])
    if not 1 <= V <= _lib.FR_NEAREST_MAX_V:
        raise ValueError(f"nearest_vertex: V in 1 .. {_lib.FR_NEAREST_MAX_V}, not {V}")
    _one_device("nearest_vertex", points, verts)
    index = torch.empty((N,), dtype=torch.int32, device=points.device)
    dist2 = torch.empty((N,), dtype=torch.float32, device=points.device)
    if N:
        _lib.launch("fr_nearest_vertex", points.device, N, points.data_ptr(), V, verts.data_ptr(), index.data_ptr(), dist2.data_ptr())
    return index, dist2


class LbsWeights(NamedTuple):
    """Coefficients of the three blendshape terms in the total loss: (lbs weights, posedirs, shapedirs)."""
    weights: float
    posedirs: float
    shapedirs: float


def reference_lbs_weights(lbs_weight: float = 10.0, var_expression=None) -> LbsWeights:
    """The coefficients MonoGaussianAvatarLoss puts on the three PLAIN mean squared errors, w = `lbs_weight`
    (config/monogaussianavatar.yaml:20; halved at the GT_lbs_milestones, train/loss.py:449-450):
      * lbs weights (train/loss.py:484-489):  loss += MSE(pred, gt) * w * 0.1                              -> 0.1 w
      * posedirs (:492-498):  loss += MSE(10 pred, 10 gt) * w * 10 = 100 MSE(pred, gt) * 10 w             -> 1000 w
      * shapedirs (:501-514, :441-444):  the MSE is a SCALAR, so mean(MSE(10 pred, 10 gt) / var / 50) * w * 10
        = 100 MSE(pred, gt) * mean(1 / var) / 50 * 10 w                                                   -> 1000 w mean(1 / var) / 50
        and without a variance (`var_expression is None`, :445) the plain 100 MSE * 10 w                  -> 1000 w"""
    w = float(lbs_weight)
    if var_expression is None:
        return LbsWeights(0.1 * w, 1000.0 * w, 1000.0 * w)
    var = torch.as_tensor(var_expression, dtype=torch.float64)
    return LbsWeights(0.1 * w, 1000.0 * w, 1000.0 * w * float((1.0 / var).mean()) / 50.0)


def lbs_terms_workspace(dev: torch.device) -> torch.Tensor:
    """A fresh zeroed workspace for `lbs_terms_and_grad(..., workspace=)`."""
    return _terms_ws.fresh(dev)


def lbs_terms_and_grad(index, lbs_weights, posedirs, shapedirs, gt_weights, gt_posedirs, gt_shapedirs,
                       terms: LbsWeights = LbsWeights(0.0, 0.0, 0.0), d_weights: Optional[torch.Tensor] = None,
                       d_posedirs: Optional[torch.Tensor] = None, d_shapedirs: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The three blendshape terms of MonoGaussianAvatarLoss (train/loss.py:418-445, :472-515) in ONE launch (`fr_lbs_terms`):
    returns `out` = the plain mean squared errors of lbs_weights [N,J], posedirs [N,36,3] and shapedirs [N,3,E] against the rows
    `index` [N] (int32, `nearest_vertex`) of gt_weights [V,J], gt_posedirs [V,36,3] and gt_shapedirs [V,3,E] — UNWEIGHTED, a
    3-element device tensor — and ADDS terms[k] * d loss_k / d pred_k into d_weights / d_posedirs / d_shapedirs (None: that
    loss only; a weight of 0 leaves its array untouched).  N == 0: nothing is launched, `out` keeps its content and without
    `out` the result is zeros.  The caller pads the ghost bone's column of FLAME's weights and
    transposes FLAME's [36, 3V] pose basis once.  `index` must name rows of the tables (the kernel clamps it to 0 .. V-1).
    `workspace`: scratch from `lbs_terms_workspace()`; by default one is kept per (device, current stream) — launches that may
    overlap must not share one.  There is no CPU path."""
    who = "lbs_terms_and_grad"
    w, P, S = (_f32(t.detach(), n, who) for t, n in zip((lbs_weights, posedirs, shapedirs), ("lbs_weights", "posedirs", "shapedirs")))
    gw, gP, gS = (_f32(t.detach(), n, who) for t, n in zip((gt_weights, gt_posedirs, gt_shapedirs),
                                                           ("gt_weights", "gt_posedirs", "gt_shapedirs")))
    if w.dim() != 2 or S.dim() != 3:
        raise RuntimeError(f"{who}: lbs_weights [N,J], shapedirs [N,3,E]")
    N, J, E, V = int(w.shape[0]), int(w.shape[1]), int(S.shape[2]), int(gw.shape[0])
    if P.shape != (N, POSE_FEATURES, 3) or S.shape != (N, 3, E) or gw.shape != (V, J) or gP.shape != (V, POSE_FEATURES, 3) or \
            gS.shape != (V, 3, E) or V < 1 or E < 1 or J < 1:
        raise RuntimeError(f"{who}: lbs_weights [N,J], posedirs [N,{POSE_FEATURES},3], shapedirs [N,3,E] and tables gt_weights "
                           f"[V,J], gt_posedirs [V,{POSE_FEATURES},3], gt_shapedirs [V,3,E]")
    if not (isinstance(index, torch.Tensor) and index.dtype == torch.int32 and index.is_contiguous() and index.shape == (N,)):
        raise RuntimeError(f"{who}: index is a contiguous int32 [N] tensor")
    grads = [(d_weights, w, "d_weights"), (d_posedirs, P, "d_posedirs"), (d_shapedirs, S, "d_shapedirs")]
    for t, like, n in grads:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape != like.shape):
            raise RuntimeError(f"{who}: {n} is a contiguous float32 tensor shaped like its prediction")
    dev = _one_device(who, w, P, S, gw, gP, gS, index, *[t for t, _, _ in grads if t is not None])
    # (N == 0 launches nothing: a caller's `out` is left as it is, a tensor made here is zeros rather than uninitialised memory)
    loss = out if out is not None else (torch.empty if N else torch.zeros)((3,), dtype=torch.float32, device=dev)
    if loss.device != dev or loss.dtype != torch.float32 or loss.numel() != 3 or not loss.is_contiguous():
        raise RuntimeError(f"{who}: `out` is a contiguous 3-element float32 tensor on the predictions' device")
    ws = _terms_ws.resolve(dev, workspace, who)
    if N == 0:
        return loss
    cfg = _lib.fr_lbs_terms_config(*[float(x) for x in terms])
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.launch("fr_lbs_terms", dev, C.byref(cfg), N, V, E, J, index.data_ptr(), w.data_ptr(), P.data_ptr(), S.data_ptr(),
                gw.data_ptr(), gP.data_ptr(), gS.data_ptr(), p(d_weights), p(d_posedirs), p(d_shapedirs), loss.data_ptr(),
                ws.data_ptr())
    return loss


def splat_attributes(features: torch.Tensor, offsets: torch.Tensor, radius: float, scene_scale: float = 1.0):
    """`forward` :196-206 plus `scales + radius` (:417), in plain torch between the caller's two MLPs: `features` [N,11] is the
    geometry network's (rgb 3, scale 3, rotation 4, opacity 1, as get_rbg_value_functorch slices it, :363-366), `offsets`
    [N,11] the Gaussian network's (scale 3, rotation 4, opacity 1, colour 3, :195).  Returns (rgb [N,3], opacity [N,1],
    scales [N,3], rotations [N,4]) as the rasterizer takes them:
        rgb = sigmoid(rgb + d_colour),  scales = sigmoid(scale + d_scale) * 0.025 / scene_scale + radius,
        rotations = normalize(rotation + d_rotation),  opacity = sigmoid(opacity + d_opacity)"""
    if features.shape[-1] != 11 or offsets.shape != features.shape:
        raise RuntimeError("splat_attributes: features [N,11] (rgb, scale, rotation, opacity), offsets [N,11] (scale, rotation, "
                           "opacity, colour)")
    rgb = torch.sigmoid(features[:, 0:3] + offsets[:, 8:11])
    scales = torch.sigmoid(features[:, 3:6] + offsets[:, 0:3]) * (0.025 / float(scene_scale)) + float(radius)
    rotations = torch.nn.functional.normalize(features[:, 6:10] + offsets[:, 3:7], dim=-1)
    opacity = torch.sigmoid(features[:, 10:11] + offsets[:, 7:8])
    return rgb, opacity, scales, rotations


def render_points(camera, xyz, rgb, opacity, scales, rotations, bg: torch.Tensor):
    """`_render` (:380-428): the rasterizer with `colors_precomp` — (image [3,H,W], radii [N]).  `camera`: anything with FoVx,
    FoVy, image_height, image_width, world_view_transform, full_proj_transform, camera_center (model.TorchCamera)."""
    rs = GaussianRasterizationSettings(
        image_height=int(camera.image_height), image_width=int(camera.image_width), tanfovx=math.tan(camera.FoVx * 0.5),
        tanfovy=math.tan(camera.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=camera.world_view_transform,
        projmatrix=camera.full_proj_transform, sh_degree=3, campos=camera.camera_center, prefiltered=False, debug=False)
    means2D = torch.zeros_like(xyz).requires_grad_(xyz.requires_grad)
    out = GaussianRasterizer(raster_settings=rs)(means3D=xyz, means2D=means2D, shs=None, colors_precomp=rgb, opacities=opacity,
                                                 scales=scales, rotations=rotations, cov3D_precomp=None)
    return out[0], out[1]


# `_upsample_points` (:441-460): (first epoch, one past the last epoch, target point count)
UPSAMPLE_TARGETS = ((0, 5, 400), (5, 10, 800), (10, 15, 1600), (15, 20, 3200), (20, 25, 6400), (25, 30, 10000), (30, 40, 20000),
                    (40, 50, 40000), (50, 60, 80000))
UPSAMPLE_FINAL = 100000          # epoch >= 60


def upsample_target(epoch: int) -> int:
    for lo, hi, n in UPSAMPLE_TARGETS:
        if lo <= epoch < hi:
            return n
    return UPSAMPLE_FINAL if epoch >= 60 else UPSAMPLE_TARGETS[0][2]


def radius_factor(epoch: int) -> float:
    """What `_upsample_points(epoch)` multiplies the radius by (:462-467)."""
    if epoch in (5, 10, 15, 20, 25, 30, 40, 50):
        return 0.75
    if epoch == 60:
        return 0.9
    if epoch > 60 and epoch % 5 == 0:
        return 0.75
    return 1.0


class MonoPoints:
    """The reference's `PointCloud` (:524-565) and the host logic around it: `points` [N,3] (a leaf that requires grad), the
    splat `radius` and the visibility of the last frame.  The caller's optimizer is rebuilt after `prune` / `upsample`, as the
    reference rebuilds its own (the parameter is a new tensor)."""

    def __init__(self, n_init_points: int = 400, max_points: int = 100000, scene_scale: float = 1.0, prune_thresh: float = 0.1,
                 device="cuda", generator: Optional[torch.Generator] = None):
        """Sphere init (:538-545): uniform points of the cube [-1, 1]^3 pushed onto the sphere of radius 0.5 / scene_scale; the
        radius of `_register_points` (:146): 0.15 * 0.75 ** log2(N / 100) / scene_scale."""
        self.max_points, self.scene_scale, self.prune_thresh = int(max_points), float(scene_scale), float(prune_thresh)
        self.device = torch.device(device)
        p = torch.rand((int(n_init_points), 3), generator=generator) * 2.0 - 1.0
        p = torch.nn.functional.normalize(p, dim=1) * (0.5 / self.scene_scale)
        self.points = p.to(self.device, torch.float32).requires_grad_(True)
        self.radius = 0.15 * (0.75 ** math.log2(self.N / 100)) / self.scene_scale
        self.visible = torch.zeros((self.N,), dtype=torch.bool, device=self.device)

    @property
    def N(self) -> int:
        return int(self.points.shape[0])

    def mark_visible(self, opacity: torch.Tensor) -> None:
        """`_render` :423-428 and `forward` :227: a point is visible once its opacity reached `prune_thresh` in a frame."""
        self.visible |= opacity.detach().reshape(-1) >= self.prune_thresh

    def prune(self, mask: torch.Tensor) -> None:
        """`PointCloud.prune` (:547-549): keep the points of the boolean `mask` [N]."""
        mask = mask.to(self.device).reshape(-1)
        if mask.dtype != torch.bool or mask.numel() != self.N:
            raise RuntimeError("MonoPoints.prune: a boolean mask [N]")
        self.points = self.points.detach()[mask].clone().requires_grad_(True)
        self.visible = torch.zeros((self.N,), dtype=torch.bool, device=self.device)

    def upsample(self, epoch: int, generator: Optional[torch.Generator] = None) -> int:
        """`_upsample_points(epoch)` (:430-467): copies of randomly drawn points, jittered by uniform noise of width `radius`
        (0.004 after epoch 100), up to the epoch's target count (never beyond `max_points`); then the radius schedule.
        `generator`: a CPU generator for the draws.  Returns the number of points added."""
        cur = self.radius
        pts = self.points.detach()
        width = cur if epoch <= 100 else 0.004
        add = min(upsample_target(epoch), self.max_points) - self.N
        if add > 0:
            noise = (torch.rand(tuple(pts.shape), generator=generator) - 0.5) * width
            idx = torch.randint(0, self.N, (add,), generator=generator)
            new = (pts + noise.to(self.device))[idx.to(self.device)]
            self.points = torch.cat([pts, new], 0).requires_grad_(True)
            self.visible = torch.zeros((self.N,), dtype=torch.bool, device=self.device)
        self.radius = radius_factor(epoch) * cur
        return max(add, 0)


__all__ = ["LbsWeights", "MonoPoints", "POSE_FEATURES", "PoseState", "deform_points", "lbs_terms_and_grad", "lbs_terms_workspace",
           "nearest_vertex", "pose_workspace", "radius_factor", "reference_lbs_weights", "render_points", "splat_attributes", "upsample_target"]
