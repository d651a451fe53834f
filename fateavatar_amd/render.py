"""`render()` — the caller-facing entry of the path (reference: volume_rendering/render_3dgs.py:7-81).

Same signature, same returned dict.  `pc` is anything with the reference GaussianModel's getters
(get_xyz, get_opacity, get_scaling, get_rotation, get_features, max_sh_degree;
volume_rendering/gaussian_model.py:105-128); `viewpoint_camera` anything with FoVx, FoVy, image_height,
image_width, world_view_transform, full_proj_transform, camera_center (volume_rendering/camera_3dgs.py:22-72).
"""
from __future__ import annotations

import math

import torch

from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_views_autograd


_zero_cache = {}


def _zero_points(means3D: torch.Tensor) -> torch.Tensor:
    """A fresh leaf tensor of zeros shaped like means3D that requires grad.  Nothing ever writes its values (the
    rasterizer only uses it as the slot whose .grad receives dL/dmeans2D), so the zeros themselves are a cached
    constant per (shape, dtype, device) and every call returns a new leaf aliasing them: no fill kernel per frame."""
    key = (tuple(means3D.shape), means3D.dtype, means3D.device)
    z = _zero_cache.get(key)
    if z is None:
        if len(_zero_cache) > 8:
            _zero_cache.clear()
        z = _zero_cache[key] = torch.zeros_like(means3D, requires_grad=False)
    return z.detach().requires_grad_(True)


def _screenspace_points(means3D: torch.Tensor, pc) -> torch.Tensor:
    """The tensor whose .grad receives the screen-space mean gradients (render_3dgs.py:21-27).  The reference adds `+ 0`
    and retains the gradient of the resulting non-leaf; a leaf collects the same .grad with one kernel less and lets
    autograd adopt the rasterizer's gradient buffer instead of copying it."""
    sp = _zero_points(means3D)
    stats = getattr(pc, "fused_densification_stats", None)
    if stats is not None:  # extension: (xyz_gradient_accum, denom) updated inside the backward kernel
        sp._fr_densification_stats = stats
    return sp


def _settings(cam, pc, bg, scaling_modifier) -> GaussianRasterizationSettings:
    """render_3dgs.py:30-46."""
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=scaling_modifier, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=pc.max_sh_degree, campos=cam.camera_center, prefiltered=False,
        debug=False)


def _activations(pc):
    """(fused, opacity, scales, rotations).  Extension: a holder that sets `fused_activations` hands
    over its RAW opacity / scaling / rotation and the HIP kernels apply sigmoid / exp / normalize (and their derivatives)
    themselves, instead of ~15 small PyTorch kernels per frame.  The default is the reference behaviour."""
    if getattr(pc, "fused_activations", False):
        return True, pc._opacity, pc._scaling, pc._rotation
    return False, pc.get_opacity, pc.get_scaling, pc.get_rotation


def _result(outs, screenspace_points) -> dict:
    """render()'s dict from a view's autograd outputs: (image, radii), with `depth_alpha` (extension) also (depth, alpha)."""
    image, radii, *planes = outs
    visible = getattr(radii, "_fr_visible", None)  # written by the preprocess kernel (same values as radii > 0)
    out = {"render": image, "viewspace_points": screenspace_points,
           "visibility_filter": visible if visible is not None else radii > 0, "radii": radii}
    if planes:
        out["depth"], out["alpha"] = planes
    return out


def render(viewpoint_camera, pc, bg_color: torch.Tensor, scaling_modifier=1.0, override_color: torch.Tensor = None,
           device='cuda', depth_alpha=False):
    """`depth_alpha=True` (extension): the dict also holds "depth" and "alpha" [1,H,W] — the alpha-weighted view-space depth
    (sum of z alpha T; expected depth is depth / alpha) and the accumulated opacity 1 - T_final — both differentiable."""
    means3D = pc.get_xyz
    screenspace_points = _screenspace_points(means3D, pc)
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, bg_color, scaling_modifier))
    fused, opacity, scales, rotations = _activations(pc)
    shs, colors_precomp = (pc.get_features, None) if override_color is None else (None, override_color)
    out = rasterizer(means3D=means3D, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp, opacities=opacity,
                     scales=scales, rotations=rotations, cov3D_precomp=None, **({"raw_activations": True} if fused else {}),
                     **({"depth_alpha": True} if depth_alpha else {}))
    return _result(out, screenspace_points)


def render_batch(viewpoint_cameras, pcs, bg_colors, scaling_modifier=1.0, slots=None, depth_alpha=False):
    """`render()` for K views IN ONE LAUNCH CHAIN (include/fr_rasterizer.h: fr_forward_batch / fr_backward_batch): the
    reference renders the frames of a batch one after the other (model/fateavatar.py:251-276), and one frame's kernels
    leave most of an MI355X idle; here every kernel of the frame is launched once for all K views, with no stream or
    hardware-queue arrangement on the caller's side.  `pcs` / `bg_colors`: one per view, or a single holder / tensor
    for all of them (shared Gaussians: autograd then sums the views' gradients).  Returns the list of render() dicts (with
    "depth" and "alpha" under `depth_alpha`, as render())."""
    K = len(viewpoint_cameras)
    if not isinstance(pcs, (list, tuple)):
        pcs = [pcs] * K
    if isinstance(bg_colors, torch.Tensor):
        bg_colors = [bg_colors] * K
    settings, tensors, points = [], [], []
    fused = bool(getattr(pcs[0], "fused_activations", False))
    empty = torch.Tensor([])
    for cam, pc, bg in zip(viewpoint_cameras, pcs, bg_colors):
        fused_k, opacity, scales, rotations = _activations(pc)
        if fused_k != fused:
            raise RuntimeError("render_batch: the views' holders must agree on fused_activations")
        means3D = pc.get_xyz
        sp = _screenspace_points(means3D, pc)
        settings.append(_settings(cam, pc, bg, scaling_modifier))
        tensors.append((means3D, sp, pc.get_features, empty, opacity, scales, rotations, empty))
        points.append(sp)
    res = rasterize_views_autograd(settings, tensors, raw_activations=fused, slots=slots, depth_alpha=depth_alpha)
    return [_result(r, sp) for r, sp in zip(res, points)]
