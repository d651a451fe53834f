"""Python host of the MI355X rasterizer: the reference's operator interface, same names,
argument meaning and error behaviour, over the C ABI in include/fr_rasterizer.h.

Mirrors (paths relative to /root/reference/submodules/diff-gaussian-rasterization/):
  GaussianRasterizationSettings   diff_gaussian_rasterization/__init__.py:157-169
  GaussianRasterizer              diff_gaussian_rasterization/__init__.py:171-220
  _RasterizeGaussians             diff_gaussian_rasterization/__init__.py:44-155
  rasterize_gaussians / rasterize_gaussians_backward / mark_visible  (the `_C` module)
                                  ext.cpp:15-19, rasterize_points.cu:35-217

All tensors must live on a HIP device ("cuda" in PyTorch-ROCm).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib

NUM_CHANNELS = 3  # cuda_rasterizer/config.h:15

# per-device guess of the binning capacity (instances); grows when a frame overflows it
_capacity_hint: dict = {}
last_counts: dict = {}  # device index -> fr_counts of the most recent forward (diagnostics)
last_forward_only: dict = {}  # device index -> whether the most recent forward was forward-only (diagnostics)


def _dev_index(t: torch.Tensor) -> int:
    if not t.is_cuda:
        raise RuntimeError("fateavatar_amd rasterizer: tensors must be on a HIP device (torch device 'cuda'); "
                           "there is no CPU path")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _f32c(*tensors) -> list:
    """Tensors as the kernels read them: float32 and contiguous (None stays None)."""
    return [t if t is None else (t if t.dtype == torch.float32 else t.float()).contiguous() for t in tensors]


def _ptrs(*tensors) -> list:
    """Device pointers for a C struct: 0 for an absent (None or empty) tensor."""
    return [0 if t is None or t.numel() == 0 else t.data_ptr() for t in tensors]


# When True, forwards never wait for their instance counts (graph-capturable, zero host syncs): the binning
# capacity is the current high-water mark and overflow is only detected by `check_async_overflow()`.
_no_wait = False


def set_no_wait(on: bool) -> None:
    """Capture mode: make rasterize_gaussians free of host synchronisation (see FR_FLAG_NO_WAIT).  Process-wide:
    prefer the scoped form `with no_wait(): ...` around a graph capture, so that renders outside the capture (a
    validation view, a second model) keep their overflow check and capacity regrow."""
    global _no_wait
    _no_wait = bool(on)


class no_wait:
    """`with rasterizer.no_wait():` — FR_FLAG_NO_WAIT for the forwards issued inside the block only."""

    def __enter__(self):
        global _no_wait
        self._prev = _no_wait
        _no_wait = True
        return self

    def __exit__(self, *exc):
        global _no_wait
        _no_wait = self._prev
        return False


# Forward-only frames (FR_FLAG_FORWARD_ONLY): the autograd-level entry points render a frame that autograd will not record
# — grad mode off (torch.no_grad(), inference mode) or no tensor input requiring grad — without the backward's hand-off.
_forward_only_auto = True


class set_forward_only:
    """`rasterizer.set_forward_only(False)` turns the automatic choice of forward-only frames off (True: on, the default),
    process-wide; `with rasterizer.set_forward_only(auto):` sets it for the block only and restores the previous setting
    on exit.  For A/B measurements: images and radii are the same either way."""

    def __init__(self, auto: bool):
        global _forward_only_auto
        self._prev, _forward_only_auto = _forward_only_auto, bool(auto)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        global _forward_only_auto
        _forward_only_auto = self._prev
        return False


def _pick_forward_only(tensors) -> bool:
    """Whether a frame of these tensor inputs can skip the backward's hand-off: autograd will not record it.  Decided
    BEFORE `Function.apply` (grad mode is always off inside `Function.forward`)."""
    if not _forward_only_auto:
        return False
    return not torch.is_grad_enabled() or not any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


_slot = 0   # which fr_handle of the device the calls of this thread of control use (see handle_slot)


class handle_slot:
    """`with rasterizer.handle_slot(k):` — render through the k-th handle of the device.  Frames of one handle are
    ordered; views that should be IN FLIGHT TOGETHER (one stream and one captured graph each) take one slot each."""

    def __init__(self, slot: int):
        self.slot = int(slot)

    def __enter__(self):
        global _slot
        self._prev, _slot = _slot, self.slot
        return self

    def __exit__(self, *exc):
        global _slot
        _slot = self._prev
        return False


def read_counts(device_index: int = 0, slot: int | None = None):
    """fr_counts of the most recent frame on this device (synchronise first)."""
    c = _lib.fr_counts()
    _lib.check(_lib.lib().fr_read_counts(_lib.handle(device_index, _slot if slot is None else slot), C.byref(c)), "fr_read_counts")
    return c


def check_async_overflow(device_index: int = 0) -> bool:
    """After synchronising: True if the last no-wait frame overflowed its binning capacity (its outputs are
    then invalid); the capacity hint is raised so that the next frame fits."""
    c = read_counts(device_index)
    last_counts[device_index] = c
    if c.overflow:
        _capacity_hint[device_index] = max(_capacity_hint.get(device_index, 0), int(c.num_instances * 1.25) + 1024)
    return bool(c.overflow)


def _params(P, degree, M, W, H, tan_fovx, tan_fovy, scale_modifier, prefiltered, debug, raw=False,
            aux=None, extra_flags=0) -> _lib.fr_params:
    flags = (_lib.FR_FLAG_NO_WAIT if _no_wait else 0) | (_lib.FR_FLAG_RAW_ACTIVATIONS if raw else 0) | int(extra_flags)
    prm = _lib.fr_params(int(P), int(degree), int(M), int(W), int(H), float(tan_fovx), float(tan_fovy),
                         float(scale_modifier), int(bool(prefiltered)), int(bool(debug)), flags)
    if aux is not None:
        prm._aux_keepalive = aux
        prm.aux = C.pointer(aux)
    return prm


def _stats3(stats):
    """(xyz_gradient_accum, denom[, overflow word]) -> the three of them (None where absent)."""
    if stats is None:
        return None, None, None
    return stats[0], stats[1], (stats[2] if len(stats) > 2 else None)


_camera_ws: dict = {}   # (device index, handle slot) -> the zeroed scratch of that handle's camera-gradient launches


def camera_workspace(dev: int, slot: int) -> torch.Tensor:
    """fr_aux_camera::camera_workspace of the backward passes of handle `slot` on device `dev`: zeroed once, left zeroed by the kernel.
    One per handle — backward passes of one handle are ordered, those of different handles (the views of a batch, frames in
    flight on several streams) may overlap and must not share one."""
    ws = _camera_ws.get((dev, slot))
    if ws is None:
        if torch.cuda.is_current_stream_capturing():    # (torch.zeros inside a capture would become part of the graph)
            raise RuntimeError(f"camera gradients: the workspace of handle slot {slot} does not exist yet and cannot be made while a "
                               "stream is being captured: run one eager backward with camera gradients through it first")
        ws = _camera_ws[(dev, slot)] = torch.zeros((_lib.lib().fr_camera_grad_workspace_bytes(),), dtype=torch.uint8,
                                                   device=torch.device("cuda", dev))
    return ws


def _camera_outputs(camera, device):
    """The (d_viewmatrix [4,4], d_projmatrix [4,4], d_campos [3]) tensors of a backward with `_camera`: True — fresh ones —
    or the caller's three buffers (any may be None: not wanted), written in place."""
    if camera is True:
        return tuple(torch.empty(sh, dtype=torch.float32, device=device) for sh in ((4, 4), (4, 4), (3,)))
    out = tuple(camera)
    if len(out) != 3 or all(t is None for t in out):
        raise RuntimeError("_camera: True, or (d_viewmatrix [4,4], d_projmatrix [4,4], d_campos [3]) buffers, not all of them None")
    for t, n in zip(out, (16, 16, 3)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
            raise RuntimeError("_camera: the buffers are contiguous float32 device tensors of 16, 16 and 3 elements")
    return out


def _aux(visible=None, grad_accum=None, denom=None, binding=None, bind_grads=None, overflow_out=None, planes=None, camera=None):
    """fr_aux (optional fused side inputs / outputs) from torch tensors, or None if nothing is asked for.  `binding`: an
    `_lib.fr_binding` descriptor (the frame is rendered straight from its mesh binding); `bind_grads`: dict with the
    backward's d_verts / d_offset (a face-local binding: d_local_xyz) / d_rotation / d_scaling tensors (any may be None).  `planes` (FR_FLAG_DEPTH_ALPHA): dict
    of the out_depth / out_alpha / dL_ddepth / dL_dalpha tensors and the `planes` scratch (any may be None; the scratch of a
    forward is set by the launcher, which sizes it with the binning buffer).  `camera` (FR_FLAG_CAMERA_GRAD): dict of the
    d_viewmatrix / d_projmatrix / d_campos tensors (any may be None) and the camera_workspace: the block returned is then the
    `base` of an `_lib.fr_aux_camera` that carries them."""
    if visible is None and grad_accum is None and denom is None and binding is None and overflow_out is None and planes is None \
            and camera is None:
        return None
    for t, dt in ((visible, (torch.bool, torch.uint8)), (grad_accum, (torch.float32,)), (denom, (torch.float32,))):
        if t is not None and (t.dtype not in dt or not t.is_contiguous() or not t.is_cuda):
            raise RuntimeError("fused side outputs must be contiguous device tensors (bool/uint8 mask, float32 stats)")
    if camera is not None:     # (FR_FLAG_CAMERA_GRAD: the block is the `base` of an fr_aux_camera, which it keeps alive)
        ext = _lib.fr_aux_camera()
        aux = ext.as_aux()
        for n, t in camera.items():
            if t is not None:
                setattr(ext, n, t.data_ptr())
        aux._camera_keepalive = (ext, camera)
        aux.visible, aux.grad_accum, aux.denom = (t.data_ptr() if t is not None else None for t in (visible, grad_accum, denom))
    else:
        aux = _lib.fr_aux(*(t.data_ptr() if t is not None else None for t in (visible, grad_accum, denom)))
    if overflow_out is not None:
        if not (overflow_out.is_cuda and overflow_out.dtype == torch.float32 and overflow_out.numel() >= 1 and overflow_out.is_contiguous()):
            raise RuntimeError("the overflow word must be a contiguous float32 device tensor")
        aux._overflow_keepalive = overflow_out
        aux.overflow_out = overflow_out.data_ptr()
    if binding is not None:
        aux._binding_keepalive = binding
        aux.binding = C.pointer(binding)
        for n in ("d_verts", "d_offset", "d_rotation", "d_scaling", "d_local_xyz"):
            t = (bind_grads or {}).get(n)
            if t is not None:
                if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                    raise RuntimeError(f"binding gradient {n} must be a contiguous float32 device tensor")
                setattr(aux, n, t.data_ptr())
    if planes is not None:
        aux._planes_keepalive = planes
        for n, t in planes.items():
            if t is not None:
                if not (t.is_cuda and t.is_contiguous() and (t.dtype == torch.float32 or n == "planes")):
                    raise RuntimeError(f"{n} must be a contiguous float32 device tensor")
                setattr(aux, n, t.data_ptr())
    return aux


def _inputs(bg, means3D, sh, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos):
    return _lib.fr_inputs(*_ptrs(bg, means3D, sh, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
                                 campos))


def _grad_shapes(P, M):
    """rasterize_gaussians_backward's results (rasterize_points.cu:151-159, 195), in the order of fr_grads."""
    return dict(dL_dmeans2D=(P, 3), dL_dcolors=(P, NUM_CHANNELS), dL_dopacity=(P, 1), dL_dmeans3D=(P, 3),
                dL_dcov3D=(P, 6), dL_dsh=(P, M, 3), dL_dscales=(P, 3), dL_drotations=(P, 4))


_GRAD_NAMES = tuple(_grad_shapes(0, 0))


class _Forward(NamedTuple):
    """What the forward of one view returns, by name.  The first six are `_C.rasterize_gaussians`' tuple
    (rasterize_points.cu:114); depth [H,W], alpha [H,W] and the opaque planes buffer exist with FR_FLAG_DEPTH_ALPHA only."""
    num_rendered: int
    color: torch.Tensor
    radii: torch.Tensor
    geom: torch.Tensor
    binning: torch.Tensor
    img: torch.Tensor
    depth: Optional[torch.Tensor] = None
    alpha: Optional[torch.Tensor] = None
    planes: Optional[torch.Tensor] = None

    def as_tuple(self) -> tuple:
        """The documented result of `rasterize_gaussians`: the reference's six, nine with the planes."""
        return tuple(self) if self.planes is not None else tuple(self[:6])


def _forward_view(args, raw=False, visible=None, binding=None, forward_only=False, depth_alpha=False) -> dict:
    """One view of a forward, from the positional arguments of `rasterize_gaussians`: its inputs as the kernels read them
    (kept alive in the view), its fr_params / fr_inputs, outputs and binning capacity.  The launcher allocates the binning
    buffer.  `forward_only`: FR_FLAG_FORWARD_ONLY (no backward may be run on the frame's buffers).  `depth_alpha`:
    FR_FLAG_DEPTH_ALPHA (the view also returns depth [H,W], alpha [H,W] and the planes scratch its backward needs)."""
    (background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
     tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug) = args
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    dev = _dev_index(means3D)
    P, H, W = means3D.size(0), int(image_height), int(image_width)
    keep = _f32c(background, means3D, sh, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos)
    M = sh.size(1) if sh.numel() != 0 else 0
    L, opts = _lib.lib(), dict(device=means3D.device)
    planes = None
    if depth_alpha:
        planes = dict(out_depth=torch.empty((H, W), dtype=torch.float32, **opts), out_alpha=torch.empty((H, W), dtype=torch.float32, **opts))
    aux = _aux(visible=visible, binding=binding, planes=planes)
    flags = (_lib.FR_FLAG_FORWARD_ONLY if forward_only else 0) | (_lib.FR_FLAG_DEPTH_ALPHA if depth_alpha else 0)
    return dict(dev=dev, W=W, H=H, opts=opts, keep=keep, inp=_inputs(*keep), aux=aux, planes=planes,
                prm=_params(P, degree, M, W, H, tan_fovx, tan_fovy, scale_modifier, prefiltered, debug, raw, aux, flags),
                out_color=torch.empty((NUM_CHANNELS, H, W), dtype=torch.float32, **opts),
                radii=torch.empty((P,), dtype=torch.int32, **opts),
                geom=torch.empty((L.fr_geometry_bytes(P),), dtype=torch.uint8, **opts),
                img=torch.empty((L.fr_image_bytes(W, H),), dtype=torch.uint8, **opts),
                cap=max(_capacity_hint.get(dev, 0), 4 * P + 65536))


def _backward_view(args, raw=False, want=None, out=None, stats=None, accumulate=(), binding=None, bind_grads=None,
                   what="rasterize_gaussians_backward", planes=None, camera=None, slot=0) -> dict:
    """One view of a backward, from the positional arguments of `rasterize_gaussians_backward` and its keyword
    arguments: the gradient tensors it returns, its inputs as the kernels read them (kept alive in the view), and its
    fr_params / fr_inputs / fr_grads.  `planes` (FR_FLAG_DEPTH_ALPHA): (planesBuffer, dL_ddepth, dL_dalpha) of a frame
    rendered with depth and alpha planes; either gradient may be None (zero).  `camera` (FR_FLAG_CAMERA_GRAD): True or three
    buffers (`_camera_outputs`); the view's result then ends with (d_viewmatrix, d_projmatrix, d_campos), and the launch takes
    the scratch of the device's handle `slot`."""
    (background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
     tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug) = args
    dev = _dev_index(means3D)
    P, H, W = means3D.size(0), dL_dout_color.size(1), dL_dout_color.size(2)
    M = sh.size(1) if sh.numel() != 0 else 0
    shapes = _grad_shapes(P, M)
    out = out or {}
    for k in accumulate:
        if out.get(k) is None:
            raise RuntimeError(f"{what}: cannot accumulate into {k}: no buffer was given for it")
    # the kernel writes every row of every array it is given, so uninitialised memory is fine
    g = {k: (torch.empty(s, device=means3D.device, dtype=torch.float32) if (want is None or k in want) else None)
         for k, s in shapes.items()}
    for k, buf in out.items():  # caller-provided gradient buffers (e.g. views into a flat gradient buffer): written in place
        if buf is not None:
            assert buf.shape == shapes[k] and buf.is_contiguous() and buf.dtype == torch.float32, k
            # a FRESH view object: autograd's AccumulateGrad only adopts an incoming gradient without
            # cloning it when nobody else holds a reference to that tensor object
            g[k] = buf.view(buf.shape)
    *keep, dpix = _f32c(background, means3D, sh, colors, None, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
                        campos, dL_dout_color)
    acc_flags = sum(1 << (_lib.FR_FLAG_ACCUMULATE_SHIFT + _GRAD_NAMES.index(k)) for k in accumulate)
    aux, pl = None, None
    if planes is not None:
        buf, dz, da = planes
        pl = dict(planes=buf, dL_ddepth=None if dz is None else _f32c(dz.reshape(H, W))[0],
                  dL_dalpha=None if da is None else _f32c(da.reshape(H, W))[0])
        acc_flags |= _lib.FR_FLAG_DEPTH_ALPHA
    cam_out, cm = (), None
    if camera is not None and camera is not False and P != 0:
        cam_out = _camera_outputs(camera, means3D.device)
        cm = dict(zip(("d_viewmatrix", "d_projmatrix", "d_campos"), cam_out), camera_workspace=camera_workspace(dev, slot))
        acc_flags |= _lib.FR_FLAG_CAMERA_GRAD
    if stats is not None or binding is not None or pl is not None or cm is not None:
        grad_accum, denom, overflow_out = _stats3(stats)
        aux = _aux(grad_accum=grad_accum, denom=denom, overflow_out=overflow_out, binding=binding, bind_grads=bind_grads, planes=pl,
                   camera=cm)
    return dict(dev=dev, g=g, cam=cam_out, keep=keep, inp=_inputs(*keep), grads=_lib.fr_grads(*_ptrs(*g.values())),
                prm=_params(P, degree, M, W, H, tan_fovx, tan_fovy, scale_modifier, False, debug, raw, aux, acc_flags),
                radii=radii.contiguous(), geom=geomBuffer, img=imageBuffer, binning=binningBuffer, dpix=dpix)


def _batch_arrays(views, slots, dev):
    """What fr_forward_batch / fr_backward_batch take per view: handles, fr_params and fr_inputs pointers, and
    `arr(key)`, the device pointers of one buffer of every view."""
    K = len(views)
    return ((C.c_void_p * K)(*[_lib.handle(dev, sl) for sl in slots]),
            (C.POINTER(_lib.fr_params) * K)(*[C.pointer(v["prm"]) for v in views]),
            (C.POINTER(_lib.fr_inputs) * K)(*[C.pointer(v["inp"]) for v in views]),
            lambda key: (C.c_void_p * K)(*[v[key].data_ptr() for v in views]))


def _launch_forward(views, slots, batch):
    """The forward of views from `_forward_view` on the device's handles `slots`: fr_forward_batch, or fr_forward for a
    single frame (`batch` False).  A view that overflows its binning capacity is rerun with the capacity it needs.
    Returns the `_Forward` record of every view."""
    K, dev, L = len(views), views[0]["dev"], _lib.lib()
    counts = (_lib.fr_counts * K)()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if batch:
            handles, prm_p, inp_p, arr = _batch_arrays(views, slots, dev)
        else:
            h, one = _lib.handle(dev, slots[0]), views[0]
        while True:
            for v in views:
                v["binning"] = torch.empty((L.fr_binning_bytes(v["cap"], v["W"], v["H"]),), dtype=torch.uint8, **v["opts"])
                if v["planes"] is not None:   # (FR_FLAG_DEPTH_ALPHA: sized with the binning buffer)
                    v["planes"]["planes"] = torch.empty((L.fr_planes_bytes(v["cap"], v["W"], v["H"]),), dtype=torch.uint8, **v["opts"])
                    v["aux"].planes = v["planes"]["planes"].data_ptr()
            if batch:
                rc = L.fr_forward_batch(K, handles, prm_p, inp_p, arr("out_color"), arr("radii"), arr("geom"), arr("img"),
                                        arr("binning"), (C.c_uint64 * K)(*[v["cap"] for v in views]), counts, stream)
            else:
                rc = L.fr_forward(h, C.byref(one["prm"]), C.byref(one["inp"]), one["out_color"].data_ptr(),
                                  one["radii"].data_ptr(), one["geom"].data_ptr(), one["img"].data_ptr(),
                                  one["binning"].data_ptr(), one["cap"], counts, stream)
            if rc != _lib.FR_ERR_BINNING_CAPACITY:
                break
            for v, c in zip(views, counts):
                if c.overflow:
                    v["cap"] = int(c.num_instances * 1.25) + 1024
    _lib.check(rc, "fr_forward_batch" if batch else "fr_forward")
    out = []
    last_forward_only[dev] = bool(views[0]["prm"].flags & _lib.FR_FLAG_FORWARD_ONLY)
    for v, c in zip(views, counts):
        if not _no_wait:  # (with it, the counts arrive later: read_counts / check_async_overflow)
            _capacity_hint[dev] = max(_capacity_hint.get(dev, 0), int(c.num_instances * 1.25) + 1024)
            last_counts[dev] = c
        pl = v["planes"] or {}
        out.append(_Forward(0 if _no_wait else int(c.num_rendered), v["out_color"], v["radii"], v["geom"], v["binning"], v["img"],
                            pl.get("out_depth"), pl.get("out_alpha"), pl.get("planes")))
    return out


def _launch_backward(views, slots, batch):
    """The backward of views from `_backward_view` on the device's handles `slots`: fr_backward_batch, or fr_backward for
    a single frame (`batch` False).  Returns the `rasterize_gaussians_backward` result tuple of every view."""
    K, dev, L = len(views), views[0]["dev"], _lib.lib()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if batch:
            handles, prm_p, inp_p, arr = _batch_arrays(views, slots, dev)
            grd_p = (C.POINTER(_lib.fr_grads) * K)(*[C.pointer(v["grads"]) for v in views])
            rc = L.fr_backward_batch(K, handles, prm_p, inp_p, arr("radii"), arr("geom"), arr("img"), arr("binning"),
                                     arr("dpix"), grd_p, stream)
        else:
            v = views[0]
            rc = L.fr_backward(_lib.handle(dev, slots[0]), C.byref(v["prm"]), C.byref(v["inp"]), v["radii"].data_ptr(),
                               v["geom"].data_ptr(), v["img"].data_ptr(), v["binning"].data_ptr(), v["dpix"].data_ptr(),
                               C.byref(v["grads"]), stream)
    _lib.check(rc, "fr_backward_batch" if batch else "fr_backward")
    return [tuple(v["g"].values()) + v["cam"] for v in views]


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, debug, _raw=False, _visible=None, _forward_only=False, _depth_alpha=False):
    """`_C.rasterize_gaussians` (rasterize_points.cu:35-115).  `_raw=True` (extension, FR_FLAG_RAW_ACTIVATIONS):
    opacity / scales / rotations are the RAW parameters and the kernels apply sigmoid / exp / normalize.
    `_forward_only=True` (extension, FR_FLAG_FORWARD_ONLY): the frame is rendered without the backward's hand-off — same
    image and radii — and its buffers cannot be handed to `rasterize_gaussians_backward`.  Never chosen here on its own.
    `_depth_alpha=True` (extension, FR_FLAG_DEPTH_ALPHA): the frame also renders its depth and alpha planes.

    Returns (num_rendered, out_color[3,H,W], radii[P] int32, geomBuffer, binningBuffer, imgBuffer); the three
    byte buffers are opaque and must be handed back to `rasterize_gaussians_backward`.  With `_depth_alpha`, three more:
    depth[H,W], alpha[H,W] and planesBuffer (opaque: `rasterize_gaussians_backward(..., _planes=(planesBuffer, dL_ddepth,
    dL_dalpha))`)."""
    v = _forward_view((background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                       projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug),
                      _raw, _visible, forward_only=_forward_only, depth_alpha=_depth_alpha)
    if v["prm"].P == 0:  # rasterize_points.cu:81 skips the rasterizer entirely
        empty, pl = torch.empty((0,), dtype=torch.uint8, device=means3D.device), v["planes"]
        return _Forward(0, v["out_color"].zero_(), v["radii"], empty, empty.clone(), empty.clone(),
                        *((pl["out_depth"].zero_(), pl["out_alpha"].zero_(), empty.clone()) if pl else ())).as_tuple()
    return _launch_forward([v], [_slot], batch=False)[0].as_tuple()


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                 viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos,
                                 geomBuffer, R, binningBuffer, imageBuffer, debug, _want=None, _out=None, _raw=False,
                                 _stats=None, _accumulate=(), _planes=None, _camera=False):
    """`_C.rasterize_gaussians_backward` (rasterize_points.cu:117-196).

    Returns (dL_dmeans2D[P,3], dL_dcolors[P,3], dL_dopacity[P,1], dL_dmeans3D[P,3], dL_dcov3D[P,6], dL_dsh[P,M,3],
    dL_dscales[P,3], dL_drotations[P,4]).  `_stats=(xyz_gradient_accum[P,1], denom[P,1])` (extension): the kernel
    also does `_add_densification_stats` (model/fateavatar.py:734-737) for the Gaussians with radii > 0.
    `_want` (extension): the names of the gradients to compute (the others come back as None); `_out`: caller-provided
    gradient buffers, written in place; `_accumulate`: names of `_out` buffers the frame's gradient is ADDED to
    (FR_FLAG_ACCUMULATE); `_planes=(planesBuffer, dL_ddepth, dL_dalpha)` (FR_FLAG_DEPTH_ALPHA): the gradients of the depth
    and alpha planes of a frame rendered with `_depth_alpha` (either may be None).
    `_camera=True` (extension, FR_FLAG_CAMERA_GRAD): three more results, (d_viewmatrix [4,4], d_projmatrix [4,4], d_campos [3]) —
    the gradients of the three camera inputs, which the reference leaves at None; or three buffers of those sizes, written in
    place (any may be None).  Entries the kernels do not read (viewmatrix column 3, projmatrix column 2) are 0."""
    v = _backward_view((background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                        projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
                        imageBuffer, debug), _raw, _want, _out, _stats, _accumulate, planes=_planes, camera=_camera, slot=_slot)
    if v["prm"].P == 0:
        cam = () if not _camera else tuple(None if t is None else t.zero_() for t in (
            _camera_outputs(_camera, means3D.device)))
        return tuple((_out[k] if k in _accumulate else torch.zeros(s, device=means3D.device, dtype=torch.float32))
                     for k, s in _grad_shapes(0, v["prm"].M).items()) + cam
    return _launch_backward([v], [_slot], batch=False)[0]


# ------------------------------------------------------------------ batched frames (fr_forward_batch / fr_backward_batch)
def rasterize_gaussians_batch(views, slots=None, raw=False, visibles=None, bindings=None, forward_only=False, depth_alpha=False):
    """K views through ONE launch chain (include/fr_rasterizer.h, fr_forward_batch): `views` is a list of the positional
    argument tuples of `rasterize_gaussians` (background ... debug), one per view; view k uses the device's handle
    `slots[k]` (default k).  Returns the list of `rasterize_gaussians` result tuples.  The results are those of K separate
    calls; what changes is that every kernel of the frame is launched once for all views.
    `bindings` (extension, fr_aux::binding): per view an `_lib.fr_binding` or None — the view's means3D / scales / rotations
    tensors are then OUTPUTS (written by the preprocess kernel from the mesh binding).  `forward_only` (extension,
    FR_FLAG_FORWARD_ONLY): every view is rendered without the backward's hand-off; never chosen here on its own.
    `depth_alpha` (extension, FR_FLAG_DEPTH_ALPHA): every view's result also holds depth, alpha and planesBuffer."""
    return [r.as_tuple() for r in _forward_batch(views, slots, raw, visibles, bindings, forward_only, depth_alpha)]


def _forward_batch(views, slots, raw, visibles, bindings, forward_only, depth_alpha) -> list:
    """`rasterize_gaussians_batch` with every view's result as its `_Forward` record."""
    K = len(views)
    if not 1 <= K <= _lib.FR_MAX_BATCH:
        raise RuntimeError(f"rasterize_gaussians_batch: 1 .. {_lib.FR_MAX_BATCH} views")
    slots = list(range(K)) if slots is None else [int(x) for x in slots]
    if len(set(slots)) != K:
        raise RuntimeError("rasterize_gaussians_batch: the views of a batch need a handle slot each")
    visibles = visibles or [None] * K
    bindings = bindings or [None] * K
    st = []
    for k, a in enumerate(views):
        if bindings[k] is not None and not all(t.is_contiguous() and t.dtype == torch.float32 for t in (a[1], a[4], a[5])):
            raise RuntimeError("rasterize_gaussians_batch: a bound view's means3D / scales / rotations are written in place")
        v = _forward_view(a, raw, visibles[k], bindings[k], forward_only, depth_alpha)
        if st and v["dev"] != st[0]["dev"]:
            raise RuntimeError("rasterize_gaussians_batch: the views of a batch live on one device")
        if v["prm"].P == 0:
            raise RuntimeError("rasterize_gaussians_batch: batched views need at least one Gaussian")
        st.append(v)
    return _launch_forward(st, slots, batch=True)


def rasterize_gaussians_backward_batch(views, slots=None, raw=False, wants=None, outs=None, stats=None, accumulates=None,
                                       bindings=None, bind_grads=None, planes=None, camera=None):
    """`rasterize_gaussians_backward` for K views in ONE launch chain (fr_backward_batch): `views` is a list of its
    positional argument tuples (background ... debug); `wants` / `outs` / `stats` / `accumulates`: per-view lists of the
    corresponding keyword arguments.  Returns the list of gradient tuples.  `bindings` / `bind_grads` (extension,
    fr_aux::binding): per view the descriptor the forward was given and a dict of the d_verts / d_offset / d_rotation /
    d_scaling tensors the kernel writes (d_verts: adds).  `planes` (FR_FLAG_DEPTH_ALPHA): per view the `_planes` tuple of
    `rasterize_gaussians_backward`; the views must agree on having one.  `camera` (FR_FLAG_CAMERA_GRAD): True, or per view
    the `_camera` argument of `rasterize_gaussians_backward`; all views or none."""
    K = len(views)
    if not 1 <= K <= _lib.FR_MAX_BATCH:
        raise RuntimeError(f"rasterize_gaussians_backward_batch: 1 .. {_lib.FR_MAX_BATCH} views")
    slots = list(range(K)) if slots is None else [int(x) for x in slots]
    wants, outs, stats, accumulates, bindings, bind_grads, planes = (x or [None] * K for x in (wants, outs, stats, accumulates,
                                                                                              bindings, bind_grads, planes))
    cameras = [camera] * K if camera is None or isinstance(camera, bool) else list(camera)
    if len(set(bool(c is not None and c is not False) for c in cameras)) != 1:
        raise RuntimeError("rasterize_gaussians_backward_batch: the views of a batch must agree on camera gradients")
    st = [_backward_view(a, raw, wants[k], outs[k], stats[k], tuple(accumulates[k] or ()), bindings[k], bind_grads[k],
                         "rasterize_gaussians_backward_batch", planes[k], cameras[k], slots[k]) for k, a in enumerate(views)]
    # fr_aux::overflow_out is OVERWRITTEN (0 or 1) by every backward: views of one launch that shared a word would race, and a
    # view that did not overflow could clear the flag of one that did (the optimizer would step on a partly zero gradient)
    words = [int(_stats3(stats[k])[2].data_ptr()) for k in range(K) if _stats3(stats[k])[2] is not None]
    if len(set(words)) != len(words):
        raise RuntimeError("rasterize_gaussians_backward_batch: the views of a batch need ONE overflow word EACH "
                           "(fused_densification_stats[2]); give every view its own statistics tuple")
    return _launch_backward(st, slots, batch=True)


class _RasterizeGaussiansBatch(torch.autograd.Function):
    """`_RasterizeGaussians` for K views rendered together.  Tensor arguments: per view the eight of `_RasterizeGaussians`
    (means3D ... cov3Ds_precomp), then — optionally — per view its settings' (viewmatrix, projmatrix, campos), which then
    receive gradients (`_camera_inputs`); outputs: per view those of `_SavedFrame`."""

    @staticmethod
    def forward(ctx, settings, raw_activations, slots, forward_only, depth_alpha, *tensors):
        K = len(settings)
        assert len(tensors) in (8 * K, 11 * K)
        ctx.raw, ctx.slots, ctx.camera = bool(raw_activations), slots, len(tensors) == 11 * K
        per_view = [tensors[8 * k:8 * k + 8] for k in range(K)]
        viss = [torch.empty((t[0].shape[0],), dtype=torch.bool, device=t[0].device) for t in per_view]
        res = _forward_batch([_forward_args(rs, *t) for rs, t in zip(settings, per_view)], slots, ctx.raw, viss, None,
                             forward_only, depth_alpha)
        return _SavedFrame.save(ctx, [
            _SavedFrame(rs, r, vis, means2D, _FrameGrads.of_frame(ctx.raw, means3D, sh, colors_precomp, opacities, scales,
                                                                  rotations, cov3Ds_precomp),
                        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, sh))
            for rs, r, vis, (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
            in zip(settings, res, viss, per_view)])

    @staticmethod
    def backward(ctx, *grad_outs):
        if not _any_grad(grad_outs):
            return (None,) * (5 + (11 if ctx.camera else 8) * len(ctx.frames))
        views, outs, planes = [], [], []
        for f, own, fw, g, pl in _SavedFrame.load(ctx, grad_outs):
            views.append(_backward_args(f.rs, own, fw, g))
            planes.append(pl)
            # (in-kernel accumulation across the views of ONE batch would race: a later view of the same parameters gets a
            # fresh tensor, which autograd adds)
            outs.append(f.grads.claim(accumulate=False)[0])
        res = rasterize_gaussians_backward_batch(views, slots=ctx.slots, raw=ctx.raw, wants=[f.grads.want for f in ctx.frames],
                                                 outs=outs, stats=[f.stats for f in ctx.frames],
                                                 planes=planes if ctx.frames[0].has_planes else None, camera=ctx.camera)
        return (None,) * 5 + tuple(t for grads in res for t in _input_grads(grads)) + \
            (tuple(t for f, grads in zip(ctx.frames, res) for t in _camera_grads(f.rs, grads)) if ctx.camera else ())


def rasterize_views_autograd(settings, per_view_tensors, raw_activations=False, slots=None, depth_alpha=False):
    """K views through one launch chain, differentiable: `settings` a list of GaussianRasterizationSettings,
    `per_view_tensors` a list of (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp) with
    empty tensors for what a view does not use.  Returns [(color, radii), ...], with `depth_alpha` (extension,
    FR_FLAG_DEPTH_ALPHA) [(color, radii, depth [1,H,W], alpha [1,H,W]), ...] (both planes differentiable)."""
    K = len(settings)
    flat = [t for v in per_view_tensors for t in v] + _camera_inputs_of(settings)
    out = _RasterizeGaussiansBatch.apply(list(settings), bool(raw_activations), list(range(K)) if slots is None else list(slots),
                                         _pick_forward_only(flat), bool(depth_alpha), *flat)
    return _per_view_outputs(out, K)


def mark_visible(means3D, viewmatrix, projmatrix):
    """`_C.mark_visible` (rasterize_points.cu:198-217)."""
    dev = _dev_index(means3D)
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=means3D.device)
    if P != 0:
        means3D, viewmatrix, projmatrix = _f32c(means3D, viewmatrix, projmatrix)
        _lib.launch("fr_mark_visible", dev, P, means3D.data_ptr(), viewmatrix.data_ptr(), projmatrix.data_ptr(), present.data_ptr())
    return present


def image_aux(imgBuffer: torch.Tensor, H: int, W: int):
    """(final_T[H,W] float32, n_contrib[H,W] int32) views into an image buffer: the per-pixel alpha channel
    (alpha = 1 - final_T; reference accum_alpha, forward.cu:369) and contributor count."""
    L = _lib.lib()
    base = imgBuffer.data_ptr()
    oT = L.fr_image_final_T(base, W, H) - base
    oN = L.fr_image_n_contrib(base, W, H) - base
    T = imgBuffer[oT:oT + 4 * H * W].view(torch.float32).view(H, W)
    N = imgBuffer[oN:oN + 4 * H * W].view(torch.int32).view(H, W)
    return T, N


def cpu_deep_copy_tuple(input_tuple):
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


def _snapshot_on_error(debug, dump, message, fn, args, **kw):
    """fn(*args, **kw); in debug mode a CPU copy of `args` is saved to `dump` if it raises (__init__.py:83-92, 132-141)."""
    if not debug:
        return fn(*args, **kw)
    cpu_args = cpu_deep_copy_tuple(args)
    try:
        return fn(*args, **kw)
    except Exception:
        torch.save(cpu_args, dump)
        print(message)
        raise


class GradOut:
    """A gradient slot a parameter tensor can carry as `tensor._fr_grad_out`: the rasterizer's backward writes the
    parameter's gradient straight into `buf` instead of allocating a tensor that autograd then copies or adds.
    The kernel OVERWRITES for the first backward after the parameter's .grad was cleared (forward() re-arms the slot
    when it sees `.grad is None`); any further backward gets a fresh tensor, which autograd adds — several renders
    from the same parameters, as model/fateavatar.py:251-276 does, accumulate correctly.

    Opt-in (`add_to_kept = True`, what FlatGaussians.accumulate_into_kept_grads() sets): a further backward is ADDED
    to the buffer by the kernel itself (FR_FLAG_ACCUMULATE) when that is provably where the parameter's gradient lives
    (`param.grad` is a view of `buf`: the gradients of an earlier `.backward()` were kept), and autograd is handed
    nothing for that parameter.  It is opt-in because the backward cannot tell `.backward()` from
    `torch.autograd.grad()`, which must not touch `param.grad`; and it never applies to the frames of ONE backward
    pass of a summed loss, whose first gradient still sits in autograd's input buffer (param.grad is None)."""

    def __init__(self, buf: torch.Tensor):
        self.buf = buf
        self.claimed = False
        self.add_to_kept = False

    @staticmethod
    def of(t):
        slot = getattr(t, "_fr_grad_out", None)
        if slot is None:
            return None
        if t.is_leaf and t.grad is None:
            slot.claimed = False   # gradients were cleared (zero_grad(set_to_none=True)): a new accumulation starts
        return slot

    def claim(self, param=None):
        """-> (buffer or None, accumulate)."""
        if not self.claimed:
            self.claimed = True
            return self.buf, False
        g = param.grad if (self.add_to_kept and param is not None and param.is_leaf) else None
        if (g is not None and g.data_ptr() == self.buf.data_ptr() and g.shape == self.buf.shape and g.is_contiguous()
                and g.dtype == self.buf.dtype):
            return self.buf, True
        return None, False


class _FrameGrads:
    """One frame's gradients as its autograd Function sees them: `want`, the names its backward computes, and the GradOut
    slots of its inputs (taken in the forward, claimed in the backward)."""

    def __init__(self, owners, sh, colors_precomp=None, cov3Ds_precomp=None, bound=False):
        """`owners`: gradient name -> the input tensor whose GradOut slot may receive it, or None.  `bound`: a frame rendered from
        its mesh binding, whose means3D / scales / rotations are kernel outputs (the kernel carries their gradients on to
        the binding's inputs)."""
        # gradients nobody can receive are not computed: dL_dcolors without colors_precomp, dL_dcov3D without
        # cov3D_precomp, dL_dsh without sh (the reference fills them in and autograd drops them)
        self.want = {"dL_dmeans2D", "dL_dopacity"} if bound else \
            {"dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dscales", "dL_drotations"}
        for k, t in (("dL_dcolors", colors_precomp), ("dL_dcov3D", cov3Ds_precomp), ("dL_dsh", sh)):
            if t is not None and t.numel():
                self.want.add(k)
        self.slots, self.owners = {}, {}
        for k, t in owners.items():
            slot = GradOut.of(t) if t is not None else None
            if slot is not None:
                self.slots[k] = slot
                if t.is_leaf:  # (leaves only: a reference to a non-leaf input from its own grad_fn's context would be a cycle)
                    self.owners[k] = t

    @staticmethod
    def of_frame(raw, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp):
        # optional extension: an input tensor may carry `_fr_grad_out`, a GradOut slot whose preallocated buffer
        # receives its gradient (zero-copy into e.g. a flat data-parallel gradient buffer)
        owners = {"dL_dmeans3D": means3D, "dL_dsh": sh if sh.numel() else None}
        if raw:  # raw parameters reach the kernels directly: their gradients can be written in place too
            owners.update(dL_dopacity=opacities, dL_dscales=scales, dL_drotations=rotations)
        return _FrameGrads(owners, sh, colors_precomp, cov3Ds_precomp)

    def claim(self, accumulate=True):
        """-> (outs, added): per slot the buffer the backward writes into (None: a fresh tensor), and the names the kernel
        ADDS to their buffer (only with `accumulate`; otherwise such a slot is left out).  The FIRST backward of a step may
        write a gradient straight into its slot's buffer; any further backward of the same step (several frames rendered
        from the same parameters) gets a fresh tensor, which autograd then adds to the first (see GradOut)."""
        outs, added = {}, []
        for k, slot in self.slots.items():
            buf, add = slot.claim(self.owners.get(k))
            if add and not accumulate:
                continue
            outs[k] = buf
            if add:
                added.append(k)
        return outs, tuple(added)


def _forward_args(rs, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp):
    """The positional arguments of `rasterize_gaussians` for a frame's eight tensor inputs, in the order of
    `_RasterizeGaussians.forward` (means2D is not one of them): diff_gaussian_rasterization/__init__.py:60-80."""
    return (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, rs.sh_degree, rs.campos,
            rs.prefiltered, rs.debug)


def _backward_args(rs, own, fw, grad_out_color):
    """The positional arguments of `rasterize_gaussians_backward` from what the forward saved — `own`: (colors_precomp,
    means3D, scales, rotations, cov3Ds_precomp, sh); `fw`: the frame's `_Forward` as `_SavedFrame.load` restores it:
    __init__.py:109-129."""
    colors_precomp, means3D, scales, rotations, cov3Ds_precomp, sh = own
    return (rs.bg, means3D, fw.radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
            rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, sh, rs.sh_degree, rs.campos, fw.geom, fw.num_rendered,
            fw.binning, fw.img, rs.debug)


_INPUT_GRADS = [(k, _GRAD_NAMES.index(k)) for k in ("dL_dmeans3D", "dL_dmeans2D", "dL_dsh", "dL_dcolors", "dL_dopacity",
                                                     "dL_dscales", "dL_drotations", "dL_dcov3D")]


def _camera_inputs(rs) -> tuple:
    """The settings' (viewmatrix, projmatrix, campos) as TENSOR inputs of the frame's autograd Function — only when autograd
    records and one of them requires grad (a `model.PoseCamera` built from leaves, a pose being refined); () otherwise, and the
    frame is then exactly the reference's: no flag, no extra launch."""
    cam = (rs.viewmatrix, rs.projmatrix, rs.campos)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in cam):
        return cam
    return ()


def _camera_inputs_of(settings) -> list:
    """`_camera_inputs` for the views of a batch, which share one launch chain: every view's three, or none."""
    cams = [_camera_inputs(rs) for rs in settings]
    return [t for rs in settings for t in (rs.viewmatrix, rs.projmatrix, rs.campos)] if any(cams) else []


def _camera_grads(rs, grads) -> tuple:
    """The last three results of a backward with `_camera` as the gradients of the settings' camera tensors."""
    return tuple(g.reshape(t.shape).to(t.dtype) for g, t in zip(grads[-3:], (rs.viewmatrix, rs.projmatrix, rs.campos)))


def _input_grads(grads, added=()):
    """The results of `rasterize_gaussians_backward` in the order of the frame's tensor inputs (means3D, means2D, sh,
    colors_precomp, opacities, scales, rotations, cov3Ds_precomp); None for the names in `added`, whose gradient is
    already in the parameter's .grad (nothing for autograd to add)."""
    return tuple([None if k in added else grads[i] for k, i in _INPUT_GRADS])


class _SavedFrame:
    """One view of a frame between its autograd Function's forward and backward (a list of them sits on `ctx.frames`): the
    ONE place that knows what a view returns to autograd — (color, radii), with planes (color, radii, depth [1,H,W],
    alpha [1,H,W]) — and what it saves — the Function's `own` tensors, then radii, geomBuffer, binningBuffer, imgBuffer and,
    with planes, planesBuffer.  It holds no tensor of the frame itself (an output kept on `ctx` would be a cycle)."""

    def __init__(self, rs, fw, visible, means2D, grads, own):
        """`visible`: the mask the preprocess kernel wrote (or None); `own`: the tensors the Function wants back in its backward."""
        # extension: the visibility mask (radii > 0) comes out of the preprocess kernel; render() picks it up from
        # `radii._fr_visible` instead of launching a compare kernel
        if visible is not None:
            fw.radii._fr_visible = visible
        # extension: `means2D._fr_densification_stats = (xyz_gradient_accum, denom)` makes the backward kernel
        # accumulate the densification statistics itself
        self.stats = getattr(means2D, "_fr_densification_stats", None)
        self.rs, self.grads, self.num_rendered, self.has_planes = rs, grads, fw.num_rendered, fw.planes is not None
        self._outputs = (fw.color, fw.radii) + ((fw.depth.unsqueeze(0), fw.alpha.unsqueeze(0)) if self.has_planes else ())
        self._saved = (*own, fw.radii, fw.geom, fw.binning, fw.img) + ((fw.planes,) if self.has_planes else ())
        self.n_own, self.n_saved, self.n_out = len(own), len(self._saved), len(self._outputs)

    @staticmethod
    def save(ctx, frames) -> tuple:
        """The end of a Function's forward: saves every view's tensors, marks the radii non-differentiable and returns
        the Function's outputs, view after view."""
        ctx.frames = frames
        # the gradient slot of the int32 `radii` output would otherwise be materialised as a zero tensor per backward
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*[t for f in frames for t in f._saved])
        outs = tuple(t for f in frames for t in f._outputs)
        ctx.mark_non_differentiable(*[f._outputs[1] for f in frames])
        for f in frames:
            del f._outputs, f._saved
        return outs

    @staticmethod
    def load(ctx, grad_outs):
        """The start of a Function's backward, view after view: (frame, its `own` tensors, its `_Forward` restored from the
        saved tensors (no color, depth, alpha), the image gradient, the `_planes` tuple (planesBuffer, dL_ddepth, dL_dalpha)
        or None)."""
        all_saved, s, o = ctx.saved_tensors, 0, 0
        for f in ctx.frames:
            saved, (g, _, *g_planes) = all_saved[s:s + f.n_saved], grad_outs[o:o + f.n_out]
            s, o = s + f.n_saved, o + f.n_out
            radii, geom, binning, img, *planes = saved[f.n_own:]
            if g is None:   # (this view's image was not differentiated, something else was: a zero image gradient)
                g = torch.zeros((NUM_CHANNELS, f.rs.image_height, f.rs.image_width), dtype=torch.float32, device=radii.device)
            yield (f, saved[:f.n_own], _Forward(f.num_rendered, None, radii, geom, binning, img, None, None, *planes), g,
                   (*planes, *g_planes) if f.has_planes else None)


def _any_grad(grad_outs) -> bool:
    """Whether anything of a Function's outputs was differentiated (if not, its backward returns None throughout)."""
    return any(g is not None for g in grad_outs)


def _per_view_outputs(outs, K) -> list:
    """A Function's flat outputs as one tuple per view (the K views of one Function agree on having planes)."""
    n = len(outs) // K
    return [tuple(outs[n * k:n * k + n]) for k in range(K)]


class _RasterizeGaussians(torch.autograd.Function):
    """diff_gaussian_rasterization/__init__.py:44-155.  Tensor arguments: (means3D, means2D, sh, colors_precomp, opacities,
    scales, rotations, cov3Ds_precomp), then raster_settings; outputs: those of `_SavedFrame`.  Optional trailing tensor
    inputs (extension): the settings' (viewmatrix, projmatrix, campos), which then receive gradients (`_camera_inputs`)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, raw_activations=False, forward_only=False, depth_alpha=False, viewmatrix=None,
                projmatrix=None, campos=None):
        rs = raster_settings
        ctx.raw = bool(raw_activations)
        ctx.camera = viewmatrix is not None   # (the three are rs.viewmatrix / projmatrix / campos: all or none)
        ctx.fr_slot = _slot   # the backward goes through the handle the forward used
        args = _forward_args(rs, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        vis = torch.empty((means3D.shape[0],), dtype=torch.bool, device=means3D.device) if means3D.is_cuda else None
        res = _snapshot_on_error(
            rs.debug, "snapshot_fw.dump", "\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.",
            rasterize_gaussians, args, _raw=ctx.raw, _visible=vis, _forward_only=forward_only, _depth_alpha=bool(depth_alpha))
        grads = _FrameGrads.of_frame(ctx.raw, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        return _SavedFrame.save(ctx, [_SavedFrame(rs, _Forward(*res), vis if means3D.shape[0] > 0 else None, means2D, grads,
                                                  (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, sh))])

    @staticmethod
    def backward(ctx, *grad_outs):
        if not _any_grad(grad_outs):
            return (None,) * 15
        (f, own, fw, grad_out_color, planes), = _SavedFrame.load(ctx, grad_outs)
        out, added = ({}, ()) if f.rs.debug else f.grads.claim()   # (debug mode claims no GradOut slot)
        with handle_slot(ctx.fr_slot):
            grads = _snapshot_on_error(
                f.rs.debug, "snapshot_bw.dump", "\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n",
                rasterize_gaussians_backward, _backward_args(f.rs, own, fw, grad_out_color), _out=out, _raw=ctx.raw,
                _stats=f.stats, _want=f.grads.want, _accumulate=added, _planes=planes, _camera=ctx.camera)
        # (autograd drops the surplus trailing None of a call with the reference's nine arguments)
        return _input_grads(grads, added) + (None,) * 4 + (_camera_grads(f.rs, grads) if ctx.camera else (None,) * 3)


def rasterize_gaussians_autograd(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                 raster_settings, raw_activations=False, depth_alpha=False):
    """`depth_alpha` (extension, FR_FLAG_DEPTH_ALPHA): (color, radii, depth, alpha) instead of (color, radii)."""
    cam = _camera_inputs(raster_settings)
    forward_only = _pick_forward_only((means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, *cam))
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, raw_activations, forward_only, depth_alpha, *cam)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class GaussianRasterizer(nn.Module):
    """diff_gaussian_rasterization/__init__.py:171-220."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            rs = self.raster_settings
            return mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, raw_activations=False, depth_alpha=False):
        """`raw_activations=True` (extension, not in the reference): opacities / scales / rotations are the RAW
        parameters; sigmoid / exp / normalize and their derivatives run inside the HIP kernels.  `depth_alpha=True`
        (extension, FR_FLAG_DEPTH_ALPHA): returns (color, radii, depth [1,H,W], alpha [1,H,W]) — depth = sum of z alpha T
        over the pixel's blended Gaussians (z: view-space depth; expected depth is depth / alpha), alpha = 1 - the final
        transmittance — both differentiable."""
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        empty = torch.Tensor([])
        if shs is None:
            shs = empty
        if colors_precomp is None:
            colors_precomp = empty
        if scales is None:
            scales = empty
        if rotations is None:
            rotations = empty
        if cov3D_precomp is None:
            cov3D_precomp = empty
        if raw_activations and (scales is None or scales.numel() == 0):
            raise Exception('raw_activations needs the scale/rotation pair')
        return rasterize_gaussians_autograd(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                            cov3D_precomp, rs, raw_activations, depth_alpha=depth_alpha)
