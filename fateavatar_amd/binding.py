"""FateAvatar's mesh binding as ONE fused op per direction.

reference: model/fateavatar.py:225-258 — face frame / scale / normal of the posed mesh
(volume_rendering/mesh_compute.py:27-59), barycentric point (volume_rendering/mesh_sampling.py:171-200),
pytorch3d's matrix_to_quaternion and quaternion_multiply, then
    gaussian._scaling  = _scaling + log(face_scale / face_scale_canonical)      (:256, cfg_model.resize_scale)
    gaussian._rotation = quaternion_multiply(face_quaternion, _rotation)         (:257)
    gaussian._xyz      = position + face_normal * shell_len * tanh(_offset)      (:258)
About forty PyTorch kernels (and their autograd twins) there; `bind_gaussians` is one HIP kernel forward and one
backward, differentiable w.r.t. verts (the delta blendshapes train through it), offset, rotation and scaling.

`bind_gaussians_face_local` is the same for GaussianAvatars' binding (model/baseline/gaussianavatars.py:144-171), the
reference's headline baseline: every Gaussian lives in the local frame of one triangle,
    gaussian._scaling  = _scaling + log(face_scaling[binding])
    gaussian._rotation = quaternion_multiply(normalize(matrix_to_quaternion(face_orien_mat))[binding], _rotation)
    gaussian._xyz      = (face_orien_mat[binding] @ _xyz) * face_scaling[binding] + face_center[binding]
The same two kernels (fr_binding::mode), differentiable w.r.t. verts, the local position, rotation and scaling.

`bind_gaussians_phong` is SplattingAvatar's binding (model/baseline/splattingavatar.py:203-246): every Gaussian is a point of
the posed mesh's Phong surface,
    gaussian._scaling  = _scaling * face_area_ratio[fidx]                                  (:244: the raw log-scale is multiplied)
    gaussian._rotation = quaternion_multiply(sum_k bary_k per_vert_quat[face[k]], _rotation)   (:235, :245)
    gaussian._xyz      = sum_k bary_k verts[face[k]] + normalize(sum_k bary_k vert_normal[face[k]]) * _uvd[:, 2]   (:224-233, :246)
`phong_canonical` holds what the mesh fixes once, `phong_frame` is the per-frame mesh pass (vertex normals, per-vertex
quaternions, face area ratios: ONE kernel without atomics where the reference runs pytorch3d's verts_normals_packed,
torch.inverse, matrix_to_quaternion and six index_add calls).  Differentiable w.r.t. uvd, rotation and scaling; the mode has no
gradient to the posed vertices.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib


def _chk(t, dtype, name):
    if not t.is_cuda:
        raise RuntimeError(f"bind_gaussians: {name} must be on a HIP device (there is no CPU path)")
    return t.to(dtype).contiguous()


def face_scale(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """compute_face_orientation(..., return_scale=True)[1] (mesh_compute.py:51-56) of one mesh: [F,1].  Used once, on
    the canonical mesh (model/fateavatar.py:84-85)."""
    verts, faces = _chk(verts, torch.float32, "verts"), _chk(faces, torch.int32, "faces")
    out = torch.empty((faces.shape[0], 1), dtype=torch.float32, device=verts.device)
    with torch.cuda.device(verts.device):
        rc = _lib.lib().fr_face_scale(verts.shape[0], faces.shape[0], verts.data_ptr(), faces.data_ptr(), out.data_ptr(),
                                      torch.cuda.current_stream(verts.device).cuda_stream)
    if rc != _lib.FR_OK:
        raise RuntimeError(f"fr_face_scale failed: {_lib.last_error()}")
    return out


def _desc(verts, faces, face_index, bary, canon, offset, rotation, scaling, shell_len, resize_scale):
    b = _lib.fr_binding()
    b.N, b.V, b.F = face_index.shape[0], verts.shape[0], faces.shape[0]
    b.verts, b.faces, b.face_index, b.bary = verts.data_ptr(), faces.data_ptr(), face_index.data_ptr(), bary.data_ptr()
    b.face_scale_canonical = canon.data_ptr() if canon is not None else None
    b.shell_len, b.resize_scale = float(shell_len), int(bool(resize_scale))
    b.offset, b.rotation, b.scaling = offset.data_ptr(), rotation.data_ptr(), scaling.data_ptr()
    return b


class _Bind(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, offset, rotation, scaling, faces, face_index, bary, canon, shell_len, resize_scale):
        verts, offset = _chk(verts, torch.float32, "verts"), _chk(offset, torch.float32, "offset")
        rotation, scaling = _chk(rotation, torch.float32, "rotation"), _chk(scaling, torch.float32, "scaling")
        faces, face_index = _chk(faces, torch.int32, "faces"), _chk(face_index, torch.int32, "face_index")
        bary = _chk(bary, torch.float32, "bary_coords")
        canon = _chk(canon, torch.float32, "face_scale_canonical") if canon is not None else None
        N, dev = face_index.shape[0], verts.device
        if verts.dim() != 2 or offset.numel() != N or rotation.shape != (N, 4) or scaling.shape != (N, 3) or bary.shape != (N, 3):
            raise RuntimeError("bind_gaussians: verts [V,3], offset [N,1], rotation [N,4], scaling [N,3], bary [N,3]")
        if resize_scale and (canon is None or canon.numel() != faces.shape[0]):
            raise RuntimeError("bind_gaussians: resize_scale needs face_scale_canonical [F,1]")
        xyz = torch.empty((N, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((N, 4), dtype=torch.float32, device=dev)
        scl = torch.empty((N, 3), dtype=torch.float32, device=dev)
        b = _desc(verts, faces, face_index, bary, canon, offset, rotation, scaling, shell_len, resize_scale)
        with torch.cuda.device(dev):
            rc = _lib.lib().fr_bind_forward(C.byref(b), xyz.data_ptr(), rot.data_ptr(), scl.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
        if rc != _lib.FR_OK:
            raise RuntimeError(f"fr_bind_forward failed: {_lib.last_error()}")
        ctx.save_for_backward(verts, offset, rotation, scaling, faces, face_index, bary, canon)
        ctx.consts = (float(shell_len), bool(resize_scale), offset.shape)
        # optional extension (see rasterizer.GradOut): a raw parameter may carry `_fr_grad_out`, a slot whose preallocated
        # buffer (a view into a flat gradient buffer) receives its gradient without a copy
        from .rasterizer import GradOut
        ctx.grad_slots = (GradOut.of(offset), GradOut.of(rotation), GradOut.of(scaling))
        return xyz, rot, scl

    @staticmethod
    def backward(ctx, g_xyz, g_rot, g_scl):
        verts, offset, rotation, scaling, faces, face_index, bary, canon = ctx.saved_tensors
        shell_len, resize_scale, offset_shape = ctx.consts
        dev, N = verts.device, face_index.shape[0]
        need_v, need_o, need_r, need_s = ctx.needs_input_grad[:4]
        c = lambda g: g.contiguous().float() if g is not None else None  # noqa: E731
        g_xyz, g_rot, g_scl = c(g_xyz), c(g_rot), c(g_scl)
        d_verts = torch.zeros_like(verts) if need_v else None

        def out(need, slot, shape):
            if not need:
                return None
            buf = slot.claim()[0] if slot is not None else None   # first backward of the step writes the slot in place
            if buf is not None and buf.numel() == int(torch.Size(shape).numel()) and buf.is_contiguous():
                return buf.view(shape)
            return torch.empty(shape, dtype=torch.float32, device=dev)

        d_off = out(need_o, ctx.grad_slots[0], (N,))
        d_rot = out(need_r, ctx.grad_slots[1], (N, 4))
        d_scl = out(need_s, ctx.grad_slots[2], (N, 3))
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        b = _desc(verts, faces, face_index, bary, canon, offset, rotation, scaling, shell_len, resize_scale)
        with torch.cuda.device(dev):
            rc = _lib.lib().fr_bind_backward(C.byref(b), p(g_xyz), p(g_rot), p(g_scl), p(d_verts), p(d_off), p(d_rot), p(d_scl),
                                             torch.cuda.current_stream(dev).cuda_stream)
        if rc != _lib.FR_OK:
            raise RuntimeError(f"fr_bind_backward failed: {_lib.last_error()}")
        return (d_verts, d_off.view(offset_shape) if d_off is not None else None, d_rot, d_scl, None, None, None, None, None,
                None)


def bind_gaussians(verts, faces, face_index, bary_coords, face_scale_canonical, offset, rotation, scaling,
                   shell_len: float, resize_scale: bool = True):
    """One frame of model/fateavatar.py:225-258.  verts [V,3] (posed), faces [F,3], face_index [N], bary_coords [N,3],
    face_scale_canonical [F,1] (`face_scale` of the canonical mesh), raw offset [N,1] / rotation [N,4] / scaling [N,3].
    Returns (xyz [N,3], rotation [N,4], scaling [N,3]): the values the reference assigns to gaussian._xyz /
    gaussian._rotation / gaussian._scaling before render()."""
    return _Bind.apply(verts, offset, rotation, scaling, faces, face_index, bary_coords, face_scale_canonical, shell_len,
                       resize_scale)


def _desc_local(verts, faces, binding, local_xyz, rotation, scaling):
    b = _lib.fr_binding()   # (zero-filled: bary, offset, face_scale_canonical, shell_len, resize_scale are not read in this mode)
    b.N, b.V, b.F = binding.shape[0], verts.shape[0], faces.shape[0]
    b.verts, b.faces, b.face_index = verts.data_ptr(), faces.data_ptr(), binding.data_ptr()
    b.rotation, b.scaling = rotation.data_ptr(), scaling.data_ptr()
    b.mode, b.local_xyz = _lib.FR_BIND_FACE_LOCAL, local_xyz.data_ptr()
    return b


class _BindFaceLocal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, local_xyz, rotation, scaling, faces, binding):
        verts, local_xyz = _chk(verts, torch.float32, "verts"), _chk(local_xyz, torch.float32, "local_xyz")
        rotation, scaling = _chk(rotation, torch.float32, "rotation"), _chk(scaling, torch.float32, "scaling")
        faces, binding = _chk(faces, torch.int32, "faces"), _chk(binding, torch.int32, "binding")
        N, dev = binding.shape[0], verts.device
        if verts.dim() != 2 or local_xyz.shape != (N, 3) or rotation.shape != (N, 4) or scaling.shape != (N, 3):
            raise RuntimeError("bind_gaussians_face_local: verts [V,3], binding [N], local_xyz [N,3], rotation [N,4], scaling [N,3]")
        xyz = torch.empty((N, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((N, 4), dtype=torch.float32, device=dev)
        scl = torch.empty((N, 3), dtype=torch.float32, device=dev)
        b = _desc_local(verts, faces, binding, local_xyz, rotation, scaling)
        with torch.cuda.device(dev):
            rc = _lib.lib().fr_bind_forward(C.byref(b), xyz.data_ptr(), rot.data_ptr(), scl.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
        if rc != _lib.FR_OK:
            raise RuntimeError(f"fr_bind_forward failed: {_lib.last_error()}")
        ctx.save_for_backward(verts, local_xyz, rotation, scaling, faces, binding)
        from .rasterizer import GradOut   # (the `_fr_grad_out` extension, as _Bind)
        ctx.grad_slots = (GradOut.of(local_xyz), GradOut.of(rotation), GradOut.of(scaling))
        return xyz, rot, scl

    @staticmethod
    def backward(ctx, g_xyz, g_rot, g_scl):
        verts, local_xyz, rotation, scaling, faces, binding = ctx.saved_tensors
        dev, N = verts.device, binding.shape[0]
        need_v, need_l, need_r, need_s = ctx.needs_input_grad[:4]
        c = lambda g: g.contiguous().float() if g is not None else None  # noqa: E731
        g_xyz, g_rot, g_scl = c(g_xyz), c(g_rot), c(g_scl)
        d_verts = torch.zeros_like(verts) if need_v else None

        def out(need, slot, shape):
            if not need:
                return None
            buf = slot.claim()[0] if slot is not None else None   # first backward of the step writes the slot in place
            if buf is not None and buf.numel() == int(torch.Size(shape).numel()) and buf.is_contiguous():
                return buf.view(shape)
            return torch.empty(shape, dtype=torch.float32, device=dev)

        d_loc = out(need_l, ctx.grad_slots[0], (N, 3))
        d_rot = out(need_r, ctx.grad_slots[1], (N, 4))
        d_scl = out(need_s, ctx.grad_slots[2], (N, 3))
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        b = _desc_local(verts, faces, binding, local_xyz, rotation, scaling)
        with torch.cuda.device(dev):
            rc = _lib.lib().fr_bind_backward_local(C.byref(b), p(g_xyz), p(g_rot), p(g_scl), p(d_verts), p(d_loc), p(d_rot),
                                                   p(d_scl), torch.cuda.current_stream(dev).cuda_stream)
        if rc != _lib.FR_OK:
            raise RuntimeError(f"fr_bind_backward_local failed: {_lib.last_error()}")
        return d_verts, d_loc, d_rot, d_scl, None, None


def bind_gaussians_face_local(verts, faces, binding, local_xyz, rotation, scaling):
    """One frame of model/baseline/gaussianavatars.py:144-171.  verts [V,3] (posed), faces [F,3], binding [N] (the face of
    every Gaussian), raw local_xyz [N,3] / rotation [N,4] / scaling [N,3].  Returns (xyz [N,3], rotation [N,4],
    scaling [N,3]): the values the reference assigns to gaussian._xyz / gaussian._rotation / gaussian._scaling before
    render()."""
    return _BindFaceLocal.apply(verts, local_xyz, rotation, scaling, faces, binding)


class PhongCanonical(NamedTuple):
    """What SplattingAvatar's binding keeps per MESH (PerVertQuaternion.prepare_cano_per_vert,
    model/baseline/splattingavatar.py:825-844) plus the vertex -> face incidence list `phong_frame` gathers by."""
    cano_verts: torch.Tensor      # [V,3] float32
    faces: torch.Tensor           # [F,3] int32
    vf_offsets: torch.Tensor      # [V+1] int32: CSR rows, the faces of every vertex ...
    vf_faces: torch.Tensor        # [3F]  int32: ... ascending within a row
    face_area: torch.Tensor       # [F]   float32: calc_face_areas of the canonical mesh (:781-791)


def phong_canonical(cano_verts: torch.Tensor, faces: torch.Tensor) -> PhongCanonical:
    """The once-per-mesh side of the Phong-surface binding, in plain torch on the tensors' device (CPU tensors are fine; move
    the result with `PhongCanonical(*[t.to(device) for t in c])`)."""
    cano = cano_verts.detach().to(torch.float32).contiguous()
    f = faces.detach().to(torch.int64)
    V, F = int(cano.shape[0]), int(f.shape[0])
    if cano.dim() != 2 or cano.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise RuntimeError("phong_canonical: cano_verts [V,3], faces [F,3]")
    if F and (int(f.min()) < 0 or int(f.max()) >= V):
        raise ValueError("phong_canonical: `faces` names a vertex the mesh does not have")
    # incidence list: the (vertex, face) pairs sorted by vertex, then by face (a face with a repeated corner is listed once
    # per corner, as the reference's three index_add calls add it)
    corner = f.reshape(-1)
    face_of = torch.arange(F, device=f.device).repeat_interleave(3)
    order = torch.argsort(corner * max(F, 1) + face_of)
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=f.device)
    offsets[1:] = torch.cumsum(torch.bincount(corner, minlength=V), dim=0)
    tri = cano[f]
    area = torch.linalg.cross(tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 1], dim=1).norm(dim=-1) / 2.0
    return PhongCanonical(cano, f.to(torch.int32).contiguous(), offsets.to(torch.int32), face_of[order].to(torch.int32).contiguous(),
                          area.contiguous())


def phong_frame(canonical: PhongCanonical, verts: torch.Tensor):
    """One frame of model/baseline/splattingavatar.py:203-215 for the posed `verts` [V,3]: (vert_normals [V,3],
    vert_quats [V,4], face_ratio [F]) — one launch on the current stream, the same bits on every call.  Not differentiable."""
    c = canonical
    verts = _chk(verts.detach(), torch.float32, "verts")
    V, F, dev = c.cano_verts.shape[0], c.faces.shape[0], verts.device
    if verts.shape != (V, 3):
        raise RuntimeError(f"phong_frame: verts must be [{V},3] like the canonical mesh")
    cano, faces = _chk(c.cano_verts, torch.float32, "cano_verts"), _chk(c.faces, torch.int32, "faces")
    off, ids = _chk(c.vf_offsets, torch.int32, "vf_offsets"), _chk(c.vf_faces, torch.int32, "vf_faces")
    area = _chk(c.face_area, torch.float32, "face_area")
    if off.numel() != V + 1 or ids.numel() != 3 * F or area.numel() != F:
        raise RuntimeError("phong_frame: the canonical data does not belong to this mesh")
    vn = torch.empty((V, 3), dtype=torch.float32, device=dev)
    vq = torch.empty((V, 4), dtype=torch.float32, device=dev)
    ratio = torch.empty((F,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().fr_phong_frame(V, F, verts.data_ptr(), cano.data_ptr(), faces.data_ptr(), off.data_ptr(), ids.data_ptr(),
                                       area.data_ptr(), vn.data_ptr(), vq.data_ptr(), ratio.data_ptr(),
                                       torch.cuda.current_stream(dev).cuda_stream)
    if rc != _lib.FR_OK:
        raise RuntimeError(f"fr_phong_frame failed: {_lib.last_error()}")
    return vn, vq, ratio


def _desc_phong(verts, faces, face_index, bary, frame, uvd, rotation, scaling):
    vn, vq, ratio = frame
    p = _lib.fr_binding_phong()   # (zero-filled: offset, face_scale_canonical, shell_len, resize_scale are not read in this mode)
    b = p.base
    b.N, b.V, b.F = face_index.shape[0], verts.shape[0], faces.shape[0]
    b.verts, b.faces, b.face_index, b.bary = verts.data_ptr(), faces.data_ptr(), face_index.data_ptr(), bary.data_ptr()
    b.rotation, b.scaling = rotation.data_ptr(), scaling.data_ptr()
    b.mode, b.local_xyz = _lib.FR_BIND_PHONG, uvd.data_ptr()
    p.vert_normals, p.vert_quats, p.face_ratio = vn.data_ptr(), vq.data_ptr(), ratio.data_ptr()
    return p.as_binding()   # (an fr_binding over the extended descriptor's memory: every caller passes it on as before)


def _chk_phong_frame(frame, V, F, who):
    vn, vq, ratio = (_chk(t, torch.float32, n) for t, n in zip(frame, ("vert_normals", "vert_quats", "face_ratio")))
    if vn.shape != (V, 3) or vq.shape != (V, 4) or ratio.numel() != F:
        raise RuntimeError(f"{who}: vert_normals [V,3], vert_quats [V,4], face_ratio [F] (`phong_frame` of the posed mesh)")
    return vn, vq, ratio


class _BindPhong(torch.autograd.Function):
    @staticmethod
    def forward(ctx, uvd, rotation, scaling, verts, faces, face_index, bary, vn, vq, ratio):
        verts, uvd = _chk(verts, torch.float32, "verts"), _chk(uvd, torch.float32, "uvd")
        rotation, scaling = _chk(rotation, torch.float32, "rotation"), _chk(scaling, torch.float32, "scaling")
        faces, face_index = _chk(faces, torch.int32, "faces"), _chk(face_index, torch.int32, "face_index")
        bary = _chk(bary, torch.float32, "bary_coords")
        N, dev = face_index.shape[0], verts.device
        if verts.dim() != 2 or uvd.shape != (N, 3) or rotation.shape != (N, 4) or scaling.shape != (N, 3) or bary.shape != (N, 3):
            raise RuntimeError("bind_gaussians_phong: verts [V,3], face_index [N], bary [N,3], uvd [N,3], rotation [N,4], scaling [N,3]")
        frame = _chk_phong_frame((vn, vq, ratio), verts.shape[0], faces.shape[0], "bind_gaussians_phong")
        xyz = torch.empty((N, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((N, 4), dtype=torch.float32, device=dev)
        scl = torch.empty((N, 3), dtype=torch.float32, device=dev)
        b = _desc_phong(verts, faces, face_index, bary, frame, uvd, rotation, scaling)
        with torch.cuda.device(dev):
            rc = _lib.lib().fr_bind_forward(C.byref(b), xyz.data_ptr(), rot.data_ptr(), scl.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
        if rc != _lib.FR_OK:
            raise RuntimeError(f"fr_bind_forward failed: {_lib.last_error()}")
        ctx.save_for_backward(verts, uvd, rotation, scaling, faces, face_index, bary, *frame)
        from .rasterizer import GradOut   # (the `_fr_grad_out` extension, as _Bind)
        ctx.grad_slots = (GradOut.of(uvd), GradOut.of(rotation), GradOut.of(scaling))
        return xyz, rot, scl

    @staticmethod
    def backward(ctx, g_xyz, g_rot, g_scl):
        verts, uvd, rotation, scaling, faces, face_index, bary, vn, vq, ratio = ctx.saved_tensors
        dev, N = verts.device, face_index.shape[0]
        need_u, need_r, need_s = ctx.needs_input_grad[:3]
        c = lambda g: g.contiguous().float() if g is not None else None  # noqa: E731
        g_xyz, g_rot, g_scl = c(g_xyz), c(g_rot), c(g_scl)

        def out(need, slot, shape):
            if not need:
                return None
            buf = slot.claim()[0] if slot is not None else None   # first backward of the step writes the slot in place
            if buf is not None and buf.numel() == int(torch.Size(shape).numel()) and buf.is_contiguous():
                return buf.view(shape)
            return torch.empty(shape, dtype=torch.float32, device=dev)

        d_uvd = out(need_u, ctx.grad_slots[0], (N, 3))
        d_rot = out(need_r, ctx.grad_slots[1], (N, 4))
        d_scl = out(need_s, ctx.grad_slots[2], (N, 3))
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        b = _desc_phong(verts, faces, face_index, bary, (vn, vq, ratio), uvd, rotation, scaling)
        with torch.cuda.device(dev):
            rc = _lib.lib().fr_bind_backward_phong(C.byref(b), p(g_xyz), p(g_rot), p(g_scl), None, p(d_uvd), p(d_rot), p(d_scl),
                                                   torch.cuda.current_stream(dev).cuda_stream)
        if rc != _lib.FR_OK:
            raise RuntimeError(f"fr_bind_backward_phong failed: {_lib.last_error()}")
        return d_uvd, d_rot, d_scl, None, None, None, None, None, None, None


def _no_vertex_gradient(verts, who):
    if isinstance(verts, torch.Tensor) and verts.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{who}: the Phong-surface binding has no vertex gradient (the per-frame mesh pass is not "
                           "differentiable); hand it `verts.detach()`")


def bind_gaussians_phong(verts, faces, face_index, bary_coords, frame, uvd, rotation, scaling):
    """One frame of model/baseline/splattingavatar.py:224-246.  verts [V,3] (posed), faces [F,3], face_index [N],
    bary_coords [N,3], `frame` = `phong_frame(canonical, verts)` of the same posed mesh, raw uvd [N,3] / rotation [N,4] /
    scaling [N,3].  Returns (xyz [N,3], rotation [N,4], scaling [N,3]): the values the reference assigns to gaussian._xyz /
    gaussian._rotation / gaussian._scaling before render().  Only the third column of uvd is read; the first two columns of its
    gradient are zeros (the reference's forward likewise: they only steer its CPU triangle walk)."""
    _no_vertex_gradient(verts, "bind_gaussians_phong")
    vn, vq, ratio = frame
    return _BindPhong.apply(uvd, rotation, scaling, verts, faces, face_index, bary_coords, vn, vq, ratio)
