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
torch.inverse, matrix_to_quaternion and six index_add calls).  Differentiable w.r.t. uvd, rotation and scaling; and, on a frame
made with `phong_frame(..., differentiable=True)`, w.r.t. the posed vertices through all four routes of the reference's forward
(`phong_frame_backward`, `phong_scatter_frame_grads`, `PhongGradBuffers`; with a detached frame a vertex gradient is refused).

`bind_gaussians_deform` is FlashAvatar's binding (model/baseline/flashavatar.py:242-276): the barycentric point moved, turned and
stretched by the ten outputs of a deformation MLP, with t = tanh(deform),
    gaussian._scaling  = _scaling * exp(t[:, 7:10])                                        (:272: the raw log-scale is multiplied)
    gaussian._rotation = quatProduct_batch(_rotation, (exp(t[:, 3]), t[:, 4:7]))           (:273, :380-390: no sign standardisation)
    gaussian._xyz      = sum_k bary_k verts[face[k]] + t[:, 0:3]                           (:262-267, :274)
The MLP stays the caller's stock PyTorch; the op is differentiable w.r.t. verts, deform, rotation and scaling.

`mesh_laplacian` is the once-per-mesh side of FateAvatar's Laplacian-smoothing term (train/loss.py:112-121,166-180): pytorch3d's
`Meshes.laplacian_packed()` as a CSR adjacency for `loss.mesh_terms_and_grad` / `loss.laplacian_smoothing_loss`.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib
from .rasterizer import GradOut


def _chk(t, dtype, name):
    if not t.is_cuda:
        raise RuntimeError(f"bind_gaussians: {name} must be on a HIP device (there is no CPU path)")
    return t.to(dtype).contiguous()


def face_scale(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """compute_face_orientation(..., return_scale=True)[1] (mesh_compute.py:51-56) of one mesh: [F,1].  Used once, on
    the canonical mesh (model/fateavatar.py:84-85)."""
    verts, faces = _chk(verts, torch.float32, "verts"), _chk(faces, torch.int32, "faces")
    out = torch.empty((faces.shape[0], 1), dtype=torch.float32, device=verts.device)
    _lib.launch("fr_face_scale", verts.device, verts.shape[0], faces.shape[0], verts.data_ptr(), faces.data_ptr(), out.data_ptr())
    return out


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


def triangle_neighbours(faces: torch.Tensor) -> torch.Tensor:
    """The edge neighbour table of the walk on the mesh (initTriangleNeighbor, submodules/simple_phongsurf/simple_phongsurf/
    src/triangle_walk.cpp:176-237), once per mesh, in plain torch on the tensor's device: int32 [F,3]; entry [f, j] describes
    the directed edge faces[f,j] -> faces[f,(j+1)%3] and holds 4 g + k of the face g and edge k that carry the reversed
    directed edge, or -1 if there is none (a boundary edge).  Defined for meshes in which every directed edge occurs at most
    once: ValueError otherwise (the reference's std::map silently keeps the last duplicate)."""
    f = faces.detach().to(torch.int64)
    if f.dim() != 2 or f.shape[1] != 3:
        raise RuntimeError("triangle_neighbours: faces [F,3]")
    F = int(f.shape[0])
    if F == 0:
        return torch.zeros((0, 3), dtype=torch.int32, device=f.device)
    if int(f.min()) < 0:
        raise ValueError("triangle_neighbours: negative vertex index")
    a, b = f.reshape(-1), f.roll(-1, dims=1).reshape(-1)          # edge 3 f + j runs a -> b
    V = int(f.max()) + 1
    key, rev = a * V + b, b * V + a
    skey, order = torch.sort(key)
    if bool((skey[1:] == skey[:-1]).any()):
        raise ValueError("triangle_neighbours: a directed edge occurs more than once (the mesh is not an oriented manifold)")
    pos = torch.searchsorted(skey, rev).clamp(max=3 * F - 1)
    found = skey[pos] == rev
    other = order[pos]                                            # = 3 g + k
    out = torch.where(found, 4 * (other // 3) + other % 3, torch.full_like(other, -1))
    return out.reshape(F, 3).to(torch.int32).contiguous()


class MeshLaplacian(NamedTuple):
    """The uniform Laplacian of a mesh as a CSR adjacency (`mesh_laplacian`): row i lists the neighbours of vertex i in
    ascending order; L[i,j] = 1 / deg(i) for a neighbour j, L[i,i] = -1 for every vertex."""
    row_ptr: torch.Tensor         # [V+1] int32
    col: torch.Tensor             # [nnz] int32
    V: int

    def to_dense(self, dtype=torch.float32) -> torch.Tensor:
        """The V x V matrix the reference applies (`meshes.laplacian_packed().to_dense()`), on the arrays' device."""
        rp, V = self.row_ptr.long(), int(self.V)
        deg = rp[1:] - rp[:-1]
        row = torch.repeat_interleave(torch.arange(V, device=rp.device), deg)
        L = torch.zeros((V, V), dtype=dtype, device=rp.device)
        L[row, self.col.long()] = (1.0 / deg.to(dtype))[row]
        L[torch.arange(V), torch.arange(V)] = -1.0
        return L


def mesh_laplacian(faces: torch.Tensor, V: int) -> MeshLaplacian:
    """pytorch3d 0.7.7's `Meshes.laplacian_packed()` (`pytorch3d.ops.laplacian`, the uniform Laplacian the reference's
    get_laplacian_smoothing_loss densifies, train/loss.py:166-180) as a CSR adjacency, once per mesh, in plain torch on the
    faces' device.  The edges are the UNIQUE undirected pairs {a, b}, a != b, among the faces' three sides (a face listed
    twice or in both windings adds nothing; a side with a repeated corner is no edge), deg(i) the number of distinct
    neighbours of vertex i; a vertex no face uses has an empty row.  `faces` naming a vertex outside 0 .. V-1: ValueError —
    the kernel that reads the result (`loss.mesh_terms_and_grad`) cannot check it."""
    f = faces.detach().to(torch.int64)
    V = int(V)
    if f.dim() != 2 or f.shape[1] != 3 or V < 0:
        raise RuntimeError("mesh_laplacian: faces [F,3], V >= 0")
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= V):
        raise ValueError("mesh_laplacian: `faces` names a vertex the mesh does not have")
    a, b = f.reshape(-1), f.roll(-1, dims=1).reshape(-1)
    keep = a != b
    lo, hi = torch.minimum(a, b)[keep], torch.maximum(a, b)[keep]
    key = torch.unique(lo * max(V, 1) + hi)                       # the undirected edges, once each
    lo, hi = key // max(V, 1), key % max(V, 1)
    both = torch.sort(torch.cat([lo * max(V, 1) + hi, hi * max(V, 1) + lo])).values   # (row, col) ascending
    row, col = both // max(V, 1), both % max(V, 1)
    if both.numel() >= 2 ** 31:
        raise ValueError("mesh_laplacian: more than 2^31 - 1 non-zeros")
    row_ptr = torch.zeros(V + 1, dtype=torch.int64, device=f.device)
    row_ptr[1:] = torch.cumsum(torch.bincount(row, minlength=V), dim=0)
    return MeshLaplacian(row_ptr.to(torch.int32).contiguous(), col.to(torch.int32).contiguous(), V)


def _phong_mesh_args(c, V, who):
    """The canonical data as `fr_phong_frame` / `fr_phong_frame_backward` take it, checked against the mesh's sizes."""
    F = c.faces.shape[0]
    cano, faces = _chk(c.cano_verts, torch.float32, "cano_verts"), _chk(c.faces, torch.int32, "faces")
    off, ids = _chk(c.vf_offsets, torch.int32, "vf_offsets"), _chk(c.vf_faces, torch.int32, "vf_faces")
    area = _chk(c.face_area, torch.float32, "face_area")
    if cano.shape != (V, 3) or off.numel() != V + 1 or ids.numel() != 3 * F or area.numel() != F:
        raise RuntimeError(f"{who}: the canonical data does not belong to this mesh")
    return cano, faces, off, ids, area


def phong_frame_backward(canonical: PhongCanonical, verts, d_vert_normals, d_vert_quats, d_face_ratio, d_verts, workspace=None):
    """The backward of `phong_frame` (`fr_phong_frame_backward`): dLoss/dverts of the mesh pass ADDED onto `d_verts` [V,3]
    (float32, contiguous, on the device) from the gradients of its three outputs (each may be None: zero).  Two launches on
    the current stream, no float atomics: the same bits on every call and graph replay.  `workspace`: a preallocated uint8
    buffer of `phong_frame_backward_workspace_bytes(V, F)` bytes (for a captured step), or None."""
    V, F, dev = canonical.cano_verts.shape[0], canonical.faces.shape[0], d_verts.device
    verts = _chk(verts.detach(), torch.float32, "verts")
    if verts.shape != (V, 3) or d_verts.shape != (V, 3) or d_verts.dtype != torch.float32 or not d_verts.is_contiguous():
        raise RuntimeError(f"phong_frame_backward: verts and d_verts must be [{V},3] float32 like the canonical mesh")
    cano, faces, off, ids, area = _phong_mesh_args(canonical, V, "phong_frame_backward")
    ups = []
    for t, shape, name in ((d_vert_normals, (V, 3), "d_vert_normals"), (d_vert_quats, (V, 4), "d_vert_quats"),
                           (d_face_ratio, (F,), "d_face_ratio")):
        if t is not None:
            t = _chk(t.detach(), torch.float32, name)
            if t.numel() != int(torch.Size(shape).numel()):
                raise RuntimeError(f"phong_frame_backward: {name} must be {list(shape)}")
        ups.append(t)
    need = phong_frame_backward_workspace_bytes(V, F)
    if workspace is None:
        workspace = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < need or not workspace.is_cuda:
        raise RuntimeError(f"phong_frame_backward: the workspace must hold {need} bytes on the device")
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.launch("fr_phong_frame_backward", dev, V, F, verts.data_ptr(), cano.data_ptr(), faces.data_ptr(), off.data_ptr(),
                ids.data_ptr(), area.data_ptr(), p(ups[0]), p(ups[1]), p(ups[2]), d_verts.data_ptr(), workspace.data_ptr())
    return d_verts


def phong_frame_backward_workspace_bytes(V: int, F: int) -> int:
    return int(_lib.lib().fr_phong_frame_backward_workspace_bytes(int(V), int(F)))


class PhongGradBuffers:
    """What the vertex gradient of ONE posed mesh is formed in, allocated once: d_verts [V,3], the gradients of `phong_frame`'s
    three arrays (d_vert_normals [V,3], d_vert_quats [V,4], d_face_ratio [F]) as views of one flat buffer — one zeroing launch
    — and the workspace of `phong_frame_backward`.  A captured step keeps one; hung on a posed-vertex tensor as
    `_fr_phong_grad`, `render_bound_batch` with a `PosedPhongBinding` uses it instead of allocating."""

    def __init__(self, V: int, F: int, device, zeroed: bool = False):
        self.V, self.F = int(V), int(F)
        n = [3 * self.V, 3 * self.V, 4 * self.V, self.F]
        self.flat = (torch.zeros if zeroed else torch.empty)((sum(n),), dtype=torch.float32, device=device)
        a, b, c, d = torch.split(self.flat, n)
        self.d_verts, self.d_vert_normals, self.d_vert_quats, self.d_face_ratio = a.view(V, 3), b.view(V, 3), c.view(V, 4), d
        self.workspace = torch.empty((max(phong_frame_backward_workspace_bytes(V, F), 1),), dtype=torch.uint8, device=device)

    def zero_(self):
        self.flat.zero_()

    def check(self, V, F, device):
        if (self.V, self.F) != (int(V), int(F)) or self.flat.device != torch.device(device):
            raise RuntimeError(f"PhongGradBuffers: made for V = {self.V}, F = {self.F} on {self.flat.device}")


class _PhongFrame(torch.autograd.Function):
    """`phong_frame(differentiable=True)`: fr_phong_frame, and fr_phong_frame_backward for the posed vertices."""

    @staticmethod
    def forward(ctx, verts, *canonical):
        c = PhongCanonical(*canonical)
        out = phong_frame(c, verts)
        ctx.save_for_backward(verts, *canonical)
        return out

    @staticmethod
    def backward(ctx, d_vn, d_vq, d_ratio):
        verts, *canonical = ctx.saved_tensors
        d_verts = torch.zeros(verts.shape, dtype=torch.float32, device=verts.device)
        phong_frame_backward(PhongCanonical(*canonical), verts, d_vn, d_vq, d_ratio, d_verts)
        return (d_verts.to(verts.dtype), *([None] * len(canonical)))


def phong_frame(canonical: PhongCanonical, verts: torch.Tensor, differentiable: bool = False):
    """One frame of model/baseline/splattingavatar.py:203-215 for the posed `verts` [V,3]: (vert_normals [V,3],
    vert_quats [V,4], face_ratio [F]) — one launch on the current stream, the same bits on every call.  By default the
    outputs are detached from `verts`.  `differentiable=True`: the same values on autograd; their backward is
    `phong_frame_backward` (the reference's autograd through verts_normals_packed, PerVertQuaternion and
    calc_face_area_change), and `bind_gaussians_phong` on them carries dLoss/dverts."""
    if differentiable:
        return _PhongFrame.apply(verts, *canonical)
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
    _lib.launch("fr_phong_frame", dev, V, F, verts.data_ptr(), cano.data_ptr(), faces.data_ptr(), off.data_ptr(), ids.data_ptr(),
                area.data_ptr(), vn.data_ptr(), vq.data_ptr(), ratio.data_ptr())
    return vn, vq, ratio


def _chk_phong_frame(frame, V, F, who):
    vn, vq, ratio = (_chk(t, torch.float32, n) for t, n in zip(frame, ("vert_normals", "vert_quats", "face_ratio")))
    if vn.shape != (V, 3) or vq.shape != (V, 4) or ratio.numel() != F:
        raise RuntimeError(f"{who}: vert_normals [V,3], vert_quats [V,4], face_ratio [F] (`phong_frame` of the posed mesh)")
    return vn, vq, ratio


def _no_vertex_gradient(verts, who):
    if isinstance(verts, torch.Tensor) and verts.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{who}: the Phong-surface binding has no vertex gradient (the per-frame mesh pass is not "
                           "differentiable); hand it `verts.detach()`")


class BindMode(NamedTuple):
    """Everything the host knows about ONE value of fr_binding::mode.  The device code holds the modes as one thing
    (csrc/fr_bind_math.hpp, one bind_fwd / bind_bwd switch); this is its counterpart: the descriptor builder, the autograd
    Function below and bound.py read a record and never ask which mode they are in."""
    value: int            # FR_BIND_*
    op: str               # the public stand-alone op (error messages)
    own: str              # the mode's own per-Gaussian parameter: as the op names it, ...
    attr: str             # ... the holder attribute that carries it, ...
    own_cols: int         # ... its shape: [N,own_cols], or with 1 anything of N elements ([N,1]), ...
    field: str            # ... the fr_binding member it travels in ...
    grad: str             # ... and the fr_aux member its gradient is written through
    backward: str         # the stand-alone backward's entry point
    reads_bary: bool      # fr_binding::bary is read
    verts_grad: bool      # the posed vertices get a gradient
    active_sh: bool       # render_bound_batch renders the frame at the holder's active_sh_degree
    shapes: str           # the shape error of the op ...
    frame_shapes: str     # ... and of render_bound_batch
    holder: str           # what render_bound_batch tells a holder without `attr`

    def grad_shape(self, N):
        """The shape the kernel writes the own parameter's gradient in."""
        return (N,) if self.own_cols == 1 else (N, self.own_cols)


SHELL = BindMode(_lib.FR_BIND_SHELL, "bind_gaussians", "offset", "_offset", 1, "offset", "d_offset", "fr_bind_backward",
                 reads_bary=True, verts_grad=True, active_sh=False,
                 shapes="verts [V,3], offset [N,1], rotation [N,4], scaling [N,3], bary [N,3]",
                 frame_shapes="verts [V,3], offset [N,1], rotation [N,4], scaling [N,3], bary [N,3]",
                 holder="a shell binding (MeshBinding) needs a holder with the offsets `_offset` [N,1]")
FACE_LOCAL = BindMode(_lib.FR_BIND_FACE_LOCAL, "bind_gaussians_face_local", "local_xyz", "_xyz", 3, "local_xyz", "d_local_xyz",
                      "fr_bind_backward_local", reads_bary=False, verts_grad=True, active_sh=True,
                      shapes="verts [V,3], binding [N], local_xyz [N,3], rotation [N,4], scaling [N,3]",
                      frame_shapes="verts [V,3], _xyz [N,3], rotation [N,4], scaling [N,3]",
                      holder="a face-local binding (FaceLocalBinding) needs a holder with the local positions `_xyz` [N,3]")
PHONG = BindMode(_lib.FR_BIND_PHONG, "bind_gaussians_phong", "uvd", "_uvd", 3, "local_xyz", "d_local_xyz", "fr_bind_backward_phong",
                 reads_bary=True, verts_grad=False, active_sh=False,
                 shapes="verts [V,3], face_index [N], bary [N,3], uvd [N,3], rotation [N,4], scaling [N,3]",
                 frame_shapes="verts [V,3], _uvd [N,3], rotation [N,4], scaling [N,3], bary [N,3]",
                 holder="a Phong-surface binding (PhongBinding) needs a holder with the parameters `_uvd` [N,3]")
DEFORM = BindMode(_lib.FR_BIND_DEFORM, "bind_gaussians_deform", "deform", "_deform", 10, "local_xyz", "d_local_xyz",
                  "fr_bind_backward_deform", reads_bary=True, verts_grad=True, active_sh=False,
                  shapes="verts [V,3], face_index [N], bary [N,3], deform [N,10], rotation [N,4], scaling [N,3]",
                  frame_shapes="verts [V,3], _deform [N,10], rotation [N,4], scaling [N,3], bary [N,3]",
                  holder="an MLP-deformed binding (DeformBinding) needs a holder with this frame's MLP outputs `_deform` [N,10]")


def _describe(mode, verts, faces, face_index, own, rotation, scaling, bary=None, canon=None, shell_len=0.0, resize_scale=False,
              frame=None):
    """The fr_binding of one frame in `mode`; `own` is the mode's own per-Gaussian parameter.  What a mode does not read is
    not handed over and stays zero.  `frame` (`phong_frame` of the posed mesh) makes it the `base` of an fr_binding_phong
    with the three arrays behind it: an fr_binding over the extended descriptor's memory, passed on like any other.  The
    descriptor holds raw pointers: the caller keeps the tensors alive until the launch."""
    phong = _lib.fr_binding_phong() if frame is not None else None
    b = phong.base if phong is not None else _lib.fr_binding()
    b.N, b.V, b.F, b.mode = face_index.shape[0], verts.shape[0], faces.shape[0], mode.value
    b.verts, b.faces, b.face_index = verts.data_ptr(), faces.data_ptr(), face_index.data_ptr()
    b.bary = bary.data_ptr() if bary is not None else None
    b.face_scale_canonical = canon.data_ptr() if canon is not None else None
    b.shell_len, b.resize_scale = float(shell_len), int(bool(resize_scale))
    b.rotation, b.scaling = rotation.data_ptr(), scaling.data_ptr()
    setattr(b, mode.field, own.data_ptr())
    if phong is None:
        return b
    phong.vert_normals, phong.vert_quats, phong.face_ratio = (t.data_ptr() for t in frame)
    return phong.as_binding()


def _check_shapes(who, text, mode, verts, faces, face_index, own, rotation, scaling, bary=None, canon=None, shell_len=0.0,
                  resize_scale=False, frame=None):
    """`_describe`'s arguments behind the name of the caller and its shape error (`BindMode.shapes` / `.frame_shapes`)."""
    N = face_index.shape[0]
    own_ok = own.numel() == N if mode.own_cols == 1 else own.shape == (N, mode.own_cols)
    if verts.dim() != 2 or not own_ok or rotation.shape != (N, 4) or scaling.shape != (N, 3) or \
            (mode.reads_bary and bary.shape != (N, 3)):
        raise RuntimeError(f"{who}: {text}")
    if resize_scale and (canon is None or canon.numel() != faces.shape[0]):
        raise RuntimeError(f"{who}: resize_scale needs face_scale_canonical [F,1]")


def _grad_buffer(need, claimed, shape, device):
    """Where a backward writes one gradient: nothing if it is not needed; `claimed`, the buffer of the parameter's GradOut slot
    (the first backward of a step writes the slot in place), if it has the right size and is contiguous; else a fresh tensor."""
    if not need:
        return None
    if claimed is not None and claimed.numel() == int(torch.Size(shape).numel()) and claimed.is_contiguous():
        return claimed.view(shape)
    return torch.empty(shape, dtype=torch.float32, device=device)


class _Bind(torch.autograd.Function):
    """The stand-alone binding op of every mode: fr_bind_forward, and the mode's backward entry point."""

    @staticmethod
    def forward(ctx, mode, verts, own, rotation, scaling, faces, face_index, bary, canon, shell_len, resize_scale, frame):
        own_shape = own.shape
        verts, own = _chk(verts, torch.float32, "verts"), _chk(own, torch.float32, mode.own)
        rotation, scaling = _chk(rotation, torch.float32, "rotation"), _chk(scaling, torch.float32, "scaling")
        faces, face_index = _chk(faces, torch.int32, "faces"), _chk(face_index, torch.int32, "face_index")
        bary = _chk(bary, torch.float32, "bary_coords") if mode.reads_bary else None
        canon = _chk(canon, torch.float32, "face_scale_canonical") if canon is not None else None
        args = (mode, verts, faces, face_index, own, rotation, scaling, bary, canon, float(shell_len), bool(resize_scale))
        _check_shapes(mode.op, mode.shapes, *args)
        if frame is not None:
            frame = _chk_phong_frame(frame, verts.shape[0], faces.shape[0], mode.op)
        N, dev = face_index.shape[0], verts.device
        xyz = torch.empty((N, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((N, 4), dtype=torch.float32, device=dev)
        scl = torch.empty((N, 3), dtype=torch.float32, device=dev)
        b = _describe(*args, frame)
        _lib.launch("fr_bind_forward", dev, C.byref(b), xyz.data_ptr(), rot.data_ptr(), scl.data_ptr())
        ctx.save_for_backward(verts, faces, face_index, own, rotation, scaling, bary, canon, *(frame or ()))
        ctx.consts = (mode, float(shell_len), bool(resize_scale), own_shape)
        # optional extension (see rasterizer.GradOut): a raw parameter may carry `_fr_grad_out`, a slot whose preallocated
        # buffer (a view into a flat gradient buffer) receives its gradient without a copy
        ctx.grad_slots = (GradOut.of(own), GradOut.of(rotation), GradOut.of(scaling))
        return xyz, rot, scl

    @staticmethod
    def backward(ctx, g_xyz, g_rot, g_scl):
        saved = ctx.saved_tensors
        *tensors, bary, canon = saved[:8]
        mode, shell_len, resize_scale, own_shape = ctx.consts
        verts, dev, N = tensors[0], tensors[0].device, tensors[2].shape[0]
        need_v, need_o, need_r, need_s = ctx.needs_input_grad[1:5]
        c = lambda g: g.contiguous().float() if g is not None else None  # noqa: E731
        g_xyz, g_rot, g_scl = c(g_xyz), c(g_rot), c(g_scl)
        claim = lambda need, slot: slot.claim()[0] if need and slot is not None else None  # noqa: E731
        d_verts = torch.zeros_like(verts) if need_v and mode.verts_grad else None
        d_own = _grad_buffer(need_o, claim(need_o, ctx.grad_slots[0]), mode.grad_shape(N), dev)
        d_rot = _grad_buffer(need_r, claim(need_r, ctx.grad_slots[1]), (N, 4), dev)
        d_scl = _grad_buffer(need_s, claim(need_s, ctx.grad_slots[2]), (N, 3), dev)
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        b = _describe(mode, *tensors, bary, canon, shell_len, resize_scale, saved[8:] or None)
        _lib.launch(mode.backward, dev, C.byref(b), p(g_xyz), p(g_rot), p(g_scl), p(d_verts), p(d_own), p(d_rot), p(d_scl))
        return (None, d_verts, d_own.view(own_shape) if d_own is not None else None, d_rot, d_scl, None, None, None, None, None,
                None, None)


def _bind(mode, verts, own, rotation, scaling, faces, face_index, bary=None, canon=None, shell_len=0.0, resize_scale=False,
          frame=None):
    if not mode.verts_grad:
        _no_vertex_gradient(verts, mode.op)   # (before any other argument is touched)
    return _Bind.apply(mode, verts, own, rotation, scaling, faces, face_index, bary, canon, shell_len, resize_scale, frame)


def bind_gaussians(verts, faces, face_index, bary_coords, face_scale_canonical, offset, rotation, scaling,
                   shell_len: float, resize_scale: bool = True):
    """One frame of model/fateavatar.py:225-258.  verts [V,3] (posed), faces [F,3], face_index [N], bary_coords [N,3],
    face_scale_canonical [F,1] (`face_scale` of the canonical mesh), raw offset [N,1] / rotation [N,4] / scaling [N,3].
    Returns (xyz [N,3], rotation [N,4], scaling [N,3]): the values the reference assigns to gaussian._xyz /
    gaussian._rotation / gaussian._scaling before render()."""
    return _bind(SHELL, verts, offset, rotation, scaling, faces, face_index, bary_coords, face_scale_canonical, shell_len,
                 resize_scale)


def bind_gaussians_face_local(verts, faces, binding, local_xyz, rotation, scaling):
    """One frame of model/baseline/gaussianavatars.py:144-171.  verts [V,3] (posed), faces [F,3], binding [N] (the face of
    every Gaussian), raw local_xyz [N,3] / rotation [N,4] / scaling [N,3].  Returns (xyz [N,3], rotation [N,4],
    scaling [N,3]): the values the reference assigns to gaussian._xyz / gaussian._rotation / gaussian._scaling before
    render()."""
    return _bind(FACE_LOCAL, verts, local_xyz, rotation, scaling, faces, binding)


def phong_scatter_frame_grads(verts, faces, face_index, bary, frame, uvd, rotation, scaling, g_xyz, g_rotation, g_scaling,
                              d_verts=None, d_vert_normals=None, d_vert_quats=None, d_face_ratio=None):
    """`fr_bind_backward_phong_frame`: the gradients of the bound values (any may be None: zero) ADDED with float atomics onto
    d_verts [V,3] and onto the gradients of `phong_frame`'s three arrays (d_vert_normals [V,3], d_vert_quats [V,4],
    d_face_ratio [F]; the caller zeroed them, any may be None).  All tensors float32 / int32, contiguous, on the device; one
    launch on the current stream."""
    b = _describe(PHONG, verts, faces, face_index, uvd, rotation, scaling, bary, frame=frame)
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.launch("fr_bind_backward_phong_frame", verts.device, C.byref(b), p(g_xyz), p(g_rotation), p(g_scaling), p(d_verts),
                p(d_vert_normals), p(d_vert_quats), p(d_face_ratio))


class _BindPhongFrame(torch.autograd.Function):
    """`bind_gaussians_phong` on a differentiable frame: `_Bind`'s two launches (the same bits for uvd / rotation / scaling),
    and fr_bind_backward_phong_frame for the posed vertices and the frame's three arrays."""

    @staticmethod
    def forward(ctx, verts, vn, vq, ratio, own, rotation, scaling, faces, face_index, bary):
        mode, own_shape = PHONG, own.shape
        verts, own = _chk(verts, torch.float32, "verts"), _chk(own, torch.float32, mode.own)
        rotation, scaling = _chk(rotation, torch.float32, "rotation"), _chk(scaling, torch.float32, "scaling")
        faces, face_index = _chk(faces, torch.int32, "faces"), _chk(face_index, torch.int32, "face_index")
        bary = _chk(bary, torch.float32, "bary_coords")
        args = (mode, verts, faces, face_index, own, rotation, scaling, bary, None, 0.0, False)
        _check_shapes(mode.op, mode.shapes, *args)
        frame = _chk_phong_frame((vn, vq, ratio), verts.shape[0], faces.shape[0], mode.op)
        N, dev = face_index.shape[0], verts.device
        xyz = torch.empty((N, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((N, 4), dtype=torch.float32, device=dev)
        scl = torch.empty((N, 3), dtype=torch.float32, device=dev)
        b = _describe(*args, frame)
        _lib.launch("fr_bind_forward", dev, C.byref(b), xyz.data_ptr(), rot.data_ptr(), scl.data_ptr())
        ctx.save_for_backward(verts, faces, face_index, own, rotation, scaling, bary, *frame)
        ctx.own_shape = own_shape
        ctx.grad_slots = (GradOut.of(own), GradOut.of(rotation), GradOut.of(scaling))
        return xyz, rot, scl

    @staticmethod
    def backward(ctx, g_xyz, g_rot, g_scl):
        verts, faces, face_index, own, rotation, scaling, bary, *frame = ctx.saved_tensors
        mode, dev, N = PHONG, verts.device, face_index.shape[0]
        need_v, need_vn, need_vq, need_ratio, need_o, need_r, need_s = ctx.needs_input_grad[:7]
        c = lambda g: g.contiguous().float() if g is not None else None  # noqa: E731
        g_xyz, g_rot, g_scl = c(g_xyz), c(g_rot), c(g_scl)
        claim = lambda need, slot: slot.claim()[0] if need and slot is not None else None  # noqa: E731
        d_own = _grad_buffer(need_o, claim(need_o, ctx.grad_slots[0]), mode.grad_shape(N), dev)
        d_rot = _grad_buffer(need_r, claim(need_r, ctx.grad_slots[1]), (N, 4), dev)
        d_scl = _grad_buffer(need_s, claim(need_s, ctx.grad_slots[2]), (N, 3), dev)
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        b = _describe(mode, verts, faces, face_index, own, rotation, scaling, bary, frame=frame)
        if need_o or need_r or need_s:
            _lib.launch(mode.backward, dev, C.byref(b), p(g_xyz), p(g_rot), p(g_scl), None, p(d_own), p(d_rot), p(d_scl))
        zeros = lambda need, t: torch.zeros_like(t) if need else None  # noqa: E731
        d_verts, d_vn, d_vq, d_ratio = (zeros(n, t) for n, t in zip((need_v, need_vn, need_vq, need_ratio), (verts, *frame)))
        _lib.launch("fr_bind_backward_phong_frame", dev, C.byref(b), p(g_xyz), p(g_rot), p(g_scl), p(d_verts), p(d_vn), p(d_vq),
                    p(d_ratio))
        return (d_verts, d_vn, d_vq, d_ratio, d_own.view(ctx.own_shape) if d_own is not None else None, d_rot, d_scl, None, None,
                None)


def _frame_on_autograd(frame):
    return torch.is_grad_enabled() and isinstance(frame, (tuple, list)) and len(frame) == 3 and \
        all(isinstance(t, torch.Tensor) and t.requires_grad for t in frame)


def bind_gaussians_phong(verts, faces, face_index, bary_coords, frame, uvd, rotation, scaling):
    """One frame of model/baseline/splattingavatar.py:224-246.  verts [V,3] (posed), faces [F,3], face_index [N],
    bary_coords [N,3], `frame` = `phong_frame(canonical, verts)` of the same posed mesh, raw uvd [N,3] / rotation [N,4] /
    scaling [N,3].  Returns (xyz [N,3], rotation [N,4], scaling [N,3]): the values the reference assigns to gaussian._xyz /
    gaussian._rotation / gaussian._scaling before render().  Only the third column of uvd is read; the first two columns of its
    gradient are zeros (the reference's forward likewise: they only steer its CPU triangle walk).

    With a `frame` whose three tensors require grad — `phong_frame(canonical, verts, differentiable=True)` — the op also hands
    gradients to `verts` (the barycentric point) and to the three frame arrays, and through them dLoss/dverts of the whole
    path is what the reference's autograd gives.  With a detached frame a `verts` that requires grad is refused: the result
    would silently lack the mesh pass's part."""
    if _frame_on_autograd(frame):
        return _BindPhongFrame.apply(verts, *frame, uvd, rotation, scaling, faces, face_index, bary_coords)
    return _bind(PHONG, verts, uvd, rotation, scaling, faces, face_index, bary_coords, frame=frame)


def bind_gaussians_deform(verts, faces, face_index, bary_coords, deform, rotation, scaling):
    """One frame of model/baseline/flashavatar.py:242-276.  verts [V,3] (posed), faces [F,3], face_index [N], bary_coords [N,3],
    deform [N,10] (the RAW outputs of the deformation MLP for this frame: tanh is applied here), raw rotation [N,4] /
    scaling [N,3].  Returns (xyz [N,3], rotation [N,4], scaling [N,3]): the values the reference assigns to gaussian._xyz /
    gaussian._rotation / gaussian._scaling before render().  Differentiable w.r.t. verts, deform, rotation and scaling."""
    return _bind(DEFORM, verts, deform, rotation, scaling, faces, face_index, bary_coords)
