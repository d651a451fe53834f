"""SplattingAvatar's `simple_phongsurf` on the device: the walk on the triangle mesh and the Phong-surface fit.

reference (submodules/simple_phongsurf/simple_phongsurf/): `PhongSurfacePy3d` (phongsurf_py3d.py:16-336) keeps the walk in C++ on
the host (src/triangle_walk.cpp; every call a device -> host copy, a loop over the points and a copy back) and fits a point to
the surface with up to outer_loop x inner_loop Adam iterations of an autograd graph (`update_corres_spt` :151-185,
`solve_delta_vwd` :256-309).  Here both are HIP kernels (csrc/fr_phongsurf.hip; C ABI `fr_triwalk`, `fr_phong_fit`): no copy,
no host synchronisation, two launches per outer round, the same bits on every run.

What is here: `update_corres_spt` (method 'uvd', N None: what SplattingAvatar calls), `triwalk_update`, `retrieve_vertices`,
`retrieve_normals`, and `.triwalk.updateSurfacePoints` on numpy arrays as the compiled module's.
NOT here: `find_corres_spt` / `init_corres_spt` / `forward` (they need pytorch3d's knn_points, and SplattingAvatar never calls
them), method 'uv' and a given N (`solve_delta_vw`), `update_corres_uvd`, texture coordinates.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .binding import triangle_neighbours

CROSS_TRIANGLE_DECAY = 0.9   # TriangleWalkOption::cross_triangle_decay (src/triangle_walk.h:16)
MAX_INNER_LOOP, MAX_OUTER_LOOP = 512, 8


def triwalk(faces_nbr: torch.Tensor, face_index: torch.Tensor, bary: torch.Tensor, delta: torch.Tensor, status: torch.Tensor,
            decay: float = CROSS_TRIANGLE_DECAY) -> None:
    """`fr_triwalk` IN PLACE on the current stream: face_index int32 [n], bary float32 [n,3], delta float32 [n,k >= 2] (a
    row-contiguous view or buffer: its row stride is passed on, so `_uvd` [P,3] goes in as it is), status int32 [4] (added to)."""
    n = int(face_index.shape[0])
    for t, dt in ((faces_nbr, torch.int32), (face_index, torch.int32), (bary, torch.float32), (delta, torch.float32), (status, torch.int32)):
        if not t.is_cuda or t.dtype != dt:
            raise RuntimeError("triwalk: int32 / float32 tensors on a HIP device (there is no CPU path)")
    if not (faces_nbr.is_contiguous() and face_index.is_contiguous() and bary.is_contiguous()) or bary.shape != (n, 3):
        raise RuntimeError("triwalk: contiguous faces_nbr [F,3], face_index [n], bary [n,3]")
    if delta.dim() != 2 or delta.shape[0] != n or delta.shape[1] < 2 or (n and delta.stride(1) != 1) or status.numel() < 4:
        raise RuntimeError("triwalk: delta [n, >= 2] with unit column stride, status [4]")
    _lib.launch_first("fr_triwalk", bary.device, faces_nbr.data_ptr(), int(faces_nbr.shape[0]), n, face_index.data_ptr(), bary.data_ptr(),
                      delta.data_ptr(), int(delta.stride(0)) if n else 2, float(decay), status.data_ptr())


class _Triwalk:
    """The compiled module's `Triwalk` (src/triangle_walk_py.cpp:20-105) as far as SplattingAvatar uses it."""

    def __init__(self, surface: "PhongSurface"):
        self._s = surface

    def updateSurfacePoints(self, spt_fidx, spt_vw, spt_delta):
        """numpy in, numpy out (int32 [n], float64 [n,2]) like the reference's; the walk itself runs on the device."""
        s = self._s
        fidx = torch.as_tensor(np.asarray(spt_fidx).astype(np.int32)).to(s.device)
        vw = torch.as_tensor(np.asarray(spt_vw).astype(np.float32)).to(s.device)
        delta = torch.as_tensor(np.asarray(spt_delta).astype(np.float32)).to(s.device)
        fidx, vw = s.triwalk_update(fidx, vw, delta)
        return fidx.cpu().numpy().astype(np.int32), vw.cpu().numpy().astype(np.float64)


class PhongSurface(torch.nn.Module):
    """PhongSurfacePy3d (phongsurf_py3d.py:16-47) for a mesh on a HIP device: V [V,3] vertices, F [F,3] faces, N [V,3] vertex
    normals.  The constructor defaults are the reference's; SplattingAvatar constructs it with outer_loop 2, inner_loop 50.
    `status` int32 [4] collects the kernels' counters (include/fr_rasterizer.h: all zero unless a walk had to be cut short or a
    point was not finite; [3] is the last fit's iteration count), `work` the last fit's per-iteration counters."""

    def __init__(self, V, F, N, outer_loop: int = 4, inner_loop: int = 500, method: str = "uvd", device=None):
        super().__init__()
        if method != "uvd":
            raise NotImplementedError("PhongSurface: method 'uv' (solve_delta_vw) is not built; SplattingAvatar uses 'uvd'")
        if not 1 <= int(outer_loop) <= MAX_OUTER_LOOP or not 1 <= int(inner_loop) <= MAX_INNER_LOOP:
            raise ValueError(f"PhongSurface: outer_loop 1 .. {MAX_OUTER_LOOP}, inner_loop 1 .. {MAX_INNER_LOOP}")
        V, F, N = torch.as_tensor(V), torch.as_tensor(F), torch.as_tensor(N)
        device = torch.device(device) if device is not None else V.device
        self.register_buffer("V", V.detach().to(device, torch.float32).contiguous())
        self.register_buffer("F", F.detach().to(device, torch.int64).contiguous())
        self.register_buffer("N", N.detach().to(device, torch.float32).contiguous())
        if self.V.dim() != 2 or self.V.shape[1] != 3 or self.N.shape != self.V.shape or self.F.dim() != 2 or self.F.shape[1] != 3:
            raise RuntimeError("PhongSurface: V [V,3], F [F,3], N [V,3]")
        if self.F.numel() and (int(self.F.min()) < 0 or int(self.F.max()) >= int(self.V.shape[0])):
            raise ValueError("PhongSurface: `F` names a vertex the mesh does not have")
        self.register_buffer("faces", self.F.to(torch.int32).contiguous())
        self.register_buffer("faces_nbr", triangle_neighbours(self.F))
        self.register_buffer("status", torch.zeros(4, dtype=torch.int32, device=device))
        self.outer_loop, self.inner_loop, self.method = int(outer_loop), int(inner_loop), method
        self.decay = CROSS_TRIANGLE_DECAY
        self.work = None
        self.triwalk = _Triwalk(self)

    @property
    def device(self):
        return self.V.device

    def triwalk_update(self, spt_fidx, spt_vw, spt_delta):
        """triwalk_update (:72-85): (spt_fidx [n], spt_vw [n,2]) walked by spt_delta [n,2]; new tensors of the inputs' dtypes."""
        fidx = spt_fidx.detach().to(self.device, torch.int32).contiguous().clone()
        vw = spt_vw.detach().to(self.device, torch.float32)
        bary = torch.cat([vw, 1.0 - vw[:, :1] - vw[:, 1:2]], dim=1).contiguous()
        delta = spt_delta.detach().to(self.device, torch.float32).contiguous()
        triwalk(self.faces_nbr, fidx, bary, delta, self.status, self.decay)
        return fidx.to(spt_fidx.dtype), bary[:, :2].to(spt_vw.dtype)

    def update_corres_spt(self, V, N, spt_fidx, spt_vw, delta_out=None):
        """update_corres_spt (:151-185) for the queries V [n,3] starting at (spt_fidx [n], spt_vw [n,2]): outer_loop rounds of the
        fit and the walk, all on the device (`fr_phong_fit`).  Returns (spt_fidx, spt_vw) as new tensors of the inputs' dtypes.
        `delta_out` (tests): a float32 [n,3] device buffer that receives the last round's delta."""
        if N is not None:
            raise NotImplementedError("PhongSurface.update_corres_spt: query normals (solve_delta_vw) are not built")
        dev = self.device
        query = V.detach().to(dev, torch.float32).contiguous()
        fidx = spt_fidx.detach().to(dev, torch.int32).contiguous().clone()
        vw = spt_vw.detach().to(dev, torch.float32)
        n = int(fidx.shape[0])
        if query.shape != (n, 3) or vw.shape != (n, 2):
            raise RuntimeError("update_corres_spt: V [n,3], spt_fidx [n], spt_vw [n,2]")
        bary = torch.cat([vw, 1.0 - vw[:, :1] - vw[:, 1:2]], dim=1).contiguous()
        self.work = torch.empty(self.outer_loop * self.inner_loop + 4, dtype=torch.int32, device=dev)
        if delta_out is not None and (delta_out.shape != (n, 3) or delta_out.dtype != torch.float32 or not delta_out.is_contiguous()
                                      or delta_out.device != dev):
            raise RuntimeError("update_corres_spt: delta_out must be a contiguous float32 [n,3] on the surface's device")
        _lib.launch_first("fr_phong_fit", dev, self.V.data_ptr(), self.N.data_ptr(), self.faces.data_ptr(), self.faces_nbr.data_ptr(),
                          int(self.V.shape[0]), int(self.faces.shape[0]), n, query.data_ptr(), fidx.data_ptr(), bary.data_ptr(),
                          self.outer_loop, self.inner_loop, float(self.decay), self.work.data_ptr(), self.status.data_ptr(),
                          delta_out.data_ptr() if delta_out is not None else None)
        return fidx.to(spt_fidx.dtype), bary[:, :2].to(spt_vw.dtype)

    def fit_iterations(self) -> list:
        """The iteration count of every round of the last `update_corres_spt` (reads the counters back: synchronises)."""
        if self.work is None:
            return []
        c = self.work[:self.outer_loop * self.inner_loop].reshape(self.outer_loop, self.inner_loop).cpu()
        return [int((row == 0).nonzero()[0]) + 1 if bool((row == 0).any()) else self.inner_loop for row in c]

    def retrieve_vertices(self, spt_fidx, spt_vw):
        """retrieve_vertices (:312-320)."""
        return _interp_bary(self.V[self.F[torch.as_tensor(spt_fidx).to(self.device).long()]], torch.as_tensor(spt_vw).to(self.device).float())

    def retrieve_normals(self, spt_fidx, spt_vw):
        """retrieve_normals (:323-327)."""
        norms = _interp_bary(self.N[self.F[spt_fidx.to(self.device).long()]], spt_vw.to(self.device).float())
        return torch.nn.functional.normalize(norms, p=2, dim=-1)


def _interp_bary(tri, vw):   # :9-14
    bary = torch.cat([vw, 1.0 - vw[..., :1] - vw[..., 1:2]], dim=-1)
    return torch.einsum("nij,ni->nj", tri, bary)


__all__ = ["CROSS_TRIANGLE_DECAY", "PhongSurface", "triwalk"]
