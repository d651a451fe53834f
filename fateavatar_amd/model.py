"""Minimal Gaussian parameter holder with the reference GaussianModel's getters
(volume_rendering/gaussian_model.py:39-50,105-128): raw parameters + exp / sigmoid / normalize
activations in stock PyTorch.  It exists so that `render()` can be driven exactly like the
reference drives it; densification, PLY I/O and optimizer surgery are out of scope.

All parameters live in ONE flat fp32 buffer (and their gradients in one flat buffer), so the
data-parallel exchange is a single all-reduce (fateavatar_amd/dp.py).
"""
from __future__ import annotations

import numpy as np
import torch

from .flat import FlatParams


class FlatGaussians(FlatParams):
    FIELDS = (("_xyz", 3), ("_features", None), ("_opacity", 1), ("_scaling", 3), ("_rotation", 4))

    def __init__(self, means3D, shs, opacities, scales, rotations, sh_degree: int, device, fused_activations=False):
        """Arguments are ACTIVATED values (numpy): they are inverted into raw parameters like
        create_from_pcd does (gaussian_model.py:137-160)."""
        super().__init__()
        self.max_sh_degree, self.M = sh_degree, shs.shape[1]
        # True: render() passes the raw parameters and the rasterizer kernels apply the activations themselves
        self.fused_activations = bool(fused_activations)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)  # noqa: E731
        op = t(opacities).reshape(-1).clamp(1e-6, 1 - 1e-6)
        self._bind([t(means3D), t(shs), torch.log(op / (1 - op)).reshape(-1, 1), torch.log(t(scales)), t(rotations)])

    @classmethod
    def from_raw(cls, xyz, features, opacity, scaling, rotation, sh_degree: int, device, fused_activations=False):
        """From RAW parameters (logit opacity, log scale, un-normalised quaternion), e.g. `ply.load_ply()`."""
        self = cls.__new__(cls)
        torch.nn.Module.__init__(self)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)  # noqa: E731
        self.max_sh_degree, self.M = sh_degree, int(np.shape(features)[1])
        self.fused_activations = bool(fused_activations)
        self._bind([t(xyz), t(features), t(opacity).reshape(-1, 1), t(scaling), t(rotation)])
        return self

    def save_ply(self, path: str) -> None:
        """GaussianModel.save_ply (gaussian_model.py:205-223)."""
        from . import ply
        g = lambda n: getattr(self, n).detach().cpu().numpy()  # noqa: E731
        ply.save_ply(path, g("_xyz"), g("_features"), g("_opacity"), g("_scaling"), g("_rotation"))

    @classmethod
    def load_ply(cls, path: str, device, max_sh_degree=None, fused_activations=False):
        """GaussianModel.load_ply (gaussian_model.py:230-269)."""
        from . import ply
        d = ply.load_ply(path, max_sh_degree)
        return cls.from_raw(d["xyz"], d["features"], d["opacity"], d["scaling"], d["rotation"], d["sh_degree"], device,
                            fused_activations)

    def widths(self):
        return [3, self.M * 3, 1, 3, 4]

    def shapes(self):
        return [(3,), (self.M, 3), (1,), (3,), (4,)]

    def _wants_slot(self, name):
        # without fused activations only these two reach the rasterizer untouched (FlatParams._wants_slot)
        return name in ("_xyz", "_features") or self.fused_activations

    def _p(self, name):
        return getattr(self, name)

    # ---- the reference getters
    @property
    def get_xyz(self):
        return self._p("_xyz")

    @property
    def get_features(self):
        return self._p("_features")

    @property
    def get_opacity(self):
        return torch.sigmoid(self._p("_opacity"))

    @property
    def get_scaling(self):
        return torch.exp(self._p("_scaling"))

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._p("_rotation"))

    def grad_of(self, name):
        return getattr(self, name).grad

    def begin_step(self):
        super().begin_step()
        self.accumulate_into_kept_grads(False)

    def accumulate_into_kept_grads(self, on: bool = True) -> None:
        """Gradient accumulation over several `.backward()` calls without `begin_step()` in between (one frame at a
        time, gradients kept): with `on`, the rasterizer's backward ADDS each further frame's gradients to the flat
        gradient buffer inside its kernel (FR_FLAG_ACCUMULATE; rasterizer.GradOut) instead of handing autograd a
        temporary to add.  Only for `.backward()`; `begin_step()` switches it off again."""
        for name, _ in self.FIELDS:
            slot = getattr(getattr(self, name), "_fr_grad_out", None)
            if slot is not None:
                slot.add_to_kept = bool(on)


class TorchCamera:
    """Device-side camera with the attribute names render() reads (camera_3dgs.py:22-72)."""

    def __init__(self, cam, device):
        self.image_height, self.image_width = cam.image_height, cam.image_width
        self.FoVx, self.FoVy = cam.FoVx, cam.FoVy
        # the three tensors are views into ONE 35-float buffer, so that copy_from is a single device copy
        self._packed = torch.from_numpy(np.concatenate([
            np.asarray(cam.world_view_transform, np.float32).reshape(-1), np.asarray(cam.full_proj_transform, np.float32).reshape(-1),
            np.asarray(cam.camera_center, np.float32).reshape(-1)])).to(device)
        self.world_view_transform = self._packed[0:16].view(4, 4)
        self.full_proj_transform = self._packed[16:32].view(4, 4)
        self.camera_center = self._packed[32:35]

    def clone(self) -> "TorchCamera":
        """A camera with its own matrix block (same intrinsics): the static input of another captured frame."""
        o = TorchCamera.__new__(TorchCamera)
        o.__dict__.update(self.__dict__)
        o._packed = self._packed.clone()
        o.world_view_transform = o._packed[0:16].view(4, 4)
        o.full_proj_transform = o._packed[16:32].view(4, 4)
        o.camera_center = o._packed[32:35]
        return o

    def copy_from(self, other: "TorchCamera") -> None:
        """Overwrite the matrices in place (same intrinsics): lets a captured HIP graph render a new view."""
        self.check_same_intrinsics(other)
        self._packed.copy_(other._packed, non_blocking=True)

    def check_same_intrinsics(self, other: "TorchCamera") -> None:
        if (other.image_height, other.image_width, other.FoVx, other.FoVy) != \
                (self.image_height, self.image_width, self.FoVx, self.FoVy):
            raise ValueError("copy_from needs a camera with the same image size and field of view")


class PoseCamera:
    """The reference's `Camera` (volume_rendering/camera_3dgs.py:22-72 around getWorld2View2_torch, tools/gs_utils/
    graphics_utils.py:51-62) built IN TORCH on the device of `R` / `T`, with the attribute names render() reads: gradients
    reach `R` [3,3] (camera-to-world rotation) and `T` [3] (world-to-view translation) through `world_view_transform`,
    `full_proj_transform` and `camera_center`.  The reference builds these three from its `cam_pose` embedding
    (model/fateavatar.py:198-204) and then loses the gradient inside its rasterizer; here `render(PoseCamera(R, T, ...), ...)`
    followed by `.backward()` fills `R.grad` / `T.grad`.

    view = R^T x + T, so world_view_transform is [[R, 0], [T, 1]] (the transposed, row-vector storage) and the camera centre is
    -R T; getWorld2View2_torch's two matrix inversions (the identity for translate = 0, scale = 1) and the reference's
    `world_view_transform.inverse()[3, :3]` are left out: they need R orthonormal and agree with this to float32 rounding."""

    def __init__(self, R, T, FoVx, FoVy, img_res, znear: float = 0.01, zfar: float = 100.0):
        from .scenes import projection_matrix
        R, T = R.squeeze(0), T.squeeze(0)
        if R.shape != (3, 3) or T.shape != (3,):
            raise ValueError("PoseCamera: R is [3,3] (or [1,3,3]), T is [3] (or [1,3])")
        self.R, self.T = R, T
        self.FoVx, self.FoVy = float(FoVx), float(FoVy)
        self.image_height, self.image_width = int(img_res[0]), int(img_res[1])
        self.znear, self.zfar = znear, zfar
        last = torch.tensor([[0.0], [0.0], [0.0], [1.0]], dtype=R.dtype, device=R.device)
        self.world_view_transform = torch.cat([torch.cat([R, T.reshape(1, 3).to(R.dtype)], 0), last], 1)
        self.projection_matrix = torch.from_numpy(projection_matrix(znear, zfar, self.FoVx, self.FoVy).T.copy()).to(
            device=R.device, dtype=R.dtype)
        self.full_proj_transform = self.world_view_transform @ self.projection_matrix
        self.camera_center = -(R @ T.to(R.dtype))
