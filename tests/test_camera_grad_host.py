"""CPU: the host side of the camera-pose gradients (FR_FLAG_CAMERA_GRAD) — the float64 reference the GPU tests use
(tests/camera_ref.py) is consistent with itself, `model.PoseCamera` is the reference's camera, the ABI additions have the C
compiler's layout, and the autograd glue hands the camera tensors over exactly when one of them requires grad."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from fateavatar_amd import _lib, model, rasterizer, scenes
from tests import camera_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("name", ["deg3", "near"])
def test_reference_satisfies_the_rigid_motion_identity(name):
    s, f, _, ref = cr.case(name)
    c = s.camera
    vis = f.radii > 0
    lim = np.abs(s.means3D[:, :2] / s.means3D[:, 2:3])   # (the scenes' camera is the identity: view space = world space)
    n_clamped = int(((lim[:, 0] > 1.3 * c.tanfovx) | (lim[:, 1] > 1.3 * c.tanfovy))[vis].sum())
    assert (n_clamped > 0) == (name == "deg3"), "deg3 exercises the clamp's stop-gradient, near has no clamped Gaussian"
    if name == "near":
        assert vis.all()
    lhs, rhs = cr.rigid_identity(c.world_view_transform, c.full_proj_transform, ref.dmeans.sum(0), ref.dcam, ref.dV, ref.dF)
    assert np.all(np.abs(lhs - rhs) <= 1e-9 * np.abs(lhs)), (lhs, rhs)
    assert np.all(np.abs(lhs) > 1e-3)   # (not 0 = 0)


@pytest.mark.parametrize("name", ["deg3", "near"])
def test_reference_dead_entries_are_exactly_zero(name):
    _, f, _, ref = cr.case(name)
    vis = f.radii > 0
    assert np.all(ref.pV[:, :, 3] == 0) and np.all(ref.pF[:, :, 2] == 0)
    assert np.all(ref.sV[:, :3] > 0) and np.all(ref.sF[:, [0, 1, 3]] > 0) and np.all(ref.scam > 0)
    # a culled Gaussian contributes to nothing
    assert np.all(ref.pV[~vis] == 0) and np.all(ref.pF[~vis] == 0) and np.all(ref.pcam[~vis] == 0)


def test_reference_live_entries_of_the_clamped_scene_are_nonzero():
    ref = cr.case("deg3")[3]
    live = np.concatenate([ref.dV[:, :3].ravel(), ref.dF[:, [0, 1, 3]].ravel(), ref.dcam])
    assert np.all(np.abs(live) > 1e-2) and np.abs(live).max() < 100


def test_pose_camera_reproduces_the_golden_cameras():
    z = np.load(os.path.join(G, "golden_camera.npz"))
    assert len(z["names"]) > 0
    for name in z["names"]:
        fx, fy = (float(v) for v in z[f"{name}_fov"])
        h, w = (int(v) for v in z[f"{name}_res"])
        R, T = torch.from_numpy(z[f"{name}_R"].astype(np.float32)), torch.from_numpy(z[f"{name}_T"].astype(np.float32))
        cam = model.PoseCamera(R.unsqueeze(0), T.unsqueeze(0), fx, fy, (h, w))
        assert (cam.image_height, cam.image_width, cam.FoVx, cam.FoVy) == (h, w, fx, fy)
        # (the tolerances tests/test_oracle_golden.py holds scenes.make_camera to)
        np.testing.assert_allclose(cam.world_view_transform.numpy(), z[f"{name}_wvt"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(cam.full_proj_transform.numpy(), z[f"{name}_full"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(cam.camera_center.numpy(), z[f"{name}_center"], rtol=0, atol=5e-6)
        np.testing.assert_allclose(cam.projection_matrix.numpy(), z[f"{name}_proj"], rtol=1e-6, atol=1e-7)


def test_pose_camera_is_differentiable_in_R_and_T():
    z = np.load(os.path.join(G, "golden_camera.npz"))
    name = z["names"][0]
    R = torch.tensor(z[f"{name}_R"], dtype=torch.float64, requires_grad=True)
    T = torch.tensor(z[f"{name}_T"], dtype=torch.float64, requires_grad=True)
    fx, fy = (float(v) for v in z[f"{name}_fov"])
    cam = model.PoseCamera(R, T, fx, fy, (32, 32))
    assert cam.world_view_transform.requires_grad and cam.full_proj_transform.requires_grad and cam.camera_center.requires_grad
    (cam.world_view_transform.sum() + cam.full_proj_transform.sum() + cam.camera_center.sum()).backward()
    assert R.grad is not None and T.grad is not None and R.grad.abs().min() > 0 and T.grad.abs().min() > 0
    with pytest.raises(ValueError):
        model.PoseCamera(torch.eye(4), torch.zeros(3), fx, fy, (32, 32))


def test_flag_and_aux_layout_match_the_c_compiler():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%d %zu %zu %zu %zu %zu %zu %zu\n", FR_FLAG_CAMERA_GRAD, sizeof(fr_aux), sizeof(fr_aux_camera), offsetof(fr_aux_camera, base),
        offsetof(fr_aux_camera, d_viewmatrix), offsetof(fr_aux_camera, d_projmatrix), offsetof(fr_aux_camera, d_campos),
        offsetof(fr_aux_camera, camera_workspace));
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    a, e = _lib.fr_aux, _lib.fr_aux_camera
    assert out == [_lib.FR_FLAG_CAMERA_GRAD, C.sizeof(a), C.sizeof(e), e.base.offset, e.d_viewmatrix.offset, e.d_projmatrix.offset,
                   e.d_campos.offset, e.camera_workspace.offset]
    assert out[0] == 16 and e.base.offset == 0
    # bit 4 is free: below the accumulate bits, none of the other flags
    assert _lib.FR_FLAG_CAMERA_GRAD < (1 << _lib.FR_FLAG_ACCUMULATE_SHIFT)
    others = (_lib.FR_FLAG_NO_WAIT, _lib.FR_FLAG_RAW_ACTIVATIONS, _lib.FR_FLAG_FORWARD_ONLY, _lib.FR_FLAG_DEPTH_ALPHA)
    assert all(_lib.FR_FLAG_CAMERA_GRAD & o == 0 for o in others)
    # fr_aux itself is unchanged — its last member is still `planes` — and the camera's members sit right behind it
    assert [f[0] for f in a._fields_][-1] == "planes" and e.d_viewmatrix.offset == C.sizeof(a)
    # the base as fr_params::aux sees it shares the extension's memory
    x = e()
    b = x.as_aux()
    b.planes, x.d_campos = 5, 7
    assert x.base.planes == 5 and C.addressof(b) == C.addressof(x) and x.d_campos == 7
    assert _lib.lib().fr_camera_grad_workspace_bytes() > 0


def _settings(requires_grad):
    s = cr.scene()
    c = s.camera
    t = lambda a: torch.tensor(a, requires_grad=requires_grad)   # noqa: E731
    return rasterizer.GaussianRasterizationSettings(
        image_height=c.image_height, image_width=c.image_width, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=torch.zeros(3),
        scale_modifier=1.0, viewmatrix=t(c.world_view_transform), projmatrix=t(c.full_proj_transform), sh_degree=0,
        campos=t(c.camera_center), prefiltered=False, debug=False)


def test_camera_tensors_are_passed_only_when_one_requires_grad(monkeypatch):
    seen = []
    monkeypatch.setattr(rasterizer._RasterizeGaussians, "apply", staticmethod(lambda *a: seen.append(a)))
    monkeypatch.setattr(rasterizer._RasterizeGaussiansBatch, "apply", staticmethod(lambda *a: seen.append(a) or ()))
    e, m = torch.Tensor([]), torch.zeros(4, 3, requires_grad=True)
    eight = (m, torch.zeros(4, 3), e, torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(4, 4), e)
    plain, posed = _settings(False), _settings(True)
    rasterizer.rasterize_gaussians_autograd(*eight, plain)
    assert len(seen[-1]) == 12, "the reference's nine arguments and the three switches: no camera tensor"
    rasterizer.rasterize_gaussians_autograd(*eight, posed)
    assert len(seen[-1]) == 15 and seen[-1][12] is posed.viewmatrix and seen[-1][13] is posed.projmatrix and seen[-1][14] is posed.campos
    only_T = plain._replace(campos=posed.campos)
    rasterizer.rasterize_gaussians_autograd(*eight, only_T)
    assert len(seen[-1]) == 15
    with torch.no_grad():
        rasterizer.rasterize_gaussians_autograd(*eight, posed)
    assert len(seen[-1]) == 12
    # a batch shares one launch chain: every view's three, or none
    rasterizer.rasterize_views_autograd([plain, plain], [eight, eight])
    assert len(seen[-1]) == 5 + 16
    rasterizer.rasterize_views_autograd([plain, posed], [eight, eight])
    assert len(seen[-1]) == 5 + 16 + 6 and seen[-1][5 + 16 + 3] is posed.viewmatrix


def test_a_camera_only_frame_is_not_forward_only():
    posed = _settings(True)
    eight = tuple(torch.zeros(2, 3) for _ in range(8))
    assert rasterizer._pick_forward_only(eight) is True
    assert rasterizer._pick_forward_only((*eight, *rasterizer._camera_inputs(posed))) is False
    assert rasterizer._camera_inputs(_settings(False)) == ()
    seen = []
    orig = rasterizer._RasterizeGaussians.apply
    try:
        rasterizer._RasterizeGaussians.apply = staticmethod(lambda *a: seen.append(a))
        rasterizer.rasterize_gaussians_autograd(*eight, posed)
    finally:
        rasterizer._RasterizeGaussians.apply = orig
    assert seen[-1][10] is False, "forward_only must be off: the backward needs the frame's hand-off"


def test_camera_buffers_are_checked():
    with pytest.raises(RuntimeError):
        rasterizer._camera_outputs((None, None, None), "cpu")
    with pytest.raises(RuntimeError):
        rasterizer._camera_outputs((torch.zeros(4, 4),) * 3, "cpu")   # (not on the device)


def test_compiled_module_exports_the_camera_backward():
    """`_C.rasterize_gaussians_backward_camera`: rasterize_gaussians_backward's 21 arguments, eleven tensors out."""
    from fateavatar_amd import torch_ext
    torch_ext.build()          # no-op when the package's build made it
    m = torch_ext.load()
    doc = m.rasterize_gaussians_backward_camera.__doc__
    assert doc.count("arg") == 21 and doc.count("torch.Tensor") == 15 + 11
    assert m.rasterize_gaussians_backward.__doc__.count("torch.Tensor") == 15 + 8      # (the reference's name is unchanged)
