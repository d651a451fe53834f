"""GPU: camera-pose gradients (FR_FLAG_CAMERA_GRAD, include/fr_rasterizer.h) against the float64 reference of
tests/camera_ref.py — dL/d(viewmatrix), dL/d(projmatrix), dL/d(campos) from `rasterize_gaussians_backward(_camera=True)`,
through autograd from a `model.PoseCamera`, and out of `AvatarStep(camera_grad=True)`.

The bound everywhere: |hip - ref| <= 1e-4 x scale per entry, scale = the reference's sum of ABSOLUTE per-Gaussian
contributions to that entry (1e-4 is the project's gradient parity, tests/test_gpu_parity.py); entries no kernel reads are
exactly 0.  Pixels where the HIP frame and the oracle blended different sets (util.flip_pixels) get a zero upstream gradient on
both sides — at most 1 % of them.

Bit-equality.  The camera kernel itself has a fixed summation order, but it sums what the blend backward accumulated with float
atomics (one add per Gaussian and 8x8 tile): a Gaussian that gets contributions from three or more tiles has an order-
dependent last bit in its accumulator row (tests/test_gpu_parity.py says the same of the per-Gaussian gradients).  So every
bit-for-bit check here runs on SINGLE-PIXEL scenes — tiny Gaussians of opacity 0.0045 .. 0.0058, whose alpha >= 1/255
footprint has a radius below half a pixel (2 x 0.3003 x ln(255 x 0.0058) = 0.235 < 0.25): each contributes to at most one
pixel, hence one tile, one add — where the whole backward is deterministic and a differing bit is the camera path's."""
from types import SimpleNamespace

import numpy as np
import pytest

from fateavatar_amd import scenes
from tests import camera_ref as cr
from tests import util

pytestmark = pytest.mark.gpu

SLOT = 260          # the handles of this module: 260 .. 289 (no other module uses them)
PARITY = 1e-4
LIVE_V = [4 * r + c for r in range(4) for c in range(3)]
LIVE_F = [4 * r + c for r in range(4) for c in (0, 1, 3)]


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch, gpu_device):
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _backward(fr, dpix, camera=True, **kw):
    """-> (the eight per-Gaussian arrays, (d_view [4,4], d_proj [4,4], d_campos [3])) as numpy."""
    from fateavatar_amd import rasterizer
    out = rasterizer.rasterize_gaussians_backward(*fr._backward_args(_t(dpix, fr.dev)), _camera=camera, **kw)
    out = [o.cpu().numpy() for o in out]
    return out[:8], tuple(out[8:])


def _frame(s, dev, slot, **kw):
    from fateavatar_amd import rasterizer
    with rasterizer.handle_slot(slot):
        return util.HipFrame(s, dev, **kw)


def _mask_flips(o, fr, dpix, what):
    """dL/dpixel with the flip pixels zeroed, and how many there were (at most 1 %)."""
    flips = util.flip_pixels(o, fr.color.cpu().numpy(), fr.final_T.cpu().numpy())
    n = int(flips.sum())
    print(f"[camera_grad] {what}: {n} of {flips.size} pixels zeroed")
    assert n <= flips.size // 100, (what, n)
    if n:
        dpix = dpix.copy()
        dpix[:, flips] = 0
    return dpix, n


def _check(got, ref, what, view_scale=None):
    """Every entry of the three arrays against the reference, scaled by its abs-sum (`view_scale`: another scale for the view
    matrix); dead entries exactly 0."""
    dV, dF, dcam = (np.asarray(g, np.float64) for g in got)
    assert dV.shape == (4, 4) and dF.shape == (4, 4) and dcam.shape == (3,), what
    assert np.isfinite(dV).all() and np.isfinite(dF).all() and np.isfinite(dcam).all(), what
    assert np.all(dV[:, 3] == 0) and np.all(dF[:, 2] == 0), (what, "dead entries")
    worst = 0.0
    for name, g, r, sc, live in (("view", dV.ravel(), ref.dV.ravel(), (ref.sV if view_scale is None else view_scale).ravel(), LIVE_V),
                                 ("proj", dF.ravel(), ref.dF.ravel(), ref.sF.ravel(), LIVE_F),
                                 ("campos", dcam, ref.dcam, ref.scam, [0, 1, 2])):
        ratio = np.abs(g[live] - r[live]) / np.maximum(sc[live], 1e-300)
        print(f"[camera_grad] {what}: {name} worst |hip - ref| / scale = {ratio.max():.3e}")
        worst = max(worst, float(ratio.max()))
        # (an entry nothing contributes to — a doubly clamped Gaussian's view[3][0] — has no scale: it is exactly 0 on both sides)
        assert np.all((sc[live] > 0) | ((g[live] == 0) & (r[live] == 0))), (what, name)
    assert worst <= PARITY, (what, worst)
    return worst


def _hip_case(name, dev, slot):
    """A shared scene of camera_ref.case through the HIP path: (scene, reference for the dL/dpixel actually used, the eight
    arrays, the camera gradients, zeroed pixels)."""
    from fateavatar_amd import rasterizer
    s, f, dpix, ref = cr.case(name)
    fr = _frame(s, dev, slot)
    dpix_m, n = _mask_flips(f, fr, dpix, name)
    if n:
        ref = cr.camera_reference(s, f, dpix_m)
    with rasterizer.handle_slot(slot):
        eight, cam = _backward(fr, dpix_m)
    return s, ref, eight, cam, n


# ------------------------------------------------------------------ 1. parity, 2. self-consistency
@pytest.mark.parametrize("name", ["deg3", "deg1"])
def test_camera_gradients_match_float64_autograd(gpu_device, name):
    """The issue's scenes (260 Gaussians, 48x40, SH degree 3 seed 3 / degree 1 seed 4; 49 of 214 visible Gaussians clamped at
    seed 3).  Measured on the MI355X (profiles/r22_camera_grad.md): worst ratio 1.1e-6 / 1.2e-6 (deg3, two runs) and 1.9e-6 /
    1.4e-6 (deg1), all in the view matrix; 0 pixels zeroed."""
    _, ref, _, cam, _ = _hip_case(name, gpu_device, SLOT)
    _check(cam, ref, name)


@pytest.mark.parametrize("name", ["deg3", "deg1", "near"])
def test_rigid_motion_identity_holds_for_the_hip_gradients_alone(gpu_device, name):
    """sum_i dL/dmeans3D_i + dL/dcampos = V[:3,:3] (dV + dF Pm^T)[3,:3], evaluated from ONE HIP backward's own outputs: immune
    to threshold flips.  Both sides are sums of per-Gaussian terms held to 1e-4 of their abs-sum, so the residual is held to
    1e-4 x the abs-sum of all of them (camera_ref.identity_scale, from the reference's per-Gaussian magnitudes)."""
    s, ref, eight, (dV, dF, dcam), _ = _hip_case(name, gpu_device, SLOT + 1)
    c = s.camera
    dmeans = eight[util.GRAD_NAMES.index("dL_dmeans3D")].astype(np.float64).sum(0)
    lhs, rhs = cr.rigid_identity(c.world_view_transform, c.full_proj_transform, dmeans, dcam, dV, dF)
    scale = cr.identity_scale(c.world_view_transform, c.full_proj_transform, ref)
    print(f"[camera_grad] identity {name}: worst |lhs - rhs| / scale = {(np.abs(lhs - rhs) / scale).max():.3e}")
    assert np.all(np.abs(lhs - rhs) <= PARITY * scale), (name, lhs, rhs, scale)
    assert np.all(np.abs(lhs) > 1e-3)


# ------------------------------------------------------------------ 3. reduction shapes
GRID_CAP = 1024     # kCamMaxBlocks (csrc/fr_camera_bwd.hip): workgroups of 256 threads
# P -> the rows left in front of the camera (all others are put behind it and culled)
SHAPES = {
    1: [0],                                                                     # one workgroup, one thread's term
    4097: list(range(70)) + list(range(2000, 2060)) + list(range(4027, 4097)),   # 17 workgroups > kDoneGroups = 16; row 4096 alone in the 17th
    GRID_CAP * 256 + 1: (list(range(70)) + list(range(GRID_CAP * 256 - 40, GRID_CAP * 256 + 1))     # straddling the cap: the last row
                         + list(range(130000, 130060))),                                               # is thread 0's SECOND visit
}


def _sparse_scene(P, rows):
    s = scenes.random_scene(P, 48, 40, sh_degree=1, seed=7, M=4, spread=0.3, scale_lo=0.01, scale_hi=0.05, opacity_lo=0.2,
                            opacity_hi=0.9, bg=(0.2, 0.5, 0.9), tanfov=0.25)
    keep = np.zeros(P, bool)
    keep[rows] = True
    s.means3D[~keep, 2] = -1.0
    if P == 1:
        # beyond the guard band in x AND y (|x/z| > 0.325, |y/z| > 0.39), reaching into the image's corner: an unclamped Gaussian's
        # contributions to view[2][0] and view[2][1] cancel analytically, and one alone would leave those two entries without a scale
        s.means3D[0], s.scales[0], s.opacities[0] = (0.34, 0.40, 1.0), (0.06, 0.05, 0.055), 0.8
    sub = scenes.GaussianScene(s.means3D[keep], s.scales[keep], s.rotations[keep], s.opacities[keep], s.shs[keep], s.sh_degree,
                               s.bg, s.camera)
    return s, sub


def _pixel_scene(P, seed, camera=None, H=48, W=40):
    """Single-pixel Gaussians (module docstring): the backward of such a frame is deterministic.  (A larger image changes
    nothing in the footprint argument: the 2D covariance stays 0.3 + at most 0.007 px^2.)"""
    s = scenes.random_scene(P, H, W, sh_degree=1, seed=seed, M=4, spread=0.2, scale_lo=1e-4, scale_hi=2e-4,
                            opacity_lo=0.0045, opacity_hi=0.0058, bg=(0.2, 0.5, 0.9), tanfov=0.25)
    if camera is not None:
        s.camera = camera
    return s


def _same_bits(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, k)


@pytest.mark.parametrize("P", list(SHAPES))
def test_reduction_shapes_against_the_reference_on_the_visible_gaussians(gpu_device, P):
    """1, 17 and (grid cap + 1 row) workgroups against the reference on the ~200 Gaussians left in front of the camera.  The
    view matrix is held to 1e-4 of camera_ref's `sV_paths`: few of these Gaussians are beyond the guard band in y, so
    view[2][1] is the sum of analytically cancelling pairs, for which the net per-Gaussian abs-sum of tests 1 and 5 is ~1e-16 —
    no float32 sum of products of size 1 gets there (measured with the net scale at P = 65 537: the worst view entry 7.8e6 times
    it; with `sV_paths`: 1.9e-7, profiles/r22_camera_grad.md)."""
    from fateavatar_amd import rasterizer
    s, sub = _sparse_scene(P, SHAPES[P])
    f = util.oracle_forward(sub)
    assert int((f.radii > 0).sum()) >= min(P, 100)
    fr = _frame(s, gpu_device, SLOT + 2)
    assert int((fr.radii > 0).sum()) == int((f.radii > 0).sum())
    dpix, _ = _mask_flips(f, fr, cr.seeded_dpix(48, 40), f"P={P}")
    ref = cr.camera_reference(sub, f, dpix)
    with rasterizer.handle_slot(SLOT + 2):
        _, cam = _backward(fr, dpix)
    _check(cam, ref, f"P={P}", view_scale=ref.sV_paths)


@pytest.mark.parametrize("P", list(SHAPES))
def test_two_calls_on_the_same_frame_give_the_same_bits(gpu_device, P):
    """The workspace is left zeroed and the summation order is fixed — with every one of the P Gaussians in front of the
    camera, so that every workgroup and both visits of the strided loop add something."""
    from fateavatar_amd import rasterizer
    H, W = (192, 160) if P > 100_000 else (48, 40)     # (tile lists of ~550 instead of ~8 700 at the largest P)
    s = _pixel_scene(P, seed=11, H=H, W=W)
    if P == 1:
        s.means3D[0] = (0.0075, 0.00875, 1.0)    # (projects to (20.1, 24.2): 0.22 px from a pixel centre, inside its footprint)
    fr = _frame(s, gpu_device, SLOT + 3)
    dpix = cr.seeded_dpix(H, W)
    with rasterizer.handle_slot(SLOT + 3):
        e1, c1 = _backward(fr, dpix)
        e2, c2 = _backward(fr, dpix)
        fr2 = util.HipFrame(s, gpu_device)       # (and a whole new frame of the same data)
        e3, c3 = _backward(fr2, dpix)
    assert np.abs(c1[0]).max() > 0 and np.abs(c1[1]).max() > 0
    _same_bits(c1, c2, f"P={P}: second call")
    _same_bits(c1, c3, f"P={P}: new frame")
    _same_bits(e1, e2, f"P={P}: per-Gaussian arrays")


# ------------------------------------------------------------------ 4. nothing else moves
def test_the_flag_changes_no_other_output_and_leaves_the_handle_clean(gpu_device):
    from fateavatar_amd import rasterizer
    a, b = _pixel_scene(3000, seed=12), _pixel_scene(1800, seed=13)
    dpix = cr.seeded_dpix(48, 40)
    fa = _frame(a, gpu_device, SLOT + 4)
    with rasterizer.handle_slot(SLOT + 4):
        plain, none = _backward(fa, dpix, camera=False)
        flagged, cam = _backward(fa, dpix)
    assert none == () and len(cam) == 3
    assert max(np.abs(g).max() for g in plain if g.size) > 0
    _same_bits(plain, flagged, "the eight per-Gaussian arrays")
    # the next frame on the same handle: the accumulator rows were re-zeroed behind the camera kernel
    fb = _frame(b, gpu_device, SLOT + 4)
    with rasterizer.handle_slot(SLOT + 4):
        after, _ = _backward(fb, dpix, camera=False)
    fb_alone = _frame(b, gpu_device, SLOT + 5)
    with rasterizer.handle_slot(SLOT + 5):
        alone, _ = _backward(fb_alone, dpix, camera=False)
    _same_bits(after, alone, "the following frame")


def test_missing_arguments_are_refused(gpu_device):
    import ctypes as C
    import torch
    from fateavatar_amd import _lib, rasterizer
    s = _pixel_scene(300, seed=14)
    fr = _frame(s, gpu_device, SLOT + 4)
    g = _t(cr.seeded_dpix(48, 40), gpu_device)
    ws = rasterizer.camera_workspace(0, SLOT + 4)
    out = torch.zeros(16, device=gpu_device)
    for cam, why in ((dict(camera_workspace=ws), "d_viewmatrix"), (dict(d_viewmatrix=out), "camera_workspace")):
        v = rasterizer._backward_view(fr._backward_args(g))
        aux = rasterizer._aux(camera=cam)
        v["prm"].aux, v["prm"]._keep = C.pointer(aux), aux
        v["prm"].flags |= _lib.FR_FLAG_CAMERA_GRAD
        rc = _lib.lib().fr_backward(_lib.handle(0, SLOT + 4), C.byref(v["prm"]), C.byref(v["inp"]), v["radii"].data_ptr(),
                                    v["geom"].data_ptr(), v["img"].data_ptr(), v["binning"].data_ptr(), v["dpix"].data_ptr(),
                                    C.byref(v["grads"]), torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT and why in _lib.last_error(), (rc, _lib.last_error())
    # any ONE output is enough, and the others are not touched
    with rasterizer.handle_slot(SLOT + 4):
        only = rasterizer.rasterize_gaussians_backward(*fr._backward_args(g), _camera=(None, None, out[:3]))[8:]
        full = rasterizer.rasterize_gaussians_backward(*fr._backward_args(g), _camera=True)[8:]
    assert only[0] is None and only[1] is None and torch.equal(only[2], full[2]) and torch.all(out[3:] == 0)


# ------------------------------------------------------------------ 5. variants
def _compare_two(got, want, scale_ref, what):
    for name, g, w, sc in zip(("view", "proj", "campos"), got, want, (scale_ref.sV, scale_ref.sF, scale_ref.scam)):
        ratio = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.where(sc > 0, sc, 1.0)
        print(f"[camera_grad] {what}: {name} worst difference / scale = {ratio.max():.3e}")
        assert np.all(ratio <= PARITY), (what, name, float(ratio.max()))


def test_raw_activations_match_the_activated_call(gpu_device):
    import torch
    from fateavatar_amd import rasterizer
    s, _, dpix, ref = cr.case("deg3")
    dev = gpu_device
    raw = util._Frame()
    raw._upload(s, dev)
    raw.op, raw.scales, raw.rots = torch.log(raw.op / (1 - raw.op)), torch.log(raw.scales), raw.rots * 1.7
    act = util._Frame()
    act._upload(s, dev)
    act.op, act.scales, act.rots = torch.sigmoid(raw.op), torch.exp(raw.scales), torch.nn.functional.normalize(raw.rots)
    with rasterizer.handle_slot(SLOT + 6):
        act._take_forward(rasterizer.rasterize_gaussians(*act._forward_args()))
    with rasterizer.handle_slot(SLOT + 7):
        raw._take_forward(rasterizer.rasterize_gaussians(*raw._forward_args(), _raw=True))
    o = SimpleNamespace(color=act.color.cpu().numpy(), final_T=act.final_T.cpu().numpy())
    dpix, _ = _mask_flips(o, raw, dpix, "raw against activated")
    with rasterizer.handle_slot(SLOT + 6):
        _, want = _backward(act, dpix)
    with rasterizer.handle_slot(SLOT + 7):
        _, got = _backward(raw, dpix, _raw=True)
    assert np.abs(want[0]).max() > 0
    _compare_two(got, want, ref, "raw activations")


def test_cov3d_precomp_input(gpu_device):
    from fateavatar_amd import rasterizer
    s, f0, dpix, _ = cr.case("deg3")
    cov = f0.cov3D.copy()
    f = util.oracle_forward(s, cov3D_precomp=cov)
    fr = _frame(s, gpu_device, SLOT + 8, cov3D_precomp=cov)
    dpix, _ = _mask_flips(f, fr, dpix, "cov3D_precomp")
    ref = cr.camera_reference(s, f, dpix, cov3D=cov)
    with rasterizer.handle_slot(SLOT + 8):
        _, cam = _backward(fr, dpix)
    _check(cam, ref, "cov3D_precomp")


def test_depth_gradient_reaches_the_view_matrix(gpu_device):
    """FR_FLAG_DEPTH_ALPHA with a seeded dL/ddepth: the depth plane's dL/dz joins column 2 of dL/d(viewmatrix)."""
    from fateavatar_amd import rasterizer
    s, f, dpix, plain = cr.case("deg3")
    dev = gpu_device
    fr = util._Frame()
    fr._upload(s, dev)
    with rasterizer.handle_slot(SLOT + 9):
        res = rasterizer.rasterize_gaussians(*fr._forward_args(), _depth_alpha=True)
    fr._take_forward(res[:6])
    dpix, _ = _mask_flips(f, fr, dpix, "depth")
    flips = util.flip_pixels(f, fr.color.cpu().numpy(), fr.final_T.cpu().numpy())
    ddepth = cr.seeded_ddepth(48, 40)
    ddepth[flips] = 0
    ref = cr.camera_reference(s, f, dpix, ddepth=ddepth)
    assert np.abs(res[6].cpu().numpy() - ref.depth)[~flips].max() <= 1e-4 * np.abs(ref.depth).max()
    with rasterizer.handle_slot(SLOT + 9):
        _, cam = _backward(fr, dpix, _planes=(res[8], _t(ddepth, dev), None))
    _check(cam, ref, "depth")
    # (the depth term is there: without it column 2 of the view gradient is the plain frame's)
    assert np.abs(ref.dV[:, 2] - plain.dV[:, 2]).max() > 100 * PARITY * ref.sV[:, 2].max()


def _other_camera():
    import math
    return scenes.look_at_camera((0.25, 0.1, -0.15), (0.0, 0.0, 1.0), (0.1, -1.0, 0.05), 2 * math.atan(0.25), 2 * math.atan(0.3), 48, 40)


def test_batched_views_equal_their_single_frame_calls(gpu_device):
    """K = 2 different cameras and sizes (5 and 3 workgroups: the shorter view's workgroups past its own leave) through
    fr_backward_batch: each view's camera gradients are its single-frame call's, bit for bit."""
    import torch
    from fateavatar_amd import rasterizer
    dev = gpu_device
    ss = [_pixel_scene(1200, seed=15), _pixel_scene(700, seed=16, camera=_other_camera())]
    dpixs = [cr.seeded_dpix(48, 40), -cr.seeded_dpix(48, 40)[::-1].copy()]
    slots = [SLOT + 10, SLOT + 11]
    batch = util.HipBatch(ss, dev, slots=slots)
    res = rasterizer.rasterize_gaussians_backward_batch([v._backward_args(_t(d, dev)) for v, d in zip(batch, dpixs)], slots=slots,
                                                        camera=True)
    torch.cuda.synchronize()
    for k in range(2):
        fr = _frame(ss[k], dev, SLOT + 12)
        with rasterizer.handle_slot(SLOT + 12):
            eight, cam = _backward(fr, dpixs[k])
        got = [t.cpu().numpy() for t in res[k]]
        assert np.abs(cam[0]).max() > 0 and np.abs(cam[1]).max() > 0
        _same_bits(got[8:], cam, f"view {k}: camera gradients")
        _same_bits(got[:8], eight, f"view {k}: per-Gaussian arrays")
    with pytest.raises(RuntimeError, match="agree"):
        rasterizer.rasterize_gaussians_backward_batch([v._backward_args(_t(d, dev)) for v, d in zip(batch, dpixs)], slots=slots,
                                                      camera=[True, None])


def test_overflowed_no_wait_frame_writes_zeros(gpu_device):
    import torch
    from fateavatar_amd import rasterizer
    s = cr.case("deg3")[0]
    dev = gpu_device
    fr = util._Frame()
    fr._upload(s, dev)
    with rasterizer.handle_slot(SLOT + 13):
        fr._take_forward(rasterizer.rasterize_gaussians(*fr._forward_args()))   # (an eager frame first: the handle's buffers)
        need = int(rasterizer.last_counts[0].num_instances)
        assert need > 500
        with rasterizer.no_wait():
            v = rasterizer._forward_view(fr._forward_args())
            v["cap"] = need // 2                                                   # half the frame's instances
            fw = rasterizer._launch_forward([v], [SLOT + 13], batch=False)[0]
        fr._take_forward(tuple(fw[:6]))
        out = torch.full((35,), 7.0, device=dev)
        g = _t(cr.seeded_dpix(48, 40), dev)
        rasterizer.rasterize_gaussians_backward(*fr._backward_args(g), _camera=(out[0:16], out[16:32], out[32:35]))
        torch.cuda.synchronize()
        assert rasterizer.read_counts(0, SLOT + 13).overflow == 1
    assert torch.all(out == 0)


def _head(dev, N, res=64, seed=3):
    """The head template with single-pixel Gaussians bound to it."""
    import torch
    from tests.test_gpu_avatar import _setup
    S = _setup(dev, N, res, 4, seed=seed)
    make = S["make"]

    def mk():
        pc = make()
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            pc._scaling.fill_(-9.0)
            pc._opacity.fill_(float(np.log(0.0050 / 0.9950)))
            pc._features_dc.copy_((torch.rand(pc.P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
            pc._offset.copy_((0.2 * torch.randn(pc.P, 1, generator=g)).to(dev))
        return pc
    S["make"] = mk
    return S


def _camera_leaves(cam):
    import copy
    leaf = copy.copy(cam)
    for n in ("world_view_transform", "full_proj_transform", "camera_center"):
        setattr(leaf, n, getattr(cam, n).detach().clone().requires_grad_(True))
    return leaf


def _leaf_grads(leaf):
    return [getattr(leaf, n).grad.cpu().numpy() for n in ("world_view_transform", "full_proj_transform", "camera_center")]


def test_bound_frame_equals_the_plain_frame_of_its_bound_arrays(gpu_device):
    """A MeshBinding frame through render_bound_batch: the camera kernel reads the means3D / scales / rotations the bound
    forward wrote — its gradients are those of a plain frame rendered from those arrays, bit for bit."""
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.avatar import _BoundFrame, _RawFrame
    from fateavatar_amd.binding import face_scale
    from fateavatar_amd.bound import MeshBinding, render_bound_batch
    from fateavatar_amd.render import render
    dev = gpu_device
    S = _head(dev, 6000)
    pc, bg = S["make"](), torch.ones(3, device=dev)
    faces = S["faces"].to(torch.int32).contiguous()
    canon = face_scale(S["canon"], faces)
    gt = torch.rand(3, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    cam_b, cam_p = _camera_leaves(S["cams"][1]), _camera_leaves(S["cams"][1])
    with rasterizer.handle_slot(SLOT + 14):
        out = render_bound_batch([cam_b], [_RawFrame(pc, None)], [S["posed"][1]], MeshBinding(faces, pc.face_index, pc.bary_coords,
                                                                                               canon, 0.05, True), bg,
                                 slots=[SLOT + 14])[0]
        torch.nn.functional.l1_loss(out["render"], gt).backward()
    xyz, rot, scl = out["bound"]
    pc.begin_step()
    with rasterizer.handle_slot(SLOT + 15):
        plain = render(cam_p, _BoundFrame(xyz, pc, rot, scl, None), bg)
        torch.nn.functional.l1_loss(plain["render"], gt).backward()
    torch.cuda.synchronize()
    assert torch.equal(out["render"], plain["render"]) and int((out["radii"] > 0).sum()) > 1000
    gb, gp = _leaf_grads(cam_b), _leaf_grads(cam_p)
    assert np.abs(gb[0]).max() > 0 and np.abs(gb[1]).max() > 0
    _same_bits(gb, gp, "bound against plain")


def test_compiled_module_returns_the_same_camera_gradients(gpu_device):
    """`_C.rasterize_gaussians_backward_camera` (csrc/torch_ext.cpp, its own handle and workspace) against the ctypes host."""
    from fateavatar_amd import rasterizer, torch_ext
    m = torch_ext.load()
    s = _pixel_scene(2500, seed=17)
    fr = _frame(s, gpu_device, SLOT + 22)
    g = _t(cr.seeded_dpix(48, 40), gpu_device)
    with rasterizer.handle_slot(SLOT + 22):
        want = [t.cpu().numpy() for t in rasterizer.rasterize_gaussians_backward(*fr._backward_args(g), _camera=True)]
    res = m.rasterize_gaussians(*fr._forward_args())
    got = [t.cpu().numpy() for t in m.rasterize_gaussians_backward_camera(*fr._backward_args(g, res))]
    assert len(got) == 11 and got[8].shape == (4, 4) and got[9].shape == (4, 4) and got[10].shape == (3,)
    assert np.abs(want[8]).max() > 0
    got[2], got[5] = got[2].reshape(want[2].shape), got[5].reshape(want[5].shape)
    _same_bits(got, want, "compiled module against ctypes host")


# ------------------------------------------------------------------ 6. autograd end to end
def _pose_chain(R, T, fovx, fovy, res):
    from fateavatar_amd.model import PoseCamera
    return PoseCamera(R, T, fovx, fovy, res)


def test_pose_camera_receives_gradients_through_render(gpu_device):
    """PoseCamera(R, T) -> render() -> L1 -> backward(): R.grad and T.grad against the float64 reference chained through the
    same camera construction in float64, within 1e-4 of the chained abs-sum scale (sum over Gaussians of |J^T g_i|)."""
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.render import render
    dev = gpu_device
    s, f, _, _ = cr.case("deg3")
    c = s.camera
    res = (c.image_height, c.image_width)
    R = torch.eye(3, device=dev, requires_grad=True)
    T = torch.zeros(3, device=dev, requires_grad=True)
    cam = _pose_chain(R, T, c.FoVx, c.FoVy, res)      # (R = I, T = 0: the scene's own camera, bit for bit)

    class Holder:                                      # the scene's activated values as they are (render()'s getters)
        max_sh_degree = s.sh_degree
        get_xyz, get_features, get_opacity = _t(s.means3D, dev), _t(s.shs, dev), _t(s.opacities, dev)
        get_scaling, get_rotation = _t(s.scales, dev), _t(s.rotations, dev)
    bg = _t(s.bg, dev)
    target = torch.rand(3, *res, generator=torch.Generator().manual_seed(3)).to(dev)
    # pixels where HIP and oracle blended different sets take no part in the loss, on either side
    fr = _frame(s, dev, SLOT + 16)
    flips = util.flip_pixels(f, fr.color.cpu().numpy(), fr.final_T.cpu().numpy())
    print(f"[camera_grad] autograd: {int(flips.sum())} of {flips.size} pixels zeroed")
    assert int(flips.sum()) <= flips.size // 100
    keep = _t((~flips).astype(np.float32), dev)
    with rasterizer.handle_slot(SLOT + 16):
        img = render(cam, Holder, bg)["render"]
        assert torch.equal(img.detach(), fr.color)
        ((img - target).abs() * keep).sum().div(img.numel()).backward()
    assert T.grad is not None and R.grad is not None
    dpix = (torch.sign(img.detach() - target) * keep / img.numel()).cpu().numpy().astype(np.float32)
    ref = cr.camera_reference(s, f, dpix)
    R64 = torch.eye(3, dtype=torch.float64, requires_grad=True)
    T64 = torch.zeros(3, dtype=torch.float64, requires_grad=True)

    def chain(Rm, Tv):
        cm = _pose_chain(Rm, Tv, c.FoVx, c.FoVy, res)
        return torch.cat([cm.world_view_transform.reshape(-1), cm.full_proj_transform.reshape(-1), cm.camera_center])
    JR, JT = torch.autograd.functional.jacobian(chain, (R64, T64))       # [35,3,3], [35,3]
    per = np.concatenate([ref.pV.reshape(-1, 16), ref.pF.reshape(-1, 16), ref.pcam], 1)       # [P,35] per-Gaussian gradients
    for name, J, got in (("R", JR.reshape(35, 9).numpy(), R.grad.cpu().numpy().reshape(-1)), ("T", JT.numpy(), T.grad.cpu().numpy())):
        contrib = per @ J                                   # [P, n]: each Gaussian's share of the chained gradient
        want, scale = contrib.sum(0), np.abs(contrib).sum(0)
        ratio = np.abs(got - want) / scale
        print(f"[camera_grad] autograd: {name}.grad worst |hip - ref| / scale = {ratio.max():.3e}")
        assert np.all(scale > 0) and np.all(ratio <= PARITY), (name, got, want, scale)


# ------------------------------------------------------------------ 7. the step
def test_avatar_step_keeps_the_camera_gradients(gpu_device):
    """AvatarStep(camera_grad=True) on the head template at 64x64: d_view / d_proj / d_campos after a graph replay are the
    eager step's bits, the first step's are autograd's through camera leaves on the same frame, and the parameters after three
    steps are those of camera_grad=False."""
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.avatar import AvatarStep, _RawFrame
    from fateavatar_amd.bound import render_bound_batch
    from fateavatar_amd.loss import l1_loss_and_grad
    dev = gpu_device
    S = _head(dev, 6000)
    bg = torch.ones(3, device=dev)
    gts = [torch.rand(3, 64, 64, generator=torch.Generator().manual_seed(10 + k)).to(dev) for k in range(4)]

    def run(slot, steps, **kw):
        pc = S["make"]()
        with rasterizer.handle_slot(slot):
            st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), bg, **kw)
            grads = []
            for it in range(steps):
                st.step(S["cams"][it % 4], S["posed"][it % 4], gts[it % 4])
                torch.cuda.synchronize()
                if st.camera_grad:
                    grads.append([t.clone().cpu().numpy() for t in (st.d_view, st.d_proj, st.d_campos)])
            st.check()
        return pc, st, grads

    pc_e, st_e, g_e = run(SLOT + 17, 4, use_graph=False, camera_grad=True)
    pc_g, st_g, g_g = run(SLOT + 18, 4, use_graph=True, camera_grad=True)
    assert st_g._graph is not None and st_e._graph is None, "steps 3 and 4 of the second run are graph replays"
    for it in range(4):
        assert np.abs(g_e[it][0]).max() > 0 and np.abs(g_e[it][1]).max() > 0 and g_e[it][0].shape == (4, 4) and g_e[it][2].shape == (3,)
        _same_bits(g_g[it], g_e[it], f"step {it}: graph against eager")
    assert torch.equal(pc_g.flat, pc_e.flat)
    pc_0, st_0, _ = run(SLOT + 19, 3, use_graph=False)
    pc_3, st_3, _ = run(SLOT + 20, 3, use_graph=False, camera_grad=True)
    assert st_0.d_view is None and torch.equal(pc_3.flat, pc_0.flat), "camera_grad changes no parameter"
    # the first step's frame through autograd with camera leaves
    pc = S["make"]()
    st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), bg, use_graph=False)
    leaf = _camera_leaves(S["cams"][0])
    with rasterizer.handle_slot(SLOT + 21):
        out = render_bound_batch([leaf], [_RawFrame(pc, None)], [S["posed"][0]], st._binding(pc), bg, slots=[SLOT + 21])[0]
        _, g = l1_loss_and_grad(out["render"], gts[0])
        out["render"].backward(g)
    torch.cuda.synchronize()
    _same_bits(_leaf_grads(leaf), g_e[0], "step 0 against autograd")


def test_the_other_steps_refuse_camera_grad(gpu_device):
    import torch
    from fateavatar_amd.avatar import AvatarBatchStep
    from fateavatar_amd.train import BoundStep
    S = _head(gpu_device, 500)
    with pytest.raises(NotImplementedError, match="camera_grad"):
        AvatarBatchStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), torch.ones(3, device=gpu_device), camera_grad=True)
    assert BoundStep.CAMERA_GRAD is False
