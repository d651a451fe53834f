"""GPU: depth and alpha planes (FR_FLAG_DEPTH_ALPHA, include/fr_rasterizer.h).

The reference is the project's own pinned path: the depth plane is what a frame of the same Gaussians renders in colour
channel 0 with colors_precomp = (z, 0, 0) (z: the view-space depth, computed in torch) over bg = (0, 1, 0), and the alpha
plane is 1 - channel 1 of that frame.  Gradients of <gC, C> + <gD, D> + <gA, A> from ONE planes frame are compared with the
sum over the plain frame (gC) and that composite frame (gD on channel 0, -gA on channel 1), dL/dz carried into means3D in
torch.  Frames with planes leave every plain output as it was, bit for bit.

Where the planes meet the CPU oracle directly (long tile lists, every sort tier, dead trailing units, one plane gradient at a
time): tests/test_gpu_planes_long_lists.py, with the reference of tests/planes_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fateavatar_amd import _lib, scenes
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 220          # the handles of this module: 220 .. 231 (no other module uses them)
PARITY = 1e-4       # aggregate rel-L2 of the gradients (tests/test_gpu_parity.py)


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch, gpu_device):
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _view(s, kw, dev, raw=False):
    v = util._Frame()
    v._upload(s, dev, **kw)
    v.raw = raw
    if raw:   # the raw parameters whose activations are the scene's
        import torch
        v.op = torch.log(v.op / (1 - v.op))
        if v.scales.numel():
            v.scales = torch.log(v.scales)
    return v


def _z(v):
    """View-space depth of every mean, in torch (row-major "transposed" view matrix: z = m[2] x + m[6] y + m[10] z + m[14])."""
    m = v.view.reshape(-1)
    return v.means3D[:, 0] * m[2] + v.means3D[:, 1] * m[6] + v.means3D[:, 2] * m[10] + m[14]


def _composite_args(v):
    """The forward arguments of the composite frame: colours (z, 0, 0), background (0, 1, 0), the same geometry."""
    import torch
    a = list(v._forward_args())
    z = _z(v)
    a[0] = torch.tensor([0.0, 1.0, 0.0], device=v.dev)
    a[2] = torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1).contiguous()
    a[14] = torch.empty(0)
    return a


def _composite_bwd_args(v, res, g):
    import torch
    a = list(v._backward_args(g, res[:6]))
    z = _z(v)
    a[0] = torch.tensor([0.0, 1.0, 0.0], device=v.dev)
    a[3] = torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1).contiguous()
    a[13] = torch.empty(0)
    return a


def _bits(res, H, W):
    from fateavatar_amd import rasterizer
    fT, nc = rasterizer.image_aux(res[5], H, W)
    return [res[1].cpu().numpy(), res[2].cpu().numpy(), fT.cpu().numpy(), nc.cpu().numpy()]


def _same_bits(a, b, what):
    for name, x, y in zip(("image", "radii", "final_T", "n_contrib"), a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, name)


def _check_planes_forward(v, res_pl, res_plain, res_comp, what):
    """(1) plain bits unchanged, (2) alpha = 1 - final_T, empty pixels 0, (3) the composite oracle."""
    H, W = v.H, v.W
    _same_bits(_bits(res_pl, H, W), _bits(res_plain, H, W), what)
    depth, alpha = res_pl[6].cpu().numpy(), res_pl[7].cpu().numpy()
    fT = _bits(res_pl, H, W)[2]
    assert np.array_equal(alpha.view(np.uint32), (np.float32(1) - fT).view(np.uint32)), what
    empty = _bits(res_pl, H, W)[3] == 0
    assert np.all(depth[empty] == 0) and np.all(alpha[empty] == 0), what
    assert np.isfinite(depth).all() and np.isfinite(alpha).all(), what
    comp = res_comp[1].cpu().numpy()
    assert np.all(np.abs(depth - comp[0]) <= 1e-6 * np.abs(comp[0]) + 1e-30), (what, float(np.abs(depth - comp[0]).max()))
    assert np.array_equal((np.float32(1) - comp[1]).view(np.uint32), alpha.view(np.uint32)), what


def _grad_targets(v, seed):
    import torch
    r = np.random.default_rng(seed)
    H, W = v.H, v.W
    gC = _t((r.uniform(-1, 1, (3, H, W)) / (H * W)).astype(np.float32), v.dev)
    gD = _t((r.uniform(-1, 1, (H, W)) / (H * W)).astype(np.float32), v.dev)
    gA = _t((r.uniform(-1, 1, (H, W)) / (H * W)).astype(np.float32), v.dev)
    comp = torch.stack([gD, -gA, torch.zeros_like(gD)]).contiguous()
    return gC, gD, gA, comp


def _expected(v, g_plain, g_comp):
    """Sum of the plain frame's and the composite frame's gradients, dL/dz (colour 0 of the composite frame) through z."""
    m = v.view.reshape(-1)
    dz = g_comp[1][:, 0:1]
    exp = {}
    for k, a, b in zip(util.GRAD_NAMES, g_plain, g_comp):
        if a is None:
            continue
        if k in ("dL_dcolors", "dL_dsh"):
            exp[k] = a                                        # (the composite colours are not the frame's parameters)
        elif k == "dL_dmeans3D":
            exp[k] = a + b + dz * m[[2, 6, 10]].view(1, 3)
        else:
            exp[k] = a + b
    return exp


def _compare(got, exp, what):
    for k, e in exp.items():
        g = got[util.GRAD_NAMES.index(k)]
        if e.numel() == 0:
            continue
        g, e = g.cpu().numpy(), e.cpu().numpy()
        assert np.isfinite(g).all(), (what, k)
        assert util.rel_l2(g, e) <= PARITY, (what, k, util.rel_l2(g, e))


def composite_single(s, kw, slot, what, raw=False):
    """One frame: forward bits, alpha, composite forward and gradient oracle; null plane gradients."""
    import torch
    from fateavatar_amd import rasterizer
    dev = torch.device("cuda:0")
    v = _view(s, kw, dev, raw)
    with rasterizer.handle_slot(slot):
        res_plain = rasterizer.rasterize_gaussians(*v._forward_args(), _raw=raw)
        res_pl = rasterizer.rasterize_gaussians(*v._forward_args(), _raw=raw, _depth_alpha=True)
    with rasterizer.handle_slot(slot + 1):
        res_comp = rasterizer.rasterize_gaussians(*_composite_args(v), _raw=raw)
    torch.cuda.synchronize()
    _check_planes_forward(v, res_pl, res_plain, res_comp, what)
    gC, gD, gA, gcomp = _grad_targets(v, slot)
    with rasterizer.handle_slot(slot):
        g_pl = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _raw=raw, _planes=(res_pl[8], gD, gA))
        g_plain = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _raw=raw)
    with rasterizer.handle_slot(slot + 1):
        g_comp = rasterizer.rasterize_gaussians_backward(*_composite_bwd_args(v, res_comp, gcomp), _raw=raw)
    torch.cuda.synchronize()
    _compare(g_pl, _expected(v, g_plain, g_comp), what)
    return v, res_pl, g_plain


CFG2 = dict(P=100_000, res=512, sh_degree=3, seed=0)


# ------------------------------------------------------------------ single frames: (1) - (4)
@pytest.mark.parametrize("group", range(4))
def test_fuzz_scenes_composite_oracle(group):
    for k in range(group * 3, group * 3 + 3):
        _, P, H, W, kw, _, name = util.fuzz_case(11, k)
        s = scenes.random_scene(P, H, W, **kw)
        composite_single(s, util.fuzz_inputs(11, k, s), SLOT, name)


@pytest.mark.parametrize("opacity", [0.1, 0.9])
def test_config2_composite_oracle(opacity):
    s = scenes.head_scene(**CFG2, opacity=opacity)
    composite_single(s, {}, SLOT, f"config2 op={opacity}")


def test_raw_activations_scale_modifier_and_cov3d():
    s = scenes.head_scene(P=20000, res=256, sh_degree=3, seed=3, opacity=0.6)
    composite_single(s, {}, SLOT, "raw", raw=True)
    composite_single(s, {"scale_modifier": 0.7}, SLOT, "scale_modifier")
    cov = util.oracle_forward(s).cov3D.copy()
    composite_single(s, {"cov3D_precomp": cov}, SLOT, "cov3D_precomp")


# ------------------------------------------------------------------ (6) null plane gradients
def test_null_plane_gradients_and_clean_accumulators():
    import torch
    from fateavatar_amd import rasterizer
    s = scenes.head_scene(P=30000, res=256, sh_degree=3, seed=7, opacity=0.5)
    v, res_pl, g_plain = composite_single(s, {}, SLOT + 2, "null")
    gC = _grad_targets(v, SLOT + 2)[0]
    zeros = torch.zeros((v.H, v.W), device=v.dev)
    _, gD, gA, _ = _grad_targets(v, 77)
    with rasterizer.handle_slot(SLOT + 2):
        # both NULL: the plain kernels; both zero: the planes kernels with nothing to add
        g_null = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _planes=(res_pl[8], None, None))
        g_zero = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _planes=(res_pl[8], zeros, zeros))
        g_after = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]))
        # two planes backward passes one behind the other on one handle: a dL/dz (ACC_Z) left in the accumulator rows by
        # the first would reach dL_dmeans3D of the second, which reads that slot
        g_pl1 = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _planes=(res_pl[8], gD, gA))
        g_pl2 = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _planes=(res_pl[8], gD, gA))
        g_pl3 = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _planes=(res_pl[8], gD, None))
        g_pl4 = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _planes=(res_pl[8], gD, None))
    with rasterizer.handle_slot(SLOT + 3):   # (a fresh handle's accumulators)
        g_fresh = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _planes=(res_pl[8], gD, None))
    torch.cuda.synchronize()
    for got, want, what in ((g_null, g_plain, "NULL"), (g_zero, g_plain, "zero"), (g_after, g_plain, "plain after planes"),
                            (g_pl2, g_pl1, "planes after planes"), (g_pl3, g_fresh, "depth only after planes"),
                            (g_pl4, g_fresh, "depth only twice")):
        for k, a, b in zip(util.GRAD_NAMES, got, want):
            if a is not None and a.numel():
                assert util.rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-5, (what, k)
    assert float(g_pl1[3].abs().max()) > 0


def test_accumulate_into_the_callers_gradients():
    """FR_FLAG_ACCUMULATE with planes: each array = what it held + the composite oracle's gradient."""
    import torch
    from fateavatar_amd import rasterizer
    dev = torch.device("cuda:0")
    s = scenes.head_scene(P=20000, res=256, sh_degree=3, seed=12, opacity=0.5)
    v = _view(s, {}, dev)
    with rasterizer.handle_slot(SLOT + 4):
        res_pl = rasterizer.rasterize_gaussians(*v._forward_args(), _depth_alpha=True)
    with rasterizer.handle_slot(SLOT + 5):
        res_comp = rasterizer.rasterize_gaussians(*_composite_args(v))
    gC, gD, gA, gcomp = _grad_targets(v, 13)
    with rasterizer.handle_slot(SLOT + 4):
        g_plain = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]))
    with rasterizer.handle_slot(SLOT + 5):
        g_comp = rasterizer.rasterize_gaussians_backward(*_composite_bwd_args(v, res_comp, gcomp))
    exp = _expected(v, g_plain, g_comp)
    names = ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_drotations")
    g = torch.Generator(device="cpu").manual_seed(5)
    held = {k: (torch.randn(exp[k].shape, generator=g) * float(exp[k].abs().mean())).to(dev) for k in names}
    out = {k: t.clone() for k, t in held.items()}
    with rasterizer.handle_slot(SLOT + 4):
        got = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res_pl[:6]), _planes=(res_pl[8], gD, gA), _out=out,
                                                      _accumulate=names)
    torch.cuda.synchronize()
    _compare(got, {k: held[k] + exp[k] for k in names}, "accumulate")


# ------------------------------------------------------------------ (7) a plane gradient for a frame without planes
def test_backward_refuses_plane_gradients_of_a_plain_frame():
    import torch
    from fateavatar_amd import rasterizer
    s = scenes.head_scene(P=20000, res=256, sh_degree=3, seed=8, opacity=0.5)
    dev = torch.device("cuda:0")
    v = _view(s, {}, dev)
    with rasterizer.handle_slot(SLOT + 3):
        res_pl = rasterizer.rasterize_gaussians(*v._forward_args(), _depth_alpha=True)
        res = rasterizer.rasterize_gaussians(*v._forward_args())
        gC, gD, gA, _ = _grad_targets(v, 5)
        ref = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res[:6]))
        for planes in ((res_pl[8], gD, None), (res_pl[8], None, gA)):
            with pytest.raises(RuntimeError, match=r"code 1\)"):
                rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res[:6]), _planes=planes)
        again = rasterizer.rasterize_gaussians_backward(*v._backward_args(gC, res[:6]))   # (nothing was enqueued)
    torch.cuda.synchronize()
    for k, a, b in zip(util.GRAD_NAMES, again, ref):
        if a is not None and a.numel():
            assert util.rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-5, k


# ------------------------------------------------------------------ (8) non-finite Gaussians
def test_non_finite_gaussians_leave_finite_planes():
    import torch
    from fateavatar_amd import rasterizer
    dev = torch.device("cuda:0")
    s = scenes.head_scene(P=20000, res=256, sh_degree=3, seed=9, opacity=0.6)
    bad = s.shs.copy()
    bad[::7, 0, 0] = np.nan
    bad[3::11, 0, 1] = np.inf
    out = []
    for shs in (s.shs, bad):
        s2 = scenes.GaussianScene(**{**s.__dict__, "shs": shs})
        v = _view(s2, {}, dev)
        with rasterizer.handle_slot(SLOT + 4):
            r = rasterizer.rasterize_gaussians(*v._forward_args(), _depth_alpha=True)
        torch.cuda.synchronize()
        out.append((r[6].cpu().numpy(), r[7].cpu().numpy(), r[1].cpu().numpy()))
    # the non-finite Gaussians are not blended: the planes are those of the scene without them
    keep = np.ones(s.P, bool)
    keep[::7] = False
    keep[3::11] = False
    s3 = scenes.GaussianScene(**{**s.__dict__, **{k: getattr(s, k)[keep] for k in ("means3D", "shs", "opacities", "scales",
                                                                                  "rotations")}})
    v = _view(s3, {}, dev)
    with rasterizer.handle_slot(SLOT + 5):
        r = rasterizer.rasterize_gaussians(*v._forward_args(), _depth_alpha=True)
    torch.cuda.synchronize()
    d, a = out[1][0], out[1][1]
    assert np.isfinite(d).all() and np.isfinite(a).all()
    # (alpha to the bit; the depth to the summation order of a tile's rows, which the dead units behind the real ones may change)
    assert np.array_equal(a.view(np.uint32), r[7].cpu().numpy().view(np.uint32))
    dc = r[6].cpu().numpy()
    assert np.all(np.abs(d - dc) <= 1e-6 * np.abs(dc) + 1e-30)


# ------------------------------------------------------------------ batches: (1), (3), (4) per view
class _ArgsView:
    """A view given by `rasterize_gaussians`' positional arguments (tests/test_known_answers.py: hip_forward_args)."""

    def __init__(self, fwd, dev):
        self.fwd, self.dev = tuple(fwd), dev
        self.means3D, self.view, self.H, self.W = fwd[1], fwd[8], int(fwd[12]), int(fwd[13])

    def _forward_args(self):
        return self.fwd

    def _backward_args(self, g, res):
        a = self.fwd
        R, _, radii, geom, binning, img = res
        return (a[0], a[1], radii, a[2], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], g, a[14], a[15], a[16], geom, R,
                binning, img, False)


def _batch_case(views, slots, what, forward_only=False):
    import torch
    from fateavatar_amd import rasterizer
    res_plain = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots)
    res_pl = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots, depth_alpha=True,
                                                  forward_only=forward_only)
    res_comp = rasterizer.rasterize_gaussians_batch([_composite_args(v) for v in views], slots=[x + 4 for x in slots])
    torch.cuda.synchronize()
    for k, v in enumerate(views):
        _check_planes_forward(v, res_pl[k], res_plain[k], res_comp[k], (what, k))
    if forward_only:
        return
    tg = [_grad_targets(v, 100 + k) for k, v in enumerate(views)]   # (every view its own plane gradients)
    g_pl = rasterizer.rasterize_gaussians_backward_batch([v._backward_args(t[0], r[:6]) for v, t, r in zip(views, tg, res_pl)],
                                                         slots=slots, planes=[(r[8], t[1], t[2]) for t, r in zip(tg, res_pl)])
    g_plain = rasterizer.rasterize_gaussians_backward_batch([v._backward_args(t[0], r[:6]) for v, t, r in zip(views, tg, res_pl)],
                                                            slots=slots)
    g_comp = rasterizer.rasterize_gaussians_backward_batch([_composite_bwd_args(v, r, t[3]) for v, t, r in zip(views, tg, res_comp)],
                                                           slots=[x + 4 for x in slots])
    torch.cuda.synchronize()
    for k, v in enumerate(views):
        _compare(g_pl[k], _expected(v, g_plain[k], g_comp[k]), (what, k))


@pytest.mark.parametrize("group", range(2))
def test_mixed_fuzz_batches(group):
    scs, kws = [], []
    for k in range(group * 4, group * 4 + 4):
        _, P, H, W, kw, _, _ = util.fuzz_case(12, k)
        s = scenes.random_scene(P, H, W, **kw)
        scs.append(s)
        kws.append(util.fuzz_inputs(12, k, s))
    import torch
    dev = torch.device("cuda:0")
    _batch_case([_view(s, kw, dev) for s, kw in zip(scs, kws)], [SLOT + k for k in range(4)], f"fuzz batch {group}")


@pytest.mark.parametrize("group", range(6))
def test_known_answer_fixtures_in_batches(group):
    """The 24 fixtures of tests/golden/known_answers.npz, four per batch (the batches of test_gpu_batch_parity): planes frames,
    full and forward-only, against the composite oracle."""
    import torch
    from tests import test_known_answers as ka
    from tests.test_gpu_batch_parity import KA_BATCHES
    dev = torch.device("cuda:0")
    views = [_ArgsView(ka.hip_forward_args(ka._scene(n)[0], dev)[0], dev) for n in KA_BATCHES[group]]
    slots = [SLOT + k for k in range(4)]
    _batch_case(views, slots, f"fixtures {group}")
    _batch_case(views, slots, f"fixtures {group} forward-only", forward_only=True)


# ------------------------------------------------------------------ the Python entry points
def test_render_entry_points_return_the_planes():
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    from fateavatar_amd.render import render, render_batch
    dev = torch.device("cuda:0")
    s = scenes.head_scene(P=20000, res=256, sh_degree=3, seed=31, opacity=0.5)
    cam, bg = TorchCamera(s.camera, dev), torch.from_numpy(s.bg).to(dev)
    pc = FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, s.sh_degree, dev, fused_activations=True)
    with rasterizer.handle_slot(SLOT + 8):
        plain = render(cam, pc, bg)
        out = render(cam, pc, bg, depth_alpha=True)
        assert set(out) == set(plain) | {"depth", "alpha"} and "depth" not in plain
        assert out["depth"].shape == (1, 256, 256) and out["alpha"].shape == (1, 256, 256)
        assert torch.equal(out["render"], plain["render"])
        with torch.no_grad():
            fo = render(cam, pc, bg, depth_alpha=True)
        assert rasterizer.last_forward_only[0] is True
        assert torch.equal(fo["depth"], out["depth"]) and torch.equal(fo["alpha"], out["alpha"])
        (out["alpha"].sum() + out["depth"].mean()).backward()
    torch.cuda.synchronize()
    g = pc.grad_of("_xyz")
    assert torch.isfinite(g).all() and g.abs().sum() > 0
    outs = render_batch([cam, cam], pc, bg, slots=[SLOT + 9, SLOT + 10], depth_alpha=True)
    for o in outs:
        assert torch.equal(o["depth"], out["depth"]) and torch.equal(o["alpha"], out["alpha"])


def _bound_frames(apc, mb, acams, posed, slots, depth_alpha):
    """render_bound_batch's launch (rasterize_gaussians_batch with fr_aux::binding) at the buffer level: per view the bits,
    the visibility mask, the bound arrays and the result tuple."""
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.avatar import _RawFrame
    from fateavatar_amd.binding import SHELL, _chk, _describe
    from fateavatar_amd.render import _settings
    bg = torch.ones(3, device=apc._offset.device)
    views, viss, descs, bound, keep = [], [], [], [], []
    for k, cam in enumerate(acams):
        N, dev = apc.P, apc._offset.device
        xyz, rot, scl = (torch.empty((N, c), device=dev) for c in (3, 4, 3))
        # (the descriptor holds raw pointers: every tensor it names stays referenced until the launch)
        t = [_chk(posed[k], torch.float32, "verts"), _chk(mb.faces, torch.int32, "faces"), _chk(mb.face_index, torch.int32, "fi"),
             _chk(apc._offset.detach(), torch.float32, "offset"), _chk(apc._rotation.detach(), torch.float32, "rotation"),
             _chk(apc._scaling.detach(), torch.float32, "scaling"),
             _chk(mb.bary_coords, torch.float32, "bary"), _chk(mb.face_scale_canonical, torch.float32, "canon")]
        keep.append(t)
        descs.append(_describe(SHELL, *t, mb.shell_len, mb.resize_scale))
        rs = _settings(cam, _RawFrame(apc, None), bg, 1.0)
        views.append(rasterizer._forward_args(rs, xyz, None, apc._features_dc.detach(), torch.empty(0), apc._opacity.detach(), scl,
                                              rot, torch.empty(0)))
        viss.append(torch.empty((N,), dtype=torch.bool, device=dev))
        bound.append((xyz, rot, scl))
    res = rasterizer.rasterize_gaussians_batch(views, slots=slots, raw=True, visibles=viss, bindings=descs, depth_alpha=depth_alpha)
    torch.cuda.synchronize()
    return [(_bits(r, v[12], v[13]) + [m.cpu().numpy()] + [t.cpu().numpy() for t in b], r)
            for r, v, m, b in zip(res, views, viss, bound)]


def test_bound_batch_planes_bits():
    """render_bound_batch's frames with planes: image, radii, final_T, n_contrib, visible and the bound arrays of the plain
    frame, bit for bit; alpha = 1 - final_T."""
    import torch
    from tests.test_gpu_forward_only import _bound_setup
    dev = torch.device("cuda:0")
    apc, mb, acams, posed = _bound_setup(dev)
    slots = [SLOT + 8 + k for k in range(4)]
    a = _bound_frames(apc, mb, acams[:4], posed, slots, False)
    b = _bound_frames(apc, mb, acams[:4], posed, slots, True)
    for k, ((x, _), (y, r)) in enumerate(zip(a, b)):
        for name, p, q in zip(("image", "radii", "final_T", "n_contrib", "visible", "xyz", "rotation", "scaling"), x, y):
            assert p.shape == q.shape and np.array_equal(p.view(np.uint8), q.view(np.uint8)), (k, name)
        alpha = r[7].cpu().numpy()
        assert np.array_equal(alpha.view(np.uint32), (np.float32(1) - y[2]).view(np.uint32)), k
        assert (alpha > 0).any() and np.isfinite(r[6].cpu().numpy()).all()


def test_bound_batch_planes_gradients_match_the_composite_oracle():
    """<gC, C> + <gD, D> + <gA, A> through render_bound_batch(depth_alpha=True) against the stand-alone binding op
    (bind_gaussians) followed by the plain frame (gC) and the composite frame (gD, -gA) with z taken from the bound means in
    torch: the gradients of offset, rotation, scaling, opacity, colour and the posed vertices."""
    import types

    import torch
    from fateavatar_amd.avatar import _RawFrame
    from fateavatar_amd.binding import bind_gaussians
    from fateavatar_amd.bound import render_bound_batch
    from fateavatar_amd.rasterizer import rasterize_views_autograd
    from fateavatar_amd.render import _settings
    from tests.test_gpu_forward_only import _bound_setup
    dev = torch.device("cuda:0")
    apc, mb, acams, posed = _bound_setup(dev)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():   # (anisotropic, rotated splats: the template's are isotropic, its rotation gradient is rounding noise)
        apc._offset.add_((0.2 * torch.randn(apc.P, 1, generator=g)).to(dev))
        apc._scaling.add_((0.5 * torch.randn(apc.P, 3, generator=g)).to(dev))
        apc._rotation.add_((0.5 * torch.randn(apc.P, 4, generator=g)).to(dev))
    K = 2
    cams = acams[:K]
    bg = torch.ones(3, device=dev)
    r = np.random.default_rng(21)
    tg = []
    for _ in range(K):
        H, W = int(cams[0].image_height), int(cams[0].image_width)
        gC = _t((r.uniform(-1, 1, (3, H, W)) / (H * W)).astype(np.float32), dev)
        gD = _t((r.uniform(-1, 1, (1, H, W)) / (H * W)).astype(np.float32), dev)
        gA = _t((r.uniform(-1, 1, (1, H, W)) / (H * W)).astype(np.float32), dev)
        tg.append((gC, gD, gA))
    names = ("_opacity", "_offset", "_features_dc", "_rotation", "_scaling")

    def run(folded):
        leaves = {n: getattr(apc, n).detach().clone().requires_grad_(True) for n in names}
        pc = types.SimpleNamespace(**leaves, face_index=apc.face_index, bary_coords=apc.bary_coords)
        verts = [posed[k].clone().requires_grad_(True) for k in range(K)]
        loss = 0.0
        if folded:
            outs = render_bound_batch(cams, [_RawFrame(pc, None)] * K, verts, mb, bg, slots=[SLOT + k for k in range(K)],
                                      depth_alpha=True)
            for o, (gC, gD, gA) in zip(outs, tg):
                loss = loss + (o["render"] * gC).sum() + (o["depth"] * gD).sum() + (o["alpha"] * gA).sum()
        else:
            faces = mb.faces.to(torch.int32).contiguous()
            empty = torch.empty(0)
            for k, (cam, (gC, gD, gA)) in enumerate(zip(cams, tg)):
                xyz, rot, scl = bind_gaussians(verts[k], faces, mb.face_index, mb.bary_coords, mb.face_scale_canonical,
                                               pc._offset, pc._rotation, pc._scaling, mb.shell_len, mb.resize_scale)
                rs = _settings(cam, _RawFrame(pc, None), bg, 1.0)
                m = rs.viewmatrix.reshape(-1)
                z = xyz[:, 0] * m[2] + xyz[:, 1] * m[6] + xyz[:, 2] * m[10] + m[14]
                comp = torch.stack([z, torch.zeros_like(z), torch.zeros_like(z)], 1).contiguous()
                rs_c = rs._replace(bg=torch.tensor([0.0, 1.0, 0.0], device=dev))
                sp = [torch.zeros_like(xyz, requires_grad=True) for _ in range(2)]
                (c_plain, _), = rasterize_views_autograd([rs], [(xyz, sp[0], pc._features_dc, empty, pc._opacity, scl, rot, empty)],
                                                         raw_activations=True, slots=[SLOT + 2 + k])
                (c_comp, _), = rasterize_views_autograd([rs_c], [(xyz, sp[1], empty, comp, pc._opacity, scl, rot, empty)],
                                                        raw_activations=True, slots=[SLOT + 4 + k])
                loss = loss + (c_plain * gC).sum() + (c_comp[0] * gD[0]).sum() - (c_comp[1] * gA[0]).sum()
        loss.backward()
        torch.cuda.synchronize()
        return {**{n: leaves[n].grad for n in names}, **{f"verts{k}": verts[k].grad for k in range(K)}}

    got, want = run(True), run(False)
    for n in want:
        a, b = got[n], want[n]
        assert a is not None and b is not None and a.shape == b.shape, n
        assert torch.isfinite(a).all() and float(b.abs().max()) > 0, n
        assert util.rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= PARITY, (n, util.rel_l2(a.cpu().numpy(), b.cpu().numpy()))


# ------------------------------------------------------------------ captured graphs
def test_planes_chains_replayed_as_graphs_match_eager():
    """Three 4-view launch chains of config-2 views with planes, forward and backward (plane gradients per view), each
    captured on its own stream and replayed in flight together: images, radii, final_T, n_contrib, depth and alpha are the
    eager frames' bits, the gradients theirs to the order of float atomics."""
    import torch
    from fateavatar_amd import rasterizer
    dev = torch.device("cuda:0")
    scs = [scenes.head_scene(view=k, n_views=12, opacity=0.5) for k in range(12)]
    chains = []
    for c in range(3):
        slots = [SLOT + 4 * c + j for j in range(4)]
        views = [_view(s, {}, dev) for s in scs[4 * c:4 * c + 4]]
        tg = [_grad_targets(v, 400 + 4 * c + k) for k, v in enumerate(views)]

        def frame():
            fw = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots, depth_alpha=True)
            gr = rasterizer.rasterize_gaussians_backward_batch([v._backward_args(t[0], r[:6]) for v, t, r in zip(views, tg, fw)],
                                                               slots=slots, planes=[(r[8], t[1], t[2]) for t, r in zip(tg, fw)])
            return fw, gr

        fw, gr = frame()
        torch.cuda.synchronize()
        want = [_bits(r, 512, 512) + [r[6].cpu().numpy(), r[7].cpu().numpy()] for r in fw]
        want_g = [[None if t is None else t.cpu().numpy() for t in g] for g in gr]
        stream = torch.cuda.Stream(device=dev)
        with rasterizer.no_wait():
            stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(stream):
                frame()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
                fw, gr = frame()
        for r in fw:   # (garbage the replays must overwrite)
            r[1].fill_(-1.0), r[2].fill_(-7), r[6].fill_(-3.0), r[7].fill_(-5.0)
        for gg in gr:
            for t in gg:
                if t is not None:
                    t.fill_(123.0)
        chains.append(dict(graph=g, stream=stream, fw=fw, gr=gr, want=want, want_g=want_g, slots=slots, views=views, tg=tg))
    torch.cuda.synchronize()
    for _ in range(3):
        for ch in chains:
            with torch.cuda.stream(ch["stream"]):
                ch["graph"].replay()
    torch.cuda.synchronize()
    for c, ch in enumerate(chains):
        for k, (r, sl) in enumerate(zip(ch["fw"], ch["slots"])):
            with rasterizer.handle_slot(sl):
                assert not rasterizer.check_async_overflow(0), (c, k)
            got = _bits(r, 512, 512) + [r[6].cpu().numpy(), r[7].cpu().numpy()]
            for name, a, b in zip(("image", "radii", "final_T", "n_contrib", "depth", "alpha"), got, ch["want"][k]):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (c, k, name)
            for name, a, b in zip(util.GRAD_NAMES, ch["gr"][k], ch["want_g"][k]):
                if a is not None and a.numel():
                    assert util.rel_l2(a.cpu().numpy(), b) < 1e-5, (c, k, name)


# ------------------------------------------------------------------ (5) both forms of both blend kernels, and the gather launch
@pytest.mark.parametrize("env", [{"FR_DENSE_PAIRS_FWD": "0", "FR_DENSE_PAIRS_BWD": "0"},
                                 {"FR_DENSE_PAIRS_FWD": "100000", "FR_DENSE_PAIRS_BWD": "100000"},
                                 {"FR_BLEND_FWD": "gather"},
                                 {"FR_CHAIN_SPINS": "0"}])   # (every hand-off of the forward chain computed from memory)
def test_blend_forms_in_a_child_process(env):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import test_gpu_depth_alpha as t\n"
            "from fateavatar_amd import scenes\n"
            "from tests import util\n"
            "for k in range(3):\n"
            "    _, P, H, W, kw, _, name = util.fuzz_case(13, k)\n"
            "    s = scenes.random_scene(P, H, W, **kw)\n"
            "    t.composite_single(s, util.fuzz_inputs(13, k, s), t.SLOT, name)\n"
            "t.composite_single(scenes.head_scene(P=30000, res=256, sh_degree=3, seed=1, opacity=0.9), {}, t.SLOT, 'opaque')\n"
            "print('CHILD OK')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (env, r.stdout[-2000:], r.stderr[-4000:])
