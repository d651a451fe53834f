"""-m gpu: the per-Gaussian kernels after their inputs moved into one round trip (k_preprocess_bwd requests everything
before it uses or stores anything; lanes past P and culled Gaussians load like everyone; the dL_dsh block goes through LDS
in 16-byte pieces when the row length allows it).

Everything is held to the CPU oracle with the yardsticks of tests/test_gpu_parity.py (`_check_forward`: forward state
bit-exact; `_check_backward`: 1e-4 relative on >= 99.9 % of the entries, rel-L2 <= max(1e-4, 8 x the measured float-order
floor), threshold flips exempt at most 2 % of the visible rows or are masked out of dL/dpixel) — never to the code under
test.  Scenes are 64 x 64 pixels: tails (P not a multiple of 64 or of the workgroup's 256, one Gaussian), waves with
visible and culled Gaussians side by side, every row length the dL_dsh staging distinguishes."""
import numpy as np
import pytest

from fateavatar_amd import scenes
from tests import util
from tests.test_gpu_parity import _check_backward, _check_forward

pytestmark = pytest.mark.gpu

GUARD = 64                       # floats on either side of a guarded gradient array
GUARD_BITS = 0x7FC0DEAD          # a NaN: arithmetic on it cannot give it back by accident, comparisons are on the bits


def _scene(P, bf, degree=3, M=16, seed=None):
    return scenes.random_scene(P, 64, 64, sh_degree=degree, seed=100 + P if seed is None else seed, M=M, behind_fraction=bf)


def _dpix(seed, H=64, W=64):
    return (np.random.default_rng(seed).uniform(-1, 1, (3, H, W)) / (H * W)).astype(np.float32)


class _Recorded:
    """A frame as `_check_backward` wants it (color, final_T, backward) that keeps the gradients of its last backward and
    hands `kw()` to rasterize_gaussians_backward (caller-owned buffers, accumulation); `post`: what the yardstick is to see."""

    def __init__(self, h, kw=None, post=None):
        self.h, self.color, self.final_T, self.kw, self.post, self.last, self.calls = h, h.color, h.final_T, kw, post, None, 0

    def backward(self, dpix):
        import torch
        from fateavatar_amd import rasterizer
        g = torch.from_numpy(np.ascontiguousarray(dpix)).to(self.h.dev)
        out = rasterizer.rasterize_gaussians_backward(*self.h._backward_args(g), **(self.kw() if self.kw else {}))
        torch.cuda.synchronize()
        self.last = {k: v.cpu().numpy() for k, v in zip(util.GRAD_NAMES, out)}
        self.calls += 1
        return self.post(self.last) if self.post else self.last


def _culled_rows_are_zero(o, grads, what):
    culled = o.radii <= 0
    for k in util.GRAD_NAMES:
        a = grads[k]
        if a.size:
            assert np.all(a[culled] == 0.0), (what, k, "a culled Gaussian has a gradient")


def _has_both(o, P):
    vis = o.radii > 0
    assert vis.any(), "the scene has no visible Gaussian"
    if P > 1:
        assert (~vis).any(), "the scene has no culled Gaussian"


def _check_frame(s, dev, what, seed):
    o = util.oracle_forward(s)
    _has_both(o, s.P)
    h = util.HipFrame(s, dev)
    _check_forward(o, h, what)
    r = _Recorded(h)
    _check_backward(o, r, _dpix(seed), what)
    _culled_rows_are_zero(o, r.last, what)
    return o, h, r


# ------------------------------------------------------------------ 1. tails and sizes
@pytest.mark.parametrize("bf", [0.0, 0.5])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 257, 300])
def test_tail_and_size_shapes(P, bf, gpu_device):
    """One Gaussian, one short of a wave, a wave, one more, one short of a workgroup, one more, a second workgroup with a
    partial wave: visible and culled Gaussians in the same waves (P = 65: 53 visible, 27 with half of them behind the camera;
    P = 1: the Gaussian is visible, the 63 other lanes of its wave are past the end)."""
    _check_frame(_scene(P, bf), gpu_device, f"tail-P{P}-bf{bf}", seed=P)


# ------------------------------------------------------------------ 2. row lengths
@pytest.mark.parametrize("degree,M", [(0, 1), (1, 4), (2, 9), (3, 16), (1, 16)])
def test_row_lengths(degree, M, gpu_device):
    """3 M = 12 and 48 floats: the 16-byte path (strides 12 and 52); 3 and 27: word by word; M = 16 at degree 1: literal zeros
    above the active degree."""
    o, _, r = _check_frame(_scene(300, 0.5, degree, M, seed=400 + 16 * degree + M), gpu_device, f"rows-d{degree}-M{M}", seed=M)
    used = (degree + 1) ** 2
    assert np.all(r.last["dL_dsh"][:, used:, :] == 0.0)


# ------------------------------------------------------------------ 3. nothing is stored outside the arrays
def _guarded(P, M, dev, fill=None):
    """Every gradient array as a view into a larger allocation with GUARD floats of GUARD_BITS on either side."""
    import torch
    from fateavatar_amd import rasterizer
    whole, views = {}, {}
    for k, shape in rasterizer._grad_shapes(P, M).items():
        n = int(np.prod(shape))
        w = torch.full((n + 2 * GUARD,), GUARD_BITS, dtype=torch.int32, device=dev).view(torch.float32)
        views[k] = w[GUARD:GUARD + n].view(shape)
        if fill is not None:
            views[k].copy_(torch.from_numpy(fill[k]).to(dev))
        whole[k] = w
    return whole, views


def _guards_intact(whole, what):
    import torch
    for k, w in whole.items():
        bits = w.view(torch.int32).cpu().numpy()
        assert np.all(bits[:GUARD] == GUARD_BITS) and np.all(bits[-GUARD:] == GUARD_BITS), (what, k, "a guard word was overwritten")


@pytest.mark.parametrize("P", [65, 257])
def test_no_store_outside_the_arrays(P, gpu_device):
    s = _scene(P, 0.5)
    o = util.oracle_forward(s)
    _has_both(o, P)
    h = util.HipFrame(s, gpu_device)
    _check_forward(o, h, f"guard-P{P}")
    whole, views = _guarded(P, 16, gpu_device)
    r = _Recorded(h, kw=lambda: dict(_out=views))
    _check_backward(o, r, _dpix(P + 1), f"guard-P{P}")
    _guards_intact(whole, f"guard-P{P}")
    # (the arrays the yardstick saw ARE the guarded buffers)
    for k in util.GRAD_NAMES:
        assert np.array_equal(views[k].cpu().numpy().view(np.uint32), r.last[k].view(np.uint32)), k
    _culled_rows_are_zero(o, r.last, f"guard-P{P}")


# ------------------------------------------------------------------ 4. accumulation
def test_accumulate_into_all_eight_arrays(gpu_device):
    """FR_FLAG_ACCUMULATE on every array: result = pre-fill + the frame's gradient.  The pre-fill of an array is uniform in
    +-max|oracle gradient| of that array, so the one rounding of the sum is <= 2^-24 x 2 max|g| = 1.2e-7 max|g| per entry: 40 x
    below the yardstick's absolute floor (5e-6 max|g|) and 800 x below its 1e-4 aggregate bound — the yardstick is given
    result - pre-fill (in double) and holds it to the oracle as it stands.  Culled rows keep their pre-fill bit for bit."""
    from oracle import oracle
    P = 257
    s = _scene(P, 0.5)
    o = util.oracle_forward(s)
    _has_both(o, P)
    h = util.HipFrame(s, gpu_device)
    _check_forward(o, h, "accumulate")
    dpix = _dpix(77)
    ob = oracle.backward(o, dpix)
    rng = np.random.default_rng(78)
    fill = {k: (rng.uniform(-1, 1, getattr(ob, k).shape) * max(float(np.abs(getattr(ob, k)).max()), 1e-6)).astype(np.float32)
            for k in util.GRAD_NAMES}
    whole, views = _guarded(P, 16, gpu_device, fill)

    def kw():   # (every backward of the yardstick starts from the pre-fill)
        import torch
        for k in util.GRAD_NAMES:
            views[k].copy_(torch.from_numpy(fill[k]).to(gpu_device))
        return dict(_out=views, _accumulate=util.GRAD_NAMES)

    r = _Recorded(h, kw=kw, post=lambda last: {k: (last[k].astype(np.float64) - fill[k]).astype(np.float32) for k in last})
    _check_backward(o, r, dpix, "accumulate")
    _guards_intact(whole, "accumulate")
    culled = o.radii <= 0
    for k in util.GRAD_NAMES:
        assert np.array_equal(r.last[k][culled].view(np.uint32), fill[k][culled].view(np.uint32)), (k, "a culled row lost its pre-fill")
        assert not np.array_equal(r.last[k][~culled], fill[k][~culled]), (k, "nothing was added")


# ------------------------------------------------------------------ 5. the accumulator rows are left zeroed
def test_second_backward_on_the_same_handle(gpu_device):
    """k_preprocess_bwd zeroes each accumulator row after reading it (now with the zeroing stores behind every load): a row
    left non-zero would double a gradient in the next backward of the handle."""
    s = _scene(257, 0.5)
    o, h, r = _check_frame(s, gpu_device, "twice-first", seed=5)
    first = r.last
    n = r.calls
    _check_backward(o, r, _dpix(5), "twice-second")
    assert r.calls > n and r.last is not first
    _culled_rows_are_zero(o, r.last, "twice-second")
    # ... and a different dL/dpixel on the same handle again
    _check_backward(o, r, _dpix(6), "twice-third")


# ------------------------------------------------------------------ 6. a batched launch whose views differ in size
class _RecordedView:
    def __init__(self, v):
        self.v, self.color, self.final_T, self.last = v, v.color, v.final_T, None

    def backward(self, dpix):
        self.last = self.v.backward(dpix)
        return self.last


def test_batched_launch_with_unequal_views(gpu_device):
    """Three views of P = 65, 300 and 1 in one launch chain (fr_forward_batch / fr_backward_batch, what render_batch issues):
    the grid is the largest view's, so the smaller views' surplus workgroups leave at once and their last waves are partial."""
    Ps = (65, 300, 1)
    ss = [_scene(P, 0.5 if P > 1 else 0.0) for P in Ps]
    batch = util.HipBatch(ss, gpu_device, slots=[208, 209, 210])
    for k, (P, s) in enumerate(zip(Ps, ss)):
        o = util.oracle_forward(s)
        _has_both(o, P)
        _check_forward(o, batch[k], f"batch-view{k}-P{P}")
        r = _RecordedView(batch[k])
        _check_backward(o, r, _dpix(60 + k), f"batch-view{k}-P{P}")
        _culled_rows_are_zero(o, r.last, f"batch-view{k}-P{P}")


def test_render_batch_with_unequal_views(gpu_device):
    """The same three sizes through `render_batch` and autograd, held to the oracle on the activated values the holders hand
    to the rasterizer: image, radii, and the gradients of the positions, the SH coefficients and the screen-space points."""
    import torch
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    from fateavatar_amd.render import render_batch
    from oracle import oracle
    Ps = (65, 300, 1)
    ss = [_scene(P, 0.5 if P > 1 else 0.0) for P in Ps]
    pcs = [FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, 3, gpu_device) for s in ss]
    cams = [TorchCamera(s.camera, gpu_device) for s in ss]
    outs = render_batch(cams, pcs, [torch.from_numpy(s.bg).to(gpu_device) for s in ss], slots=[208, 209, 210])
    fs, ws = [], []
    for k, (s, pc, out) in enumerate(zip(ss, pcs, outs)):
        c = s.camera
        f = oracle.forward(bg=s.bg, means3D=pc.get_xyz.detach().cpu().numpy(), opacities=pc.get_opacity.detach().cpu().numpy(),
                           viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, campos=c.camera_center,
                           tanfovx=c.tanfovx, tanfovy=c.tanfovy, H=64, W=64, shs=pc.get_features.detach().cpu().numpy(),
                           sh_degree=3, scales=pc.get_scaling.detach().cpu().numpy(), rotations=pc.get_rotation.detach().cpu().numpy())
        img = out["render"].detach().cpu().numpy()
        assert np.array_equal(out["radii"].cpu().numpy(), f.radii), k
        # (render() does not return final_T: a threshold flip is a pixel outside the forward tolerance; it gets no gradient)
        bad = np.any(np.abs(img - f.color) > 1e-5 + 1e-4 * np.abs(f.color), axis=0)
        assert bad.sum() <= 3, (k, int(bad.sum()))
        w = _dpix(70 + k)
        w[:, bad] = 0.0
        fs.append(f), ws.append(w)
    torch.autograd.backward([o["render"] for o in outs], grad_tensors=[torch.from_numpy(w).to(gpu_device) for w in ws])
    torch.cuda.synchronize()
    for k, (pc, out, f, w) in enumerate(zip(pcs, outs, fs, ws)):
        b = oracle.backward(f, w)
        culled = f.radii <= 0
        for name, got, ref in (("means2D", out["viewspace_points"].grad.cpu().numpy(), b.dL_dmeans2D),
                               ("xyz", pc.grad_of("_xyz").cpu().numpy(), b.dL_dmeans3D),
                               ("features", pc.grad_of("_features").cpu().numpy(), b.dL_dsh)):
            assert util.rel_l2(got, ref) < 1e-4, (k, name, util.rel_l2(got, ref))
            assert np.all(got[culled] == 0.0), (k, name)


# ------------------------------------------------------------------ 7. the planes instance
def test_planes_instance_against_the_composite_oracle(gpu_device):
    """k_preprocess_bwd_planes (a backward with a depth and an alpha gradient).  tests/test_gpu_depth_alpha.py's reference —
    the gradients of <gC, C> + <gD, D> + <gA, A> are those of the plain frame under gC plus those of the composite frame
    (colours (z, 0, 0) over background (0, 1, 0)) under (gD, -gA, 0), dL/dz carried into the means through the view matrix —
    evaluated here on the CPU oracle, with that file's bound (rel-L2 <= 1e-4 per array).  Pixels whose blend sequence flipped
    against the oracle get no gradient (tests/test_gpu_parity.py, `_check_backward_no_exemptions`)."""
    import torch
    from fateavatar_amd import rasterizer
    from oracle import oracle
    P = 257
    s = _scene(P, 0.5)
    c = s.camera
    o = util.oracle_forward(s)
    _has_both(o, P)
    v = util._Frame()
    v._upload(s, gpu_device)
    with rasterizer.handle_slot(211):
        res = rasterizer.rasterize_gaussians(*v._forward_args(), _depth_alpha=True)
        torch.cuda.synchronize()
        v._take_forward(res[:6])
        _check_forward(o, v, "planes")
        bad = util.flip_pixels(o, v.color.cpu().numpy(), v.final_T.cpu().numpy())
        assert bad.sum() <= 3
        rng = np.random.default_rng(79)
        gC = (rng.uniform(-1, 1, (3, 64, 64)) / 4096).astype(np.float32)
        gD = (rng.uniform(-1, 1, (64, 64)) / 4096).astype(np.float32)
        gA = (rng.uniform(-1, 1, (64, 64)) / 4096).astype(np.float32)
        gC[:, bad], gD[bad], gA[bad] = 0.0, 0.0, 0.0
        t = lambda a: torch.from_numpy(a).to(gpu_device)  # noqa: E731
        got = rasterizer.rasterize_gaussians_backward(*v._backward_args(t(gC)), _planes=(res[8], t(gD), t(gA)))
        torch.cuda.synchronize()
    got = {k: a.cpu().numpy() for k, a in zip(util.GRAD_NAMES, got)}
    m = c.world_view_transform.astype(np.float32).reshape(-1)
    z = (s.means3D[:, 0] * m[2] + s.means3D[:, 1] * m[6] + s.means3D[:, 2] * m[10] + m[14]).astype(np.float32)
    comp = oracle.forward(bg=np.array([0.0, 1.0, 0.0], np.float32), means3D=s.means3D, opacities=s.opacities,
                          viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, campos=c.camera_center,
                          tanfovx=c.tanfovx, tanfovy=c.tanfovy, H=64, W=64, sh_degree=s.sh_degree,
                          colors_precomp=np.stack([z, np.zeros_like(z), np.zeros_like(z)], 1), scales=s.scales, rotations=s.rotations)
    assert np.array_equal(comp.radii, o.radii)
    b_plain = oracle.backward(o, gC)
    b_comp = oracle.backward(comp, np.stack([gD, -gA, np.zeros_like(gD)]))
    dz = b_comp.dL_dcolors[:, 0:1]
    culled = o.radii <= 0
    for k in util.GRAD_NAMES:
        a, b = getattr(b_plain, k), getattr(b_comp, k)
        if k in ("dL_dcolors", "dL_dsh"):
            want = a                                   # (the composite colours are not the frame's parameters)
        elif k == "dL_dmeans3D":
            want = a + b + dz * m[[2, 6, 10]].reshape(1, 3)
        else:
            want = a + b
        assert np.isfinite(got[k]).all(), k
        assert util.rel_l2(got[k], want) <= 1e-4, (k, util.rel_l2(got[k], want))
        assert np.all(got[k][culled] == 0.0), k
