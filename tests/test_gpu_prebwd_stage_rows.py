"""-m gpu: the per-Gaussian backward stages a wave's dL_dsh rows through LDS in passes of FR_PREBWD_STAGE_ROWS Gaussians
(fr_preprocess_bwd.hip: the rows of Gaussians [p R, p R + R) of the wave are written, then stored as one contiguous run, pass
after pass), every wave on its own: no workgroup barrier.

What can go wrong is at the pass boundaries: a row written into the wrong slot of the block or stored at the wrong offset, a
short last pass, a culled Gaussian's zero row, a pass that overwrites the block before the previous one was read.  The scenes
are the smallest that put a boundary everywhere it can be for 32- and 16-row passes: P = 31, 32, 33 (one short block, exactly
one, a second pass of one row), 95, 96, 97 (the same in a second wave) and 289 (a second workgroup whose last pass has one
row).  Every one has visible and culled Gaussians side by side in its partial blocks.

Everything is held to the CPU oracle with the yardsticks of tests/test_gpu_parity.py through the helpers of
tests/test_gpu_pre_round_trips.py — never to the code under test."""
import numpy as np
import pytest

from tests import util
from tests.test_gpu_parity import _check_backward, _check_forward
from tests.test_gpu_pre_round_trips import (_check_frame, _culled_rows_are_zero, _dpix, _guarded, _guards_intact, _has_both,
                                            _Recorded, _RecordedView, _scene)

pytestmark = pytest.mark.gpu

SH_C0 = np.float32(0.28209479177387814)   # bSH_C0, as the kernel holds it


# ------------------------------------------------------------------ 1. pass boundaries
@pytest.mark.parametrize("bf", [0.0, 0.5])
@pytest.mark.parametrize("P", [31, 32, 33, 95, 96, 97, 289])
def test_pass_boundaries(P, bf, gpu_device):
    """M = 16 (rows of 48 floats, stride 52).  `_check_frame` asserts that the scene has visible and culled Gaussians, holds
    forward and backward to the oracle and requires the culled rows to be exactly zero."""
    _check_frame(_scene(P, bf), gpu_device, f"stage-P{P}-bf{bf}", seed=P)


# ------------------------------------------------------------------ 2. every row where it belongs, bit for bit
@pytest.mark.parametrize("P", [33, 97, 289])
def test_row_placement_bit_for_bit(P, gpu_device):
    """dL_dsh[i, 0, c] is ONE IEEE multiply, float32(bSH_C0) * dRGB[c] (no contraction in this object), and dRGB[c] is
    dL_dcolors[i, c] of the same backward where the colour channel was not clamped, 0 where it was: independent of the order
    of the blend backward's atomics, so a row that landed in another Gaussian's place shows in the bits.  The forward state is
    bit-exact against the oracle (`_check_forward`), so the oracle's `clamped` is the kernel's."""
    o, _, r = _check_frame(_scene(P, 0.5), gpu_device, f"bits-P{P}", seed=1000 + P)
    vis = o.radii > 0
    free = (o.clamped == 0) & vis[:, None]
    held = (o.clamped != 0) & vis[:, None]
    assert free.sum() >= 0.9 * 3 * vis.sum(), (int(free.sum()), int(vis.sum()))
    dsh0, dcol = r.last["dL_dsh"][:, 0, :], r.last["dL_dcolors"]
    want = SH_C0 * dcol.astype(np.float32)
    assert want.dtype == np.float32
    bad = free & (dsh0.view(np.uint32) != want.view(np.uint32))
    assert not bad.any(), (P, "rows whose first coefficient is not bSH_C0 * dL_dcolors", np.argwhere(bad)[:8].tolist())
    assert np.all(dsh0[held] == 0.0), (P, "a clamped channel has a gradient")
    # (and the rows are not trivially zero)
    assert np.count_nonzero(dsh0[free]) > 0


# ------------------------------------------------------------------ 3. both 16-byte row lengths across a boundary
@pytest.mark.parametrize("degree,M", [(1, 4), (3, 16), (1, 16)])
def test_row_lengths_across_a_boundary(degree, M, gpu_device):
    """3 M = 12 (the stride IS the row length) and 48 (stride 52) at P = 97; M = 16 at degree 1: literal zeros above the active
    degree."""
    _, _, r = _check_frame(_scene(97, 0.5, degree, M), gpu_device, f"stage-rows-d{degree}-M{M}", seed=97 + M)
    used = (degree + 1) ** 2
    assert r.last["dL_dsh"].shape == (97, M, 3)
    assert np.all(r.last["dL_dsh"][:, used:, :] == 0.0)


# ------------------------------------------------------------------ 4. nothing is stored outside the arrays
@pytest.mark.parametrize("P", [33, 97])
def test_no_store_outside_the_arrays(P, gpu_device):
    s = _scene(P, 0.5)
    o = util.oracle_forward(s)
    _has_both(o, P)
    h = util.HipFrame(s, gpu_device)
    _check_forward(o, h, f"stage-guard-P{P}")
    whole, views = _guarded(P, 16, gpu_device)
    r = _Recorded(h, kw=lambda: dict(_out=views))
    _check_backward(o, r, _dpix(P + 1), f"stage-guard-P{P}")
    _guards_intact(whole, f"stage-guard-P{P}")
    for k in util.GRAD_NAMES:
        assert np.array_equal(views[k].cpu().numpy().view(np.uint32), r.last[k].view(np.uint32)), k
    _culled_rows_are_zero(o, r.last, f"stage-guard-P{P}")


# ------------------------------------------------------------------ 5. accumulation across a boundary
def test_accumulate_across_a_boundary(gpu_device):
    """FR_FLAG_ACCUMULATE on all eight arrays at P = 97, pre-filled as in test_accumulate_into_all_eight_arrays (uniform in
    +-max|oracle gradient| per array: the one rounding of the sum is 40 x below the yardstick's absolute floor): result -
    pre-fill is held to the oracle, culled rows keep their pre-fill bit for bit.  dL_dsh's old values are loaded pass by pass."""
    from oracle import oracle
    P = 97
    s = _scene(P, 0.5)
    o = util.oracle_forward(s)
    _has_both(o, P)
    h = util.HipFrame(s, gpu_device)
    _check_forward(o, h, "stage-accumulate")
    dpix = _dpix(177)
    ob = oracle.backward(o, dpix)
    rng = np.random.default_rng(178)
    fill = {k: (rng.uniform(-1, 1, getattr(ob, k).shape) * max(float(np.abs(getattr(ob, k)).max()), 1e-6)).astype(np.float32)
            for k in util.GRAD_NAMES}
    whole, views = _guarded(P, 16, gpu_device, fill)

    def kw():   # (every backward of the yardstick starts from the pre-fill)
        import torch
        for k in util.GRAD_NAMES:
            views[k].copy_(torch.from_numpy(fill[k]).to(gpu_device))
        return dict(_out=views, _accumulate=util.GRAD_NAMES)

    r = _Recorded(h, kw=kw, post=lambda last: {k: (last[k].astype(np.float64) - fill[k]).astype(np.float32) for k in last})
    _check_backward(o, r, dpix, "stage-accumulate")
    _guards_intact(whole, "stage-accumulate")
    culled = o.radii <= 0
    for k in util.GRAD_NAMES:
        assert np.array_equal(r.last[k][culled].view(np.uint32), fill[k][culled].view(np.uint32)), (k, "a culled row lost its pre-fill")
        assert not np.array_equal(r.last[k][~culled], fill[k][~culled]), (k, "nothing was added")


# ------------------------------------------------------------------ 6. the accumulator rows are left zeroed
def test_second_backward_on_the_same_handle(gpu_device):
    o, h, r = _check_frame(_scene(97, 0.5), gpu_device, "stage-twice-first", seed=15)
    first, n = r.last, r.calls
    _check_backward(o, r, _dpix(15), "stage-twice-second")
    assert r.calls > n and r.last is not first
    _culled_rows_are_zero(o, r.last, "stage-twice-second")
    _check_backward(o, r, _dpix(16), "stage-twice-third")


# ------------------------------------------------------------------ 7. one batched launch of unequal views
def test_batched_launch_with_unequal_views(gpu_device):
    """P = 33, 97 and 1 in one launch chain: the grid is the largest view's; the first view's wave ends one row into its second
    pass, the last view is one Gaussian."""
    Ps = (33, 97, 1)
    ss = [_scene(P, 0.5 if P > 1 else 0.0) for P in Ps]
    batch = util.HipBatch(ss, gpu_device, slots=[212, 213, 214])
    for k, (P, s) in enumerate(zip(Ps, ss)):
        o = util.oracle_forward(s)
        _has_both(o, P)
        _check_forward(o, batch[k], f"stage-batch-view{k}-P{P}")
        r = _RecordedView(batch[k])
        _check_backward(o, r, _dpix(160 + k), f"stage-batch-view{k}-P{P}")
        _culled_rows_are_zero(o, r.last, f"stage-batch-view{k}-P{P}")


# ------------------------------------------------------------------ 8. the planes instance
def test_planes_instance_across_a_boundary(gpu_device):
    """k_preprocess_bwd_planes at P = 97 against the composite-oracle reference of
    test_planes_instance_against_the_composite_oracle (tests/test_gpu_pre_round_trips.py): the gradients of
    <gC, C> + <gD, D> + <gA, A> are those of the plain frame under gC plus those of the composite frame (colours (z, 0, 0) over
    background (0, 1, 0)) under (gD, -gA, 0), dL/dz carried into the means through the view matrix; rel-L2 <= 1e-4 per array;
    pixels whose blend sequence flipped against the oracle get no gradient."""
    import torch
    from fateavatar_amd import rasterizer
    from tests.planes_ref import PlanesRef
    P = 97
    s = _scene(P, 0.5)
    ref = PlanesRef(s)   # (the oracle's plain and composite frames; asserts that their radii agree)
    o = ref.o
    _has_both(o, P)
    v = util._Frame()
    v._upload(s, gpu_device)
    with rasterizer.handle_slot(215):
        res = rasterizer.rasterize_gaussians(*v._forward_args(), _depth_alpha=True)
        torch.cuda.synchronize()
        v._take_forward(res[:6])
        _check_forward(o, v, "stage-planes")
        bad = util.flip_pixels(o, v.color.cpu().numpy(), v.final_T.cpu().numpy())
        assert bad.sum() <= 3
        rng = np.random.default_rng(179)
        gC = (rng.uniform(-1, 1, (3, 64, 64)) / 4096).astype(np.float32)
        gD = (rng.uniform(-1, 1, (64, 64)) / 4096).astype(np.float32)
        gA = (rng.uniform(-1, 1, (64, 64)) / 4096).astype(np.float32)
        gC[:, bad], gD[bad], gA[bad] = 0.0, 0.0, 0.0
        t = lambda a: torch.from_numpy(a).to(gpu_device)  # noqa: E731
        got = rasterizer.rasterize_gaussians_backward(*v._backward_args(t(gC)), _planes=(res[8], t(gD), t(gA)))
        torch.cuda.synchronize()
    got = {k: a.cpu().numpy() for k, a in zip(util.GRAD_NAMES, got)}
    want = ref.sum_gradients(gC, np.stack([gD, -gA, np.zeros_like(gD)]))
    culled = o.radii <= 0
    for k in util.GRAD_NAMES:
        assert np.isfinite(got[k]).all(), k
        assert util.rel_l2(got[k], want[k]) <= 1e-4, (k, util.rel_l2(got[k], want[k]))
        assert np.all(got[k][culled] == 0.0), k
