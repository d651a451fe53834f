"""-m gpu: the per-Gaussian kernels' hand-offs stored as whole lines.

  * `GeomView::dcolor_ddir` is planar, [9][P] (k_preprocess_fwd writes it; k_preprocess_bwd and k_camera_bwd read it);
  * a wave's 64 blend records (`rec_tmpl`) leave k_preprocess_fwd through the wave's LDS region as one contiguous run, where
    the region has the room (M >= 4; SH degree 0 keeps one store per Gaussian), the rows of culled Gaussians and of the lanes
    past P untouched;
  * k_preprocess_bwd zeroes a wave's accumulator rows as one run of min(64, P - first) rows of 64 bytes.

None of this changes a value, so everything is held to the CPU oracle with the yardsticks of tests/test_gpu_parity.py
(`_check_forward`: forward state and records bit-exact; `_check_backward`: 1e-4 relative, rel-L2 <= max(1e-4, 8 x the measured
float-order floor)) and, for the camera gradient, tests/test_gpu_camera_grad.py's float64 reference at 1e-4 of scale — never to
the code under test.  Images are 40 x 24 pixels (5 x 3 tiles of 8 x 8, two 16 x 16 columns partial): P = 1, 63, 65 and 130 give
a single lane, a partial wave, a full wave plus one lane and two waves plus two lanes, with Gaussians behind the camera in
between the visible ones.

The handles of this module: 430 .. 439 (no other module uses them)."""
import numpy as np
import pytest

from fateavatar_amd import scenes
from tests import util
from tests.test_gpu_parity import _check_backward, _check_forward
from tests.test_gpu_pre_round_trips import _Recorded, _RecordedView, _culled_rows_are_zero, _guarded, _guards_intact, _has_both

pytestmark = pytest.mark.gpu

SLOT = 430
H, W = 24, 40


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch, gpu_device):
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


def _scene(P, degree=3, M=None, bf=None, seed=None):
    bf = (0.5 if P > 1 else 0.0) if bf is None else bf
    if seed is None:
        seed = 900 + P + 7 * degree if P > 1 else 2   # (seed 2: the single Gaussian is inside the image)
    return scenes.random_scene(P, H, W, sh_degree=degree, seed=seed, M=M, behind_fraction=bf)


def _dpix(seed):
    return (np.random.default_rng(seed).uniform(-1, 1, (3, H, W)) / (H * W)).astype(np.float32)


def _check_frame(s, dev, what, seed):
    o = util.oracle_forward(s)
    _has_both(o, s.P)
    h = util.HipFrame(s, dev)
    _check_forward(o, h, what)
    r = _Recorded(h)
    _check_backward(o, r, _dpix(seed), what)
    _culled_rows_are_zero(o, r.last, what)
    return o, h, r


# ------------------------------------------------------------------ 1. tails x the three LDS layouts of the forward
@pytest.mark.parametrize("degree,M", [(3, 16), (1, 4), (0, 1)], ids=["deg3-M16", "deg1-M4", "deg0-M1"])
@pytest.mark.parametrize("P", [1, 63, 65, 130])
def test_forward_and_backward_against_the_oracle(P, degree, M, gpu_device):
    """M = 16: the records are staged behind the counting tables (the SH rows are in registers).  M = 4: in the dead SH block,
    which they fill exactly (64 x 12 floats = 3 072 bytes).  M = 1: no room, every thread stores its own record."""
    _check_frame(_scene(P, degree, M), gpu_device, f"P{P}-d{degree}-M{M}", seed=P + degree)


def test_degree_1_of_a_16_coefficient_row(gpu_device):
    """SH degree 1 evaluated from M = 16 rows (the M = 16 layout, planes 3 .. 8 of dcolor_ddir from three coefficients only)."""
    _check_frame(_scene(130, 1, 16), gpu_device, "P130-d1-M16", seed=3)


# ------------------------------------------------------------------ 2. culled and non-finite Gaussians between visible ones
class _Kept:
    """The rows `keep` of a frame, as a frame of the clean scene (tests/test_gpu_nonfinite.py, `Kept`)."""

    def __init__(self, h, keep):
        import torch
        self._h, self._keep, self.last = h, keep, None
        self.num_rendered, self.color, self.final_T = h.num_rendered, h.color, h.final_T
        self.radii = h.radii[torch.from_numpy(keep).to(h.radii.device)]

    def geometry(self, field, cols, **kw):
        return self._h.geometry(field, cols, **kw)[self._keep]

    def backward(self, dpix):
        self.last = self._h.backward(dpix)
        return {k: v[self._keep] for k, v in self.last.items()}


def test_non_finite_gaussians_between_visible_ones(gpu_device):
    """Every fifth visible Gaussian of 130 made non-finite, alternately in its position (dropped by the geometry: no record, the
    48 bytes between its neighbours' staged rows are not stored), in a higher SH coefficient and in the DC coefficient (dropped
    by the colour stage, AFTER its instances were counted: a record of opacity 0 and colour 0).  The frame is held to the
    oracle of the scene without those rows; their gradient rows are exactly zero; their records are what the contract says."""
    P = 130
    s = _scene(P, 3, 16)
    vis = np.nonzero(util.oracle_forward(s).radii > 0)[0]
    assert vis.size >= 40
    bad_rows = vis[::5]
    bad = np.zeros(P, bool)
    bad[bad_rows] = True
    for j, i in enumerate(bad_rows):
        if j % 3 == 0:
            s.means3D[i, j % 2] = np.nan
        elif j % 3 == 1:
            s.shs[i, 5, j % 3] = np.inf
        else:
            s.shs[i, 0, 1] = np.nan
    keep = ~bad
    clean = scenes.GaussianScene(s.means3D[keep], s.scales[keep], s.rotations[keep], s.opacities[keep], s.shs[keep], s.sh_degree,
                                 s.bg, s.camera)
    o = util.oracle_forward(clean)
    _has_both(o, clean.P)
    h = util.HipFrame(s, gpu_device)
    assert np.all(h.radii.cpu().numpy()[bad] == 0)
    v = _Kept(h, keep)
    _check_forward(o, v, "nonfinite")
    _check_backward(o, v, _dpix(11), "nonfinite")
    for k, a in v.last.items():
        assert np.isfinite(a).all(), k
        if a.size:
            assert np.all(a[bad] == 0.0), (k, "a dropped Gaussian has a gradient")
    _culled_rows_are_zero(o, {k: a[keep] for k, a in v.last.items()}, "nonfinite")
    # the dead colours' records: opacity 0 and colour 0, their own id (columns 5, 6 .. 8, 9 of the record)
    rec = h.geometry(8, 12)
    dead = [int(i) for j, i in enumerate(bad_rows) if j % 3 != 0]
    assert len(dead) >= 4
    assert np.all(rec[dead, 5:9] == 0.0)
    assert np.array_equal(rec[dead, 9].view(np.uint32), np.asarray(dead, np.uint32))


# ------------------------------------------------------------------ 3. the accumulator rows are left zero
@pytest.mark.parametrize("P", [65, 130])
def test_second_backward_equals_the_first(P, gpu_device):
    """Two backward passes in a row on one handle: a row (or a part of one) left non-zero by the wave's zeroing run would be
    added to the second pass.  Both are held to the oracle; and a third pass with another dL/dpixel."""
    o, h, r = _check_frame(_scene(P), gpu_device, f"twice-first-P{P}", seed=5)
    first = r.last
    _check_backward(o, r, _dpix(5), f"twice-second-P{P}")
    assert r.last is not first
    for k in util.GRAD_NAMES:
        # (same frame, same dL/dpixel: the two passes differ by the order of the blend backward's float atomics at most —
        # 1e-5 rel-L2, tests/test_gpu_nonfinite.py's bound for two runs of one frame; a row added twice is an error of order 1)
        assert util.rel_l2(r.last[k], first[k]) <= 1e-5, (k, util.rel_l2(r.last[k], first[k]))
    _culled_rows_are_zero(o, r.last, f"twice-second-P{P}")
    _check_backward(o, r, _dpix(6), f"twice-third-P{P}")


# ------------------------------------------------------------------ 4. accumulate mode adds
def test_accumulate_mode_adds(gpu_device):
    """FR_FLAG_ACCUMULATE on all eight arrays (tests/test_gpu_pre_round_trips.py's construction: a pre-fill uniform in
    +-max|oracle gradient| per array, the yardstick sees result - pre-fill): the accumulator rows are zeroed by the same run."""
    from oracle import oracle
    P = 130
    s = _scene(P)
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

    def kw():
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


# ------------------------------------------------------------------ 5. a batched call of two views with different P
def test_batch_of_two_views_with_different_sizes(gpu_device):
    """P = 130 (degree 3) and P = 63 (degree 1, M = 4) in one launch chain: the grid and the LDS are the larger view's, each
    view addresses its own planes (k * P of ITS P) and stages its records in its own layout."""
    cases = ((130, 3, 16), (63, 1, 4))
    ss = [_scene(P, d, M) for P, d, M in cases]
    batch = util.HipBatch(ss, gpu_device, slots=[SLOT, SLOT + 1])
    for k, ((P, d, M), s) in enumerate(zip(cases, ss)):
        o = util.oracle_forward(s)
        _has_both(o, P)
        _check_forward(o, batch[k], f"batch-view{k}-P{P}")
        r = _RecordedView(batch[k])
        _check_backward(o, r, _dpix(60 + k), f"batch-view{k}-P{P}")
        _culled_rows_are_zero(o, r.last, f"batch-view{k}-P{P}")


# ------------------------------------------------------------------ 6. the camera gradient reads the planes, too
def test_camera_gradient_with_sh(gpu_device):
    """tests/test_gpu_camera_grad.py's degree-3 scene (260 Gaussians, 48 x 40) against its float64 reference at 1e-4 of scale:
    dL/dcampos is the sum of the SH colours' direction derivatives, which k_camera_bwd reads from `dcolor_ddir`."""
    from tests.test_gpu_camera_grad import _check, _hip_case
    _, ref, _, cam, _ = _hip_case("deg3", gpu_device, SLOT + 2)
    _check(cam, ref, "whole-lines deg3")
    assert np.abs(np.asarray(cam[2])).max() > 0


# ------------------------------------------------------------------ 7. a bound frame
def test_bound_frame_against_the_oracle_on_its_bound_arrays(gpu_device):
    """A MeshBinding frame (the binding evaluated inside k_preprocess_fwd / k_preprocess_bwd, SH degree 0) twice on one handle.
    Forward: the image against the CPU oracle on the arrays the bound forward wrote, activated in torch (what
    test_render_api_autograd_path holds raw frames to: 1e-5 + 1e-4 |ref| on 99.99 % of the values).  Backward: the parameter
    gradients of the second pass equal the first's within 1e-5 rel-L2 — the accumulator rows were left zero — and those of the
    unfolded path (the stand-alone binding op in front of a plain frame, stock autograd between them) within 2e-4 rel-L2
    (tests/test_gpu_phong.py:122)."""
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.avatar import _BoundFrame, _RawFrame
    from fateavatar_amd.binding import bind_gaussians, face_scale
    from fateavatar_amd.bound import MeshBinding, render_bound_batch
    from fateavatar_amd.render import render
    from oracle import oracle
    from tests.test_gpu_avatar import _setup
    dev = gpu_device
    S = _setup(dev, 1500, 64, 2, seed=3)
    bg = torch.ones(3, device=dev)
    faces = S["faces"].to(torch.int32).contiguous()
    canon = face_scale(S["canon"], faces)
    gt = torch.rand(3, 64, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    cam = S["cams"][1]
    names = ("_opacity", "_offset", "_rotation", "_scaling", "_features_dc")

    def bound_pass(pc):
        pc.begin_step()
        with rasterizer.handle_slot(SLOT + 3):
            out = render_bound_batch([cam], [_RawFrame(pc, None)], [S["posed"][1]],
                                     MeshBinding(faces, pc.face_index, pc.bary_coords, canon, 0.05, True), bg, slots=[SLOT + 3])[0]
            torch.nn.functional.l1_loss(out["render"], gt).backward()
        torch.cuda.synchronize()
        return out, {n: getattr(pc, n).grad.detach().cpu().numpy().copy() for n in names}

    pc = S["make"]()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        pc._features_dc.copy_((torch.rand(pc.P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        pc._opacity.fill_(float(np.log(0.6 / 0.4)))
        # (anisotropic: with the holder's three equal scales dL/drotation is analytically zero, and what a backward returns
        # for it is rounding noise no two passes agree on)
        pc._scaling.add_((0.5 * torch.randn(tuple(pc._scaling.shape), generator=g)).to(dev))
    out1, g1 = bound_pass(pc)
    for n in names:
        getattr(pc, n).grad = None
    out2, g2 = bound_pass(pc)
    assert torch.equal(out1["render"], out2["render"]) and int((out1["radii"] > 0).sum()) > 500
    for n in names:
        assert np.abs(g1[n]).max() > 0, n
        assert util.rel_l2(g2[n], g1[n]) <= 1e-5, (n, util.rel_l2(g2[n], g1[n]))

    # forward against the oracle on the bound arrays
    xyz, rot, scl = out1["bound"]
    c = cam
    npf = lambda t: t.detach().cpu().numpy().astype(np.float32)  # noqa: E731
    f = oracle.forward(bg=npf(bg), means3D=npf(xyz), opacities=npf(torch.sigmoid(pc._opacity)), viewmatrix=npf(c.world_view_transform),
                       projmatrix=npf(c.full_proj_transform), campos=npf(c.camera_center), tanfovx=float(np.tan(c.FoVx * 0.5)), tanfovy=float(np.tan(c.FoVy * 0.5)),
                       H=64, W=64, shs=npf(pc._features_dc), sh_degree=0, scales=npf(torch.exp(scl)),
                       rotations=npf(torch.nn.functional.normalize(rot)))
    img = npf(out1["render"])
    assert util.frac_close(img, f.color, 1e-4, 1e-5) >= 0.9999, util.frac_close(img, f.color, 1e-4, 1e-5)
    assert np.array_equal(out1["radii"].cpu().numpy() > 0, f.radii > 0)

    # backward against the unfolded path
    for n in names:
        getattr(pc, n).grad = None
    pc.begin_step()
    with rasterizer.handle_slot(SLOT + 4):
        x3, r3, s3 = bind_gaussians(S["posed"][1], faces, pc.face_index, pc.bary_coords, canon, pc._offset, pc._rotation,
                                    pc._scaling, 0.05, True)
        plain = render(cam, _BoundFrame(x3, pc, r3, s3, None), bg)
        torch.nn.functional.l1_loss(plain["render"], gt).backward()
    torch.cuda.synchronize()
    assert torch.equal(plain["render"], out1["render"])
    for n in names:
        got, want = g1[n], getattr(pc, n).grad.detach().cpu().numpy()
        assert util.rel_l2(got, want) <= 2e-4, (n, util.rel_l2(got, want))
