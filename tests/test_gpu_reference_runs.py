"""-m gpu: every fused entry point of the avatar methods on the inputs of tests/golden/reference_*.npz, held DIRECTLY to what the
reference's own Python computed on them in float64 (tests/golden/make_reference_runs.py) — not to a restatement of it.

The bound of each output is the one its module's own GPU test states, imported from that test: image_loss_ref.LOSS_ATOL /
GRAD_REL_L2 / GRAD_ENTRY; FACTOR x e32 under CEILING (test_gpu_mlp, test_gpu_splatting_loss); ROW_FACTOR / ELEMENT_FACTOR
(test_gpu_mono, test_gpu_mono_pose, and test_gpu_flame's blocks); the counted 2^-24 bounds of the splatting, Huber, regulariser, blendshape-term and mesh-term
tests.  e32 — the reference's own float32 error — and the row / element yardsticks come from the fixture.  Inputs that meet a gate
were drawn clear of it (the margins are in the fixture): no element is left out of any comparison.  The achieved error and the
recorded e32 are printed per output.  Reads tests/golden/ only."""
import pytest

from tests import image_loss_ref, mesh_terms_ref, mlp_ref
from tests.reference_runs import EPS, Case, rel
from tests.test_gpu_mlp import CEILING, FACTOR
from tests.test_gpu_mono import ROW_FACTOR, _row_metric, _terms_roundings
from tests.test_gpu_mono_pose import ELEMENT_FACTOR, _element_metric
from tests.test_reference_runs_host import FLAME_CASES, FLAME_OUTPUTS, SKIN_OUTPUTS, flame_model, mlp_weights, mono_tables, mono_var, \
    skinning_inputs

pytestmark = pytest.mark.gpu

HUBER_RTOL = 1e-6       # test_gpu_flash.test_huber_loss_and_grad_matches_the_restatement: loss words and gradient entries, relative


def _say(case, name, err, what="rel-L2"):
    print(f"{case.name} {name}: kernel {what} {err:.3e}   (reference's own float32 run {case.e32(name):.3e}, "
          f"ratio {err / max(case.e32(name), 1e-300):.2f})")


# ------------------------------------------------------------------ the image terms
@pytest.mark.parametrize("name", ["dssim_3x33x47", "dssim_1x7x5"])
def test_image_loss_d_ssim_against_the_recorded_run(gpu_device, name):
    """`image_loss_and_grad` with weights (0, 1): words 0 and 2 are d_ssim, the gradient is d_ssim's."""
    import torch
    from fateavatar_amd.loss import image_loss_and_grad
    c = Case(name)
    loss3, grad = image_loss_and_grad(c.inp("img").to(gpu_device), c.inp("gt").to(gpu_device), (0.0, 1.0))
    torch.cuda.synchronize()
    want, g64 = float(c.out("loss")), c.out("d_img")
    dl = max(abs(float(loss3[0]) - want), abs(float(loss3[2]) - want))
    diff = grad.cpu().double() - g64
    rl2, ent = float(diff.norm() / g64.norm()), float(diff.abs().max() / g64.abs().max())
    print(f"{name}: d_ssim {float(loss3[2]):.9g} want {want:.9g} err {dl:.3e} (e32 {c.e32('loss') * want:.3e} absolute)")
    _say(c, "d_img", rl2)
    print(f"{name} d_img: worst entry / max|g| {ent:.3e}")
    assert bool(torch.isfinite(loss3).all()) and bool(torch.isfinite(grad).all())
    assert dl <= image_loss_ref.LOSS_ATOL and rl2 <= image_loss_ref.GRAD_REL_L2 and ent <= image_loss_ref.GRAD_ENTRY


def test_image_loss_with_the_reference_mix_against_the_recorded_run(gpu_device):
    """GaussianAvatarsLoss' image part, 0.8 L1 + 0.2 d_ssim (`REFERENCE_IMAGE_LOSS`), on the recorded full-loss case."""
    import torch
    from fateavatar_amd.loss import image_loss_and_grad
    from fateavatar_amd.rigged import REFERENCE_IMAGE_LOSS as W
    c = Case("ga")
    loss3, grad = image_loss_and_grad(c.inp("img").to(gpu_device), c.inp("gt").to(gpu_device), W)
    torch.cuda.synchronize()
    want3 = torch.stack([W.rgb_weight * c.out("rgb_loss") + W.dssim_weight * c.out("dssim_loss"), c.out("rgb_loss"), c.out("dssim_loss")])
    dl, rl2, ent = image_loss_ref.errors(loss3, grad, want3, c.out("d_img"))
    print(f"ga image term: loss err {dl:.3e}, worst entry / max|g| {ent:.3e}")
    _say(c, "d_img", rl2)
    assert dl <= image_loss_ref.LOSS_ATOL and rl2 <= image_loss_ref.GRAD_REL_L2 and ent <= image_loss_ref.GRAD_ENTRY


def test_pixel_loss_against_the_recorded_run(gpu_device):
    """`pixel_loss_and_grad` with `PixelLoss()`: test_gpu_splatting_loss.test_pixel_loss_matches_float64's rule, FACTOR x e32 with
    a word's e32 counting as no less than one float32 rounding.  The first word is a sum of the other two with positive
    weights: it is allowed their allowances, weighted, and two roundings (a product, the sum) of its own."""
    import torch
    from fateavatar_amd.loss import PixelLoss, pixel_loss_and_grad
    from tests.test_gpu_splatting_loss import FACTOR as PIXEL_FACTOR
    c = Case("splat")
    w = PixelLoss()
    loss3, grad = pixel_loss_and_grad(c.inp("img").to(gpu_device), c.inp("gt").to(gpu_device), w)
    torch.cuda.synchronize()
    e = rel(grad, c.out("d_img"))
    _say(c, "d_img", e)
    assert e <= PIXEL_FACTOR * c.e32("d_img")
    allowed = {}
    for k, n in ((1, "rgb_loss"), (2, "mse_loss")):
        err, want = abs(float(loss3[k]) - float(c.out(n))), float(c.out(n))
        allowed[n] = PIXEL_FACTOR * max(c.e32(n), EPS) * want
        _say(c, n, err / want, "relative error")
        assert err <= allowed[n], (n, err, allowed[n])
    total = w.rgb_weight * float(c.out("rgb_loss")) + w.mse_weight * float(c.out("mse_loss"))
    bound = w.rgb_weight * allowed["rgb_loss"] + w.mse_weight * allowed["mse_loss"] + 2 * EPS * total
    print(f"splat first word: {float(loss3[0]):.9g} want {total:.9g} |d| {abs(float(loss3[0]) - total):.3e} bound {bound:.3e}")
    assert abs(float(loss3[0]) - total) <= bound


def test_scale_term_against_the_recorded_run(gpu_device):
    """`scale_term_and_grad` with `ScaleTerm()`: test_scale_term_matches_float64_autograd's bound (1e-4 + 2 x 2^-24) on the loss and
    on every entry, the count exact, unselected rows untouched."""
    import torch
    from fateavatar_amd.loss import ScaleTerm, scale_term_and_grad
    c = Case("splat")
    want = c.out("d_scaling")
    selected = (want != 0).any(dim=1)
    assert bool(((want != 0).sum(dim=1) <= 1).all()) and 0 < int(selected.sum()) < want.shape[0]
    d = torch.zeros(want.shape, device=gpu_device)
    out = scale_term_and_grad(c.inp("scaling").to(gpu_device), d, terms=ScaleTerm())
    torch.cuda.synchronize()
    got, loss64 = d.cpu().double(), float(c.out("scale_loss"))
    err = (got - want).abs()
    _say(c, "scale_loss", abs(float(out[0]) - loss64) / loss64, "relative error")
    _say(c, "d_scaling", rel(got, want))
    print(f"splat d_scaling: max |got - want| / |want| {float((err / want.abs().clamp_min(1e-300)).max()):.3e}, selected {int(out[1])}")
    assert float(out[1]) == int(selected.sum())
    assert abs(float(out[0]) - loss64) <= (1e-4 + 2 * EPS) * loss64
    assert bool(torch.isfinite(got).all()) and bool((err <= (1e-4 + 2 * EPS) * want.abs()).all())
    assert torch.equal((got != 0).any(dim=1), selected)


@pytest.mark.parametrize("name", ["huber_plain", "huber_mouth"])
def test_huber_loss_against_the_recorded_run(gpu_device, name):
    """`huber_loss_and_grad` with `REFERENCE_HUBER_LOSS`: the total within 1e-6 relative, every gradient entry within rtol 1e-6 —
    here of the reference's float64 gradient itself."""
    import torch
    from fateavatar_amd.loss import REFERENCE_HUBER_LOSS, huber_loss_and_grad
    c = Case(name)
    mask = c.inp("mask").to(gpu_device) if c.has("mask") else None
    loss3, grad = huber_loss_and_grad(c.inp("img").to(gpu_device), c.inp("gt").to(gpu_device), REFERENCE_HUBER_LOSS, mask=mask)
    torch.cuda.synchronize()
    want, g64, got = float(c.out("loss")), c.out("d_img"), grad.cpu().double()
    _say(c, "loss", abs(float(loss3[0]) - want) / want, "relative error")
    _say(c, "d_img", rel(got, g64))
    worst = float(((got - g64).abs() / g64.abs().clamp_min(1e-300))[g64 != 0].max())
    print(f"{name} d_img: worst relative entry {worst:.3e}")
    assert abs(float(loss3[0]) - want) <= HUBER_RTOL * want
    assert (float(loss3[2]) > 0) == (mask is not None)
    assert bool(((got - g64).abs() <= HUBER_RTOL * g64.abs()).all())


def test_gaussian_regularisers_against_the_recorded_run(gpu_device):
    """`gaussian_regularisers` with `REFERENCE_REGULARISERS`: test_regulariser_kernel_matches_float64_autograd's bounds."""
    import torch
    from fateavatar_amd.loss import gaussian_regularisers
    from fateavatar_amd.rigged import REFERENCE_REGULARISERS as R
    from tests.test_gpu_rigged_density import _reg_roundings
    c = Case("ga")
    P = c.inp("scaling").shape[0]
    d_s, d_x = torch.zeros(P, 3, device=gpu_device), torch.zeros(P, 3, device=gpu_device)
    out = gaussian_regularisers(c.inp("scaling").to(gpu_device), c.inp("xyz").to(gpu_device), d_s, d_x,
                                weights=(R.scale_weight, R.xyz_weight), thresholds=(R.threshold_scale, R.threshold_xyz))
    torch.cuda.synchronize()
    for n, got in (("d_scaling", d_s), ("d_xyz", d_x)):
        want, got = c.out(n), got.cpu().double()
        _say(c, n, rel(got, want))
        assert float(want.abs().max()) > 0 and bool((want == 0).any())
        assert bool(torch.isfinite(got).all()) and bool(((got - want).abs() <= (1e-4 + 2 * EPS) * want.abs()).all()), n
    for k, n in enumerate(("scale_loss", "xyz_loss")):
        want = float(c.out(n))
        _say(c, n, abs(float(out[k]) - want) / want, "relative error")
        assert abs(float(out[k]) - want) <= (1e-4 + _reg_roundings(P) * EPS) * want, n


# ------------------------------------------------------------------ FateAvatar's mesh terms
def test_mesh_terms_against_the_recorded_run(gpu_device):
    """`mesh_terms_and_grad` at (1e5, 0.3) and at `REFERENCE_MESH_TERMS`: test_mesh_terms_kernel_matches_float64's counted bounds
    (their magnitudes M^r, M^g from tests/mesh_terms_ref.py; the losses and the gradient they are applied to from the record)."""
    import torch
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS, MeshTerms, mesh_terms_and_grad
    from tests.test_gpu_mesh_terms import _grad_bound, _lap_of, _loss_bounds
    c = Case("fate")
    vo, v, faces = c.inp("verts_orig"), c.inp("verts"), c.inp("faces").numpy()
    V = vo.shape[0]
    lap = _lap_of(faces, V, gpu_device)
    for weights, want in (((c.param("laplacian_weight"), c.param("flame_weight")), c.out("configured_d_verts") + c.out("flame_d_verts")),
                          (tuple(REFERENCE_MESH_TERMS), c.out("configured_d_verts"))):
        t = mesh_terms_ref.float64_terms(faces, V, vo, v, *weights)
        t.update(lap=float(c.out("laplacian_loss")), flame=float(c.out("flame_flame_loss")), grad=want)
        d_verts = torch.zeros(V, 3, device=gpu_device)
        out = mesh_terms_and_grad(v.to(gpu_device), vo.to(gpu_device), lap, MeshTerms(*weights), d_verts=d_verts)
        torch.cuda.synchronize()
        err = (d_verts.cpu().double() - want).abs()
        bound = _grad_bound(t, weights, V, want)
        print(f"fate weights {weights}: d_verts rel-L2 {rel(d_verts, want):.3e} (reference's own float32 run "
              f"{c.e32('configured_d_verts'):.3e}), max |got - want| / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool(torch.isfinite(d_verts).all()) and int((err > bound).sum()) == 0
        b_lap, b_flame = _loss_bounds(t, V)
        for n, got, want_l, b in (("laplacian_loss", float(out[0]), t["lap"], b_lap), ("flame_flame_loss", float(out[1]), t["flame"], b_flame)):
            _say(c, n, abs(got - want_l) / want_l, "relative error")
            assert want_l > 0 and abs(got - want_l) <= b, (n, got, want_l, b)


# ------------------------------------------------------------------ MonoGaussianAvatar
@pytest.mark.parametrize("name", ["lbs_ghost", "lbs_var_ghost", "lbs_e7_j5"])
def test_lbs_terms_against_the_recorded_run(gpu_device, name):
    """`lbs_terms_and_grad` with `reference_lbs_weights(10, var)`: test_lbs_terms_losses_and_added_gradients' bounds — every word
    within the counted R x 2^-24, the added gradient within rel-L2 1e-6 and every entry within 4 x 2^-24 (buffers start at 0) —
    and the recorded TOTAL is the coefficients times the three words."""
    import torch
    from fateavatar_amd.mono import lbs_terms_and_grad, reference_lbs_weights
    dev = gpu_device
    c = Case(name, inputs_of="lbs_ghost")
    var = mono_var(c)
    coeff = reference_lbs_weights(c.param("lbs_weight"), var)
    pred = [c.inp(k).to(dev) for k in ("lbs_weights", "posedirs", "shapedirs")]
    N, J, E = pred[0].shape[0], pred[0].shape[1], pred[2].shape[2]
    bufs = [torch.zeros_like(t) for t in pred]
    out = lbs_terms_and_grad(c.inp("index").to(torch.int32).to(dev), *pred, *[t.to(dev) for t in mono_tables(c)], coeff, *bufs)
    torch.cuda.synchronize()
    counted = _terms_roundings(N, E, J)
    # the recorded words are 1, 100 and 100 (x mean(1 / var) / 50) times the plain mean squared errors the kernel returns
    word = (1.0, 100.0, 100.0 * (float((1.0 / var.double()).mean()) / 50.0 if var is not None else 1.0))
    total, total_bound = 0.0, 0.0
    for k, n in enumerate(("lbs_loss", "posedirs_loss", "shapedirs_loss")):
        want, got = float(c.out(n)), word[k] * float(out[k])
        _say(c, n, abs(got - want) / want, f"relative error (of the {counted[k]} roundings allowed: {abs(got - want) / want / EPS:.2f})")
        assert want > 0 and abs(got - want) <= counted[k] * EPS * want, (n, got, want)
        total += float(coeff[k]) * float(out[k])
        total_bound += counted[k] * EPS * float(coeff[k]) * want / word[k]
    want = float(c.out("loss"))
    _say(c, "loss", abs(total - want) / want, "relative error")
    assert abs(total - want) <= total_bound + 4 * EPS * want       # (three products and two additions on the host, in float64)
    for buf, n in zip(bufs, ("d_lbs_weights", "d_posedirs", "d_shapedirs")):
        g64, got = c.out(n), buf.cpu().double()
        e = rel(got, g64)
        entry = float(((got - g64).abs() / g64.abs().clamp_min(1e-300)).max())
        _say(c, n, e)
        print(f"{name} {n}: worst entry {entry / EPS:.2f} of the 4 roundings allowed")
        assert e <= 1e-6 and entry <= 4 * EPS, (n, e, entry)


@pytest.mark.parametrize("name", ["skin_65_50_6", "skin_257_7_5"])
def test_deform_points_against_the_recorded_run(gpu_device, name):
    """`deform_points(frame_grad=True)`: the bounds of test_deform_points_matches_the_float64_restatement and
    test_pose_gradients_match_the_float64_restatement — xyz within 1e-5 + 1e-5 |ref|, every gradient within rel-L2 2e-4, every
    ROW of a per-point gradient within ROW_FACTOR and every ELEMENT of a pose gradient within ELEMENT_FACTOR times the worst the
    REFERENCE's own float32 run reaches at N = 4 099 of the recipe (recorded, asserted to lie in (0, 2e-6] and (0, 2e-5])."""
    import torch
    from fateavatar_amd.mono import PoseState, deform_points
    c = Case(name)
    x, canonical, frame, g = skinning_inputs(c, torch.float32, gpu_device)
    leaves = [t.requires_grad_(True) for t in x + list(frame)]
    xyz = deform_points(*leaves[:4], PoseState(*canonical), PoseState(*leaves[4:]), frame_grad=True)
    grads = torch.autograd.grad(xyz, leaves, g)
    torch.cuda.synchronize()
    got, want = xyz.detach().cpu().double(), c.out("xyz")
    _say(c, "xyz", rel(got, want))
    print(f"{name} xyz: max |d| {float((got - want).abs().max()):.3e} (reference's own float32 run {c.scalar('xyz_max32'):.3e})")
    assert bool(torch.isfinite(got).all()) and float(((got - want).abs() - 1e-5 * want.abs()).max()) <= 1e-5
    for n, gg in zip(SKIN_OUTPUTS, grads):
        gg, r = gg.cpu(), c.out(f"d_{n}")
        assert gg.shape == r.shape and bool(torch.isfinite(gg).all()) and float(r.abs().max()) > 0, n
        e = rel(gg, r)
        _say(c, f"d_{n}", e)
        assert e <= 2e-4, (n, e)
        per_point = n in SKIN_OUTPUTS[:4]
        m32 = c.scalar(f"d_{n}_row32" if per_point else f"d_{n}_element32")
        m = float((_row_metric if per_point else _element_metric)(gg, r).max())
        factor = ROW_FACTOR if per_point else ELEMENT_FACTOR
        print(f"{name} d_{n}: worst {'row' if per_point else 'element'} {m:.3e}, the reference's own float32 worst {m32:.3e}, "
              f"ratio {m / m32:.2f} of the {factor} allowed")
        assert 0 < m32 <= (2e-6 if per_point else 2e-5), (n, m32)
        assert m <= factor * m32, (n, m, m32)
    assert bool((grads[6][:, 3, :] == 0).all())


# ------------------------------------------------------------------ FateAvatar's perceptual term
def test_perceptual_against_the_recorded_run(gpu_device):
    """`Perceptual` on the recorded images at the reference's own 224 x 224 (a narrow VGG-16: every width 64): the loss against
    what VGGPerceptualLoss computed in float64, at test_gpu_vgg's bound with the RECORDED e32; the gradient against the pinned
    float64 backward at the device's own saved activations, at the same bound with the float32 restatement's error (the
    reference's own float32 gradient is 2.7e-3 from its float64 one at this size — decisions that flip — and no yardstick:
    the fixture's notes).  Also the first test at the production extent: 100 352 rows, unsplit plans, k_vgg_tap_loss's
    grid-stride loop looping (802 816 float4 against FR_VGG_LOSS_BLOCKS workgroups), a 6-fold upsampling with clamped rows."""
    import torch
    from fateavatar_amd import _lib
    from fateavatar_amd.perceptual import Perceptual, VggFeatures
    from tests import vgg_ref
    from tests.test_gpu_vgg import FLOOR, _bound, _rel
    from tests.test_reference_runs_host import VGG_SIZE
    dev = gpu_device
    c = Case("vgg")
    W, B = mlp_weights(c)
    layers = vgg_ref.NARROW
    img, gt = c.inp("img"), c.inp("gt")
    H, Wd = img.shape[1:]
    p = Perceptual(VggFeatures(layers, W, B, size=VGG_SIZE, device=dev))
    assert VGG_SIZE[0] * VGG_SIZE[1] * 64 // 4 > _lib.FR_VGG_LOSS_BLOCKS * 256          # (the terms' loop does loop)
    loss = torch.full((1 + p.n_terms,), float("nan"), device=dev)
    grad = torch.full((3, H, Wd), float("nan"), device=dev)
    p.loss_and_grad(img.to(dev), gt.to(dev), loss_out=loss, grad_out=grad, weight=1.0)
    torch.cuda.synchronize()
    loss, grad = loss.cpu(), grad.cpu()
    saved = [vgg_ref.nchw(a) for a in p.saved_activations()]
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all()) and p.n_terms == 4
    want = c.out("loss").reshape(1)
    err = _rel(loss[0:1], want)
    _say(c, "loss", err, "relative error")
    assert err <= _bound(c.e32("loss")), (err, c.e32("loss"))
    # the sum of the terms, added in order in float32 as the kernel adds them
    s = torch.zeros((), dtype=torch.float32)
    for t in loss[1:]:
        s = s + t
    assert torch.equal(s, loss[0]) and bool((loss[1:] > 0).all())
    pin64 = vgg_ref.pinned_backward(W, layers, saved, (H, Wd), VGG_SIZE, torch.float64)
    pin32 = vgg_ref.pinned_backward(W, layers, saved, (H, Wd), VGG_SIZE, torch.float32)
    e32, err = _rel(pin32, pin64), _rel(grad, pin64)
    print(f"vgg d_img (pinned, 224 x 224): kernel {err:.3e}  float32 restatement {e32:.3e}  ratio {err / max(e32, FLOOR):.2f}")
    # (for scale only: against the reference's recorded float64 gradient, decisions and all)
    print(f"vgg d_img against the recorded float64 gradient, end to end: {_rel(grad, c.out('d_img')):.3e}")
    assert float(pin64.abs().max()) > 0 and err <= _bound(e32), (err, e32)


# ------------------------------------------------------------------ FLAME with FateAvatar's deltas
# the pose recipe (tests/test_gpu_flame._pose) whose block yardstick a recorded case is held to
FLAME_RECIPES = dict(flame_chain="randn", flame_star="randn", flame_tree_small=("theta", 2e-4), flame_zero=("theta", 0.0),
                     flame_rest="rest", flame_large="large")


@pytest.mark.parametrize("name", FLAME_CASES)
def test_flame_against_the_recorded_run(gpu_device, name):
    """`FlameMesh.forward_into` / `backward_from` on what lbs() itself computed in float64 on a chain, a star and a mixed tree
    and at zero, tiny, partly zero and near-pi / near-2-pi rotations: test_gpu_flame's FACTOR x e32 under CEILING with the
    RECORDED e32, and its block-by-block bound.  At zero pose pose_feature and d_delta_posedirs are exactly zero in the record
    and must be here."""
    import torch
    from tests.test_gpu_flame import _check_blocks, _mesh, _run
    dev = gpu_device
    c = Case(name, inputs_of="flame_chain")
    m = flame_model(c)
    fm = _mesh(m, dev)
    got = _run(fm, m, dev)
    torch.cuda.synchronize()
    assert int(fm.workspace_zeroed_part().count_nonzero()) == 0 and fm.parents.tolist() == m["parents"].tolist()
    r64 = {n: c.out(n) for n in FLAME_OUTPUTS}
    for n in FLAME_OUTPUTS:
        t, want = got[n].cpu(), r64[n]
        assert t.shape == want.shape and bool(torch.isfinite(t).all()), n
        if float(want.abs().max()) == 0:
            assert name == "flame_zero" and n in ("pose_feature", "d_delta_posedirs") and c.e32(n) == 0, n
            assert int(t.count_nonzero()) == 0, n
            print(f"{name} {n}: exactly zero, as recorded")
            continue
        e = rel(t, want)
        _say(c, n, e)
        assert e <= FACTOR * c.e32(n), (n, e, c.e32(n))
        assert e <= CEILING, (n, e)
    _check_blocks(got, r64, m["n_exp"], FLAME_RECIPES[name], name)


# ------------------------------------------------------------------ FlashAvatar's embedding and MLP
def test_embed_points_against_the_recorded_run(gpu_device):
    """`embed_points` on the device (plain torch): test_gpu_mlp's FACTOR x e32.  The arguments x 2^k are exact, so the error is the
    device's sinf / cosf alone."""
    import torch
    from fateavatar_amd.mlp import embed_points
    c = Case("embed")
    got = embed_points(c.inp("points").to(gpu_device)).cpu()
    e = rel(got, c.out("embed"))
    _say(c, "embed", e)
    print(f"embed: worst entry {float((got.double() - c.out('embed')).abs().max()) / EPS:.2f} x 2^-24")
    assert got.shape == (257, 51) and torch.equal(got[:, :3], c.inp("points"))
    assert e <= FACTOR * c.e32("embed")


def test_deform_mlp_against_the_recorded_run(gpu_device):
    """`DeformMLP` forward and backward at N = 257 (one point past two 128-point tiles and past a 256-point weight-gradient
    chunk), two hidden layers: FACTOR x e32 for each of out, d_cond, d_weights, d_bias, the gradients under CEILING, per layer too.
    (`d_weights` is recorded rounded to float32: that moves the truth by at most 2^-24 relative, inside FACTOR x e32 = 1.5e-6.)"""
    import torch
    from fateavatar_amd.mlp import DeformMLP
    dev = gpu_device
    c = Case("mlp")
    W, B = mlp_weights(c)
    L = len(W) - 1
    net = mlp_ref.RefMLP(W[0].shape[1], W[-1].shape[0], hidden_layers=L)
    with torch.no_grad():
        for m, w, b in zip(list(net.fcs) + [net.output_linear], W, B):
            m.weight.copy_(w)
            m.bias.copy_(b)
    N, Dc = c.inp("E").shape[0], c.inp("cond").shape[0]
    mlp = DeformMLP.from_torch(net, c.inp("E").to(dev), Dc)
    cond = c.inp("cond").to(dev)
    out, d_cond = torch.full((N, 10), float("nan"), device=dev), torch.full((Dc,), float("nan"), device=dev)
    mlp.flat_grad.fill_(float("nan"))
    mlp.forward_into(cond, out)
    mlp.backward_from(c.inp("d_out").to(dev), cond, d_cond)
    torch.cuda.synchronize()
    got = dict(out=out, d_cond=d_cond, d_weights=torch.cat([mlp.grad_weight(i).reshape(-1) for i in range(L + 1)]),
               d_bias=torch.cat([mlp.grad_bias(i).reshape(-1) for i in range(L + 1)]))
    for n, t in got.items():
        t = t.cpu()
        e = rel(t, c.out(n))
        _say(c, n, e)
        assert bool(torch.isfinite(t).all()) and float(c.out(n).abs().max()) > 0
        assert e <= FACTOR * c.e32(n), (n, e, c.e32(n))
        if n != "out":
            assert e <= CEILING, (n, e)
    ow = ob = 0
    for i, w in enumerate(W):
        for n, t, start, size in (("d_weights", mlp.grad_weight(i), ow, w.numel()), ("d_bias", mlp.grad_bias(i), ob, w.shape[0])):
            e = rel(t, c.out(n)[start:start + size])
            print(f"mlp {n} of layer {i}: rel-L2 {e:.3e}")
            assert e <= CEILING, (n, i, e)
        ow, ob = ow + w.numel(), ob + w.shape[0]
