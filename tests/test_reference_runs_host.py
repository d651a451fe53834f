"""CPU: the torch restatements the kernel tests are held to, against RECORDED runs of the reference's own Python
(tests/golden/reference_*.npz, written by tests/golden/make_reference_runs.py from the reference's unmodified functions).

The restatements (image_loss_ref, splatting_loss_ref, flash_ref, mlp_ref, rigged_density_ref, mono_ref, mesh_terms_ref, flame_ref) were
written by whoever wrote the kernels, from the same reading of the reference: a misread coefficient, gate or order of
subtraction would be wrong on both sides of every kernel test.  Here each of them runs on the fixture's float32 inputs
  * in float64 and reproduces the reference's float64 result to rel-L2 <= 1e-12 (rounding differences are a few 1e-16; a
    transcription error shows at 1e-3 or more), and
  * in float32 and stays within 4 x e32, the rel-L2 of the reference's own float32 run against its float64 run (a scalar's
    e32 counting as no less than one float32 rounding: reference_runs.float32_allowance),
and the host-side constants of the package are held to the recorded `Params` and `out` dictionaries."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import flame_ref, flash_ref, image_loss_ref, mesh_terms_ref, mlp_ref, mono_ref, rigged_density_ref, splatting_loss_ref, vgg_ref
from tests.reference_runs import Case, everything, float32_allowance, rel

FLOAT64_BOUND = 1e-12
DTYPES = (torch.float64, torch.float32)


def _hold(case, results):
    """`results`: {dtype: {output name: tensor}} of a restatement on the case's inputs, every recorded output present."""
    assert sorted(results[torch.float64]) == sorted(case.outputs()), (sorted(results[torch.float64]), sorted(case.outputs()))
    for name in case.outputs():
        want = case.out(name)
        e64, e32 = rel(results[torch.float64][name], want), rel(results[torch.float32][name], want)
        allowed = float32_allowance(case, name)
        print(f"{case.name} {name}: float64 restatement {e64:.3e} (bound {FLOAT64_BOUND:.0e}); float32 restatement {e32:.3e}, "
              f"reference's own float32 run {case.e32(name):.3e}, allowed {allowed:.3e}")
        assert results[torch.float64][name].dtype == torch.float64 and results[torch.float32][name].dtype == torch.float32, name
        assert float(want.abs().max()) > 0, name
        assert e64 <= FLOAT64_BOUND, (case.name, name, e64)
        assert e32 <= allowed, (case.name, name, e32, allowed)


def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


def test_fixtures_hold_arrays_scalars_and_notes():
    arrays, notes = everything()
    assert "Tensor.cuda" in notes and "rounded to float32" in notes and "laplacian_dense" in notes
    for k, a in arrays.items():
        assert a.dtype.kind in "fi" and a.dtype.itemsize in (4, 8), (k, a.dtype)
        assert bool(torch.isfinite(torch.from_numpy(a.astype("float64"))).all()), k
    # (vgg_d_img: the one output recorded WITHOUT an e32 — the fixture's notes say why no float32 gradient error is to be held)
    assert "NO float32 gradient error" in notes
    assert all(k.endswith("_e32") or f"{k}_e32" in arrays or "_in_" in k or "_param_" in k or "_margin" in k or k.endswith("32")
               or k == "vgg_d_img" for k in arrays)


# ------------------------------------------------------------------ the image terms
@pytest.mark.parametrize("name", ["dssim_3x33x47", "dssim_1x7x5"])
def test_d_ssim_restatement(name):
    c = Case(name)
    res = {}
    for dt in DTYPES:
        _, ds, _, gs = image_loss_ref.terms(c.inp("img"), c.inp("gt"), dt)
        res[dt] = dict(loss=ds, d_img=gs)
    _hold(c, res)


def test_splatting_restatement_and_constants():
    from fateavatar_amd.loss import PixelLoss, ScaleTerm
    c = Case("splat")
    R = splatting_loss_ref.REFERENCE
    assert c.scalar("margin") > 1e-4
    # the constants, against the reference's Params and its `out`
    assert R == {k: c.param(k) for k in ("rgb_weight", "mse_weight", "scale_weight", "scale_threshold", "max_scaling")}
    assert tuple(PixelLoss()) == (c.param("rgb_weight"), c.param("mse_weight"))
    assert tuple(ScaleTerm()) == (c.param("scale_weight"), c.param("scale_threshold"), c.param("max_scaling"))
    assert c.param("lpips_weight") == 0
    total = PixelLoss().rgb_weight * c.out("rgb_loss") + PixelLoss().mse_weight * c.out("mse_loss") + ScaleTerm().weight * c.out("scale_loss")
    assert rel(total, c.out("loss")) <= FLOAT64_BOUND
    res = {}
    for dt in DTYPES:
        words, g = splatting_loss_ref.pixel_terms(c.inp("img"), c.inp("gt"), R["rgb_weight"], R["mse_weight"], dt)
        s_loss, count, gs, sel = splatting_loss_ref.scale_term(c.inp("scaling"), R["scale_weight"], R["scale_threshold"], R["max_scaling"], dt)
        assert 0 < count < 1000 and int(sel.sum()) == count
        res[dt] = dict(loss=words[0] + R["scale_weight"] * s_loss, rgb_loss=words[1], mse_loss=words[2], scale_loss=s_loss, d_img=g,
                       d_scaling=gs)
    _hold(c, res)


@pytest.mark.parametrize("name", ["huber_plain", "huber_mouth"])
def test_huber_restatement_and_constants(name):
    from fateavatar_amd.loss import REFERENCE_HUBER_LOSS
    c = Case(name)
    assert (flash_ref.ALPHA, flash_ref.MASK_WEIGHT) == tuple(REFERENCE_HUBER_LOSS)
    assert c.param("lpips_weight") == 0 and c.param("huber_weight") == 1
    res = {}
    for dt in DTYPES:
        x = _leaf(c.inp("img"), dt)
        mask = c.inp("mask").to(dt) if c.has("mask") else None
        total, _, mouth = flash_ref.huber_loss(x, c.inp("gt").to(dt), mask, *REFERENCE_HUBER_LOSS)
        assert (float(mouth.detach()) > 0) == (name == "huber_mouth")
        (g,) = torch.autograd.grad(total, x)
        res[dt] = dict(loss=total.detach(), d_img=g)
    _hold(c, res)
    # a wrong threshold or mouth weight does not pass: the recorded loss moves by far more than the bound
    if name == "huber_mouth":
        x, gt, m = c.inp("img").double(), c.inp("gt").double(), c.inp("mask").double()
        assert rel(flash_ref.huber_loss(x, gt, m, 0.1, 39.0)[0], c.out("loss")) > 1e-3
        assert rel(flash_ref.huber_loss(x, gt, m, 0.11, 40.0)[0], c.out("loss")) > 1e-3


def test_gaussianavatars_restatement_and_constants():
    from fateavatar_amd.rigged import REFERENCE_IMAGE_LOSS, REFERENCE_REGULARISERS
    c = Case("ga")
    R = rigged_density_ref.REFERENCE
    assert c.scalar("margin_scale") >= 0.01 and c.scalar("margin_xyz") >= 0.01
    assert R == {k: c.param(k) for k in ("scale_weight", "xyz_weight", "threshold_scale", "threshold_xyz")}
    assert tuple(REFERENCE_REGULARISERS) == tuple(R[k] for k in ("scale_weight", "xyz_weight", "threshold_scale", "threshold_xyz"))
    assert tuple(REFERENCE_IMAGE_LOSS) == (c.param("rgb_weight"), c.param("dssim_weight"))
    total = REFERENCE_IMAGE_LOSS.rgb_weight * c.out("rgb_loss") + REFERENCE_IMAGE_LOSS.dssim_weight * c.out("dssim_loss") \
        + R["scale_weight"] * c.out("scale_loss") + R["xyz_weight"] * c.out("xyz_loss")
    assert rel(total, c.out("loss")) <= FLOAT64_BOUND
    res = {}
    for dt in DTYPES:
        t = image_loss_ref.terms(c.inp("img"), c.inp("gt"), dt)
        words, g = image_loss_ref.combine(t, tuple(REFERENCE_IMAGE_LOSS))
        s, x = _leaf(c.inp("scaling"), dt), _leaf(c.inp("xyz"), dt)
        ls, lx = rigged_density_ref.regularisers(s, x, R["threshold_scale"], R["threshold_xyz"])
        gs, gx = torch.autograd.grad(R["scale_weight"] * ls + R["xyz_weight"] * lx, (s, x))
        res[dt] = dict(loss=words[0] + R["scale_weight"] * ls.detach() + R["xyz_weight"] * lx.detach(), rgb_loss=words[1],
                       dssim_loss=words[2], scale_loss=ls.detach(), xyz_loss=lx.detach(), d_img=g, d_scaling=gs, d_xyz=gx)
    _hold(c, res)
    # the float64 helper the kernel test reads is the same thing
    ls, lx, gs, gx = rigged_density_ref.regulariser_grads(c.inp("scaling"), c.inp("xyz"), **R)
    assert rel(gs, c.out("d_scaling")) <= FLOAT64_BOUND and rel(gx, c.out("d_xyz")) <= FLOAT64_BOUND


# ------------------------------------------------------------------ FateAvatar's mesh terms
def test_mesh_terms_restatement_and_constants():
    """What the reference does WITH the Laplacian matrix; the matrix rule itself (pytorch3d's, absent when the fixture was
    made) stays pinned by the hand-written matrices of tests/test_mesh_terms_host.py."""
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS
    c = Case("fate")
    assert tuple(REFERENCE_MESH_TERMS) == (c.param("laplacian_weight"), c.param("configured_flame_weight"))
    assert c.param("rgb_weight") == 1.0
    # (FateAvatarLoss's out['rgb_loss'] is the very tensor out['loss'] is added to in place, so the record has no separate L1
    # word: the restatement's L1 of the same image stands in the identity)
    l1 = image_loss_ref.terms(c.inp("img"), c.inp("gt"), torch.float64)[0]
    total = l1 + REFERENCE_MESH_TERMS.laplacian_weight * c.out("configured_laplacian_loss")
    assert rel(total, c.out("configured_loss")) <= FLOAT64_BOUND
    V, faces = c.inp("verts").shape[0], c.inp("faces").numpy()
    w_lap, w_flame = c.param("laplacian_weight"), c.param("flame_weight")
    res = {}
    for dt in DTYPES:
        L = mesh_terms_ref.laplacian_dense(faces, V, dt)
        vo = c.inp("verts_orig").to(dt)
        l1 = image_loss_ref.terms(c.inp("img"), c.inp("gt"), dt)[0]
        v = _leaf(c.inp("verts"), dt)
        lap, flame = mesh_terms_ref.laplacian_smoothing(L, vo, v), mesh_terms_ref.flame_distance(vo, v)
        (g_lap,), (g_flame,) = torch.autograd.grad(lap, v, retain_graph=True), torch.autograd.grad(flame, v)
        lap, flame = lap.detach(), flame.detach()
        res[dt] = dict(laplacian_loss=lap, laplacian_d_verts=g_lap, configured_laplacian_loss=lap, configured_loss=l1 + w_lap * lap,
                       configured_d_verts=w_lap * g_lap, flame_flame_loss=flame, flame_loss=l1 + w_flame * flame,
                       flame_d_verts=w_flame * g_flame)
    _hold(c, res)
    t = mesh_terms_ref.float64_terms(faces, V, c.inp("verts_orig"), c.inp("verts"), w_lap, w_flame)
    assert rel(t["grad"], c.out("configured_d_verts") + c.out("flame_d_verts")) <= FLOAT64_BOUND
    assert abs(t["lap"] - float(c.out("laplacian_loss"))) <= FLOAT64_BOUND * t["lap"]
    assert abs(t["flame"] - float(c.out("flame_flame_loss"))) <= FLOAT64_BOUND * t["flame"]


# ------------------------------------------------------------------ MonoGaussianAvatar
def mono_tables(c, dtype=torch.float32):
    """(gt_weights [V,J], gt_posedirs [V,36,3], gt_shapedirs [V,3,E]) as `lbs_terms_and_grad` takes them, from FLAME's tables as
    the reference's loss receives them: a zero column in front for the ghost bone, the [36, 3 V] pose basis transposed."""
    w, P, S = c.inp("flame_lbs_weights").to(dtype), c.inp("flame_posedirs").to(dtype), c.inp("flame_shapedirs").to(dtype)
    if c.inp("lbs_weights").shape[1] == w.shape[1] + 1:
        w = torch.cat([torch.zeros_like(w[:, :1]), w], dim=1)
    return w.contiguous(), P.reshape(36, -1, 3).transpose(0, 1).contiguous(), S.contiguous()


def mono_var(c):
    return c.inp("var_expression") if c.has("var_expression") else None


@pytest.mark.parametrize("name", ["lbs_ghost", "lbs_var_ghost", "lbs_e7_j5"])
def test_lbs_terms_restatement_and_coefficients(name):
    from fateavatar_amd.mono import reference_lbs_weights
    c = Case(name, inputs_of="lbs_ghost")
    var = mono_var(c)
    assert (var is not None) == (name == "lbs_var_ghost")
    coeff = reference_lbs_weights(c.param("lbs_weight"), var)
    assert c.param("lbs_weight") == 10.0 and coeff == reference_lbs_weights(var_expression=var)
    # the three recorded words are 1, 100 and 100 (x mean(1 / var) / 50) times the plain mean squared errors
    word = (1.0, 100.0, 100.0 * (float((1.0 / var.double()).mean()) / 50.0 if var is not None else 1.0))
    res = {}
    for dt in DTYPES:
        leaves = [_leaf(c.inp(k), dt) for k in ("lbs_weights", "posedirs", "shapedirs")]
        t = mono_ref.lbs_terms(c.inp("index"), *leaves, *mono_tables(c, dt))
        total = (t * torch.tensor(tuple(coeff), dtype=dt)).sum()
        grads = torch.autograd.grad(total, leaves)
        t = t.detach()
        res[dt] = dict(lbs_loss=word[0] * t[0], posedirs_loss=word[1] * t[1], shapedirs_loss=word[2] * t[2], loss=total.detach(),
                       d_lbs_weights=grads[0], d_posedirs=grads[1], d_shapedirs=grads[2])
    _hold(c, res)
    if var is not None:           # the variance matters: the coefficient without it misses the recorded total
        plain = (res[torch.float64]["lbs_loss"] * coeff[0] + res[torch.float64]["posedirs_loss"] / 100 * coeff[1]
                 + mono_ref.lbs_terms(c.inp("index"), *[c.inp(k).double() for k in ("lbs_weights", "posedirs", "shapedirs")],
                                      *mono_tables(c, torch.float64))[2] * reference_lbs_weights(10.0).shapedirs)
        assert rel(plain, c.out("loss")) > 1e-3


def skinning_inputs(c, dtype, device="cpu"):
    """(the four per-point inputs, the canonical state, the frame's state, g) of a skinning case."""
    to = lambda k: c.inp(k).to(dtype).to(device)  # noqa: E731
    return [to(k) for k in ("points", "shapedirs", "posedirs", "lbs_weights")], \
        tuple(to(k) for k in ("canonical_betas", "canonical_pose_feature", "canonical_transforms")), \
        tuple(to(k) for k in ("betas", "pose_feature", "transforms")), to("g")


SKIN_OUTPUTS = ("points", "shapedirs", "posedirs", "lbs_weights", "betas", "pose_feature", "transforms")


@pytest.mark.parametrize("name", ["skin_65_50_6", "skin_257_7_5"])
def test_point_skinning_restatement(name):
    c = Case(name)
    res = {}
    for dt in DTYPES:
        x, canonical, frame, g = skinning_inputs(c, dt)
        leaves = [t.requires_grad_(True) for t in x + list(frame)]
        xyz = mono_ref.deform_points(*leaves[:4], canonical, tuple(leaves[4:]))
        grads = torch.autograd.grad(xyz, leaves, g)
        res[dt] = dict(xyz=xyz.detach(), **{f"d_{n}": t for n, t in zip(SKIN_OUTPUTS, grads)})
    _hold(c, res)
    # the written backward and the kernels' closed forms, which the host tests derive from the restatement, against the record
    x, canonical, frame, g = skinning_inputs(c, torch.float64)
    for which, got in (("written backward", mono_ref.deform_points_backward(*x, canonical, frame, g)),
                       ("closed form", mono_ref.deform_points_closed_form(*x, canonical, frame, g)[1:])):
        for n, t in zip(SKIN_OUTPUTS[:4], got):
            assert rel(t, c.out(f"d_{n}")) <= 1e-11, (which, n, rel(t, c.out(f"d_{n}")))
    assert bool((c.out("d_transforms")[:, 3, :] == 0).all())
    for n in SKIN_OUTPUTS[:4]:
        assert 0 < c.scalar(f"d_{n}_row32") <= 2e-6
    for n in SKIN_OUTPUTS[4:]:
        assert 0 < c.scalar(f"d_{n}_element32") <= 2e-5


# ------------------------------------------------------------------ FLAME with FateAvatar's deltas
FLAME_CASES = ("flame_chain", "flame_star", "flame_tree_small", "flame_zero", "flame_rest", "flame_large")
FLAME_OUTPUTS = ("verts", "pose_feature", "A", "d_delta_exp", "d_delta_posedirs", "d_delta_vertex", "d_expression", "d_pose")
FLAME_TABLES = ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "delta_shapedirs", "delta_posedirs", "delta_vertex",
                "expression", "g")


def flame_model(c):
    """The model dict of tests/flame_ref.run from a recorded FLAME case (float32 tensors, as every run read them)."""
    m = {k: c.inp(k) for k in FLAME_TABLES + ("pose",)}
    m["parents"] = c.inp("parents")
    m["n_shape"], m["n_exp"] = int(c.param("n_shape")), int(c.param("n_exp"))
    return m


@pytest.mark.parametrize("name", FLAME_CASES)
def test_flame_restatement_on_other_trees_and_pose_regimes(name):
    """tests/flame_ref.py in float64 against lbs() itself on a chain, a star and a mixed tree, at zero, tiny, partly zero and
    near-pi / near-2-pi rotations: 1e-12 of the largest magnitude (tests/test_flame_host.py's bound); what is exactly zero in
    the record is exactly zero here."""
    c = Case(name, inputs_of="flame_chain")
    m = flame_model(c)
    assert sorted(c.outputs()) == sorted(FLAME_OUTPUTS) and m["v_template"].shape == (65, 3) and (m["n_shape"], m["n_exp"]) == (2, 5)
    assert all(0 <= int(m["parents"][i]) < i for i in range(1, 5)) and int(m["parents"][0]) == -1
    r = flame_ref.run(m, torch.float64)
    assert int(r["d_delta_shapedirs"][:, :, :m["n_shape"]].count_nonzero()) == 0
    r["d_delta_exp"] = r.pop("d_delta_shapedirs")[:, :, m["n_shape"]:]
    zero = ("pose_feature", "d_delta_posedirs") if name == "flame_zero" else ()
    for k in FLAME_OUTPUTS:
        want = c.out(k)
        scale, worst = float(want.abs().max()), float((r[k] - want).abs().max())
        print(f"{name} {k}: float64 restatement max |d| {worst:.3e} of max |want| {scale:.3e}; reference's own float32 run {c.e32(k):.3e}")
        assert r[k].dtype == torch.float64 and r[k].shape == want.shape
        assert (scale == 0) == (k in zero), k
        assert worst <= FLOAT64_BOUND * scale, (k, worst, scale)
    # the stable form of the rotation is the same function: it differs from the reference's form by float64 rounding alone
    s = flame_ref.run(m, torch.float64, stable_rotation=True)
    for k in ("verts", "pose_feature", "A", "d_delta_posedirs", "d_pose"):
        want = c.out(k)
        assert float((s[k] - want).abs().max()) <= 1e-9 * max(float(want.abs().max()), 1e-30) or k in zero, k
    if name == "flame_tree_small":
        # what the regime is recorded for: the reference's own float32 run loses four digits here, on exactly these outputs
        assert c.e32("pose_feature") > 2e-5 and c.e32("d_pose") > 2e-5 and c.e32("verts") < 1e-6


# ------------------------------------------------------------------ FlashAvatar's embedding, MLP and quaternion product
def mlp_weights(c, dtype=torch.float32):
    n = sum(1 for k in c.arrays if k.startswith(f"{c.name}_in_weight_"))
    return [c.inp(f"weight_{i}").to(dtype) for i in range(n)], [c.inp(f"bias_{i}").to(dtype) for i in range(n)]


def test_embedding_restatement_and_the_package_function():
    from fateavatar_amd.mlp import embed_points
    c = Case("embed")
    for fn in (mlp_ref.embed, embed_points):
        _hold(c, {dt: dict(embed=fn(c.inp("points").to(dt))) for dt in DTYPES})
    # the MLP case is fed the reference's float32 embedding of these points
    assert rel(Case("mlp").inp("E"), c.out("embed")) <= 4 * c.e32("embed")


def test_mlp_restatement():
    from tests.test_gpu_mlp import SEED_MARGIN
    c = Case("mlp")
    assert c.scalar("margin") >= SEED_MARGIN and c.inp("E").shape == (257, 51) and c.inp("cond").shape == (59,)
    res = {}
    for dt in DTYPES:
        W, B = mlp_weights(c, dt)
        assert len(W) == 3
        r = mlp_ref.run(W, B, c.inp("E"), c.inp("cond"), c.inp("d_out"))
        res[dt] = dict(out=r["out"], d_cond=r["d_cond"], d_weights=torch.cat([t.reshape(-1) for t in r["d_weights"]]),
                       d_bias=torch.cat([t.reshape(-1) for t in r["d_bias"]]))
    # d_weights is recorded rounded to float32 (the fixture's notes): held to one float32 rounding in the norm, not to 1e-12
    want = c.out("d_weights")
    e = rel(res[torch.float64].pop("d_weights"), want)
    e32 = rel(res[torch.float32].pop("d_weights"), want)
    print(f"mlp d_weights: float64 restatement {e:.3e} of a float32-rounded record; float32 restatement {e32:.3e}, "
          f"reference's own {c.e32('d_weights'):.3e}")
    assert e <= 2.0 ** -24 and e32 <= 4 * c.e32("d_weights") + 2.0 ** -24
    outputs = c.outputs
    c.outputs = lambda: [n for n in outputs() if n != "d_weights"]
    _hold(c, res)


# ------------------------------------------------------------------ FateAvatar's perceptual term
VGG_SIZE = (224, 224)           # the reference's hard-coded resize


def test_perceptual_restatement():
    """tests/vgg_ref.py against VGGPerceptualLoss as it is (its normalisation with float32 statistics, its resize, its four
    slices of a narrow VGG-16 in torchvision's layout): loss and gradient in float64 to 1e-12, the float32 loss within 4 x e32.
    No float32 gradient is held: the reference's own is 2.7e-3 from its float64 one at this size (decisions that flip)."""
    from fateavatar_amd.perceptual import VGG16_LAYERS, torchvision_indices
    c = Case("vgg")
    W, B = mlp_weights(c)
    layers = vgg_ref.NARROW
    assert len(W) == len(layers) == len(VGG16_LAYERS) and c.outputs() == ["loss"]
    assert [(y[2], y[3]) for y in layers] == [(y.pool_before, y.tap_after) for y in VGG16_LAYERS]
    assert torchvision_indices(layers) == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21]
    assert all(tuple(w.shape) == (co, ci, 3, 3) and tuple(b.shape) == (co,) for (ci, co, _, _), w, b in zip(layers, W, B))
    img, gt = c.inp("img"), c.inp("gt")
    assert img.shape == (3, 37, 53)
    loss64, g64 = vgg_ref.autograd_gradient(W, B, layers, img, gt, VGG_SIZE, torch.float64)
    r64 = vgg_ref.forward(W, B, layers, img, gt, VGG_SIZE, torch.float64)
    r32 = vgg_ref.forward(W, B, layers, img, gt, VGG_SIZE, torch.float32)
    _hold(c, {torch.float64: dict(loss=r64["loss"]), torch.float32: dict(loss=r32["loss"])})
    e_loss, e_grad = rel(loss64, c.out("loss")), rel(g64, c.out("d_img"))
    print(f"vgg: float64 restatement through autograd: loss {e_loss:.3e}, d_img {e_grad:.3e} (bound {FLOAT64_BOUND:.0e})")
    assert float(c.out("d_img").abs().max()) > 0 and e_loss <= FLOAT64_BOUND and e_grad <= FLOAT64_BOUND
    # the reference's float32 loss is the recorded e32 away from its float64 one
    assert math.isclose(rel(c.scalar("loss32"), c.out("loss")), c.e32("loss"), rel_tol=1e-6)
    # what the record found: statistics built in float64 miss it (1.4e-10 in the loss, 2.3e-8 in the gradient)
    x = torch.stack([img, gt]).double()
    wrong = F.interpolate((x - torch.tensor(vgg_ref.MEAN, dtype=torch.float64).view(1, 3, 1, 1))
                          / torch.tensor(vgg_ref.STD, dtype=torch.float64).view(1, 3, 1, 1), mode="bilinear", size=VGG_SIZE, align_corners=False)
    assert rel(wrong, r64["x"]) > 1e-9 and rel(wrong, r64["x"]) < 1e-6


def test_quaternion_product_restatement():
    c = Case("quat")
    _hold(c, {dt: dict(product=flash_ref.quat_product(c.inp("q1").to(dt), c.inp("q2").to(dt))) for dt in DTYPES})
    # the order matters: the product the other way round is another quaternion
    assert rel(flash_ref.quat_product(c.inp("q2").double(), c.inp("q1").double()), c.out("product")) > 1e-2
    assert math.isclose(float(c.inp("q1").norm(dim=1).mean()), 1.0, rel_tol=1e-6)
