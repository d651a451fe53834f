"""-m gpu: the fused LPIPS term (fr_lpips_loss_grad in csrc/fr_vgg.hip, perceptual.Lpips) on the device against the float64
restatement of tests/lpips_ref.py, with tests/test_gpu_vgg.py's bound: a quantity's rel-L2 error against float64 is at most
min(FACTOR x max(e32, 2^-24), CEILING), e32 being the float32 CPU restatement's own error for that quantity.

The reference is the DEFINITION in include/fr_rasterizer.h, restated from stock torch ops: neither `lpips` nor `torchvision` is
installed where this was written and the reference project does not vendor `lpips`, so no run of the reference's own module
could be recorded (tests/golden has none for this term), and the weights are seeded stand-ins.

As in tests/test_gpu_vgg.py the forward is compared directly and the backward twice: against the PINNED float64 backward at the
device's own saved activations (ReLU masks, pool argmaxes; the tap seed is continuous and has no decision of its own), and end
to end against float64 autograd on inputs whose float64 decisions are clear.  Dead pixels (all-zero feature vectors, where stock
autograd is NaN) in the rendered image, in the target and in both, identical images, the GEMM split plans, taps beyond one sweep
of k_lpips_tap's grid, widths that are odd multiples of 64, flat regions (vgg_ref.patchwork) and the call contract have tests of
their own."""
import functools

import pytest

from tests import lpips_ref, vgg_ref
from tests.test_gpu_vgg import CEILING, CLEAR, FACTOR, FLOOR, MASK_Z, ODD_CASES, WIDE_CASES, _background_interior, _bound, _rel

pytestmark = pytest.mark.gpu

STACKS = {"lpips13": lpips_ref.LPIPS13, "small": vgg_ref.SMALL, "wide": vgg_ref.WIDE, "odd": vgg_ref.ODD}
# (stack, H, W, size_h, size_w)
CASES = [("lpips13", 32, 32, 32, 32),     # deepest map 2 x 2
         ("lpips13", 48, 32, 48, 32),     # non-square, ragged M
         ("lpips13", 16, 16, 16, 16),     # deepest map 1 x 1: all halo, a one-pixel mean
         ("lpips13", 37, 53, 32, 32),     # resized (LPIPS itself does not; the descriptor may)
         ("small", 24, 24, 24, 24)]       # descriptor generality: adjacent taps, a tap behind a pool
END_TO_END = [CASES[0], CASES[2], CASES[4]]
# The first seed from 0 on at which the float64 restatement keeps every ReLU and pool decision CLEAR (lpips_ref.decisions_clear),
# found by this same float64-only search on the CPU; the loop in _clear_case still checks the criterion.
FIRST_CLEAR_SEED = {CASES[0]: 71, CASES[2]: 2, CASES[4]: 5}
# k_lpips_tap runs FR_VGG_LOSS_BLOCKS workgroups of four waves, one pixel a wave: 4096 pixels a sweep (tests/test_lpips_host.py
# holds the arithmetic against the library's constant).  CASES stay inside one sweep; these do not:
PAST_THE_CAP = [("small", 70, 62, 70, 62),       # tap 1: 4340 pixels, a second sweep that 61 workgroups take part in; tap 2: 1085
                                                 # pixels, not a multiple of 4 — the last workgroup has three idle waves
                ("lpips13", 80, 64, 80, 64)]     # tap 1: 5120 pixels (the smallest such size divisible by 16); 1280, 320, 80, 20
# vgg_ref.patchwork's flat regions (identity sizes): a pool, the 13-layer trunk, and the stack whose GEMMs add the seed in the
# MASK epilogue and the split-reduce
PATCHWORK = [("small", 24, 24, 24, 24), ("lpips13", 32, 32, 32, 32), ("wide", 32, 32, 32, 32)]


@functools.lru_cache(maxsize=None)
def _weights(stack):
    W, B = vgg_ref.he_weights(STACKS[stack], seed=11 + len(STACKS[stack]))
    return W, B, lpips_ref.lin_weights(STACKS[stack], seed=7)


@functools.lru_cache(maxsize=None)
def _case(stack, H, W, sh, sw, patchwork=False):
    """Weights, images and both restatements' forwards on the CPU: computed once, shared, never modified."""
    import torch
    Wt, B, lin = _weights(stack)
    img, gt = (vgg_ref.patchwork if patchwork else vgg_ref.images)(H, W, seed=1000 * H + W)
    r64 = lpips_ref.forward(Wt, B, lin, STACKS[stack], img, gt, (sh, sw), torch.float64)
    r32 = lpips_ref.forward(Wt, B, lin, STACKS[stack], img, gt, (sh, sw), torch.float32)
    return dict(W=Wt, B=B, lin=lin, img=img, gt=gt, r64=r64, r32=r32)


@functools.lru_cache(maxsize=None)
def _clear_case(stack, H, W, sh, sw):
    import torch
    Wt, B, lin = _weights(stack)
    layers = STACKS[stack]
    for attempt in range(400):
        img, gt = vgg_ref.images(H, W, seed=FIRST_CLEAR_SEED[(stack, H, W, sh, sw)] + attempt)
        r64 = lpips_ref.forward(Wt, B, lin, layers, img, gt, (sh, sw), torch.float64)
        if lpips_ref.decisions_clear(r64, layers, CLEAR):
            break
    else:
        raise AssertionError("no seed keeps the float64 decisions clear of their thresholds")
    loss64, g64 = lpips_ref.autograd_gradient(Wt, B, lin, layers, img, gt, (sh, sw), torch.float64)
    loss32, g32 = lpips_ref.autograd_gradient(Wt, B, lin, layers, img, gt, (sh, sw), torch.float32)
    return dict(img=img, gt=gt, loss64=loss64, g64=g64, loss32=loss32, g32=g32, attempts=attempt + 1)


def _lpips(layers, W, B, lin, size, dev, weight=0.05):
    from fateavatar_amd.perceptual import Lpips, VggFeatures
    return Lpips(VggFeatures(layers, W, B, size=size, device=dev), lin, weight)


def _ids(c):
    return f"{c[0]}-{c[1]}x{c[2]}-to-{c[3]}x{c[4]}"


def _held_to_float64(dev, name, layers, c, hw, size, tile=None):
    """The held set: input, every activation, the terms and the loss against float64; the ReLU decisions inside the band; the
    gradient against the pinned float64 backward at the device's own activations.  `c`: W, B, lin, img, gt, r64, r32."""
    import torch
    H, W = hw
    r64, r32 = c["r64"], c["r32"]
    p = _lpips(layers, c["W"], c["B"], c["lin"], size, dev)
    if tile is not None:
        p.tile = tile
    T = sum(1 for y in layers if y[3])
    assert p.n_terms == T
    loss = torch.full((1 + T,), float("nan"), device=dev)
    grad = torch.full((3, H, W), float("nan"), device=dev)      # every element is to be OVERWRITTEN
    p.loss_and_grad(c["img"].to(dev), c["gt"].to(dev), loss_out=loss, grad_out=grad, weight=1.0)
    torch.cuda.synchronize()
    loss, grad = loss.cpu(), grad.cpu()
    saved = [vgg_ref.nchw(a) for a in p.saved_activations()]
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    assert len(saved) == len(layers) and all(s.shape == a.shape for s, a in zip(saved, r64["a"]))

    def held(what, got, ref64, ref32):
        e32, err = _rel(ref32, ref64), _rel(got, ref64)
        print(f"{name} {what}: kernel {err:.3e}  float32 restatement {e32:.3e}  ratio {err / max(e32, FLOOR):.2f}")
        assert float(ref64.abs().max()) > 0
        assert err <= _bound(e32), (what, err, e32)

    held("input", vgg_ref.nchw(p.saved_input()), r64["x"], r32["x"])
    for l in range(len(layers)):
        held(f"activation {l}", saved[l], r64["a"][l], r32["a"][l])
    held("terms", loss[1:], torch.stack(r64["terms"]), torch.stack(r32["terms"]))
    held("loss", loss[0:1], r64["loss"].reshape(1), r32["loss"].reshape(1))
    # the per-pixel reciprocal norms the backward reads
    taps = [l for l, y in enumerate(layers) if y[3]]
    for k, (l, px) in enumerate(zip(taps, p.saved_pixel_scalars())):
        px = px.cpu()
        for i, which in enumerate("ab"):
            r_64, r_32 = (lpips_ref._unit(r["a"][l][i], r["a"][l].dtype)[1] for r in (r64, r32))
            held(f"tap {k} r_{which}", px[..., i], r_64, r_32)

    flips = band = 0
    for l in range(len(layers)):
        z = r64["z"][l]
        tol = MASK_Z * float(z.pow(2).mean().sqrt())
        diff = (saved[l] > 0) != (z > 0)
        flips += int(diff.sum())
        band += int((z.abs() < tol).sum())
        if diff.any():
            assert float(z[diff].abs().max()) < tol, ("mask", l, float(z[diff].abs().max()), tol)
    print(f"{name} ReLU decisions that differ from float64's: {flips} (float64 units inside the band: {band})")
    assert flips <= band

    pin64 = lpips_ref.pinned_backward(c["W"], c["lin"], layers, saved, (H, W), size, torch.float64)
    pin32 = lpips_ref.pinned_backward(c["W"], c["lin"], layers, saved, (H, W), size, torch.float32)
    held("d_image (pinned)", grad, pin64, pin32)
    return loss, grad, saved, p


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_and_pinned_backward_against_float64(gpu_device, case):
    stack, H, W, sh, sw = case
    _held_to_float64(gpu_device, _ids(case), STACKS[stack], _case(*case), (H, W), (sh, sw))


def test_dead_pixels_are_finite_and_take_no_gradient(gpu_device):
    """lpips_ref.dead_pixel_case: 123 rendered pixels at tap 1 and 16 at tap 2 are all-zero vectors in float64
    (tests/test_lpips_host.py), where stock autograd is NaN.  The device has them too, its loss and gradient are finite, the
    terms match the restatement (which applies the rule) and the gradient the pinned backward; the pixels' scalars are 0."""
    import torch
    dev = gpu_device
    layers = vgg_ref.SMALL
    W, B, lin, img, gt = lpips_ref.dead_pixel_case()
    c = dict(W=W, B=B, lin=lin, img=img, gt=gt, r64=lpips_ref.forward(W, B, lin, layers, img, gt, (24, 24), torch.float64),
             r32=lpips_ref.forward(W, B, lin, layers, img, gt, (24, 24), torch.float32))
    loss, grad, saved, p = _held_to_float64(dev, "dead-pixels", layers, c, (24, 24), (24, 24))
    dead = lpips_ref.dead_pixels(saved, layers)
    print("dead pixels on the device:", dead)
    assert dead == [(123, 0), (16, 0)]
    for l, px in zip((1, 2), p.saved_pixel_scalars()):
        px = px.cpu()
        d = saved[l][0].pow(2).sum(0) == 0
        assert bool((px[d][:, 0] == 0).all()) and bool((px[d][:, 2] == 0).all()) and bool((px[d][:, 1] > 0).all())
        assert bool((px[~d][:, 0] > 0).all()) and bool(torch.isfinite(px).all())
    assert float(grad.abs().max()) > 0


@pytest.mark.parametrize("case", PAST_THE_CAP + ODD_CASES, ids=_ids)
def test_past_the_grid_cap_and_odd_widths_against_float64(gpu_device, case):
    """The held set where k_lpips_tap's pixel loop takes a second sweep (PAST_THE_CAP: a wave carries its sum over two pixels,
    `px` rows written in the second sweep are read by k_lpips_seed, and a tap of 1085 pixels leaves waves of the last workgroup
    idle in the last-workgroup sum), and on vgg_ref.ODD, whose taps hold 3, 5 and 7 values a lane behind the kernel's `j < nv`
    guards and whose GEMMs have 3, 5 and 7 column tiles."""
    stack, H, W, sh, sw = case
    _held_to_float64(gpu_device, _ids(case), STACKS[stack], _case(*case), (H, W), (sh, sw))


def test_past_the_grid_cap_same_bits_on_every_launch(gpu_device):
    import torch
    dev = gpu_device
    stack, H, W, sh, sw = PAST_THE_CAP[0]
    c = _case(*PAST_THE_CAP[0])
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    p = _lpips(STACKS[stack], c["W"], c["B"], c["lin"], (sh, sw), dev)
    first = [t.clone() for t in p.loss_and_grad(img, gt)]
    second = [t.clone() for t in p.loss_and_grad(img, gt)]
    torch.cuda.synchronize()
    assert float(first[0][0]) > 0 and float(first[1].abs().max()) > 0
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


@functools.lru_cache(maxsize=None)
def _dead_target_case():
    import torch
    W, B, lin, img, gt = lpips_ref.dead_target_case()
    return dict(W=W, B=B, lin=lin, img=img, gt=gt, r64=lpips_ref.forward(W, B, lin, vgg_ref.SMALL, img, gt, (24, 24), torch.float64),
                r32=lpips_ref.forward(W, B, lin, vgg_ref.SMALL, img, gt, (24, 24), torch.float32))


def _check_dead_classes(classes, pxs, both, rendered, target):
    """The per-pixel scalars (r_a, r_b, T / n_a) on each class of dead pixels; `both`, `rendered`, `target`: the positions of
    those classes in a tap's triple of masks (the swapped call exchanges the last two)."""
    import torch
    for masks, px in zip(classes, pxs):
        assert bool(torch.isfinite(px).all())
        t = px[masks[target]]
        assert bool((t[:, 1] == 0).all()) and bool((t[:, 0] > 0).all())
        r = px[masks[rendered]]
        assert bool((r[:, 0] == 0).all()) and bool((r[:, 2] == 0).all()) and bool((r[:, 1] > 0).all())
        assert bool((px[masks[both]] == 0).all())
        live = ~(masks[0] | masks[1] | masks[2])
        assert bool((px[live][:, :2] > 0).all())


def test_dead_targets_and_doubly_dead_pixels(gpu_device):
    """lpips_ref.dead_target_case: per tap (31, 92, 138) and (1, 15, 21) pixels are dead in both images, in the rendered one
    alone and in the target alone in float64 (tests/test_lpips_host.py).  The device has all three classes at both taps, holds
    the restatement's terms and the pinned backward, and its scalars say which is which: r_b == 0 at a dead target under a live
    rendered pixel, r_a == 0 and T / n_a == 0 at a dead rendered pixel, all three 0 where both are dead.  With the images
    swapped the terms are the same (the term is symmetric) and the two one-sided classes change places."""
    import torch
    dev = gpu_device
    layers = vgg_ref.SMALL
    c = _dead_target_case()
    loss, grad, saved, p = _held_to_float64(dev, "dead-targets", layers, c, (24, 24), (24, 24))
    classes = lpips_ref.dead_classes(saved, layers)
    counts = [tuple(int(m.sum()) for m in masks) for masks in classes]
    counts64 = [tuple(int(m.sum()) for m in masks) for masks in lpips_ref.dead_classes(c["r64"]["a"], layers)]
    print(f"dead-targets (both, rendered only, target only) per tap on the device: {counts}  float64: {counts64}")
    assert all(n > 0 for tap in counts for n in tap)
    pxs = [px.cpu().clone() for px in p.saved_pixel_scalars()]
    _check_dead_classes(classes, pxs, both=0, rendered=1, target=2)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    # ---- swapped: the same terms, the classes change places (the gradient, the other image's, is not compared)
    loss_s, grad_s = p.loss_and_grad(c["gt"].to(dev), c["img"].to(dev), weight=1.0)
    torch.cuda.synchronize()
    loss_s = loss_s.cpu()
    assert bool(torch.isfinite(loss_s).all()) and bool(torch.isfinite(grad_s).all())
    ref64, ref32 = torch.stack(c["r64"]["terms"]), torch.stack(c["r32"]["terms"])
    e32, err = _rel(ref32, ref64), _rel(loss_s[1:], ref64)
    print(f"dead-targets swapped terms: kernel {err:.3e}  float32 restatement {e32:.3e}  ratio {err / max(e32, FLOOR):.2f}")
    assert err <= _bound(e32), (err, e32)
    swapped = lpips_ref.dead_classes([vgg_ref.nchw(a) for a in p.saved_activations()], layers)
    for masks, masks_s in zip(classes, swapped):
        assert torch.equal(masks_s[0], masks[0]) and torch.equal(masks_s[1], masks[2]) and torch.equal(masks_s[2], masks[1])
    _check_dead_classes(classes, [px.cpu() for px in p.saved_pixel_scalars()], both=0, rendered=2, target=1)


@pytest.mark.parametrize("case", PATCHWORK, ids=_ids)
def test_flat_regions_against_float64(gpu_device, case):
    """The held set on vgg_ref.patchwork under the LPIPS term kind: the VGG_TERM_LPIPS instantiations of k_vgg_unpool, of the
    MASK epilogue and of the split-reduce add a seed read from a buffer where the L1 term computes a sign.  Thousands of live
    pool windows are exact ties (none in vgg_ref.WIDE, which has no pool: there only the live zero tap differences count), and
    inside the shared background a^ - b^ is exactly 0, so T / n_a is exactly 0 and the interior of the quadrant takes a gradient
    of exactly 0, tied pools included.  The interior is empty for the 13-layer trunk at 32 x 32 (its margin is 195 pixels)."""
    import torch
    stack, H, W, sh, sw = case
    layers = STACKS[stack]
    c = _case(*case, patchwork=True)
    loss, grad, saved, p = _held_to_float64(gpu_device, _ids(case) + " patchwork", layers, c, (H, W), (sh, sw))
    ties64, zeros64 = vgg_ref.live_ties(c["r64"]["a"], layers)
    ties, zeros = vgg_ref.live_ties(saved, layers)
    print(f"{_ids(case)} patchwork: live tied windows {ties} on the device (float64: {ties64}), live zero tap differences {zeros} "
          f"(float64: {zeros64})")
    if any(y[2] for y in layers):
        assert ties64 >= 1000
    assert zeros64 >= 1000
    assert 2 * ties >= ties64 and 2 * zeros >= zeros64
    rows, cols = _background_interior(layers, H, W, sh, sw)
    print(f"{_ids(case)} patchwork: shared-background interior {rows} x {cols} pixels")
    assert (rows > 0 and cols > 0) == (stack != "lpips13")
    assert bool((grad[:, :rows, :cols] == 0).all())
    assert float(grad[:, H // 2:, :].abs().max()) > 0 and float(grad[:, :, W // 2:].abs().max()) > 0
    # inside the interior the two images' activations are the same bits, layer by layer
    for (h, w), a in zip(p.features.extents(), p.saved_activations()):
        k = rows // (H // h)
        if k:
            assert torch.equal(a[0, :k, :k], a[1, :k, :k])


@pytest.mark.parametrize("stack,hw,patchwork", [("small", (24, 24), False), ("lpips13", (32, 32), False), ("small", (24, 24), True)],
                         ids=["small-hw0", "lpips13-hw1", "small-patchwork"])
def test_identical_images_give_exact_zeros(gpu_device, stack, hw, patchwork):
    import torch
    dev = gpu_device
    Wt, B, lin = _weights(stack)
    x = (vgg_ref.patchwork if patchwork else vgg_ref.images)(*hw, seed=9)[0].to(dev)
    p = _lpips(STACKS[stack], Wt, B, lin, hw, dev)
    loss = torch.full((1 + p.n_terms,), float("nan"), device=dev)
    grad = torch.full_like(x, float("nan"))
    p.loss_and_grad(x, x.clone(), loss_out=loss, grad_out=grad, weight=1.0)
    torch.cuda.synchronize()
    assert bool((loss == 0).all()) and bool((grad == 0).all())
    assert all(float(a.abs().max()) > 0 for a in p.saved_activations())
    X = torch.randn(x.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    buf = X.clone()
    p.loss_and_grad(x, x.clone(), grad_out=buf, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(buf, X)


@functools.lru_cache(maxsize=None)
def _wide_case(stack, H, W, sh, sw):
    import torch
    Wt, B, lin = _weights("wide")
    img, gt = vgg_ref.images(H, W, seed=1000 * H + W)
    return dict(W=Wt, B=B, lin=lin, img=img, gt=gt, r64=lpips_ref.forward(Wt, B, lin, vgg_ref.WIDE, img, gt, (sh, sw), torch.float64),
                r32=lpips_ref.forward(Wt, B, lin, vgg_ref.WIDE, img, gt, (sh, sw), torch.float32))


@pytest.mark.parametrize("case", WIDE_CASES, ids=_ids)
def test_every_split_plan_against_float64(gpu_device, case):
    """vgg_ref.WIDE at the three sizes whose GEMMs take one, three and nine planes: the tap-1 seed goes through the in-kernel
    MASK epilogue or the split-reduce's (tests/test_lpips_host.py says which), the last tap's is the first GEMM's operand; and
    the larger tile changes no bit."""
    import torch
    from fateavatar_amd import _lib
    dev = gpu_device
    stack, H, W, sh, sw = case
    c = _wide_case(*case)
    loss, grad, saved, p = _held_to_float64(dev, _ids(case), vgg_ref.WIDE, c, (H, W), (sh, sw), tile=_lib.FR_VGG_TILE_AUTO)
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    for tile in (_lib.FR_VGG_TILE_64, _lib.FR_VGG_TILE_128):
        p.tile = tile
        loss_t, g_t = p.loss_and_grad(img, gt, weight=1.0)
        torch.cuda.synchronize()
        assert torch.equal(loss_t.cpu(), loss) and torch.equal(g_t.cpu(), grad), tile


@pytest.mark.parametrize("case", END_TO_END, ids=_ids)
def test_gradient_end_to_end_against_float64_autograd(gpu_device, case):
    import torch
    dev = gpu_device
    stack, H, W, sh, sw = case
    c = _clear_case(*case)
    Wt, B, lin = _weights(stack)
    p = _lpips(STACKS[stack], Wt, B, lin, (sh, sw), dev)
    loss, grad = p.loss_and_grad(c["img"].to(dev), c["gt"].to(dev), weight=1.0)
    torch.cuda.synchronize()
    e32, err = _rel(c["g32"], c["g64"]), _rel(grad.cpu(), c["g64"])
    print(f"{_ids(case)} end to end after {c['attempts']} draws: kernel {err:.3e}  float32 autograd {e32:.3e}  ratio {err / max(e32, FLOOR):.2f}")
    assert float(c["g64"].abs().max()) > 0
    assert err <= _bound(e32), (err, e32)
    l32, lerr = _rel(c["loss32"].reshape(1), c["loss64"].reshape(1)), _rel(loss[0:1].cpu(), c["loss64"].reshape(1))
    print(f"{_ids(case)} loss: kernel {lerr:.3e}  float32 {l32:.3e}")
    assert lerr <= _bound(l32), (lerr, l32)


def test_accumulate_weight_and_forward_only(gpu_device):
    import torch
    dev = gpu_device
    stack, H, W, sh, sw = CASES[3]
    c = _case(*CASES[3])
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    p = _lpips(STACKS[stack], c["W"], c["B"], c["lin"], (sh, sw), dev, weight=0.05)
    assert p.weight == 0.05 and p.n_terms == 5
    loss1, g1 = (t.clone() for t in p.loss_and_grad(img, gt, weight=1.0))
    loss_q, g_q = p.loss_and_grad(img, gt, weight=0.25)
    assert torch.equal(loss_q, loss1)
    assert torch.allclose(g_q, 0.25 * g1, rtol=1e-6, atol=0) and float(g1.abs().max()) > 0
    g_q = g_q.clone()
    loss_d, g_d = p.loss_and_grad(img, gt)                                  # the object's own weight
    assert torch.allclose(g_d, 0.05 * g1, rtol=1e-6, atol=0)
    X = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    buf = X.clone()
    p.loss_and_grad(img, gt, grad_out=buf, accumulate=True, weight=0.25)
    assert torch.equal(buf, X + g_q)                                        # (rounded on its own, then added)
    with pytest.raises(ValueError, match="accumulate"):
        p.loss_and_grad(img, gt, accumulate=True)
    loss_f, none = p.loss_and_grad(img, gt, grad_out=False)                 # the metric
    assert none is None and torch.equal(loss_f, loss1)
    total = torch.zeros((), device=dev)
    for t in loss1[1:]:
        total = total + t                                                   # the last tap's launch adds the terms in order
    assert torch.equal(loss1[0], total)
    with pytest.raises(ValueError, match="Lpips: gt"):
        p.loss_and_grad(img, gt[:, :-1])
    with pytest.raises(ValueError, match="Lpips: loss_out"):
        p.loss_and_grad(img, gt, loss_out=torch.zeros(2, device=dev))
    with pytest.raises(ValueError, match="one vector per tap"):
        _lpips(STACKS[stack], c["W"], c["B"], c["lin"][:4], (sh, sw), dev)


def test_same_bits_on_every_launch_and_graph_replay(gpu_device):
    import torch
    from fateavatar_amd import _lib
    dev = gpu_device
    stack, H, W, sh, sw = CASES[0]
    c = _case(*CASES[0])
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    p = _lpips(STACKS[stack], c["W"], c["B"], c["lin"], (sh, sw), dev)
    first = [t.clone() for t in p.loss_and_grad(img, gt)]
    second = [t.clone() for t in p.loss_and_grad(img, gt)]
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    s_loss, s_grad = torch.zeros(6, device=dev), torch.zeros(3, H, W, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p.loss_and_grad(img, gt, loss_out=s_loss, grad_out=s_grad)
    for _ in range(3):
        s_loss.fill_(float("nan"))
        s_grad.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_loss, first[0]) and torch.equal(s_grad, first[1])
    assert int(p._workspace[:_lib.FR_VGG_REDUCE_BYTES].count_nonzero()) == 0


def test_autograd_op_hands_out_the_same_gradient(gpu_device):
    import torch
    from fateavatar_amd.perceptual import lpips_loss
    dev = gpu_device
    stack, H, W, sh, sw = CASES[4]
    c = _case(*CASES[4])
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    p = _lpips(STACKS[stack], c["W"], c["B"], c["lin"], (sh, sw), dev)
    loss, g = (t.clone() for t in p.loss_and_grad(img, gt, weight=1.0))
    leaf = img.clone().requires_grad_(True)
    out = lpips_loss(leaf, gt, p)
    assert out.requires_grad and out.dim() == 0 and torch.equal(out.detach(), loss[0])
    out.backward()
    assert torch.equal(leaf.grad, g)
    leaf.grad = None
    (0.05 * p(leaf, gt)).backward()
    assert torch.allclose(leaf.grad, 0.05 * g, rtol=1e-6, atol=0)
    with torch.no_grad():
        assert torch.equal(lpips_loss(img, gt, p), loss[0])
    with pytest.raises(RuntimeError, match="target"):
        lpips_loss(leaf, gt.clone().requires_grad_(True), p)


def test_lin_with_mixed_signs(gpu_device):
    """The learnt weights are non-negative in the package, but nothing in the kernels needs that: signed weights, terms of
    either sign, the same bounds."""
    import torch
    stack, H, W, sh, sw = CASES[4]
    layers = STACKS[stack]
    Wt, B, _ = _weights(stack)
    lin = lpips_ref.lin_weights(layers, seed=8, signed=True)
    assert all(bool((w < 0).any()) and bool((w > 0).any()) for w in lin)
    img, gt = vgg_ref.images(H, W, seed=77)
    c = dict(W=Wt, B=B, lin=lin, img=img, gt=gt, r64=lpips_ref.forward(Wt, B, lin, layers, img, gt, (sh, sw), torch.float64),
             r32=lpips_ref.forward(Wt, B, lin, layers, img, gt, (sh, sw), torch.float32))
    _held_to_float64(gpu_device, "signed-lin", layers, c, (H, W), (sh, sw))
