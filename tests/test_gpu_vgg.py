"""-m gpu: the fused perceptual term (csrc/fr_vgg.hip, fateavatar_amd/perceptual.py) on the device against the float64
restatement of tests/vgg_ref.py, with bounds MEASURED on the float32 restatement.

The bound (tests/test_gpu_mlp.py's): a quantity's rel-L2 error against float64 may be at most FACTOR x e32, e32 being the float32
CPU restatement's own rel-L2 error against float64 for the same quantity (another summation order: a k-ordered fmaf chain against
blocked sums), and never more than CEILING.  e32 is floored at 2^-24: a result stored as float32 carries up to half an ulp of
relative error however it was computed, so no bound below FACTOR x 2^-24 can be asked of a float32 number (this matters for the
scalar losses only, where the restatement's error can come out near zero by chance).

The forward is continuous and is compared directly.  The backward is not (a ReLU mask, a pool argmax or a tap sign that float32
rounding carries across its threshold moves the gradient by far more than rounding), so it is compared twice: against the PINNED
float64 backward evaluated at the device's own saved activations, on every shape; and against float64 autograd end to end on
inputs drawn until the float64 network keeps every decision clear of its threshold.

Noise images at 24 x 24 leave two things out, which have cases of their own: decisions that land EXACTLY on their thresholds —
flat image regions (vgg_ref.patchwork) and identical images, where the first-maximum rule of the pool's backward and
sign(0) = 0 decide the gradient — and the plans of the GEMM split over the taps that sizes above 24 x 24 take under the library's
own flags (WIDE_CASES: one and three planes; tests/test_vgg_host.py asserts that the cases take them)."""
import functools

import pytest

from tests import vgg_ref

pytestmark = pytest.mark.gpu

FACTOR, CEILING, FLOOR = 4.0, 2e-4, 2.0 ** -24
MASK_Z = 1e-5            # a decision that differs from float64's lies within MASK_Z x the layer's RMS pre-activation of its threshold
CLEAR = 2e-5             # the end-to-end inputs keep every float64 decision this x RMS clear of its threshold
STACKS = {"vgg16": vgg_ref.VGG16, "small": vgg_ref.SMALL, "wide": vgg_ref.WIDE, "narrow": vgg_ref.NARROW, "odd": vgg_ref.ODD}
# (stack, H, W, size_h, size_w)
CASES = [("vgg16", 37, 53, 24, 24),       # non-integer downsampling, ragged M in every block
         ("vgg16", 13, 17, 24, 24),       # upsampling, the clamped source coordinates
         ("vgg16", 24, 24, 24, 24),       # identity
         ("vgg16", 29, 23, 16, 16),       # deepest map 2 x 2: all halo
         ("vgg16", 20, 40, 16, 32),       # non-square
         ("small", 24, 24, 24, 24)]       # descriptor generality: 3 -> 64, 64 -> 64 tap, pool, 64 -> 128 tap
END_TO_END = [CASES[0], CASES[2], CASES[3]]
# vgg_ref.patchwork's flat regions, at resizes that keep them bit-flat (tests/test_vgg_host.py holds what the inputs do to float64)
PATCHWORK = [("small", 24, 24, 24, 24),   # identity
             ("vgg16", 48, 48, 24, 24),   # exact halving: 0.5 v + 0.5 v
             ("vgg16", 32, 32, 32, 32)]   # identity
# vgg_ref.WIDE at the sizes where its GEMMs (layers 1 to 3) take each plan of the split over the taps UNDER THE DEFAULT FLAGS —
# CASES' sizes split every GEMM into nine planes.  Plans by perceptual.gemm_splits, forward / gradient, layers 1, 2, 3:
WIDE_CASES = [("wide", 31, 39, 26, 30),   # 3 3 3 / 9 3 3: three planes (VGG-16's block 4 at 224^2), ragged M = 1560 / 780
              ("wide", 32, 32, 32, 32),   # 1 1 1 / 9 3 3: the forward exactly at tiles == 256
              ("wide", 40, 24, 64, 32)]   # 1 1 1 / 9 1 1: the gradient unsplit too (at tiles == 256), SEED and MASK epilogues in-kernel
# vgg_ref.ODD: GEMMs with N = 192, 320 and 448 — three, five and seven 64-column tiles, where every other stack has 1, 2, 4 or 8
ODD_CASES = [("odd", 16, 16, 16, 16),     # M = 512 / 128: whole 64-row tiles
             ("odd", 24, 40, 24, 40)]     # non-square, M = 1920 / 480: ragged against 128 rows


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _bound(e32):
    return min(FACTOR * max(e32, FLOOR), CEILING)


@functools.lru_cache(maxsize=None)
def _weights(stack):
    return vgg_ref.he_weights(STACKS[stack], seed=11 + len(STACKS[stack]))


@functools.lru_cache(maxsize=None)
def _case(stack, H, W, sh, sw, patchwork=False):
    """Weights, images and both restatements' forwards on the CPU: computed once, shared, never modified."""
    import torch
    Wt, B = _weights(stack)
    img, gt = (vgg_ref.patchwork if patchwork else vgg_ref.images)(H, W, seed=1000 * H + W)
    r64 = vgg_ref.forward(Wt, B, STACKS[stack], img, gt, (sh, sw), torch.float64)
    r32 = vgg_ref.forward(Wt, B, STACKS[stack], img, gt, (sh, sw), torch.float32)
    return dict(W=Wt, B=B, img=img, gt=gt, r64=r64, r32=r32)


# The seed each end-to-end case starts its draws from: the first seed from 0 on at which the float64 restatement is clear, found by
# running this same float64-only search on the CPU (with all three decision kinds the margin leaves about one draw in five
# hundred at 24 x 24: 427, 351 and 7 draws from seed 0).  Recorded so that the test does not spend its seconds on draws known to
# fail; the loop below still checks the criterion and goes on to the next seed should the weights or the restatement change.
FIRST_CLEAR_SEED = {("vgg16", 37, 53, 24, 24): 426, ("vgg16", 24, 24, 24, 24): 350, ("vgg16", 29, 23, 16, 16): 6}


@functools.lru_cache(maxsize=None)
def _clear_case(stack, H, W, sh, sw):
    """Inputs re-drawn (next seed, at most 400) until the FLOAT64 network alone keeps every decision — a ReLU pre-activation, a
    tap difference where either side is live, a live pool window's top two — CLEAR x its layer's RMS away from its threshold,
    with float64 and float32 autograd's gradients."""
    import torch
    Wt, B = _weights(stack)
    layers = STACKS[stack]
    for attempt in range(400):
        img, gt = vgg_ref.images(H, W, seed=FIRST_CLEAR_SEED[(stack, H, W, sh, sw)] + attempt)
        r64 = vgg_ref.forward(Wt, B, layers, img, gt, (sh, sw), torch.float64)
        if vgg_ref.decisions_clear(r64, layers, CLEAR):
            break
    else:
        raise AssertionError("no seed keeps the float64 decisions clear of their thresholds")
    loss64, g64 = vgg_ref.autograd_gradient(Wt, B, layers, img, gt, (sh, sw), torch.float64)
    loss32, g32 = vgg_ref.autograd_gradient(Wt, B, layers, img, gt, (sh, sw), torch.float32)
    return dict(img=img, gt=gt, loss64=loss64, g64=g64, loss32=loss32, g32=g32, attempts=attempt + 1)


def _perceptual(stack, size, dev, **kw):
    from fateavatar_amd.perceptual import Perceptual, VggFeatures
    Wt, B = _weights(stack)
    return Perceptual(VggFeatures(STACKS[stack], Wt, B, size=size, device=dev, **kw))


def _ids(c):
    return f"{c[0]}-{c[1]}x{c[2]}-to-{c[3]}x{c[4]}"


def _held_to_float64(dev, case, c, tile=None):
    """The held set of a case: the forward quantities against float64, the decisions inside the band, the gradient against the
    pinned float64 backward at the device's own saved activations — each at the module's bound, each with its ratio line.
    `c`: weights, images and both restatements' forwards (of `_case`).  Returns (losses, gradient, saved activations, object)."""
    import torch
    stack, H, W, sh, sw = case
    layers = STACKS[stack]
    r64, r32 = c["r64"], c["r32"]
    p = _perceptual(stack, (sh, sw), dev)
    if tile is not None:
        p.tile = tile
    T = sum(1 for y in layers if y[3])
    loss = torch.full((1 + T,), float("nan"), device=dev)
    grad = torch.full((3, H, W), float("nan"), device=dev)      # every element is to be OVERWRITTEN
    p.loss_and_grad(c["img"].to(dev), c["gt"].to(dev), loss_out=loss, grad_out=grad, weight=1.0)
    torch.cuda.synchronize()
    loss, grad = loss.cpu(), grad.cpu()
    saved = [vgg_ref.nchw(a) for a in p.saved_activations()]
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    assert len(saved) == len(layers) and all(s.shape == a.shape for s, a in zip(saved, r64["a"]))

    def held(name, got, ref64, ref32):
        e32, err = _rel(ref32, ref64), _rel(got, ref64)
        print(f"{_ids(case)} {name}: kernel {err:.3e}  float32 restatement {e32:.3e}  ratio {err / max(e32, FLOOR):.2f}")
        assert float(ref64.abs().max()) > 0
        assert err <= _bound(e32), (name, err, e32)

    # ---- the forward, directly: the network's input, every saved activation, the terms, their sum
    held("input", vgg_ref.nchw(p.saved_input()), r64["x"], r32["x"])
    for l in range(len(layers)):
        held(f"activation {l}", saved[l], r64["a"][l], r32["a"][l])
    held("terms", loss[1:], torch.stack(r64["terms"]), torch.stack(r32["terms"]))
    held("loss", loss[0:1], r64["loss"].reshape(1), r32["loss"].reshape(1))

    # ---- the decisions: a ReLU mask or a tap sign differs from float64's only at its threshold, and no more often than float64
    # has units inside that band
    flips = band = 0
    for l, (ci, co, pool, tap) in enumerate(layers):
        z = r64["z"][l]
        tol = MASK_Z * float(z.pow(2).mean().sqrt())
        diff = (saved[l] > 0) != (z > 0)
        flips += int(diff.sum())
        band += int((z.abs() < tol).sum())
        if diff.any():
            assert float(z[diff].abs().max()) < tol, ("mask", l, float(z[diff].abs().max()), tol)
        if tap:
            d64 = r64["a"][l][0] - r64["a"][l][1]
            diff = torch.sign(saved[l][0] - saved[l][1]) != torch.sign(d64)
            flips += int(diff.sum())
            band += int((d64.abs() < tol).sum())
            if diff.any():
                assert float(d64[diff].abs().max()) < tol, ("tap sign", l, float(d64[diff].abs().max()), tol)
    print(f"{_ids(case)} decisions that differ from float64's: {flips} (float64 units inside the band: {band})")
    assert flips <= band

    # ---- the backward at the device's own decisions
    pin64 = vgg_ref.pinned_backward(c["W"], layers, saved, (H, W), (sh, sw), torch.float64)
    pin32 = vgg_ref.pinned_backward(c["W"], layers, saved, (H, W), (sh, sw), torch.float32)
    held("d_image (pinned)", grad, pin64, pin32)
    return loss, grad, saved, p


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_and_pinned_backward_against_float64(gpu_device, case):
    _held_to_float64(gpu_device, case, _case(*case))


def _background_interior(layers, H, W, sh, sw):
    """(rows, columns) of the shared-background quadrant (top-left, both images 1.0) that NO unit with a view out of the quadrant
    reaches: a unit whose receptive field lies inside the quadrant computes the same number for both images (the same chain on
    the same values), so its tap difference is exactly 0 and it seeds no gradient; a source pixel gets a gradient only from
    units whose field holds it, and one more than vgg_ref.receptive_margin(layers) resized pixels away from the quadrant's
    inner edges lies in no field that crosses them.  (The image's own border is no edge: the padding is the same for both.)"""
    fy, fx = H // sh, W // sw
    assert (fy * sh, fx * sw) == (H, W) and fy in (1, 2) and fx in (1, 2)       # source pixel P blends into resized pixel P // f only
    margin = vgg_ref.receptive_margin(layers)
    return fy * max(sh // 2 - margin, 0), fx * max(sw // 2 - margin, 0)


@pytest.mark.parametrize("case", PATCHWORK, ids=_ids)
def test_flat_regions_against_float64(gpu_device, case):
    """The held set on images with flat regions, where thousands of live pool windows are exact ties and thousands of live tap
    differences exactly 0 (tests/test_vgg_host.py shows that either rule's opposite moves this gradient by 0.17 to 0.80 rel-L2):
    k_vgg_unpool's first-maximum rule and sign_of(0) == 0 decide the gradient here.  The device keeps the ties — every output
    element of a layer is the same chain of operations, so equal inputs give equal bits — and the interior of the shared
    background takes a gradient of exactly 0.  (The interior is empty for VGG-16 at these sizes: its receptive field, 91 resized
    pixels, is wider than the quadrant; test_shared_background_takes_no_gradient_at_production_size has the room.)"""
    stack, H, W, sh, sw = case
    layers = STACKS[stack]
    c = _case(*case, patchwork=True)
    loss, grad, saved, p = _held_to_float64(gpu_device, case, c)
    ties64, zeros64 = vgg_ref.live_ties(c["r64"]["a"], layers)
    ties, zeros = vgg_ref.live_ties(saved, layers)
    print(f"{_ids(case)} patchwork: live tied windows {ties} on the device (float64: {ties64}), live zero tap differences {zeros} "
          f"(float64: {zeros64})")
    assert ties64 >= 1000 and zeros64 >= 1000
    assert 2 * ties >= ties64 and 2 * zeros >= zeros64
    rows, cols = _background_interior(layers, H, W, sh, sw)
    print(f"{_ids(case)} patchwork: shared-background interior {rows} x {cols} pixels")
    assert bool((grad[:, :rows, :cols] == 0).all())
    assert float(grad[:, H // 2:, :].abs().max()) > 0


def test_shared_background_takes_no_gradient_at_production_size(gpu_device):
    """VGG-16 at 224^2 (identity), where the background quadrant (112 pixels) is wider than the stack's receptive field: its
    interior's gradient is exactly 0, through the unsplit and the three-plane GEMMs of that size.  No reference is computed."""
    import torch
    dev = gpu_device
    H = W = 224
    rows, cols = _background_interior(vgg_ref.VGG16, H, W, H, W)
    assert rows == cols == 112 - 91
    img, gt = vgg_ref.patchwork(H, W, seed=5)
    p = _perceptual("vgg16", (H, W), dev)
    grad = torch.full((3, H, W), float("nan"), device=dev)
    loss, _ = p.loss_and_grad(img.to(dev), gt.to(dev), grad_out=grad, weight=1.0)
    torch.cuda.synchronize()
    grad = grad.cpu()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all()) and float(loss[0]) > 0
    assert bool((grad[:, :rows, :cols] == 0).all())
    assert float(grad[:, H // 2:, :].abs().max()) > 0 and float(grad[:, :, W // 2:].abs().max()) > 0
    # inside the quadrant the two images' activations are the same bits, layer by layer
    for (h, w), a in zip(p.features.extents(), p.saved_activations()):
        s = H // h
        k = (112 - 91) // s
        if k:
            assert torch.equal(a[0, :k, :k], a[1, :k, :k])


@pytest.mark.parametrize("stack,hw,size,patchwork", [("small", (24, 24), (24, 24), False), ("small", (24, 24), (24, 24), True),
                                                     ("vgg16", (37, 53), (24, 24), False), ("vgg16", (48, 48), (24, 24), True)],
                         ids=["small-noise", "small-patchwork", "vgg16-noise", "vgg16-patchwork"])
def test_identical_images_give_exact_zeros(gpu_device, stack, hw, size, patchwork):
    """loss_and_grad(x, x): both branches run the same chain on the same values, so every term is exactly 0.0, every tap sign
    is sign_of(0) = 0 and the gradient is exactly 0.0 everywhere; accumulating it leaves a buffer's bits alone."""
    import torch
    dev = gpu_device
    x = (vgg_ref.patchwork if patchwork else vgg_ref.images)(*hw, seed=9)[0].to(dev)
    p = _perceptual(stack, size, dev)
    loss = torch.full((1 + p.n_terms,), float("nan"), device=dev)
    grad = torch.full_like(x, float("nan"))
    p.loss_and_grad(x, x.clone(), loss_out=loss, grad_out=grad, weight=1.0)
    torch.cuda.synchronize()
    assert bool((loss == 0).all()) and bool((grad == 0).all())
    assert all(float(a.abs().max()) > 0 for a in p.saved_activations())                 # (the network is not dead)
    X = torch.randn(x.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    buf = X.clone()
    p.loss_and_grad(x, x.clone(), grad_out=buf, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(buf, X)


@pytest.mark.parametrize("case", WIDE_CASES, ids=_ids)
def test_every_split_plan_against_float64(gpu_device, case):
    """The held set under the library's own flags at sizes whose GEMMs take the one-plane and three-plane plans (WIDE_CASES;
    tests/test_vgg_host.py asserts which), and the larger tile changes no bit at any of them — at 26 x 30 M is ragged
    against 128 rows as well."""
    import torch
    from fateavatar_amd import _lib
    dev = gpu_device
    c = _case(*case)
    loss, grad, saved, p = _held_to_float64(dev, case, c, tile=_lib.FR_VGG_TILE_AUTO)
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    acts = [a.clone() for a in p.saved_activations()]
    for tile in (_lib.FR_VGG_TILE_64, _lib.FR_VGG_TILE_128):
        p.tile = tile
        loss_t, g_t = p.loss_and_grad(img, gt, weight=1.0)
        torch.cuda.synchronize()
        assert torch.equal(loss_t.cpu(), loss) and torch.equal(g_t.cpu(), grad), tile
        assert all(torch.equal(a, b) for a, b in zip(p.saved_activations(), acts)), tile


@pytest.mark.parametrize("case", ODD_CASES, ids=_ids)
def test_odd_widths_against_float64(gpu_device, case):
    """The held set on vgg_ref.ODD, whose widths are odd multiples of 64: the forward GEMMs' N is 192, 320 and 448, the gradient
    GEMMs' 320, 192 and 64, and the last column tile of each is the third, fifth or seventh — no power of two anywhere."""
    _held_to_float64(gpu_device, case, _case(*case))


@pytest.mark.parametrize("case", END_TO_END, ids=_ids)
def test_gradient_end_to_end_against_float64_autograd(gpu_device, case):
    import torch
    dev = gpu_device
    stack, H, W, sh, sw = case
    c = _clear_case(*case)
    p = _perceptual(stack, (sh, sw), dev)
    loss, grad = p.loss_and_grad(c["img"].to(dev), c["gt"].to(dev), weight=1.0)
    torch.cuda.synchronize()
    e32, err = _rel(c["g32"], c["g64"]), _rel(grad.cpu(), c["g64"])
    print(f"{_ids(case)} end to end after {c['attempts']} draws: kernel {err:.3e}  float32 autograd {e32:.3e}  ratio {err / max(e32, FLOOR):.2f}")
    assert float(c["g64"].abs().max()) > 0
    assert err <= _bound(e32), (err, e32)
    l32, lerr = _rel(c["loss32"].reshape(1), c["loss64"].reshape(1)), _rel(loss[0:1].cpu(), c["loss64"].reshape(1))
    print(f"{_ids(case)} loss: kernel {lerr:.3e}  float32 {l32:.3e}")
    assert lerr <= _bound(l32), (lerr, l32)


def test_identity_size_copies_the_image_exactly(gpu_device):
    import torch
    dev = gpu_device
    p = _perceptual("small", (24, 24), dev, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    img, gt = vgg_ref.images(24, 24, seed=3)
    p.loss_and_grad(img.to(dev), gt.to(dev), grad_out=False)
    x = vgg_ref.nchw(p.saved_input())
    assert torch.equal(x[0], img) and torch.equal(x[1], gt)


def test_accumulate_weight_forward_only_and_the_tile_choice(gpu_device):
    import torch
    from fateavatar_amd import _lib
    dev = gpu_device
    stack, H, W, sh, sw = CASES[0]
    c = _case(*CASES[0])
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    p = _perceptual(stack, (sh, sw), dev)
    assert p.weight == 0.1
    loss1, g1 = p.loss_and_grad(img, gt, weight=1.0)
    loss1, g1 = loss1.clone(), g1.clone()
    # weight scales d_image alone
    loss_q, g_q = p.loss_and_grad(img, gt, weight=0.25)
    assert torch.equal(loss_q, loss1)
    assert torch.allclose(g_q, 0.25 * g1, rtol=1e-6, atol=0) and float(g1.abs().max()) > 0
    loss_d, g_d = p.loss_and_grad(img, gt)                                  # the object's own weight
    assert torch.allclose(g_d, 0.1 * g1, rtol=1e-6, atol=0)
    # accumulate adds weight x g to what the buffer holds
    X = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    buf = X.clone()
    p.loss_and_grad(img, gt, grad_out=buf, accumulate=True, weight=0.25)
    assert torch.allclose(buf, X + g_q, rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="accumulate"):
        p.loss_and_grad(img, gt, accumulate=True)
    # forward only: the same losses, no gradient
    loss_f, none = p.loss_and_grad(img, gt, grad_out=False)
    assert none is None and torch.equal(loss_f, loss1)
    # the GEMM tile changes no bit: every output element is the same k-ordered chain
    for tile in (_lib.FR_VGG_TILE_64, _lib.FR_VGG_TILE_128):
        p.tile = tile
        loss_t, g_t = p.loss_and_grad(img, gt, weight=1.0)
        assert torch.equal(loss_t, loss1) and torch.equal(g_t, g1), tile
    # no GEMM split over the taps (at these sizes the library splits every one): another summation order, the same bounds
    r64, r32 = c["r64"], c["r32"]
    for tile in (_lib.FR_VGG_NO_SPLIT, _lib.FR_VGG_TILE_128 | _lib.FR_VGG_NO_SPLIT):
        p.tile = tile
        loss_u, g_u = p.loss_and_grad(img, gt, weight=1.0)
        for l, a in enumerate(p.saved_activations()):
            e32, err = _rel(r32["a"][l], r64["a"][l]), _rel(vgg_ref.nchw(a), r64["a"][l])
            print(f"unsplit (tile flags {tile}) activation {l}: kernel {err:.3e}  float32 restatement {e32:.3e}")
            assert err <= _bound(e32), (tile, l, err, e32)
        assert _rel(g_u, g1) <= 1e-5 and _rel(loss_u, loss1) <= 1e-6
        assert not torch.equal(g_u, g1)                                     # (it IS another path)
    p.tile = _lib.FR_VGG_TILE_AUTO
    # refusals of the wrapper
    with pytest.raises(ValueError, match="gt"):
        p.loss_and_grad(img, gt[:, :-1])
    with pytest.raises(ValueError, match="loss_out"):
        p.loss_and_grad(img, gt, loss_out=torch.zeros(2, device=dev))


def test_same_bits_on_every_launch_and_graph_replay(gpu_device):
    import torch
    dev = gpu_device
    stack, H, W, sh, sw = CASES[0]
    c = _case(*CASES[0])
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    p = _perceptual(stack, (sh, sw), dev)
    first = [t.clone() for t in p.loss_and_grad(img, gt)]
    second = [t.clone() for t in p.loss_and_grad(img, gt)]
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    s_loss, s_grad = torch.zeros(5, device=dev), torch.zeros(3, H, W, device=dev)
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
    # the head of the workspace (counters and partials) is left zeroed
    from fateavatar_amd import _lib
    assert int(p._workspace[:_lib.FR_VGG_REDUCE_BYTES].count_nonzero()) == 0


def test_autograd_op_hands_out_the_same_gradient(gpu_device):
    import torch
    from fateavatar_amd.perceptual import vgg_perceptual_loss
    dev = gpu_device
    stack, H, W, sh, sw = CASES[5]
    c = _case(*CASES[5])
    img, gt = c["img"].to(dev), c["gt"].to(dev)
    p = _perceptual(stack, (sh, sw), dev)
    loss, g = p.loss_and_grad(img, gt, weight=1.0)
    loss, g = loss.clone(), g.clone()
    leaf = img.clone().requires_grad_(True)
    out = vgg_perceptual_loss(leaf, gt, p)
    assert out.requires_grad and out.dim() == 0 and torch.equal(out.detach(), loss[0])
    out.backward()
    assert torch.equal(leaf.grad, g)
    leaf.grad = None
    (0.1 * p(leaf, gt)).backward()
    assert torch.allclose(leaf.grad, 0.1 * g, rtol=1e-6, atol=0)
    with torch.no_grad():
        assert torch.equal(vgg_perceptual_loss(img, gt, p), loss[0])
    with pytest.raises(RuntimeError, match="target"):
        vgg_perceptual_loss(leaf, gt.clone().requires_grad_(True), p)
