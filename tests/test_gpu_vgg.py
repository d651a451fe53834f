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
inputs drawn until the float64 network keeps every decision clear of its threshold."""
import functools

import pytest

from tests import vgg_ref

pytestmark = pytest.mark.gpu

FACTOR, CEILING, FLOOR = 4.0, 2e-4, 2.0 ** -24
MASK_Z = 1e-5            # a decision that differs from float64's lies within MASK_Z x the layer's RMS pre-activation of its threshold
CLEAR = 2e-5             # the end-to-end inputs keep every float64 decision this x RMS clear of its threshold
STACKS = {"vgg16": vgg_ref.VGG16, "small": vgg_ref.SMALL}
# (stack, H, W, size_h, size_w)
CASES = [("vgg16", 37, 53, 24, 24),       # non-integer downsampling, ragged M in every block
         ("vgg16", 13, 17, 24, 24),       # upsampling, the clamped source coordinates
         ("vgg16", 24, 24, 24, 24),       # identity
         ("vgg16", 29, 23, 16, 16),       # deepest map 2 x 2: all halo
         ("vgg16", 20, 40, 16, 32),       # non-square
         ("small", 24, 24, 24, 24)]       # descriptor generality: 3 -> 64, 64 -> 64 tap, pool, 64 -> 128 tap
END_TO_END = [CASES[0], CASES[2], CASES[3]]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _bound(e32):
    return min(FACTOR * max(e32, FLOOR), CEILING)


@functools.lru_cache(maxsize=None)
def _weights(stack):
    return vgg_ref.he_weights(STACKS[stack], seed=11 + len(STACKS[stack]))


@functools.lru_cache(maxsize=None)
def _case(stack, H, W, sh, sw):
    """Weights, images and both restatements' forwards on the CPU: computed once, shared, never modified."""
    import torch
    Wt, B = _weights(stack)
    img, gt = vgg_ref.images(H, W, seed=1000 * H + W)
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


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_and_pinned_backward_against_float64(gpu_device, case):
    import torch
    dev = gpu_device
    stack, H, W, sh, sw = case
    layers = STACKS[stack]
    c = _case(*case)
    r64, r32 = c["r64"], c["r32"]
    p = _perceptual(stack, (sh, sw), dev)
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
