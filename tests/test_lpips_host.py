"""No GPU: what the LPIPS term's tests stand on — tests/lpips_ref.py's closed-form seed and dead-pixel rule against float64
autograd, the input statistics, the 13-layer table's limits, the workspace formula, the state-dict key table, the exported
symbols, and what the GPU tests' inputs do to the float64 network (live everywhere / dead where constructed)."""
import ctypes as C

import pytest
import torch

from tests import lpips_ref, vgg_ref

LPIPS13 = lpips_ref.LPIPS13


def _features(layers=LPIPS13, size=(32, 32), seed=5):
    from fateavatar_amd.perceptual import VggFeatures
    W, B = vgg_ref.he_weights(layers, seed)
    return VggFeatures(layers, W, B, size=size)


def _random_tap(C_, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.relu(torch.randn(C_, h, w, generator=g, dtype=torch.float64))
    b = torch.relu(torch.randn(C_, h, w, generator=g, dtype=torch.float64))
    lin = torch.randn(C_, generator=g, dtype=torch.float64) / C_            # (mixed signs: the closed form does not need w >= 0)
    return a, b, lin


def test_closed_form_seed_is_float64_autograd_on_live_pixels():
    a, b, lin = _random_tap(64, 5, 7, seed=1)
    leaf = a.clone().requires_grad_(True)
    term = lpips_ref.tap_term_stock(leaf, b, lin) / (5 * 7)
    (g,) = torch.autograd.grad(term, leaf)
    seed = lpips_ref.tap_seed(a, b, lin)
    assert float(g.abs().max()) > 1e-4
    assert float((seed - g).abs().max()) < 1e-15
    assert abs(float(lpips_ref.tap_term(a, b, lin)) - float(term.detach())) < 1e-15
    # and autograd through the restatement's own term
    leaf2 = a.clone().requires_grad_(True)
    (g2,) = torch.autograd.grad(lpips_ref.tap_term(leaf2, b, lin), leaf2)
    assert float((seed - g2).abs().max()) < 1e-15


def test_dead_pixel_rule_is_autograd_with_those_pixels_masked_out():
    a, b, lin = _random_tap(64, 6, 6, seed=2)
    a[:, :2, :3] = 0.0                       # six dead rendered pixels
    b[:, 5, 5] = 0.0                         # one dead target pixel
    dead_a = a.pow(2).sum(0) == 0
    dead_b = b.pow(2).sum(0) == 0
    assert int(dead_a.sum()) == 6 and int(dead_b.sum()) == 1
    # stock autograd is NaN here: the deviation the header states
    leaf = a.clone().requires_grad_(True)
    (g_stock,) = torch.autograd.grad(lpips_ref.tap_term_stock(leaf, b, lin), leaf)
    assert bool(torch.isnan(g_stock[:, dead_a]).all())
    # the rule: live pixels through the stock formula, a dead rendered pixel contributes sum_c w_c b^_c^2 and no gradient
    both = ~dead_a & ~dead_b
    leaf = a.clone().requires_grad_(True)
    bh = b / (b.pow(2).sum(0, keepdim=True).sqrt() + lpips_ref.EPS)
    ah_live = leaf[:, dead_b & ~dead_a] / (leaf[:, dead_b & ~dead_a].pow(2).sum(0, keepdim=True).sqrt() + lpips_ref.EPS)
    total = (lpips_ref.tap_term_stock(leaf[:, both], b[:, both], lin)
             + (lin.view(-1, 1) * bh[:, dead_a].pow(2)).sum()            # dead rendered: 0 - b^
             + (lin.view(-1, 1) * ah_live.pow(2)).sum()) / 36                        # dead target: a^ - 0
    (g,) = torch.autograd.grad(total, leaf)
    assert bool((g[:, dead_a] == 0).all())
    seed = lpips_ref.tap_seed(a, b, lin)
    assert bool((seed[:, dead_a] == 0).all()) and bool(torch.isfinite(seed).all())
    assert float((seed - g).abs().max()) < 1e-15
    assert abs(float(lpips_ref.tap_term(a, b, lin)) - float(total.detach())) < 1e-15
    leaf = a.clone().requires_grad_(True)
    (g2,) = torch.autograd.grad(lpips_ref.tap_term(leaf, b, lin), leaf)
    assert bool(torch.isfinite(g2).all()) and float((seed - g2).abs().max()) < 1e-15


def test_input_statistics_for_both_normalize_modes():
    from fateavatar_amd import perceptual as P
    assert P.LPIPS_SHIFT == lpips_ref.SHIFT and P.LPIPS_SCALE == lpips_ref.SCALE
    mean, std = P.lpips_mean_std(True)
    # (2 x - 1 - shift) / scale == (x - mean) / std with the ImageNet statistics, to float32's last bit
    assert torch.equal(torch.tensor(mean, dtype=torch.float32), torch.tensor(P.IMAGENET_MEAN, dtype=torch.float32))
    assert torch.equal(torch.tensor(std, dtype=torch.float32), torch.tensor(P.IMAGENET_STD, dtype=torch.float32))
    x = torch.rand(3, 9, 11, dtype=torch.float64)
    sh, sc = (torch.tensor(v, dtype=torch.float64).view(3, 1, 1) for v in (P.LPIPS_SHIFT, P.LPIPS_SCALE))
    m, s = (torch.tensor(v, dtype=torch.float64).view(3, 1, 1) for v in (mean, std))
    assert float(((2 * x - 1 - sh) / sc - (x - m) / s).abs().max()) < 1e-14
    assert P.lpips_mean_std(False) == (P.LPIPS_SHIFT, P.LPIPS_SCALE)
    f = P.Lpips.trunk((32, 48))
    assert f.mean == mean and f.std == std and f.size == (32, 48) and len(f.layers) == 13 and len(f.taps) == 5
    assert P.Lpips.trunk((16, 16), normalize=False).mean == P.LPIPS_SHIFT


def test_the_thirteen_layer_table_and_its_limits():
    from fateavatar_amd import perceptual as P
    assert tuple(tuple(y) for y in P.LPIPS_VGG16_LAYERS) == LPIPS13
    assert P.torchvision_indices(P.LPIPS_VGG16_LAYERS) == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [i for i, y in enumerate(P.LPIPS_VGG16_LAYERS) if y.tap_after] == [1, 3, 6, 9, 12]
    for size in ((16, 16), (32, 48), (512, 512)):
        P.check_layers(P.LPIPS_VGG16_LAYERS, size)
    for size in ((24, 24), (32, 40), (8, 16), (30, 32)):         # four pools: both extents divisible by 16
        with pytest.raises(ValueError, match="divisible"):
            P.check_layers(P.LPIPS_VGG16_LAYERS, size)
    # a tap wider than 512 is the LPIPS kernels' limit alone
    from fateavatar_amd import _lib
    wide = ((3, 64, False, False), (64, 576, False, True))
    f = _features(wide, (8, 8))
    L = _lib.lib()
    assert L.fr_vgg_workspace_bytes(C.byref(f.describe(8, 8))) > 0
    assert L.fr_lpips_workspace_bytes(C.byref(f.describe(8, 8))) == 0
    assert L.fr_lpips_workspace_bytes(None) == 0


def test_workspace_bytes_is_the_documented_formula():
    from fateavatar_amd import _lib
    from fateavatar_amd.perceptual import lpips_workspace_bytes, workspace_bytes
    L = _lib.lib()
    r256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for layers, size in ((LPIPS13, (512, 512)), (LPIPS13, (32, 32)), (LPIPS13, (48, 32)), (LPIPS13, (16, 16)), (vgg_ref.SMALL, (24, 24)),
                         (vgg_ref.WIDE, (26, 30)), (((3, 64, False, True),), (5, 7))):
        f = _features(layers, size)
        got = L.fr_lpips_workspace_bytes(C.byref(f.describe(37, 53)))
        assert got == lpips_workspace_bytes(f) and got % 256 == 0
        # the VGG layout in front, unchanged: saved_input() and saved_activations() keep their offsets
        assert got > workspace_bytes(f) == L.fr_vgg_workspace_bytes(C.byref(f.describe(37, 53)))
    # the 13-layer trunk at 512^2 by hand: three floats a pixel per tap, one seed buffer of the widest tap but the last
    f = _features(LPIPS13, (512, 512))
    extra = sum(r256(3 * 4 * (512 >> k) ** 2) for k in range(5)) + 4 * 64 * 512 * 512
    assert lpips_workspace_bytes(f) - workspace_bytes(f) == extra
    assert lpips_workspace_bytes(f) == 834668800            # the header's figure
    # a single layer has no tap but the last: no seed buffer
    f = _features(((3, 64, False, True),), (5, 7))
    assert lpips_workspace_bytes(f) - workspace_bytes(f) == r256(3 * 4 * 35)


def test_entry_point_refuses_what_fr_vgg_loss_grad_refuses_and_a_null_lin():
    from fateavatar_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 1024)()
    addr = (C.addressof(buf) + 255) // 256 * 256

    def describe(layers, **over):
        d = _lib.fr_vgg()
        d.n_layers, d.H, d.W, d.size_h, d.size_w, d.tile = len(layers), 8, 8, 24, 24, 0
        for c in range(3):
            d.mean[c], d.std[c] = 0.5, 0.25
        for i, y in enumerate(layers):
            d.layers[i] = _lib.fr_vgg_layer(*[int(v) for v in y])
        d.weights_fwd = d.weights_bwd = d.image = d.target = addr
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def refused(d, lin=addr, loss=addr, grad=addr, ws=addr, what=""):
        rc = L.fr_lpips_loss_grad(C.byref(d) if d is not None else None, lin, 0.1, 0, loss, grad, ws, None)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, what
        assert "fr_lpips_loss_grad" in _lib.last_error(), what

    good = [(3, 64, 0, 0), (64, 64, 0, 1), (64, 128, 1, 1)]
    assert L.fr_lpips_workspace_bytes(C.byref(describe(good))) > 0
    refused(None, what="null descriptor")
    refused(describe([(3, 64, 0, 1), (64, 64, 0, 0)]), what="last layer no tap")
    refused(describe([(3, 96, 0, 1)]), what="c_out")
    refused(describe([(3, 64, 0, 0), (64, 576, 0, 1)]), what="tap wider than 512")
    refused(describe(good, size_w=25), what="size")
    refused(describe(good, tile=7), what="tile")
    for field in ("weights_fwd", "weights_bwd", "image", "target"):
        refused(describe(good, **{field: None}), what="null " + field)
    refused(describe(good), lin=None, what="null lin")
    refused(describe(good), lin=addr + 4, what="misaligned lin")
    refused(describe(good), loss=None, what="null loss_out")
    refused(describe(good), ws=None, what="null workspace")
    refused(describe(good), ws=addr + 128, what="misaligned workspace")
    refused(describe(good), grad=addr + 2, what="misaligned d_image")


def test_exports_and_header():
    import os
    from fateavatar_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fr_rasterizer.h")).read()
    for sym in ("fr_lpips_workspace_bytes", "fr_lpips_loss_grad"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym) and sym + "(" in header
    assert "DEAD PIXELS" in header


def test_state_dicts_round_trip_through_the_key_table():
    from fateavatar_amd import perceptual as P
    assert P.LPIPS_LIN_KEYS == tuple(f"lin{k}.model.1.weight" for k in range(5))
    W, B = vgg_ref.he_weights(LPIPS13, seed=3)
    lin = lpips_ref.lin_weights(LPIPS13, seed=4)
    trunk_sd = P.VggFeatures(LPIPS13, W, B, size=(16, 16)).state_dict()
    assert sorted(trunk_sd) == sorted(f"features.{i}.{n}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28) for n in ("weight", "bias"))
    lin_sd = {k: w.view(1, -1, 1, 1) for k, w in zip(P.LPIPS_LIN_KEYS, lin)}

    # (an Lpips needs a device: the host half of from_state_dicts is the trunk and the key walk)
    class _Host(P.Lpips):
        def __init__(self, features, lin, weight):
            self.features, self.lin, self.weight = features, [w.clone() for w in lin], weight

    got = _Host.from_state_dicts(trunk_sd, lin_sd, size=(16, 16), weight=0.01)
    assert got.weight == 0.01 and got.features.mean == P.IMAGENET_MEAN and got.features.size == (16, 16)
    assert all(torch.equal(a, b) for a, b in zip(got.features.weights, W)) and all(torch.equal(a, b) for a, b in zip(got.features.biases, B))
    assert all(torch.equal(a, b) for a, b in zip(got.lin, lin))
    back = got.lin_state_dict()
    assert sorted(back) == sorted(lin_sd) and all(torch.equal(back[k], lin_sd[k]) for k in lin_sd)
    with pytest.raises(KeyError, match="lin3"):
        _Host.from_state_dicts(trunk_sd, {k: v for k, v in lin_sd.items() if not k.startswith("lin3")}, size=(16, 16))
    with pytest.raises(ValueError, match="lin0"):
        _Host.from_state_dicts(trunk_sd, dict(lin_sd, **{"lin0.model.1.weight": lin_sd["lin1.model.1.weight"]}), size=(16, 16))
    with pytest.raises(KeyError, match="features.28"):
        _Host.from_state_dicts({k: v for k, v in trunk_sd.items() if "28" not in k}, lin_sd, size=(16, 16))


def test_python_refusals_come_before_the_device():
    from fateavatar_amd import perceptual as P
    with pytest.raises(TypeError, match="Lpips"):
        P.Lpips("vgg")
    with pytest.raises(RuntimeError, match="Lpips needs device tensors"):
        P.Lpips(_features(vgg_ref.SMALL, (24, 24)))
    with pytest.raises(ValueError, match="more than 512"):
        P.Lpips(_features(((3, 64, False, False), (64, 576, False, True)), (8, 8)))
    with pytest.raises(TypeError, match="Lpips"):
        P.lpips_loss(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8), None)


def test_restatement_pinned_backward_at_its_own_decisions_is_autograd():
    W, B = vgg_ref.he_weights(LPIPS13, seed=24)
    lin = lpips_ref.lin_weights(LPIPS13, seed=7)
    img, gt = vgg_ref.images(37, 53, seed=3)
    r = lpips_ref.forward(W, B, lin, LPIPS13, img, gt, (32, 32))
    loss, g = lpips_ref.autograd_gradient(W, B, lin, LPIPS13, img, gt, (32, 32))
    pin = lpips_ref.pinned_backward(W, lin, LPIPS13, r["a"], (37, 53), (32, 32))
    assert float(g.abs().max()) > 0 and float((pin - g).norm() / g.norm()) < 1e-13


def test_gpu_cases_keep_every_tap_pixel_live_in_float64():
    """tests/test_gpu_lpips.py's noise inputs: no tap pixel of either image is dead or near it (smallest norm >= 1.2), so the
    kernel's dead-pixel branch is not what those cases measure; the dead-pixel case has its own test."""
    from tests import test_gpu_lpips as T
    smallest = []
    for case in T.CASES:
        c = T._case(*case)
        layers = T.STACKS[case[0]]
        smallest.append(min(float(c["r64"]["a"][l].pow(2).sum(1).sqrt().min()) for l, y in enumerate(layers) if y[3]))
    print("smallest tap norms:", smallest)
    assert min(smallest) >= 1.2


def test_dead_pixel_construct_yields_dead_pixels_in_float64():
    W, B, lin, img, gt = lpips_ref.dead_pixel_case()
    r = lpips_ref.forward(W, B, lin, vgg_ref.SMALL, img, gt, (24, 24))
    assert lpips_ref.dead_pixels(r["a"], vgg_ref.SMALL) == [(123, 0), (16, 0)]
    loss, g = lpips_ref.autograd_gradient(W, B, lin, vgg_ref.SMALL, img, gt, (24, 24))
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and float(loss) > 0
    pin = lpips_ref.pinned_backward(W, lin, vgg_ref.SMALL, r["a"], (24, 24), (24, 24))
    assert float((pin - g).norm() / g.norm()) < 1e-13


def test_dead_target_construct_yields_all_three_classes_in_float64():
    W, B, lin, img, gt = lpips_ref.dead_target_case()
    r = lpips_ref.forward(W, B, lin, vgg_ref.SMALL, img, gt, (24, 24))
    assert lpips_ref.dead_pixels(r["a"], vgg_ref.SMALL) == [(123, 169), (16, 22)]
    # (both dead, rendered only, target only)
    assert [tuple(int(m.sum()) for m in masks) for masks in lpips_ref.dead_classes(r["a"], vgg_ref.SMALL)] == [(31, 92, 138), (1, 15, 21)]
    assert abs(float(r["loss"]) - 0.0138) < 5e-5
    loss, g = lpips_ref.autograd_gradient(W, B, lin, vgg_ref.SMALL, img, gt, (24, 24))
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and float(loss) == float(r["loss"])
    pin = lpips_ref.pinned_backward(W, lin, vgg_ref.SMALL, r["a"], (24, 24), (24, 24))
    assert float((pin - g).norm() / g.norm()) < 1e-13


def test_dead_target_rule_is_stock_autograd():
    """The target half of the dead-pixel rule is the package's own behaviour: the target takes no gradient, b / (0 + eps) is a
    finite 0, so STOCK autograd through the formula as the package writes it is finite at a dead target under a live rendered
    pixel — and equals the restatement's closed-form seed there, at both taps of the dead-target case."""
    W, B, lin, img, gt = lpips_ref.dead_target_case()
    r = lpips_ref.forward(W, B, lin, vgg_ref.SMALL, img, gt, (24, 24))
    taps = [l for l, y in enumerate(vgg_ref.SMALL) if y[3]]
    for l, w, (both, rendered, target) in zip(taps, lin, lpips_ref.dead_classes(r["a"], vgg_ref.SMALL)):
        a, b = r["a"][l][0], r["a"][l][1]
        assert int(target.sum()) > 0 and bool((b[:, target] == 0).all()) and bool((a[:, target].pow(2).sum(0) > 0).all())
        leaf = a[:, target].clone().requires_grad_(True)
        term = lpips_ref.tap_term_stock(leaf, b[:, target], w.double()) / (a.shape[1] * a.shape[2])
        (g,) = torch.autograd.grad(term, leaf)
        seed = lpips_ref.tap_seed(a, b, w)[:, target]
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert float((seed - g).abs().max()) <= 1e-12 * float(g.abs().max())


def test_new_gpu_cases_pass_the_tap_kernels_grid_cap_and_have_odd_widths():
    """k_lpips_tap: FR_VGG_LOSS_BLOCKS workgroups of four waves, one pixel a wave and sweep.  A change of the cap breaks this
    test instead of silently emptying tests/test_gpu_lpips.py's second sweep."""
    from fateavatar_amd import _lib
    from fateavatar_amd import perceptual as P
    from tests import test_gpu_lpips as T
    sweep = 4 * _lib.FR_VGG_LOSS_BLOCKS
    first_taps = []
    for stack, H, W, sh, sw in T.PAST_THE_CAP:
        f = _features(T.STACKS[stack], (sh, sw))
        taps = [h * w for (h, w), y in zip(f.extents(), f.layers) if y.tap_after]
        first_taps.append(taps[0])
        assert sweep < taps[0] < 2 * sweep and all(t < sweep for t in taps[1:])
    assert first_taps == [70 * 62, 80 * 64] and (35 * 31) % 4 != 0 and (70 * 62 - sweep) // 4 == 61
    assert all(h * w <= sweep for c in T.CASES for h, w in [c[3:5]])                  # the earlier cases: one sweep
    P.check_layers(vgg_ref.ODD, (16, 16))
    P.check_layers(vgg_ref.ODD, (24, 40))
    assert {c // 64 for _, c, _, tap in vgg_ref.ODD if tap} == {3, 5, 7}
    assert [c[0] for c in T.PAST_THE_CAP + T.ODD_CASES] == ["small", "lpips13", "odd", "odd"]


def test_patchwork_cases_have_ties_and_an_interior_in_float64():
    """tests/test_gpu_lpips.py's flat-region cases in float64: more than 1000 live tied pool windows wherever the stack has a
    pool (vgg_ref.WIDE has none: 0), more than 1000 live units whose rendered and target values are equal, no dead pixel, and
    a non-empty interior of the shared background for the two shallow stacks."""
    from tests import test_gpu_lpips as T
    from tests.test_gpu_vgg import _background_interior
    seen = {}
    for case in T.PATCHWORK:
        c = T._case(*case, patchwork=True)
        layers = T.STACKS[case[0]]
        seen[case[0]] = (vgg_ref.live_ties(c["r64"]["a"], layers), _background_interior(layers, *case[1:]))
        assert lpips_ref.dead_pixels(c["r64"]["a"], layers) == [(0, 0)] * sum(1 for y in layers if y[3])
    print(seen)
    assert seen["small"][0][0] >= 1000 and seen["lpips13"][0][0] >= 1000 and seen["wide"][0][0] == 0
    assert all(v[0][1] >= 1000 for v in seen.values())
    assert seen["small"][1] == (3, 3) and seen["wide"][1] == (8, 8) and seen["lpips13"][1] == (0, 0)


def test_wide_cases_send_the_seed_through_every_epilogue():
    """vgg_ref.WIDE has taps behind layers 1 and 3 and no pool: the tap-1 seed is added by the epilogue of layer 2's gradient
    GEMM (N = 512) — in-kernel where that GEMM is unsplit, in the split-reduce where it is split — and the last tap's seed is
    the operand the backward starts from.  tests/test_gpu_vgg.py's three sizes take 3, 3 and 1 planes there."""
    from fateavatar_amd.perceptual import gemm_splits
    from tests.test_gpu_vgg import WIDE_CASES
    assert [gemm_splits(c[3] * c[4], 512) for c in WIDE_CASES] == [3, 3, 1]
