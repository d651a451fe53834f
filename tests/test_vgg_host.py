"""CPU: the host side of the fused perceptual term (fateavatar_amd/perceptual.py, csrc/fr_vgg.hip) — the C ABI's struct and
workspace formula, every refusal that is decided before the device is touched, both weight packings against torch's own
convolutions, torchvision's key naming, the halo and resize index math enumerated in a stand-alone host program, and the
restatement of tests/vgg_ref.py against itself.  The kernels: tests/test_gpu_vgg.py."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch
import torch.nn.functional as F

from tests import vgg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _features(layers=vgg_ref.VGG16, size=(24, 24), seed=5):
    from fateavatar_amd.perceptual import VggFeatures
    W, B = vgg_ref.he_weights(layers, seed)
    return VggFeatures(layers, W, B, size=size)


def test_abi_struct_and_constants_match_the_header():
    from fateavatar_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(fr_vgg), sizeof(fr_vgg_layer), offsetof(fr_vgg, tile), offsetof(fr_vgg, mean),
        offsetof(fr_vgg, std), offsetof(fr_vgg, layers), offsetof(fr_vgg, weights_fwd), offsetof(fr_vgg, image), offsetof(fr_vgg, target));
 printf("%d %d %d %d %d %d %d\n", FR_VGG_MAX_LAYERS, FR_VGG_LOSS_BLOCKS, (int)FR_VGG_REDUCE_BYTES, FR_VGG_TILE_AUTO, FR_VGG_TILE_64, FR_VGG_TILE_128,
        FR_VGG_NO_SPLIT);
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    v = _lib.fr_vgg
    assert out[:9] == [C.sizeof(v), C.sizeof(_lib.fr_vgg_layer), v.tile.offset, v.mean.offset, v.std.offset, v.layers.offset,
                       v.weights_fwd.offset, v.image.offset, v.target.offset]
    assert out[9:] == [_lib.FR_VGG_MAX_LAYERS, _lib.FR_VGG_LOSS_BLOCKS, _lib.FR_VGG_REDUCE_BYTES, _lib.FR_VGG_TILE_AUTO,
                       _lib.FR_VGG_TILE_64, _lib.FR_VGG_TILE_128, _lib.FR_VGG_NO_SPLIT]
    header = open(os.path.join(ROOT, "include", "fr_rasterizer.h")).read()
    for sym in ("fr_vgg_workspace_bytes", "fr_vgg_loss_grad"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym) and sym + "(" in header


def test_workspace_bytes_is_the_documented_formula():
    from fateavatar_amd import _lib
    from fateavatar_amd.perceptual import workspace_bytes
    L = _lib.lib()
    r256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    for layers, size in ((vgg_ref.VGG16, (224, 224)), (vgg_ref.VGG16, (24, 24)), (vgg_ref.VGG16, (16, 32)), (vgg_ref.SMALL, (24, 24)),
                         (((3, 64, False, True),), (5, 7))):
        f = _features(layers, size)
        got = L.fr_vgg_workspace_bytes(C.byref(f.describe(37, 53)))
        assert got == workspace_bytes(f) and got % 256 == 0
        assert got == L.fr_vgg_workspace_bytes(C.byref(f.describe(1, 1)))          # the image's own extent does not enter
    # VGG-16 at 224^2 by hand: the saved activations of both images are 2 x 13.2 M floats
    acts = 2 * 4 * (2 * 64 * 224 * 224 + 2 * 128 * 112 * 112 + 3 * 256 * 56 * 56 + 3 * 512 * 28 * 28)
    want = (r256(_lib.FR_VGG_REDUCE_BYTES) + r256(2 * 224 * 224 * 3 * 4) + acts + 2 * 4 * 64 * 112 * 112 + 2 * 4 * 64 * 224 * 224
            + 4 * 64 * 112 * 112 + 4 * 3 * 1568 * 512)          # (the largest split GEMM: block 4's forward, three planes)
    assert L.fr_vgg_workspace_bytes(C.byref(_features(vgg_ref.VGG16, (224, 224)).describe(512, 512))) == want
    assert L.fr_vgg_workspace_bytes(None) == 0
    from fateavatar_amd.perceptual import gemm_splits
    assert [gemm_splits(*mn) for mn in ((1568, 512), (784, 512), (784, 256), (6272, 256), (100352, 64), (1152, 64))] == [3, 3, 9, 1, 1, 9]


def _describe(layers, size=(24, 24), H=8, W=8, addr=None, **over):
    from fateavatar_amd import _lib
    d = _lib.fr_vgg()
    d.n_layers, d.H, d.W, d.size_h, d.size_w, d.tile = len(layers), H, W, size[0], size[1], 0
    for c in range(3):
        d.mean[c], d.std[c] = 0.5, 0.25
    for i, y in enumerate(layers[:_lib.FR_VGG_MAX_LAYERS]):
        d.layers[i] = _lib.fr_vgg_layer(*[int(v) for v in y])
    d.weights_fwd = d.weights_bwd = d.image = d.target = addr
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_entry_point_refuses_bad_descriptors_before_anything_is_enqueued():
    from fateavatar_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 1024)()
    addr = (C.addressof(buf) + 255) // 256 * 256
    good = [(3, 64, 0, 0), (64, 64, 0, 1), (64, 128, 1, 1)]

    def refused(d, loss=addr, grad=addr, ws=addr, what=""):
        rc = L.fr_vgg_loss_grad(C.byref(d) if d is not None else None, 0.1, 0, loss, grad, ws, None)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT, what
        assert "fr_vgg_loss_grad" in _lib.last_error(), what
        if d is not None:
            assert L.fr_vgg_workspace_bytes(C.byref(d)) == 0 or what.startswith("ptr"), what

    assert L.fr_vgg_workspace_bytes(C.byref(_describe(good, addr=addr))) > 0
    bad_tables = {
        "c_in of layer 0": [(4, 64, 0, 1)],
        "c_in does not follow c_out": [(3, 64, 0, 0), (32, 64, 0, 1)],
        "c_out not a multiple of 64": [(3, 96, 0, 1)],
        "c_out 32": [(3, 32, 0, 1)],
        "c_out zero": [(3, 0, 0, 1)],
        "pool on layer 0": [(3, 64, 1, 1)],
        "last layer no tap": [(3, 64, 0, 1), (64, 64, 0, 0)],
        "seventeen layers": [(3, 64, 0, 0)] + [(64, 64, 0, 1)] * 16,
    }
    for what, table in bad_tables.items():
        d = _describe(table, addr=addr)
        if what == "seventeen layers":
            d.n_layers = 17
        refused(d, what=what)
    refused(_describe([], addr=addr), what="no layers")
    # every later c_in a multiple of 32 is implied by c_out % 64 == 0 and c_in == the c_out in front: the table cannot say otherwise
    refused(_describe(good, size=(24, 25), addr=addr), what="size_w = 25 is not divisible by 2")
    refused(_describe(good + [(128, 128, 1, 1), (128, 128, 1, 1), (128, 128, 1, 1)], size=(24, 24), addr=addr), what="24 is not divisible by 16")
    refused(_describe(good, size=(0, 24), addr=addr), what="size 0")
    refused(_describe(good, size=(24, 65536), addr=addr), what="size too large")
    refused(_describe(good, H=0, addr=addr), what="H W == 0")
    refused(_describe(good, W=0, addr=addr), what="H W == 0")
    refused(_describe(good, addr=addr, tile=7), what="tile")
    d = _describe(good, addr=addr)
    d.std[1] = 0.0
    refused(d, what="std 0")
    refused(None, what="ptr: null descriptor")
    for field in ("weights_fwd", "weights_bwd", "image", "target"):
        refused(_describe(good, addr=addr, **{field: None}), what="ptr: null " + field)
    refused(_describe(good, addr=addr), loss=None, what="ptr: null loss_out")
    refused(_describe(good, addr=addr), ws=None, what="ptr: null workspace")
    refused(_describe(good, addr=addr), ws=addr + 128, what="ptr: misaligned workspace")
    refused(_describe(good, addr=addr), grad=addr + 2, what="ptr: misaligned d_image")
    refused(_describe(good, addr=addr, image=addr + 1), what="ptr: misaligned image")
    refused(_describe(good, addr=addr, weights_bwd=addr + 4), what="ptr: misaligned weights")
    assert L.fr_vgg_workspace_bytes(C.byref(_describe(good, addr=addr, tile=_lib.FR_VGG_TILE_128 | _lib.FR_VGG_NO_SPLIT))) > 0


def test_python_refusals_come_before_the_device():
    from fateavatar_amd.avatar import AvatarBatchStep
    from fateavatar_amd.perceptual import ConvLayer, Perceptual, VggFeatures, check_layers
    for layers, size, match in (([ConvLayer(3, 64, tap_after=True)] * 2, (8, 8), "c_in"),
                                ([ConvLayer(3, 96, tap_after=True)], (8, 8), "multiple of 64"),
                                ([ConvLayer(3, 64), ConvLayer(64, 64, True, True)], (8, 9), "divisible"),
                                ([ConvLayer(3, 64)], (8, 8), "tap"),
                                ([ConvLayer(3, 64, True, True)], (8, 8), "layer 0"),
                                ([ConvLayer(3, 64)] + [ConvLayer(64, 64, tap_after=True)] * 16, (8, 8), "layers")):
        with pytest.raises(ValueError, match=match):
            check_layers(layers, size)
    check_layers([ConvLayer(*y) for y in vgg_ref.VGG16], (224, 224))
    with pytest.raises(ValueError, match="weight is"):
        VggFeatures(vgg_ref.SMALL, [torch.zeros(64, 3, 3, 3)] * 3, [torch.zeros(64)] * 3, size=(8, 8))
    f = _features(vgg_ref.SMALL, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        Perceptual(f)
    with pytest.raises(TypeError, match="VggFeatures"):
        Perceptual(torch.nn.Conv2d(3, 64, 3))
    with pytest.raises(NotImplementedError, match="perceptual"):
        AvatarBatchStep(None, None, None, None, None, perceptual=object())


def test_both_weight_packings_are_torchs_own_convolutions():
    from fateavatar_amd.perceptual import pack_backward, pack_forward
    g = torch.Generator().manual_seed(2)
    for ci, co in ((3, 64), (64, 128), (96, 64)):
        w, b = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64), torch.randn(co, generator=g, dtype=torch.float64)
        x = torch.randn(1, ci, 5, 7, generator=g, dtype=torch.float64)
        pf = pack_forward(w, b)
        assert pf.numel() == 9 * ci * co + co and torch.equal(pf[9 * ci * co:], b)
        Wf = pf[:9 * ci * co].view(9 * ci, co)
        # the implicit GEMM on the CPU: row (y, x) of A holds the nine neighbours' channels, tap-major, channel-minor
        cols = F.unfold(x, 3, padding=1).view(ci, 9, 5 * 7).permute(2, 1, 0).reshape(5 * 7, 9 * ci)
        got = (cols @ Wf + b).t().reshape(1, co, 5, 7)
        assert torch.allclose(got, F.conv2d(x, w, b, padding=1), rtol=1e-12, atol=1e-12)
        # row k = (3 ky + kx) c_in + ci holds W[:, ci, ky, kx]
        assert torch.equal(Wf[(3 * 2 + 1) * ci + 2], w[:, 2, 2, 1])
        # the data gradient: the SAME gathered GEMM over the second packing is conv_transpose2d
        dz = torch.randn(1, co, 5, 7, generator=g, dtype=torch.float64)
        Wb = pack_backward(w).view(9 * co, ci)
        cols = F.unfold(dz, 3, padding=1).view(co, 9, 5 * 7).permute(2, 1, 0).reshape(5 * 7, 9 * co)
        got = (cols @ Wb).t().reshape(1, ci, 5, 7)
        assert torch.allclose(got, F.conv_transpose2d(dz, w, padding=1), rtol=1e-12, atol=1e-12)
        assert torch.equal(Wb[(3 * 0 + 1) * co + 5], w[5, :, 2, 1])
        # and as a convolution's own weight: out channels = c_in, taps flipped
        as_conv = Wb.view(3, 3, co, ci).permute(3, 2, 0, 1)
        assert torch.allclose(F.conv2d(dz, as_conv, padding=1), F.conv_transpose2d(dz, w, padding=1), rtol=1e-12, atol=1e-12)


def test_torchvision_keys_round_trip():
    from fateavatar_amd.perceptual import VggFeatures, torchvision_indices
    assert torchvision_indices(vgg_ref.VGG16) == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21]
    W, B = vgg_ref.he_weights(vgg_ref.VGG16, 9)
    sd = {}
    for i, w, b in zip([0, 2, 5, 7, 10, 12, 14, 17, 19, 21], W, B):
        sd[f"features.{i}.weight"], sd[f"features.{i}.bias"] = w, b
    sd["features.24.weight"], sd["classifier.0.weight"] = torch.zeros(512, 512, 3, 3), torch.zeros(8, 8)     # ignored
    f = VggFeatures.from_state_dict(sd, size=(24, 24))
    assert len(f.layers) == 10 and f.taps == [1, 3, 6, 9] and f.size == (24, 24)
    back = f.state_dict()
    assert list(back) == [k for k in sd if not k.startswith(("features.24", "classifier"))]
    assert all(torch.equal(back[k], sd[k]) for k in back)
    g = VggFeatures.from_state_dict({"vgg." + k: v for k, v in sd.items()}, prefix="vgg.", size=(24, 24))
    assert torch.equal(g.packed_fwd, f.packed_fwd) and torch.equal(g.packed_bwd, f.packed_bwd)
    assert f.packed_fwd.numel() == sum(w.numel() + b.numel() for w, b in zip(W, B)) and f.packed_bwd.numel() == sum(w.numel() for w in W)
    with pytest.raises(KeyError, match="features.19.bias"):
        VggFeatures.from_state_dict({k: v for k, v in sd.items() if k != "features.19.bias"})
    assert VggFeatures.vgg16(size=(32, 32)).extents()[-1] == (4, 4)


HALO_PROGRAM = r'''
#include <stdio.h>
#include "fr_vgg_math.hpp"
using namespace fr;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 10) printf("line %d: %s\n", __LINE__, #c); } } while (0)
int main() {
    // every (row, tap) of the deepest and the first maps of the test shapes, two images: in range or flagged
    const int shapes[][2] = {{2, 2}, {3, 3}, {4, 4}, {2, 4}, {1, 1}, {1, 5}, {16, 16}, {24, 24}, {16, 32}};
    long checked = 0;
    for (auto& s : shapes) {
        const int h = s[0], w = s[1], M = 2 * h * w;
        for (int m = 0; m < M; m++) {
            const int p = m % (h * w), y = p / w, x = p % w, img = m / (h * w);
            for (int tap = 0; tap < 9; tap++) {
                const int nb = vgg_neighbour(m, y, x, h, w, tap);
                const int ny = y + tap / 3 - 1, nx = x + tap % 3 - 1;
                const bool inside = ny >= 0 && ny < h && nx >= 0 && nx < w;
                if (!inside) CHECK(nb == -1);
                else {
                    CHECK(nb >= 0 && nb < M);
                    CHECK(nb / (h * w) == img);                          // never the other image
                    CHECK(nb == img * h * w + ny * w + nx);
                }
                checked++;
            }
        }
    }
    // the resize: taps in range, identity exact, and the gather's candidate range holds every output that blends a source
    const int sizes[][2] = {{37, 24}, {53, 24}, {13, 24}, {17, 24}, {24, 24}, {29, 16}, {23, 16}, {20, 16}, {40, 32}, {512, 224}, {1, 8}, {8, 1}, {64, 24}};
    for (auto& s : sizes) {
        const int in = s[0], out = s[1];
        const float scale = (float)in / (float)out;
        for (int o = 0; o < out; o++) {
            int i0, i1; float lam;
            vgg_source(o, scale, in, i0, i1, lam);
            CHECK(i0 >= 0 && i0 < in && i1 >= i0 && i1 <= i0 + 1 && i1 < in);
            CHECK(lam >= 0.f && lam <= 1.f);
            if (in == out) CHECK(i0 == o && lam == 0.f);
            for (int i = i0; i <= i1; i++) {
                int lo, hi;
                vgg_source_range(i, scale, out, lo, hi);
                CHECK(lo >= 0 && hi <= out - 1 && lo <= o && o <= hi);
            }
            float total = 0.f;
            for (int i = 0; i < in; i++) total += vgg_source_weight(o, i, scale, in);
            CHECK(total > 0.999f && total < 1.001f);
            checked++;
        }
        for (int i = 0; i < in; i++) {
            int lo, hi;
            vgg_source_range(i, scale, out, lo, hi);
            CHECK(lo >= 0 && hi <= out - 1);
        }
    }
    printf("%s %ld\n", fails ? "FAILED" : "ok", checked);
    return fails ? 1 : 0;
}'''


def test_halo_and_resize_index_math_enumerated_in_a_stand_alone_program():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "halo.cpp"), os.path.join(d, "halo")
        open(src, "w").write(HALO_PROGRAM)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                               "-I", os.path.join(ROOT, "fateavatar_amd", "csrc"), src, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[0] == "ok", out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 20000


def test_resize_math_is_torchs_interpolate():
    """vgg_source restated in Python against F.interpolate(bilinear, align_corners=False), identity included."""
    import numpy as np

    def resize(x, out):
        n = x.shape[0]
        scale = np.float32(n) / np.float32(out)
        y = np.zeros(out, dtype=np.float64)
        for o in range(out):
            s = max(np.float32(scale * np.float32(o + 0.5) - np.float32(0.5)), np.float32(0))
            i0 = min(int(s), n - 1)
            i1 = i0 + (1 if i0 < n - 1 else 0)
            lam = float(np.float32(s - np.float32(i0)))
            y[o] = (1 - lam) * x[i0] + lam * x[i1]
        return y
    g = torch.Generator().manual_seed(0)
    for n, out in ((37, 24), (13, 24), (24, 24), (29, 16), (40, 32), (512, 224)):
        x = torch.rand(n, generator=g, dtype=torch.float64)
        want = F.interpolate(x.view(1, 1, 1, n).float(), size=(1, out), mode="bilinear", align_corners=False).view(out).double()
        got = torch.from_numpy(resize(x.numpy(), out))
        assert torch.allclose(got, want, rtol=0, atol=2e-6), (n, out)
        if n == out:
            assert torch.equal(got, x)


def test_restatement_pinned_backward_at_its_own_decisions_is_autograd():
    for layers, hw, size in ((vgg_ref.SMALL, (11, 9), (8, 12)), (vgg_ref.VGG16, (13, 17), (8, 8))):
        W, B = vgg_ref.he_weights(layers, 3)
        img, gt = vgg_ref.images(*hw, seed=4)
        r = vgg_ref.forward(W, B, layers, img, gt, size)
        loss, g = vgg_ref.autograd_gradient(W, B, layers, img, gt, size)
        pinned = vgg_ref.pinned_backward(W, layers, r["a"], hw, size)
        assert float(g.abs().max()) > 0 and float(loss) == float(r["loss"])
        assert float((pinned - g).norm() / g.norm()) < 1e-12
        assert vgg_ref.decisions_clear(r, layers, 0.0) and not vgg_ref.decisions_clear(r, layers, 1.0)


def test_restatement_normalises_with_float32_statistics():
    """The reference's mean and std are float32 buffers that take the image's dtype afterwards (recorded run `vgg`,
    tests/test_reference_runs_host.py); the kernel's descriptor holds them as float."""
    from fateavatar_amd.perceptual import IMAGENET_MEAN, IMAGENET_STD
    assert (vgg_ref.MEAN, vgg_ref.STD) == (IMAGENET_MEAN, IMAGENET_STD)
    x = torch.rand(1, 3, 4, 5, generator=torch.Generator().manual_seed(0))
    m32, s32 = torch.tensor(vgg_ref.MEAN).double().view(1, 3, 1, 1), torch.tensor(vgg_ref.STD).double().view(1, 3, 1, 1)
    assert torch.equal(vgg_ref.preprocess(x, (4, 5), torch.float64), (x.double() - m32) / s32)
    assert not torch.equal(m32.view(3), torch.tensor(vgg_ref.MEAN, dtype=torch.float64))


def test_receptive_margin_counted_by_hand():
    # conv: 1 + 1; conv, conv: 2 + 2; SMALL: s 1 -> (1,1) -> (2,2), pool -> hi 3, s 2, conv -> (4,5)
    assert vgg_ref.receptive_margin(((3, 64, False, True),)) == 2
    assert vgg_ref.receptive_margin(vgg_ref.SMALL[:2]) == 4 and vgg_ref.receptive_margin(vgg_ref.SMALL) == 9
    assert vgg_ref.receptive_margin(vgg_ref.VGG16) == 42 + 49
    # the rule itself, on SMALL: an input pixel reaches exactly the deepest units whose field holds it
    W, B = vgg_ref.he_weights(vgg_ref.SMALL, 1)
    leaf = torch.rand(1, 3, 24, 24, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    h = leaf
    for (ci, co, pool, tap), w in zip(vgg_ref.SMALL, W):
        h = F.conv2d(F.max_pool2d(h, 2) if pool else h, w.double().abs(), padding=1)     # (positive weights: nothing cancels)
    for unit in (0, 3, 11):
        (g,) = torch.autograd.grad(h[0, 0, unit, unit], leaf, retain_graph=True)
        cols = g[0].abs().sum((0, 1)).nonzero().view(-1)
        assert int(cols.max()) - int(cols.min()) <= vgg_ref.receptive_margin(vgg_ref.SMALL)
        if unit == 3:       # (clear of both borders: the whole field)
            assert int(cols.max()) - int(cols.min()) == vgg_ref.receptive_margin(vgg_ref.SMALL)


def test_wide_cases_take_every_split_plan():
    """tests/test_gpu_vgg.py's WIDE_CASES between them run every plan of the split over the taps that a GEMM kind can take —
    under the library's own flags.  Should vgg_splits (restated by perceptual.gemm_splits, which
    test_workspace_bytes_is_the_documented_formula holds to the library) change, this fails instead of the coverage going."""
    from fateavatar_amd.perceptual import VggFeatures, gemm_splits
    from tests.test_gpu_vgg import STACKS, WIDE_CASES
    from tests.test_gpu_vgg import CASES

    def plans(stack, sh, sw):
        """(forward plans, gradient plans) of layers 1 .. L-1 (layer 0 and its gradient are no GEMMs)."""
        layers = STACKS[stack]
        extents = VggFeatures(layers, *vgg_ref.he_weights(layers, 0), size=(sh, sw)).extents()
        return ([gemm_splits(2 * h * w, co) for (ci, co, _, _), (h, w) in list(zip(layers, extents))[1:]],
                [gemm_splits(h * w, ci) for (ci, co, _, _), (h, w) in list(zip(layers, extents))[1:]])

    wide = {(sh, sw): plans(stack, sh, sw) for stack, H, W, sh, sw in WIDE_CASES}
    assert wide == {(26, 30): ([3, 3, 3], [9, 3, 3]), (32, 32): ([1, 1, 1], [9, 3, 3]), (64, 32): ([1, 1, 1], [9, 1, 1])}
    forward = {s for fw, _ in wide.values() for s in fw}
    gradient = {s for _, bw in wide.values() for s in bw[:-1]}          # with a stored dZ as its operand
    seed = {bw[-1] for _, bw in wide.values()}                          # the last layer's: dZ computed in the fetch (SEED)
    assert forward == {1, 3} and gradient == {1, 3, 9} and seed == {1, 3}
    # nine planes forward (and nine on a SEED gradient): every GEMM of the older cases
    older = [plans(stack, sh, sw) for stack, H, W, sh, sw in CASES]
    assert all(set(fw) | set(bw) == {9} for fw, bw in older)
    # the boundary itself: a grid of exactly 256 tiles is not split, one of 255 is
    assert -(-2 * 32 * 32 // 64) * (512 // 64) == 256 and -(-64 * 32 // 64) * (512 // 64) == 256
    assert [gemm_splits(m, 512) for m in (2048 - 64, 2048)] == [3, 1] and [gemm_splits(m, 64) for m in (85 * 64, 85 * 64 + 1)] == [9, 3]


# (stack, H, W, size_h, size_w): resizes that keep a flat region bit-flat — the identity and an exact halving
PATCHWORK_CASES = [("small", 24, 24, 24, 24), ("vgg16", 48, 48, 24, 24), ("vgg16", 32, 32, 32, 32)]
PATCHWORK_STACKS = {"small": vgg_ref.SMALL, "vgg16": vgg_ref.VGG16}


@pytest.mark.parametrize("case", PATCHWORK_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-to-{c[3]}x{c[4]}")
def test_patchwork_puts_live_decisions_on_their_thresholds(case):
    """The patchwork images do what noise cannot: thousands of LIVE pool windows are exact ties and thousands of LIVE tap
    differences exactly 0, so that the two rules the kernel's comments state — the first maximum takes a window's gradient,
    sign(0) = 0 — decide a large part of the gradient.  Shown by mutation: the pinned backward with either rule replaced by
    its opposite moves by more than 0.1 rel-L2 (on the suite's noise images: by exactly 0)."""
    stack, H, Wd, sh, sw = case
    layers = PATCHWORK_STACKS[stack]
    W, B = vgg_ref.he_weights(layers, seed=11 + len(layers))
    img, gt = vgg_ref.patchwork(H, Wd, seed=1000 * H + Wd)
    assert bool((img[:, :H // 2, :Wd // 2] == 1).all()) and bool((gt[:, :H // 2, :Wd // 2] == 1).all())
    assert torch.equal(img[:, H // 2:, Wd // 2:], vgg_ref.images(H, Wd, seed=1000 * H + Wd)[0][:, H // 2:, Wd // 2:])
    r = vgg_ref.forward(W, B, layers, img, gt, (sh, sw))
    ties, zeros = vgg_ref.live_ties(r["a"], layers)
    print(f"{case}: live tied windows {ties}, live zero tap differences {zeros}")
    assert ties >= 1000 and zeros >= 1000
    loss, g = vgg_ref.autograd_gradient(W, B, layers, img, gt, (sh, sw))
    pinned = vgg_ref.pinned_backward(W, layers, r["a"], (H, Wd), (sh, sw))
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    assert float(g.abs().max()) > 0 and rel(pinned, g) <= 1e-12
    last = vgg_ref.pinned_backward(W, layers, r["a"], (H, Wd), (sh, sw), one_hot=lambda a: vgg_ref._window_one_hot(a, last=True))
    plus = vgg_ref.pinned_backward(W, layers, r["a"], (H, Wd), (sh, sw), sign=vgg_ref.sign_plus_at_zero)
    print(f"{case}: last maximum moves the gradient by {rel(last, pinned):.3f}, sign(0) = +1 by {rel(plus, pinned):.3f}")
    assert rel(last, pinned) > 0.1 and rel(plus, pinned) > 0.1
    # and noise has none of it: the same mutations change no bit there
    img, gt = vgg_ref.images(H, Wd, seed=1000 * H + Wd)
    r = vgg_ref.forward(W, B, layers, img, gt, (sh, sw))
    assert vgg_ref.live_ties(r["a"], layers) == (0, 0)
