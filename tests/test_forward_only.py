"""CPU: forward-only frames (FR_FLAG_FORWARD_ONLY) — the flag's value in the header, the ctypes binding and the library, the
hand-off accessors (pure pointer arithmetic, no device memory is touched), and the host's automatic choice."""
import ctypes as C
import os
import re

import pytest
import torch

from fateavatar_amd import _lib, rasterizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fr_rasterizer.h")


def test_header_binding_and_library_agree_on_the_flag():
    m = re.search(r"#define\s+FR_FLAG_FORWARD_ONLY\s+(\d+)", open(HDR).read())
    assert m and int(m.group(1)) == _lib.FR_FLAG_FORWARD_ONLY == 4
    assert _lib.FR_FLAG_FORWARD_ONLY & (_lib.FR_FLAG_NO_WAIT | _lib.FR_FLAG_RAW_ACTIVATIONS) == 0
    # the library reads bit 2 as the flag: two views that disagree on it are refused before anything touches a handle or
    # the device (host memory stands in for the handles and for the inputs, which are never dereferenced)
    L = _lib.lib()
    fake = [C.create_string_buffer(4096) for _ in range(2)]
    handles = (C.c_void_p * 2)(*[C.addressof(b) for b in fake])
    dummy = C.addressof(fake[0])
    inp = _lib.fr_inputs(background=dummy, means3D=dummy, shs=dummy, opacities=dummy, scales=dummy, rotations=dummy,
                         viewmatrix=dummy, projmatrix=dummy, campos=dummy)

    def call(flags0, flags1):
        prms = [_lib.fr_params(10, 0, 1, 16, 16, 0.5, 0.5, 1.0, 0, 0, f) for f in (flags0, flags1)]
        prm_p = (C.POINTER(_lib.fr_params) * 2)(*[C.pointer(p) for p in prms])
        inp_p = (C.POINTER(_lib.fr_inputs) * 2)(C.pointer(inp), C.pointer(inp))
        ptrs = (C.c_void_p * 2)(dummy, dummy)
        return L.fr_forward_batch(2, handles, prm_p, inp_p, ptrs, ptrs, ptrs, ptrs, ptrs, (C.c_uint64 * 2)(1024, 1024), None, None)

    for f0, f1 in ((0, _lib.FR_FLAG_FORWARD_ONLY), (_lib.FR_FLAG_FORWARD_ONLY, 0),
                   (_lib.FR_FLAG_NO_WAIT, _lib.FR_FLAG_NO_WAIT | _lib.FR_FLAG_FORWARD_ONLY)):
        assert call(f0, f1) == _lib.FR_ERR_INVALID_ARGUMENT
        assert "FR_FLAG_FORWARD_ONLY" in _lib.last_error()


def test_binning_region_accessor_is_exported_and_lays_out_the_hand_off():
    L = _lib.lib()
    assert "fr_debug_binning_region" in _lib.EXPORTS and hasattr(L, "fr_debug_binning_region")
    base = 1 << 40   # (an address only: the accessor does pointer arithmetic)
    for cap, W, H in ((1000, 64, 64), (123457, 512, 512), (0, 17, 33)):
        total = L.fr_binning_bytes(cap, W, H)
        T = ((W + 7) // 8) * ((H + 7) // 8)
        units = cap // 64 + T + 1
        want = {0: 8 * cap, 1: 512 * units, 2: 32 * units, 3: 1024 * units}
        spans = []
        for region, size in want.items():
            n = C.c_size_t(12345)
            p = L.fr_debug_binning_region(base, cap, W, H, region, C.byref(n))
            assert p is not None and n.value == size, (region, cap, n.value, size)
            assert base <= p and p + n.value <= base + total, (region, cap)
            spans.append((p, p + n.value))
            assert L.fr_debug_binning_region(base, cap, W, H, region, None) == p
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))   # no two regions overlap
        for bad in (-1, 4, 99):
            n = C.c_size_t(7)
            assert L.fr_debug_binning_region(base, cap, W, H, bad, C.byref(n)) is None and n.value == 0


def test_geometry_accessor_names_the_direction_derivative():
    L = _lib.lib()
    base = 1 << 40
    for P in (1, 1000, 100_000):
        total = L.fr_geometry_bytes(P)
        p9 = L.fr_debug_geometry_field(base, P, 9)
        p10 = L.fr_debug_geometry_field(base, P, 10)
        assert p9 is not None and base <= p9 and p9 + 36 * P <= base + total
        assert p10 is not None and base <= p10 and p10 + 4 * P <= base + total
        assert p9 % 256 == 0 and p10 % 256 == 0
        rec = L.fr_debug_geometry_field(base, P, 8)
        clamped = L.fr_debug_geometry_field(base, P, 6)
        for a, n in ((p9, 36 * P), (p10, 4 * P), (clamped, P)):   # the hand-off fields are outside the blend records
            assert a >= rec + 48 * P or a + n <= rec
        assert L.fr_debug_geometry_field(base, P, 11) is None


@pytest.fixture
def _restore_auto():
    prev = rasterizer._forward_only_auto
    yield
    rasterizer._forward_only_auto = prev


def test_set_forward_only_is_process_wide_or_scoped(_restore_auto):
    assert rasterizer._forward_only_auto is True          # the default: chosen automatically
    rasterizer.set_forward_only(False)                    # a plain call: process-wide
    assert rasterizer._forward_only_auto is False
    with rasterizer.set_forward_only(True):               # a block: restored on exit
        assert rasterizer._forward_only_auto is True
        with rasterizer.set_forward_only(False):
            assert rasterizer._forward_only_auto is False
        assert rasterizer._forward_only_auto is True
    assert rasterizer._forward_only_auto is False
    with pytest.raises(ZeroDivisionError):
        with rasterizer.set_forward_only(True):
            1 / 0
    assert rasterizer._forward_only_auto is False         # (restored when the block raises, too)
    rasterizer.set_forward_only(True)
    assert rasterizer._forward_only_auto is True


def test_forward_only_is_picked_exactly_when_autograd_will_not_record(_restore_auto):
    leaf = torch.zeros(4, requires_grad=True)
    plain = torch.zeros(4)
    empty = torch.Tensor([])
    pick = rasterizer._pick_forward_only
    assert pick((plain, empty, plain)) is True                 # nothing requires grad
    assert pick((plain, leaf, empty)) is False                 # autograd records the frame
    with torch.no_grad():
        assert pick((plain, leaf)) is True                     # grad mode off
    with torch.inference_mode():
        assert pick((plain,)) is True
    with torch.enable_grad():
        assert pick((leaf * 2, plain)) is False                # a non-leaf that requires grad
    with rasterizer.set_forward_only(False):                   # A/B switch: never forward-only
        with torch.no_grad():
            assert pick((plain, leaf)) is False
        assert pick((plain,)) is False
