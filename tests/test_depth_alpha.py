"""CPU: depth and alpha planes (FR_FLAG_DEPTH_ALPHA) — the flag's value in the header, the ctypes binding and the library,
the new fr_aux members and size query, the argument checks (host memory stands in for handles and inputs, which are never
dereferenced), and the Python entry points' refusal of CPU tensors."""
import ctypes as C
import os
import re

import pytest
import torch

from fateavatar_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fr_rasterizer.h")


def test_header_binding_and_library_agree_on_the_flag():
    m = re.search(r"#define\s+FR_FLAG_DEPTH_ALPHA\s+(\d+)", open(HDR).read())
    assert m and int(m.group(1)) == _lib.FR_FLAG_DEPTH_ALPHA == 8
    taken = _lib.FR_FLAG_NO_WAIT | _lib.FR_FLAG_RAW_ACTIVATIONS | _lib.FR_FLAG_FORWARD_ONLY
    assert _lib.FR_FLAG_DEPTH_ALPHA & taken == 0
    assert _lib.FR_FLAG_DEPTH_ALPHA < (1 << _lib.FR_FLAG_ACCUMULATE_SHIFT)


def test_aux_gains_the_plane_members_at_its_end():
    names = [f[0] for f in _lib.fr_aux._fields_]
    assert names[-5:] == ["out_depth", "out_alpha", "dL_ddepth", "dL_dalpha", "planes"]
    assert names[:9] == ["visible", "grad_accum", "denom", "binding", "d_verts", "d_offset", "d_rotation", "d_scaling",
                         "overflow_out"]
    a = _lib.fr_aux(1, 2, 3)   # (positional construction of the old members still works)
    assert (a.visible, a.grad_accum, a.denom, a.out_depth, a.planes) == (1, 2, 3, None, None)


def test_planes_size_query_is_exported_and_small():
    L = _lib.lib()
    assert "fr_planes_bytes" in _lib.EXPORTS and hasattr(L, "fr_planes_bytes")
    assert L.fr_planes_bytes(0, 8, 8) <= 4096                         # one tile, two units: a few hundred bytes
    for cap, W, H in ((1000, 64, 64), (123457, 512, 512), (0, 17, 33)):
        T = ((W + 7) // 8) * ((H + 7) // 8)
        units = cap // 64 + T + 1
        n = L.fr_planes_bytes(cap, W, H)
        assert 512 * units <= n <= 512 * units + 1024, (cap, W, H, n)
        assert n < L.fr_binning_bytes(cap, W, H)
    # frames without the flag keep their scratch sizes (the values of the parent build)
    assert L.fr_binning_bytes(1000, 64, 64) >= 1000 * 56


def _fake_call(flags, aux_list, n=2):
    """fr_forward_batch on host memory: every check runs before a handle or a device pointer is touched."""
    L = _lib.lib()
    fake = [C.create_string_buffer(4096) for _ in range(n)]
    handles = (C.c_void_p * n)(*[C.addressof(b) for b in fake])
    dummy = C.addressof(fake[0])
    inp = _lib.fr_inputs(background=dummy, means3D=dummy, shs=dummy, opacities=dummy, scales=dummy, rotations=dummy,
                         viewmatrix=dummy, projmatrix=dummy, campos=dummy)
    prms = []
    for f, aux in zip(flags, aux_list):
        p = _lib.fr_params(10, 0, 1, 16, 16, 0.5, 0.5, 1.0, 0, 0, f)
        if aux is not None:
            p.aux = C.pointer(aux)
        prms.append(p)
    prm_p = (C.POINTER(_lib.fr_params) * n)(*[C.pointer(p) for p in prms])
    inp_p = (C.POINTER(_lib.fr_inputs) * n)(*[C.pointer(inp)] * n)
    ptrs = (C.c_void_p * n)(*[dummy] * n)
    return L.fr_forward_batch(n, handles, prm_p, inp_p, ptrs, ptrs, ptrs, ptrs, ptrs, (C.c_uint64 * n)(*[1024] * n), None, None)


def test_batch_views_must_agree_on_the_flag():
    F = _lib.FR_FLAG_DEPTH_ALPHA
    buf = C.create_string_buffer(64)
    full = _lib.fr_aux(out_depth=C.addressof(buf), out_alpha=C.addressof(buf), planes=C.addressof(buf))
    for f0, f1 in ((0, F), (F, 0), (_lib.FR_FLAG_FORWARD_ONLY, _lib.FR_FLAG_FORWARD_ONLY | F)):
        assert _fake_call((f0, f1), (full, full)) == _lib.FR_ERR_INVALID_ARGUMENT
        assert "FR_FLAG_DEPTH_ALPHA" in _lib.last_error()


@pytest.mark.parametrize("missing", ["aux", "out_depth", "out_alpha", "planes"])
def test_the_flag_needs_both_planes_and_the_scratch(missing):
    buf = C.create_string_buffer(64)
    kw = dict(out_depth=C.addressof(buf), out_alpha=C.addressof(buf), planes=C.addressof(buf))
    if missing != "aux":
        kw.pop(missing)
    aux = None if missing == "aux" else _lib.fr_aux(**kw)
    assert _fake_call((_lib.FR_FLAG_DEPTH_ALPHA,), (aux,), n=1) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "FR_FLAG_DEPTH_ALPHA" in _lib.last_error()


def test_a_plane_gradient_needs_the_flag():
    L = _lib.lib()
    fake = C.create_string_buffer(4096)
    dummy = C.addressof(fake)
    inp = _lib.fr_inputs(background=dummy, means3D=dummy, shs=dummy, opacities=dummy, scales=dummy, rotations=dummy,
                         viewmatrix=dummy, projmatrix=dummy, campos=dummy)
    for field in ("dL_ddepth", "dL_dalpha"):
        aux = _lib.fr_aux(**{field: dummy})
        prm = _lib.fr_params(10, 0, 1, 16, 16, 0.5, 0.5, 1.0, 0, 0, 0)
        prm.aux = C.pointer(aux)
        grads = _lib.fr_grads()
        rc = L.fr_backward(dummy, C.byref(prm), C.byref(inp), dummy, dummy, dummy, dummy, dummy, C.byref(grads), None)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT and "FR_FLAG_DEPTH_ALPHA" in _lib.last_error()


def test_render_with_planes_on_cpu_tensors_raises():
    from fateavatar_amd import scenes
    from fateavatar_amd.render import render
    s = scenes.head_scene(P=64, res=32, sh_degree=0, seed=0)

    class Cam:
        FoVx = FoVy = 0.8
        image_height = image_width = 32
        world_view_transform = torch.eye(4)
        full_proj_transform = torch.eye(4)
        camera_center = torch.zeros(3)

    class PC:
        get_xyz = torch.from_numpy(s.means3D)
        get_opacity = torch.from_numpy(s.opacities)
        get_scaling = torch.from_numpy(s.scales)
        get_rotation = torch.from_numpy(s.rotations)
        get_features = torch.from_numpy(s.shs)
        max_sh_degree = s.sh_degree

    with pytest.raises(RuntimeError, match="no CPU path"):
        render(Cam(), PC(), torch.zeros(3), depth_alpha=True)
