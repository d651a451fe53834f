"""CPU: FlashAvatar's MLP-deformed binding (model/baseline/flashavatar.py:242-276) and Huber term (train/loss.py:217-239) — the
torch restatement every GPU test is held to (tests/flash_ref.py) against hand cases, gradcheck and the written backward
formulas, the C ABI of the new mode and of the Huber launch, and the host side of `FlashGaussians` / `FlashStep` /
`DeformBinding`."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import flash_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mesh(seed=5, V=9, F=7, N=23, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    verts = torch.randn(V, 3, generator=g, dtype=dtype)
    faces = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(F)]).to(torch.int32)
    fi = torch.randint(0, F, (N,), generator=g).to(torch.int32)
    bary = torch.rand(N, 3, generator=g, dtype=dtype)
    bary = bary / bary.sum(1, keepdim=True)
    return verts, faces, fi, bary, g


# ------------------------------------------------------------------ the restatement: hand cases
def test_zero_deform_is_the_barycentric_point_and_leaves_rotation_and_scaling_alone():
    verts, faces, fi, bary, g = _mesh(dtype=torch.float32)
    N = fi.shape[0]
    rot, scl = torch.randn(N, 4, generator=g), torch.randn(N, 3, generator=g)
    xyz, r, s = R.deform_bind(verts, faces, fi, bary, torch.zeros(N, 10), rot, scl)
    tri = verts[faces.long()[fi.long()]]
    assert torch.equal(xyz, (tri * bary.unsqueeze(-1)).sum(1))
    assert torch.equal(r, rot)          # (r, v) (x) (1, 0) = (r, v) bit for bit: products with 1 and sums with +-0
    assert torch.equal(s, scl)


def test_quaternion_product_keeps_its_sign():
    i, j, k = torch.tensor([[0.0, 1, 0, 0]]), torch.tensor([[0.0, 0, 1, 0]]), torch.tensor([[0.0, 0, 0, 1]])
    assert torch.equal(R.quat_product(i, j), k)
    assert torch.equal(R.quat_product(j, i), -k)                      # the reverse order gives the negative: not standardised
    a, b = torch.tensor([[0.5, 1.0, -2.0, 0.25]]), torch.tensor([[-1.5, 0.5, 0.75, 2.0]])
    want = torch.tensor([[0.5 * -1.5 - (0.5 - 1.5 + 0.5), 0.5 * 0.5 - 1.5 * 1.0 + (-2.0 * 2.0 - 0.25 * 0.75),
                          0.5 * 0.75 - 1.5 * -2.0 + (0.25 * 0.5 - 1.0 * 2.0), 0.5 * 2.0 - 1.5 * 0.25 + (1.0 * 0.75 + 2.0 * 0.5)]])
    got = R.quat_product(a, b)
    assert torch.allclose(got, want, atol=1e-6)
    assert float(got[0, 0]) < 0          # a negative real part stays negative
    # through the binding: rotation (x) (exp(tanh(d3)), tanh(d4:7)) with a negative real part
    verts, faces, fi, bary, _ = _mesh(N=1, dtype=torch.float32)
    d = torch.zeros(1, 10)
    d[0, 3:7] = torch.tensor([0.3, -0.2, 0.9, 0.1])
    rot = torch.tensor([[-0.7, 0.1, 0.2, -0.3]])
    _, r, _ = R.deform_bind(verts, faces, fi, bary, d, rot, torch.zeros(1, 3))
    t = torch.tanh(d[0])
    delta = torch.cat([torch.exp(t[3:4]), t[4:7]])[None]
    assert torch.equal(r, R.quat_product(rot, delta)) and float(r[0, 0]) < 0


def test_huber_hand_values():
    h = lambda x: float(R.huber(torch.tensor([x], dtype=torch.float64))[0])  # noqa: E731
    assert h(0.05) == pytest.approx(0.00125, abs=1e-15)
    assert h(0.3) == pytest.approx(0.025, abs=1e-15)
    for x in (0.1, -0.1):                # both branches meet at |x| = alpha
        assert h(x) == pytest.approx(0.005, abs=1e-15)
        assert 0.5 * x * x == pytest.approx(0.1 * (abs(x) - 0.05), abs=1e-15)
    assert h(0.0) == 0.0
    # the mask term with a half-valued mask: h(0.5 d); d = 0.3 -> 0.15 is linear, d = 0.1 -> 0.05 quadratic
    img = torch.tensor([0.3, 0.1, 0.0, -0.3], dtype=torch.float64).reshape(1, 2, 2)
    mask = torch.full((1, 2, 2), 0.5, dtype=torch.float64)
    total, hub, mouth = R.huber_loss(img, torch.zeros_like(img), mask)
    assert float(hub) == pytest.approx((0.025 + 0.005 + 0 + 0.025) / 4, abs=1e-15)
    assert float(mouth) == pytest.approx((0.1 * (0.15 - 0.05) + 0.5 * 0.05 ** 2 + 0 + 0.1 * (0.15 - 0.05)) / 4, abs=1e-15)
    assert float(total) == pytest.approx(float(hub) + 40 * float(mouth), abs=1e-15)
    t2, h2, m2 = R.huber_loss(img, torch.zeros_like(img))
    assert float(m2) == 0.0 and float(t2) == float(h2) == float(hub)
    # a [1,H,W] mask is broadcast over the channels
    img3 = img.expand(3, 2, 2).contiguous()
    assert float(R.huber_loss(img3, torch.zeros_like(img3), mask)[2]) == pytest.approx(float(mouth), abs=1e-15)


# ------------------------------------------------------------------ gradients
def test_gradcheck_of_both_functions():
    verts, faces, fi, bary, g = _mesh()
    N = fi.shape[0]
    x = [verts.clone().requires_grad_(True), (1.5 * torch.randn(N, 10, generator=g, dtype=torch.float64)).requires_grad_(True),
         torch.randn(N, 4, generator=g, dtype=torch.float64).requires_grad_(True),
         torch.randn(N, 3, generator=g, dtype=torch.float64).requires_grad_(True)]
    assert torch.autograd.gradcheck(lambda v, d, r, s: R.deform_bind(v, faces, fi, bary, d, r, s), x)
    # Huber: away from |d| = alpha and |m d| = alpha, where the second derivative jumps (the first does not)
    img = torch.tensor([[0.02, -0.05, 0.3], [0.5, -0.25, 0.07]], dtype=torch.float64).reshape(1, 2, 3).repeat(3, 1, 1)
    img = (img * torch.tensor([1.0, 0.8, 1.3], dtype=torch.float64).reshape(3, 1, 1)).requires_grad_(True)
    mask = torch.tensor([[0.0, 1.0, 0.5], [0.9, 0.3, 1.0]], dtype=torch.float64).reshape(1, 2, 3)
    gt = torch.zeros(3, 2, 3, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda i: R.huber_loss(i, gt, mask)[0], [img])
    assert torch.autograd.gradcheck(lambda i: R.huber_loss(i, gt)[0], [img])


def test_the_written_backward_formulas_equal_autograd():
    """The backward of the binding and the gradient of the Huber term as the device code evaluates them, coded once here,
    against float64 autograd of the restatement: 1e-12."""
    verts, faces, fi, bary, g = _mesh(seed=11, N=40)
    N = fi.shape[0]
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    deform, rot, scl = 1.5 * rn(N, 10), rn(N, 4), rn(N, 3)
    g_xyz, g_rot, g_scl = rn(N, 3), rn(N, 4), rn(N, 3)
    x = [t.clone().requires_grad_(True) for t in (verts, deform, rot, scl)]
    out = R.deform_bind(x[0], faces, fi, bary, x[1], x[2], x[3])
    torch.autograd.backward(out, [g_xyz, g_rot, g_scl])
    # ---- by hand
    t = torch.tanh(deform)
    e3, es = torch.exp(t[:, 3]), torch.exp(t[:, 7:10])
    a, b = rot, torch.cat([e3[:, None], t[:, 4:7]], dim=1)
    aw, ax, ay, az = a.unbind(1)
    bw, bx, by, bz = b.unbind(1)
    gw, gx, gy, gz = g_rot.unbind(1)
    d_delta = torch.stack([gw * aw + gx * ax + gy * ay + gz * az, -gw * ax + gx * aw + gy * az - gz * ay,
                           -gw * ay - gx * az + gy * aw + gz * ax, -gw * az + gx * ay - gy * ax + gz * aw], dim=1)
    d_rot = torch.stack([gw * bw + gx * bx + gy * by + gz * bz, -gw * bx + gx * bw - gy * bz + gz * by,
                         -gw * by + gx * bz + gy * bw - gz * bx, -gw * bz - gx * by + gy * bx + gz * bw], dim=1)
    g_t = torch.cat([g_xyz, (d_delta[:, 0] * e3)[:, None], d_delta[:, 1:4], g_scl * scl * es], dim=1)
    d_deform = g_t * (1 - t * t)
    d_scl = g_scl * es
    d_verts = torch.zeros_like(verts)
    corners = faces.long()[fi.long()]
    for k in range(3):
        d_verts.index_add_(0, corners[:, k], bary[:, k:k + 1] * g_xyz)
    for name, got, want in zip(("verts", "deform", "rotation", "scaling"), (d_verts, d_deform, d_rot, d_scl), (p.grad for p in x)):
        err = float((got - want).abs().max())
        assert err <= 1e-12, (name, err)
    # ---- Huber
    H, W = 5, 7
    img, gt = 0.3 * rn(3, H, W), 0.3 * rn(3, H, W)
    mask = torch.rand(1, H, W, generator=g, dtype=torch.float64)
    for m in (mask, None):
        i = img.clone().requires_grad_(True)
        R.huber_loss(i, gt, m)[0].backward()
        d = img - gt
        hp = lambda v: torch.where(v.abs() < R.ALPHA, v, R.ALPHA * torch.sign(v))  # noqa: E731
        want = hp(d) if m is None else hp(d) + R.MASK_WEIGHT * m * hp(m * d)
        assert float((i.grad - want / d.numel()).abs().max()) <= 1e-12


# ------------------------------------------------------------------ the C ABI
def test_abi_keeps_the_descriptors_and_adds_the_mode_and_the_huber_config():
    from fateavatar_amd import _lib
    assert _lib.FR_BIND_DEFORM == 4
    assert (_lib.FR_BIND_SHELL, _lib.FR_BIND_FACE_LOCAL, _lib.FR_BIND_PHONG) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "fr_rasterizer.h")).read()
    assert "#define FR_BIND_DEFORM 4" in header and "flashavatar.py" in header and "unassigned" in header
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu %zu\n", sizeof(fr_binding), offsetof(fr_binding, mode), offsetof(fr_binding, local_xyz), sizeof(fr_binding_phong));
 printf("%zu %zu %zu %zu\n", sizeof(fr_aux), offsetof(fr_aux, d_local_xyz), offsetof(fr_aux, d_verts), offsetof(fr_aux, planes));
 printf("%zu %zu %zu %d\n", sizeof(fr_huber_config), offsetof(fr_huber_config, alpha), offsetof(fr_huber_config, mask_weight), FR_BIND_DEFORM);
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    B, A, Hc = _lib.fr_binding, _lib.fr_aux, _lib.fr_huber_config
    assert out == [C.sizeof(B), B.mode.offset, B.local_xyz.offset, C.sizeof(_lib.fr_binding_phong),
                   C.sizeof(A), A.d_local_xyz.offset, A.d_verts.offset, A.planes.offset,
                   C.sizeof(Hc), Hc.alpha.offset, Hc.mask_weight.offset, 4]
    # the sizes and offsets the descriptors had before this mode (LP64)
    assert out[:8] == [104, 88, 96, 128, 120, 72, 32, 112]
    assert [n for n, _ in B._fields_][-2:] == ["mode", "local_xyz"]
    assert [n for n, _ in Hc._fields_] == ["alpha", "mask_weight"]


def test_new_symbols_are_declared_exported_and_listed():
    from fateavatar_amd import _lib
    header = open(os.path.join(ROOT, "include", "fr_rasterizer.h")).read()
    for sym in ("fr_bind_backward_deform", "fr_huber_workspace_bytes", "fr_huber_loss_grad"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym) and sym + "(" in header
    assert _lib.lib().fr_huber_workspace_bytes() >= 17 * 128 + 2 * 1024 * 4


def test_validation_refuses_bad_deform_descriptors_before_anything_is_enqueued():
    """No GPU: every call below fails its argument check, which runs in front of the first HIP call."""
    from fateavatar_amd import _lib
    L = _lib.lib()
    one = 0x1000      # any non-null "pointer": never dereferenced
    needed = ("face_index", "bary", "local_xyz", "rotation", "scaling")

    def desc(without=None, mode=_lib.FR_BIND_DEFORM):
        b = _lib.fr_binding()
        b.N, b.V, b.F = 4, 3, 1
        b.verts = b.faces = one
        b.mode = mode
        for n in needed:
            if n != without:
                setattr(b, n, one)
        return b

    for n in needed:
        b = desc(without=n)
        assert L.fr_bind_forward(C.byref(b), one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT, n
        assert "FR_BIND_DEFORM" in _lib.last_error(), n
        assert L.fr_bind_backward_deform(C.byref(b), None, None, None, None, one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT, n
        # ... and as a frame's binding
        b.N = 5
        aux = _lib.fr_aux()
        aux.binding = C.pointer(b)
        prm = _lib.fr_params(P=5, D=0, M=1, W=16, H=16, tan_fovx=0.5, tan_fovy=0.5, scale_modifier=1.0,
                             flags=_lib.FR_FLAG_RAW_ACTIVATIONS, aux=C.pointer(aux))
        inp = _lib.fr_inputs(background=one, means3D=one, shs=one, opacities=one, scales=one, rotations=one, viewmatrix=one,
                             projmatrix=one, campos=one)
        g = _lib.fr_grads()
        assert L.fr_backward(C.c_void_p(one), C.byref(prm), C.byref(inp), one, one, one, one, one, C.byref(g), None) == \
            _lib.FR_ERR_INVALID_ARGUMENT, n
        assert "FR_BIND_DEFORM" in _lib.last_error(), n
    # each backward entry point refuses the other modes' descriptors
    b = desc()
    for name in ("fr_bind_backward", "fr_bind_backward_local", "fr_bind_backward_phong"):
        assert getattr(L, name)(C.byref(b), None, None, None, None, None, None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT, name
    shell = desc(mode=_lib.FR_BIND_SHELL)
    shell.offset = one
    local = desc(mode=_lib.FR_BIND_FACE_LOCAL)
    phong = _lib.fr_binding_phong()
    pb = phong.as_binding()
    pb.N, pb.V, pb.F, pb.mode = 4, 3, 1, _lib.FR_BIND_PHONG
    pb.verts = pb.faces = pb.face_index = pb.bary = pb.local_xyz = pb.rotation = pb.scaling = one
    phong.vert_normals = phong.vert_quats = phong.face_ratio = one
    for other in (shell, local, pb):
        assert L.fr_bind_backward_deform(C.byref(other), None, None, None, None, None, None, None, None) == \
            _lib.FR_ERR_INVALID_ARGUMENT, other.mode
        assert "FR_BIND_DEFORM" in _lib.last_error()
    # mode 3 is still unknown
    b.mode = 3
    assert L.fr_bind_forward(C.byref(b), one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "mode" in _lib.last_error()
    assert L.fr_bind_backward_deform(C.byref(b), None, None, None, None, None, None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT


def test_huber_launch_refuses_its_bad_arguments():
    from fateavatar_amd import _lib
    L = _lib.lib()
    one = 0x1000
    cfg = _lib.fr_huber_config(0.1, 40.0)
    good = [C.byref(cfg), 3, 4, 4, one, one, None, None, one, one]
    for k in (0, 4, 5, 8, 9):             # cfg, img, gt, loss, workspace
        bad = list(good)
        bad[k] = None
        assert L.fr_huber_loss_grad(*bad, None) == _lib.FR_ERR_INVALID_ARGUMENT, k
        assert "fr_huber_loss_grad" in _lib.last_error()
    for alpha in (0.0, -0.1, float("nan")):
        bad = list(good)
        bad[0] = C.byref(_lib.fr_huber_config(alpha, 40.0))
        assert L.fr_huber_loss_grad(*bad, None) == _lib.FR_ERR_INVALID_ARGUMENT, alpha
        assert "alpha" in _lib.last_error()
    bad = list(good)
    bad[4] = one + 4                      # the float4 walk needs 16-byte alignment
    assert L.fr_huber_loss_grad(*bad, None) == _lib.FR_ERR_INVALID_ARGUMENT
    # n == 0 launches nothing: accepted without a device
    empty = list(good)
    empty[1] = 0
    assert L.fr_huber_loss_grad(*empty, None) == _lib.FR_OK


# ------------------------------------------------------------------ the host side of the model
def test_describe_writes_the_deform_pointer_into_local_xyz():
    from fateavatar_amd import _lib
    from fateavatar_amd.binding import DEFORM, _check_shapes, _describe
    N = 6
    verts, faces, fi = torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    deform, rot, scl, bary = torch.zeros(N, 10), torch.zeros(N, 4), torch.zeros(N, 3), torch.zeros(N, 3)
    b = _describe(DEFORM, verts, faces, fi, deform, rot, scl, bary)
    assert isinstance(b, _lib.fr_binding) and b.mode == _lib.FR_BIND_DEFORM == DEFORM.value
    assert (b.N, b.V, b.F) == (N, 5, 2)
    assert b.local_xyz == deform.data_ptr() and b.bary == bary.data_ptr()
    assert b.rotation == rot.data_ptr() and b.scaling == scl.data_ptr() and b.face_index == fi.data_ptr()
    assert b.offset is None and b.face_scale_canonical is None and b.shell_len == 0.0 and b.resize_scale == 0
    assert DEFORM.grad_shape(N) == (N, 10) and DEFORM.grad == "d_local_xyz" and DEFORM.backward == "fr_bind_backward_deform"
    assert DEFORM.verts_grad and DEFORM.reads_bary and not DEFORM.active_sh
    _check_shapes("t", DEFORM.shapes, DEFORM, verts, faces, fi, deform, rot, scl, bary)
    with pytest.raises(RuntimeError, match=r"deform \[N,10\]"):
        _check_shapes("t", DEFORM.shapes, DEFORM, verts, faces, fi, torch.zeros(N, 3), rot, scl, bary)


def test_grad_shape_serves_any_width():
    from fateavatar_amd.binding import FACE_LOCAL, PHONG, SHELL
    assert SHELL.grad_shape(7) == (7,) and FACE_LOCAL.grad_shape(7) == (7, 3) and PHONG.grad_shape(7) == (7, 3)
    assert SHELL._replace(own_cols=5).grad_shape(4) == (4, 5)


def test_deform_binding_names_its_mode_and_a_holder_without_deform_is_refused():
    from fateavatar_amd.binding import DEFORM
    from fateavatar_amd.bound import DeformBinding, render_bound_batch
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    db = DeformBinding(faces, torch.zeros(4, dtype=torch.int32), torch.full((4, 3), 1 / 3))
    assert db.mode is DEFORM and DeformBinding._fields == ("faces", "face_index", "bary_coords")
    assert db.describe_args() == (db.bary_coords,)

    class NoDeform:   # a FateAvatar-style holder: an offset, no MLP outputs
        max_sh_degree = 0
        _offset = torch.zeros(4, 1)
        _rotation, _scaling, _opacity = torch.zeros(4, 4), torch.zeros(4, 3), torch.zeros(4, 1)
        get_features = torch.zeros(4, 1, 3)
    with pytest.raises(RuntimeError, match="_deform"):
        render_bound_batch([object()], NoDeform(), [torch.zeros(3, 3)], db, torch.ones(3))


def test_flash_gaussians_fields_shapes_and_initial_values():
    """_register_init_gaussian (flashavatar.py:196-219) in the group order of train/optim.py:45-51."""
    from fateavatar_amd.flash import FlashGaussians
    N, F = 37, 11
    g = torch.Generator().manual_seed(2)
    fi = torch.randint(0, F, (N,), generator=g)
    bary = torch.rand(N, 3, generator=g)
    bary = bary / bary.sum(1, keepdim=True)
    pc = FlashGaussians(fi, bary, -4.5, "cpu")
    assert [n for n, _ in pc.FIELDS] == ["_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling"]
    assert pc.max_sh_degree == 3 and pc.active_sh_degree == 0 and pc.P == N and pc.fused_activations
    assert torch.equal(pc.face_index, fi.to(torch.int32)) and torch.equal(pc.bary_coords, bary)
    shapes = {"_opacity": (N, 1), "_features_dc": (N, 1, 3), "_features_rest": (N, 15, 3), "_rotation": (N, 4), "_scaling": (N, 3)}
    off = 0
    for name, w in pc.FIELDS:
        p = getattr(pc, name)
        assert tuple(p.shape) == shapes[name] and p.requires_grad and p.numel() == N * w
        assert p.data_ptr() == pc.flat.data_ptr() + 4 * off          # one flat buffer, fields in group order
        assert p._fr_grad_out.buf.data_ptr() == pc.flat_grad.data_ptr() + 4 * off
        off += p.numel()
    assert off == pc.flat.numel() == pc.flat_grad.numel() == N * 56
    assert float(pc._features_dc.detach().abs().max()) == 0 and float(pc._features_rest.detach().abs().max()) == 0
    assert torch.equal(pc._rotation.detach(), torch.tensor([[1.0, 0, 0, 0]]).expand(N, 4))
    assert torch.allclose(torch.sigmoid(pc._opacity.detach()), torch.full((N, 1), 0.1), atol=1e-7)
    assert torch.equal(pc._scaling.detach(), torch.full((N, 3), -4.5))
    verts = torch.randn(9, 3, generator=g)
    faces = torch.randint(0, 9, (F, 3), generator=g)
    pts = pc.canonical_points(verts, faces)
    assert torch.allclose(pts, (verts[faces[fi]] * bary.unsqueeze(-1)).sum(1))


def test_flash_step_groups_are_the_references():
    """train/optim.py:45-51 with config/flashavatar.yaml:22-25.  (The constructor allocates device state; the groups only need
    the holder and the rates.)"""
    from fateavatar_amd.flash import FLASH_LRS, FlashGaussians, FlashStep
    N = 21
    assert FLASH_LRS == dict(opacity=0.05, feature_dc=0.0025, feature_rest=0.0025 / 20, rotation=0.001, scaling=0.005)
    st = FlashStep.__new__(FlashStep)
    st.pc, st.lr = FlashGaussians(torch.zeros(N, dtype=torch.int64), torch.full((N, 3), 1 / 3), -4.0, "cpu"), dict(FLASH_LRS)
    assert st.adam_segments() == [(N * 1, 0.05), (N * 3, 0.0025), (N * 45, 0.0025 / 20), (N * 4, 0.001), (N * 3, 0.005)]
    assert sum(n for n, _ in st.adam_segments()) == st.pc.flat.numel()
    assert FlashStep.GAUSSIAN_ATTRIBUTES == ["_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "face_index",
                                             "bary_coords"]


def test_huber_loss_and_grad_has_no_cpu_path():
    from fateavatar_amd.loss import REFERENCE_HUBER_LOSS, HuberLoss, huber_loss_and_grad
    assert REFERENCE_HUBER_LOSS == HuberLoss(0.1, 40.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        huber_loss_and_grad(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
