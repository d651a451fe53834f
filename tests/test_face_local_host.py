"""CPU: GaussianAvatars' face-local binding (model/baseline/gaussianavatars.py:144-171) — the torch restatement every GPU
test is held to (tests/face_local_ref.py) against the golden mesh vectors and against finite differences, the C ABI of the
new mode, and the host side of `RiggedGaussians` / `RiggedStep` / `render_bound_batch`."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.face_local_ref import face_local_bind, matrix_to_quaternion, quaternion_candidates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "golden_binding.npz"))


def test_restatement_on_the_golden_meshes_is_finite_and_places_xyz_as_the_fixture_says():
    """Every output finite on the golden meshes (degenerate face included), and xyz = orientation @ local * scale + centre
    with the FIXTURE's orientation and scale, evaluated in float64 numpy.  Bound: the float32 evaluation rounds three
    products, two additions, the scale product and the centre's two additions, division and final addition — at most
    8 roundings of 2^-24 relative to the magnitudes summed, (|R| |local|) s + |c|."""
    faces = torch.from_numpy(G["faces"])
    F = faces.shape[0]
    rng = np.random.default_rng(3)
    binding = np.concatenate([np.arange(F), rng.integers(0, F, 3 * F)]).astype(np.int32)   # every face, the degenerate one too
    N = binding.shape[0]
    local = rng.normal(size=(N, 3)).astype(np.float32)
    rot = rng.normal(size=(N, 4)).astype(np.float32)
    scl = rng.normal(size=(N, 3)).astype(np.float32)
    for b in range(G["verts"].shape[0]):
        verts = torch.from_numpy(G["verts"][b])
        xyz, r, s = face_local_bind(verts, faces, torch.from_numpy(binding), torch.from_numpy(local), torch.from_numpy(rot),
                                    torch.from_numpy(scl))
        assert xyz.dtype == torch.float32
        for t in (xyz, r, s):
            assert bool(torch.isfinite(t).all())
        R = G["orientation"][b].astype(np.float64)[binding]                  # [N,3,3]
        sc = G["scale"][b].astype(np.float64)[binding]                       # [N,1]
        tri = G["verts"][b].astype(np.float64)[G["faces"].astype(np.int64)[binding]]   # [N,3,3]
        centre = tri.mean(axis=1)
        want = np.einsum("nij,nj->ni", R, local.astype(np.float64)) * sc + centre
        mag = np.einsum("nij,nj->ni", np.abs(R), np.abs(local).astype(np.float64)) * sc + np.abs(tri).sum(axis=1) / 3
        err = np.abs(xyz.numpy().astype(np.float64) - want)
        assert (err <= 8 * 2.0 ** -24 * mag + 1e-300).all(), float((err / np.maximum(mag, 1e-300)).max())


def test_helper_quaternion_conversion_is_the_oracles_with_a_finite_backward():
    """The helper's matrix_to_quaternion: oracle.binding's forward bit for bit (golden meshes, the posed head template), the
    oracle's gradient wherever that is finite, and a finite (zero-subgradient) one where the oracle's where/sqrt form is NaN."""
    from fateavatar_amd import insta
    from oracle import binding as B
    meshes = [(G["verts"][b], G["faces"]) for b in range(G["verts"].shape[0])]
    _, posed, faces = insta.synthetic_sequence(3, 64, 0)
    meshes += [(posed[k], faces) for k in range(3)]
    n_nan = 0
    for verts, f in meshes:
        R = B.face_orientation(torch.from_numpy(verts), torch.from_numpy(f))[0]
        assert torch.equal(matrix_to_quaternion(R), B.matrix_to_quaternion(R))
        w = torch.from_numpy(np.random.default_rng(1).normal(size=(R.shape[0], 4)).astype(np.float32))
        grads = []
        for fn in (matrix_to_quaternion, B.matrix_to_quaternion):
            Rg = R.clone().requires_grad_(True)
            (fn(Rg) * w).sum().backward()
            grads.append(Rg.grad)
        assert bool(torch.isfinite(grads[0]).all())
        ok = torch.isfinite(grads[1]).all(-1).all(-1)
        n_nan += int((~ok).sum())
        assert torch.equal(grads[0][ok], grads[1][ok])
    assert n_nan > 0        # (the reason the helper exists: the template does hold such faces)


def _random_mesh(seed, V=40, F=64, N=160):
    rng = np.random.default_rng(seed)
    verts = rng.normal(size=(V, 3))
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int64)
    binding = np.concatenate([np.arange(F), rng.integers(0, F, N - F)]).astype(np.int64)
    return verts, faces, binding, rng.normal(size=(N, 3)), rng.normal(size=(N, 4)), rng.normal(size=(N, 3)), rng


def test_restatement_gradients_agree_with_central_finite_differences():
    """float64 autograd of the restatement against central differences (h = 1e-6: truncation ~h^2, rounding ~1e-16 / h)
    to 1e-6 relative, for verts, local_xyz, rotation and scaling, on a seeded mesh whose faces use all four candidates of
    matrix_to_quaternion.  This pins the torch autograd the GPU gradients are compared with."""
    verts, faces, binding, local, rot, scl, rng = _random_mesh(11)
    faces_t, binding_t = torch.from_numpy(faces), torch.from_numpy(binding)
    used = np.bincount(quaternion_candidates(torch.from_numpy(verts), faces_t).numpy(), minlength=4)
    assert (used > 0).all(), used
    w = [rng.normal(size=s) for s in ((binding.shape[0], 3), (binding.shape[0], 4), (binding.shape[0], 3))]

    def loss(v, l, r, s):
        out = face_local_bind(v, faces_t, binding_t, l, r, s)
        return sum((o * torch.from_numpy(wk)).sum() for o, wk in zip(out, w))

    x = [torch.from_numpy(a.copy()).requires_grad_(True) for a in (verts, local, rot, scl)]
    loss(*x).backward()
    h = 1e-6
    for k, name in enumerate(("verts", "local_xyz", "rotation", "scaling")):
        base = [t.detach().clone() for t in x]
        fd = np.zeros(base[k].numel())
        flat = base[k].view(-1)
        for i in range(flat.numel()):
            keep = float(flat[i])
            flat[i] = keep + h
            up = float(loss(*base))
            flat[i] = keep - h
            dn = float(loss(*base))
            flat[i] = keep
            fd[i] = (up - dn) / (2 * h)
        got = x[k].grad.numpy().reshape(-1)
        rel = np.linalg.norm(got - fd) / np.linalg.norm(fd)
        print(f"{name}: rel-L2 of autograd against finite differences {rel:.3e}")
        assert rel <= 1e-6, (name, rel)


# ------------------------------------------------------------------ the C ABI of the mode
def test_abi_has_the_mode_fields_with_the_c_compilers_layout():
    from fateavatar_amd import _lib
    assert _lib.FR_BIND_SHELL == 0 and _lib.FR_BIND_FACE_LOCAL == 1
    names = [n for n, _ in _lib.fr_binding._fields_]
    assert names[-2:] == ["mode", "local_xyz"]                       # appended: the fields in front keep their offsets
    aux_names = [n for n, _ in _lib.fr_aux._fields_]
    assert aux_names.index("d_local_xyz") == aux_names.index("overflow_out") + 1   # behind the binding's other members
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "fr_rasterizer.h"
int main(void){
 printf("%zu %zu %zu %zu\n", sizeof(fr_binding), offsetof(fr_binding, scaling), offsetof(fr_binding, mode), offsetof(fr_binding, local_xyz));
 printf("%zu %zu %zu %zu\n", sizeof(fr_aux), offsetof(fr_aux, planes), offsetof(fr_aux, d_local_xyz), offsetof(fr_aux, overflow_out));
 printf("%d %d\n", FR_BIND_SHELL, FR_BIND_FACE_LOCAL);
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert out[:4] == [C.sizeof(_lib.fr_binding), _lib.fr_binding.scaling.offset, _lib.fr_binding.mode.offset,
                       _lib.fr_binding.local_xyz.offset]
    assert out[4:8] == [C.sizeof(_lib.fr_aux), _lib.fr_aux.planes.offset, _lib.fr_aux.d_local_xyz.offset,
                        _lib.fr_aux.overflow_out.offset]
    assert out[8:] == [_lib.FR_BIND_SHELL, _lib.FR_BIND_FACE_LOCAL]
    assert _lib.fr_binding().mode == _lib.FR_BIND_SHELL              # a zeroed descriptor is a shell binding


def test_new_symbol_is_declared_exported_and_listed():
    from fateavatar_amd import _lib
    assert "fr_bind_backward_local" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "fr_bind_backward_local")
    assert "fr_bind_backward_local(" in open(os.path.join(ROOT, "include", "fr_rasterizer.h")).read()


def test_validation_refuses_bad_face_local_descriptors_before_anything_is_enqueued():
    """No GPU: every call below fails its argument check, which runs in front of the first HIP call."""
    from fateavatar_amd import _lib
    L = _lib.lib()
    one = 0x1000      # any non-null "pointer": never dereferenced
    b = _lib.fr_binding()
    b.N, b.V, b.F = 4, 3, 1
    b.verts = b.faces = b.face_index = b.rotation = b.scaling = one
    b.mode = _lib.FR_BIND_FACE_LOCAL
    assert L.fr_bind_forward(C.byref(b), one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "local_xyz" in _lib.last_error()
    b.local_xyz, b.mode = one, 7
    assert L.fr_bind_forward(C.byref(b), one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "mode" in _lib.last_error()
    b.mode = _lib.FR_BIND_SHELL            # the shell binding's own entry point does not take a face-local one, and back
    assert L.fr_bind_backward_local(C.byref(b), None, None, None, None, None, None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT
    b.mode = _lib.FR_BIND_FACE_LOCAL
    assert L.fr_bind_backward(C.byref(b), None, None, None, None, None, None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT
    # a frame rendered from the binding: N != P
    aux = _lib.fr_aux()
    aux.binding = C.pointer(b)
    prm = _lib.fr_params(P=5, D=0, M=1, W=16, H=16, tan_fovx=0.5, tan_fovy=0.5, scale_modifier=1.0,
                         flags=_lib.FR_FLAG_RAW_ACTIVATIONS, aux=C.pointer(aux))
    inp = _lib.fr_inputs(background=one, means3D=one, shs=one, opacities=one, scales=one, rotations=one, viewmatrix=one,
                         projmatrix=one, campos=one)
    h = C.c_void_p(one)
    cnt = _lib.fr_counts()
    assert L.fr_forward(h, C.byref(prm), C.byref(inp), one, one, one, one, one, 1024, C.byref(cnt), None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "N must equal P" in _lib.last_error()


# ------------------------------------------------------------------ the host side of the rigged model
def test_rigged_gaussians_fields_shapes_and_initial_values():
    """_register_init_gaussian (gaussianavatars.py:97-120) in the group order of train/optim.py:73-80."""
    from fateavatar_amd.rigged import RiggedGaussians
    F = 37
    pc = RiggedGaussians.one_per_face(F, "cpu")
    assert [n for n, _ in pc.FIELDS] == ["_xyz", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling"]
    assert pc.max_sh_degree == 3 and pc.active_sh_degree == 0 and pc.P == F
    assert torch.equal(pc.binding, torch.arange(F, dtype=torch.int32))
    shapes = {"_xyz": (F, 3), "_opacity": (F, 1), "_features_dc": (F, 1, 3), "_features_rest": (F, 15, 3), "_rotation": (F, 4),
              "_scaling": (F, 3)}
    off = 0
    for name, w in pc.FIELDS:
        p = getattr(pc, name)
        assert tuple(p.shape) == shapes[name] and p.requires_grad and p.numel() == F * w
        assert p.data_ptr() == pc.flat.data_ptr() + 4 * off          # one flat buffer, fields in group order
        assert p._fr_grad_out.buf.data_ptr() == pc.flat_grad.data_ptr() + 4 * off
        off += p.numel()
    assert off == pc.flat.numel() == pc.flat_grad.numel()
    assert all(float(getattr(pc, n).detach().abs().max()) == 0 for n in ("_xyz", "_scaling", "_features_rest"))
    assert torch.equal(pc._rotation.detach(), torch.tensor([[1.0, 0, 0, 0]]).expand(F, 4))
    assert torch.allclose(torch.sigmoid(pc._opacity.detach()), torch.full((F, 1), 0.1), atol=1e-7)
    dc = pc._features_dc.detach()
    assert float(dc.min()) >= 0 and float(dc.max()) <= 1 / 255.0 and float(dc.std()) > 0     # random colour / 255 (:101)
    assert tuple(pc.get_features.shape) == (F, 16, 3)


def test_rigged_step_groups_are_the_references():
    """train/optim.py:73-80 with config/gaussianavatars.yaml:26-31.  (The constructor allocates device state; the groups
    only need the holder and the rates.)"""
    from fateavatar_amd.rigged import RIGGED_LRS, RiggedGaussians, RiggedStep
    P = 21
    st = RiggedStep.__new__(RiggedStep)
    st.pc, st.lr = RiggedGaussians.one_per_face(P, "cpu"), dict(RIGGED_LRS)
    assert st.adam_segments() == [(P * 3, 0.005), (P * 1, 0.05), (P * 3, 0.0025), (P * 45, 0.0025 / 20), (P * 4, 0.001),
                                  (P * 3, 0.017)]
    assert sum(n for n, _ in st.adam_segments()) == st.pc.flat.numel()


def test_render_bound_batch_refuses_a_face_local_binding_without_local_positions():
    from fateavatar_amd.bound import FaceLocalBinding, MeshBinding, render_bound_batch

    class NoXyz:      # a FateAvatar-style holder: an offset, no local position
        max_sh_degree = 0
        _offset = torch.zeros(4, 1)
        _rotation, _scaling, _opacity = torch.zeros(4, 4), torch.zeros(4, 3), torch.zeros(4, 1)
        get_features = torch.zeros(4, 1, 3)
    fl = FaceLocalBinding(torch.zeros((1, 3), dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="_xyz"):
        render_bound_batch([object()], NoXyz(), [torch.zeros(3, 3)], fl, torch.ones(3))
    # positional use of the shell binding's six fields is what it was
    mb = MeshBinding(1, 2, 3, 4, 0.05)
    assert mb.faces == 1 and mb.shell_len == 0.05 and mb.resize_scale is True and len(mb) == 6
