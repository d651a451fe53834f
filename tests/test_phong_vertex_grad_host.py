"""CPU: the vertex gradient of SplattingAvatar's Phong-surface binding (model/baseline/splattingavatar.py:203-246) — the
reference every GPU test of tests/test_gpu_phong_vertex_grad.py is held to (tests/phong_ref.py in float64 under torch autograd,
`verts` the leaf) against central differences, the argument checks of the two new entry points, and the new opt-in names."""
import ctypes as C
import inspect
import os

import numpy as np
import torch

from tests import phong_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loss_of_verts(cano, faces, fi, bary, uvd, rot, scl, w):
    """verts -> sum(w . bound values) through `mesh_frame` + `phong_bind`, everything float64."""
    def loss(verts):
        out = P.phong_bind(verts, faces, fi, bary, P.mesh_frame(cano, faces, verts), uvd, rot, scl)
        return sum((o * g).sum() for o, g in zip(out, w))
    return loss


def test_reference_vertex_gradient_agrees_with_central_differences():
    """On `turned_mesh()` (well posed: asserted first) float64 autograd of d_verts agrees with central differences (h = 1e-6) at
    five coordinates, the last vertex — which has exactly one face — among them, to 1e-6 relative.  Measured: <= 1e-7."""
    cano, verts, faces, fi, bary = P.turned_mesh()
    P.assert_turned_mesh_is_well_posed(cano, verts, faces)
    rng = np.random.default_rng(5)
    N, V = fi.shape[0], verts.shape[0]
    t = lambda a: torch.from_numpy(np.asarray(a)).double() if np.asarray(a).dtype.kind == "f" else torch.from_numpy(np.asarray(a))  # noqa: E731
    uvd, rot, scl = (t(0.05 * rng.normal(size=(N, 3))), t(rng.normal(size=(N, 4))), t(rng.normal(size=(N, 3))))
    w = [t(rng.normal(size=s)) for s in ((N, 3), (N, 4), (N, 3))]
    loss = _loss_of_verts(t(cano), t(faces), t(fi), t(bary), uvd, rot, scl, w)
    v = t(verts).requires_grad_(True)
    loss(v).backward()
    g = v.grad
    assert bool(torch.isfinite(g).all())
    h = 1e-6
    coords = [(V - 1, 0), (V - 1, 2), (0, 1), (int(faces[0, 1]), 0), (V // 2, 2)]
    assert int((faces == V - 1).sum()) == 1
    for i, c in coords:
        with torch.no_grad():
            vp, vm = v.detach().clone(), v.detach().clone()
            vp[i, c] += h
            vm[i, c] -= h
            fd = float((loss(vp) - loss(vm)) / (2 * h))
        rel = abs(fd - float(g[i, c])) / max(abs(fd), 1e-300)
        print(f"d_verts[{i},{c}]: autograd {float(g[i, c]):.9e}, central difference {fd:.9e}, rel {rel:.2e}")
        assert abs(fd) > 0 and rel <= 1e-6, (i, c, rel)


def test_new_entry_points_are_declared_exported_and_listed():
    from fateavatar_amd import _lib
    header = open(os.path.join(ROOT, "include", "fr_rasterizer.h")).read()
    for sym in ("fr_bind_backward_phong_frame", "fr_phong_frame_backward", "fr_phong_frame_backward_workspace_bytes"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym) and sym + "(" in header
    # the refusal of the frame's own backward stays in the header
    assert "fr_aux::d_verts" in header and "FR_ERR_INVALID_ARGUMENT" in header
    assert "fr_phong_grad" in open(os.path.join(ROOT, "fateavatar_amd", "csrc", "Makefile")).read().split("STRICT_UNITS :=")[1].split("\n")[0]
    L = _lib.lib()
    assert L.fr_phong_frame_backward_workspace_bytes(5023, 10006) == 5023 * 7 * 4
    assert L.fr_phong_frame_backward_workspace_bytes(0, 0) == 0


def test_validation_refuses_bad_arguments_before_anything_is_enqueued():
    """No GPU: every call below fails its argument check, which runs in front of the first HIP call."""
    from fateavatar_amd import _lib
    L = _lib.lib()
    one = 0x1000      # any non-null "pointer": never dereferenced
    # ---- fr_phong_frame_backward: V, F, six mesh arrays, three upstream gradients (optional), d_verts, workspace
    args = [3, 1] + [one] * 11
    for k in range(2, 8):                                   # a NULL among the required mesh arrays
        bad = list(args)
        bad[k] = None
        assert L.fr_phong_frame_backward(*bad, None) == _lib.FR_ERR_INVALID_ARGUMENT, k
        assert "fr_phong_frame_backward" in _lib.last_error() and "null mesh array" in _lib.last_error()
    for k, word in ((11, "d_verts"), (12, "workspace")):
        bad = list(args)
        bad[k] = None
        assert L.fr_phong_frame_backward(*bad, None) == _lib.FR_ERR_INVALID_ARGUMENT, k
        assert word in _lib.last_error()
    assert L.fr_phong_frame_backward(-1, 1, *[one] * 11, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "negative" in _lib.last_error()
    assert L.fr_phong_frame_backward(3, -1, *[one] * 11, None) == _lib.FR_ERR_INVALID_ARGUMENT
    # ---- fr_bind_backward_phong_frame: a mode other than FR_BIND_PHONG, and an incomplete Phong descriptor
    p = _lib.fr_binding_phong()
    b = p.as_binding()
    b.N, b.V, b.F = 4, 3, 1
    b.verts = b.faces = b.face_index = b.rotation = b.scaling = b.bary = b.local_xyz = b.offset = one
    p.vert_normals = p.vert_quats = p.face_ratio = one
    for mode in (_lib.FR_BIND_SHELL, _lib.FR_BIND_FACE_LOCAL, _lib.FR_BIND_DEFORM):
        b.mode = mode
        assert L.fr_bind_backward_phong_frame(C.byref(b), one, one, one, one, one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT, mode
        assert "fr_bind_backward_phong_frame" in _lib.last_error() and "FR_BIND_PHONG" in _lib.last_error()
    b.mode = 3
    assert L.fr_bind_backward_phong_frame(C.byref(b), one, one, one, one, one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "mode" in _lib.last_error()
    b.mode, p.vert_quats = _lib.FR_BIND_PHONG, None
    assert L.fr_bind_backward_phong_frame(C.byref(b), one, one, one, one, one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "FR_BIND_PHONG" in _lib.last_error()
    assert L.fr_bind_backward_phong_frame(None, one, one, one, one, one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT
    # the old entry point keeps refusing a vertex gradient
    p.vert_quats = one
    assert L.fr_bind_backward_phong(C.byref(b), None, None, None, one, one, one, one, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "vertex gradient" in _lib.last_error()


def test_the_capability_arrives_under_new_opt_in_names():
    from fateavatar_amd.binding import PhongGradBuffers, phong_frame, phong_frame_backward  # noqa: F401
    from fateavatar_amd.bound import PhongBinding, PosedPhongBinding
    from fateavatar_amd.splatting import SplattingStep
    sig = inspect.signature(phong_frame)
    assert list(sig.parameters) == ["canonical", "verts", "differentiable"] and sig.parameters["differentiable"].default is False
    sig = inspect.signature(SplattingStep.__init__)
    assert sig.parameters["mesh_grad"].default is False and sig.parameters["vertex_grad"].default is False
    assert PosedPhongBinding._fields == PhongBinding._fields == ("faces", "face_index", "bary_coords", "canonical")
    assert PosedPhongBinding.mode is PhongBinding.mode
    assert SplattingStep.VERTEX_GRAD is False and "mesh_grad" in SplattingStep.VERTEX_GRAD_MISSING
