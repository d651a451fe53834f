"""The stand-alone binding op of every mode with gradient slots (`rasterizer.GradOut`) on its parameters: the one autograd
Function behind `bind_gaussians`, `bind_gaussians_face_local` and `bind_gaussians_phong`."""
import numpy as np
import pytest

from tests import phong_ref

pytestmark = pytest.mark.gpu

V, F, N = 40, 64, 160       # two full waves and a part wave; several Gaussians share each face


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("mode", ["shell", "face_local", "phong"])
def test_op_writes_the_first_gradient_into_the_slots_and_adds_the_second(gpu_device, mode):
    """Two calls of the public op on leaves that carry `_fr_grad_out` slots, the second without clearing `.grad`, against the
    same two calls on plain leaves (`.grad` cleared in between).  The gradients of the own parameter, rotation and scaling are
    per-lane stores: compared bit for bit.  d_verts is summed by float atomics: rel-L2 < 5e-5, the bound
    test_gpu_face_local.py holds the vertex gradient to where two runs differ by summation order only."""
    import torch
    from fateavatar_amd import binding
    from fateavatar_amd.rasterizer import GradOut
    dev = gpu_device
    cano, posed, faces, face_index, bary = (torch.from_numpy(a).to(dev) for a in phong_ref.turned_mesh(V=V, F=F, N=N))
    gen = torch.Generator().manual_seed(11)
    own_shape = (N, 1) if mode == "shell" else (N, 3)
    raw = [(0.3 * torch.randn(s, generator=gen)).to(dev) for s in (own_shape, (N, 4), (N, 3))]
    weights = [[torch.randn(s, generator=gen).to(dev) for s in ((N, 3), (N, 4), (N, 3))] for _ in range(2)]
    if mode == "shell":
        canon = binding.face_scale(cano, faces)
        op = lambda v, o, r, s: binding.bind_gaussians(v, faces, face_index, bary, canon, o, r, s, 0.05, True)  # noqa: E731
    elif mode == "face_local":
        op = lambda v, o, r, s: binding.bind_gaussians_face_local(v, faces, face_index, o, r, s)  # noqa: E731
    else:
        frame = binding.phong_frame(binding.phong_canonical(cano, faces), posed)
        op = lambda v, o, r, s: binding.bind_gaussians_phong(v, faces, face_index, bary, frame, o, r, s)  # noqa: E731
    verts_grad = mode != "phong"

    def leaves():
        return posed.clone().requires_grad_(verts_grad), [t.clone().requires_grad_(True) for t in raw]

    def backward(v, params, w):
        torch.autograd.backward(list(op(v, *params)), w)
        torch.cuda.synchronize()

    # plain leaves, one gradient per call
    want, want_v = [], []
    for w in weights:
        v, params = leaves()
        backward(v, params, w)
        want.append([p.grad.clone() for p in params])
        want_v.append(v.grad.clone() if verts_grad else None)
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in want[-1])
    assert not torch.equal(want[0][1], want[1][1])            # (the two calls have different gradients)

    # leaves with slots: views into one flat gradient buffer
    v, params = leaves()
    flat = torch.full((sum(p.numel() for p in params),), float("nan"), device=dev)
    off = 0
    for p in params:
        p._fr_grad_out = GradOut(flat[off:off + p.numel()].view(p.shape))
        off += p.numel()
    backward(v, params, weights[0])
    for name, p, g in zip(("own", "rotation", "scaling"), params, want[0]):
        assert p.grad.data_ptr() == p._fr_grad_out.buf.data_ptr(), name      # 1. written in place, adopted without a copy
        assert p.grad.shape == p.shape, name                                 # 3. the shell's d_offset is [N,1] again
        assert torch.equal(p._fr_grad_out.buf, g), name
    backward(v, params, weights[1])                                          # 2. `.grad` not cleared: a fresh tensor, added
    for name, p, g1, g2 in zip(("own", "rotation", "scaling"), params, *want):
        assert p.grad.data_ptr() == p._fr_grad_out.buf.data_ptr(), name
        assert torch.equal(p.grad, g1 + g2), name
    if verts_grad:
        err = _rel(v.grad, want_v[0] + want_v[1])
        print(f"{mode}: d_verts of two backwards, rel-L2 {err:.3e}")
        assert err < 5e-5 and float(v.grad.abs().max()) > 0
    else:
        assert v.grad is None
    assert np.isfinite(flat.cpu().numpy()).all()                             # every element of every slot was written
