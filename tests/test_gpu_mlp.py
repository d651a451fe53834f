"""-m gpu: the fused deformation MLP (csrc/fr_mlp.hip, fateavatar_amd/mlp.py) on the device — forward and backward against the
float64 restatement of tests/mlp_ref.py with a bound MEASURED on the float32 restatement, the same bits on every launch and graph
replay, and FlashStep(deformer=...) against the existing route (the torch MLP outside the step).

The bound: the float32 restatement on the CPU has a rel-L2 error e32 against float64 for each of the outputs, d_weights, d_bias
and d_cond; the kernels may have at most 4 x e32 (another summation order: a k-ordered fmaf chain against blocked sums), and
never more than the ceiling 2e-4 tests/test_gpu_flash.py holds its gradients to."""
import functools

import numpy as np
import pytest

from tests import mlp_ref

pytestmark = pytest.mark.gpu

FACTOR, CEILING = 4.0, 2e-4
MASK_Z = 1e-5            # a unit whose ReLU mask differs from float64's has |z| < MASK_Z x the layer's RMS pre-activation
SHAPES = [(51, 59), (51, 109), (51, 8), (3, 0)]       # (De, Dc): the reference's, a full-width input, an odd total, no condition


def _sizes():
    from fateavatar_amd import _lib
    T, chunk = _lib.FR_MLP_POINT_TILE, _lib.FR_MLP_CHUNK
    return [1, T - 1, T, T + 1, 3 * chunk + 5]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _cat(ts):
    import torch
    return torch.cat([t.reshape(-1) for t in ts])


SEED_MARGIN = 1e-6       # the inputs are drawn until no float64 pre-activation lies within this x its layer's RMS of zero


def _keeps_clear_of_zero(W, B, E, cond):
    """Whether every hidden pre-activation of the float64 network is at least SEED_MARGIN x its layer's RMS away from 0."""
    import torch
    with torch.no_grad():
        h = torch.cat([E.double(), cond.double().expand(E.shape[0], cond.shape[0])], dim=1)
        for w, b in zip(W[:-1], B[:-1]):
            z = torch.nn.functional.linear(h, w, b)
            if float(z.abs().min()) < SEED_MARGIN * float(z.pow(2).mean().sqrt()):
                return False
            h = torch.relu(z)
    return True


@functools.lru_cache(maxsize=None)
def _case(De, Dc, L, N):
    """One network and its inputs on the CPU from a seed of the shape, with the float64 and the float32 restatement's results
    (computed once, shared, never modified).  A ReLU's derivative jumps at 0, so a unit that float32 rounding carries across 0
    changes the gradients by far more than rounding: the inputs are re-drawn (next seed) until the FLOAT64 network has no
    pre-activation within SEED_MARGIN x RMS of 0 — ten times the float32 error of a pre-activation (1e-7 x RMS, the `out`
    figures below), decided by the reference alone."""
    import torch
    rng = torch.get_rng_state()
    torch.manual_seed(17 + De + Dc + L)
    net = mlp_ref.RefMLP(De + Dc, 10, hidden_layers=L)
    torch.set_rng_state(rng)
    W = [fc.weight.detach() for fc in net.fcs] + [net.output_linear.weight.detach()]
    B = [fc.bias.detach() for fc in net.fcs] + [net.output_linear.bias.detach()]
    W64, B64 = [w.double() for w in W], [b.double() for b in B]
    for attempt in range(400):
        g = torch.Generator().manual_seed(1000 * De + 10 * Dc + L + 7 * N + 100003 * attempt)
        pts = torch.rand(N, 3, generator=g) * 0.4 - 0.2
        E = mlp_ref.embed(pts) if De == 51 else torch.randn(N, De, generator=g)
        cond = 0.5 * torch.randn(Dc, generator=g)
        d_out = torch.randn(N, 10, generator=g)
        if _keeps_clear_of_zero(W64, B64, E, cond):
            break
    else:
        raise AssertionError("no seed keeps the float64 pre-activations clear of zero")
    r64 = mlp_ref.run(W64, B64, E, cond, d_out)
    r32 = mlp_ref.run(W, B, E, cond, d_out)
    return dict(net=net, E=E.contiguous(), cond=cond, d_out=d_out, r64=r64, r32=r32, attempts=attempt + 1)


def _flipped_units_are_at_zero(masks, z64, who):
    """`masks`: per hidden layer a bool [N,256] (unit is on); every disagreement with float64's sign sits at |z| < MASK_Z x RMS."""
    flips = 0
    for l, (m, z) in enumerate(zip(masks, z64)):
        diff = m != (z > 0)
        flips += int(diff.sum())
        if diff.any():
            worst, rms = float(z[diff].abs().max()), float(z.pow(2).mean().sqrt())
            assert worst < MASK_Z * rms, (who, l, worst, rms)
    return flips


@pytest.mark.parametrize("N", _sizes())
@pytest.mark.parametrize("L", [1, 6, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}+{s[1]}")
def test_forward_and_backward_against_float64(gpu_device, shape, L, N):
    import torch
    from fateavatar_amd.mlp import DeformMLP
    dev = gpu_device
    De, Dc = shape
    c = _case(De, Dc, L, N)
    r64, r32 = c["r64"], c["r32"]
    # the float32 restatement itself keeps its masks (the seed is a fair one)
    _flipped_units_are_at_zero([z > 0 for z in r32["z"]], r64["z"], "float32 restatement")
    mlp = DeformMLP.from_torch(c["net"], c["E"].to(dev), Dc)
    cond = c["cond"].to(dev)
    d_cond = torch.full((Dc,), float("nan"), device=dev)
    out = torch.full((N, 10), float("nan"), device=dev)
    mlp.flat_grad.fill_(float("nan"))                 # every element is to be OVERWRITTEN
    mlp.forward_into(cond, out)
    mlp.backward_from(c["d_out"].to(dev), cond, d_cond)
    torch.cuda.synchronize()
    flips = _flipped_units_are_at_zero([mlp.saved_activation(l).cpu() > 0 for l in range(L)], r64["z"], "kernel")
    got = dict(out=out.cpu(), d_weights=_cat([mlp.grad_weight(i) for i in range(L + 1)]).cpu(),
               d_bias=_cat([mlp.grad_bias(i) for i in range(L + 1)]).cpu(), d_cond=d_cond.cpu())
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    for name, v in got.items():
        if name == "d_cond" and Dc == 0:
            continue
        ref64 = _cat(r64[name]) if isinstance(r64[name], list) else r64[name].reshape(-1)
        ref32 = _cat(r32[name]) if isinstance(r32[name], list) else r32[name].reshape(-1)
        e32, err = _rel(ref32, ref64), _rel(v.reshape(-1), ref64)
        print(f"De={De} Dc={Dc} L={L} N={N} {name}: kernel {err:.3e}  float32 restatement {e32:.3e}  ratio {err / max(e32, 1e-300):.2f}"
              f"  mask flips {flips}")
        assert float(ref64.abs().max()) > 0
        assert err <= FACTOR * e32, (name, err, e32)
        if name != "out":
            assert err <= CEILING, (name, err)
    # per layer, so that a small layer cannot hide behind a large one: the ceiling
    for i in range(L + 1):
        for name, v, ref in (("d_weights", mlp.grad_weight(i), r64["d_weights"][i]), ("d_bias", mlp.grad_bias(i), r64["d_bias"][i])):
            assert _rel(v.cpu(), ref) <= CEILING, (name, i, _rel(v.cpu(), ref))


def test_autograd_op_hands_out_the_same_gradients(gpu_device):
    import torch
    from fateavatar_amd.mlp import DeformMLP
    dev = gpu_device
    c = _case(51, 59, 6, 129)
    mlp = DeformMLP.from_torch(c["net"], c["E"].to(dev), 59)
    cond = c["cond"].to(dev).requires_grad_(True)
    out = mlp(cond)
    assert out.requires_grad and tuple(out.shape) == (129, 10)
    out.backward(c["d_out"].to(dev))
    assert torch.equal(mlp.flat.grad, mlp.flat_grad) and mlp.flat.grad.data_ptr() != mlp.flat_grad.data_ptr()
    assert _rel(cond.grad.cpu(), c["r64"]["d_cond"]) <= CEILING
    assert _rel(out.detach().cpu(), c["r64"]["out"]) <= 1e-5
    with pytest.raises(ValueError, match=r"contiguous \[59\]"):
        mlp(torch.zeros(58, device=dev))
    with pytest.raises(TypeError, match="float32"):
        mlp(torch.zeros(59, device=dev, dtype=torch.float64))


def test_same_bits_on_every_launch_and_replay_and_gradients_are_overwritten(gpu_device):
    import torch
    from fateavatar_amd import _lib
    from fateavatar_amd.mlp import DeformMLP
    dev = gpu_device
    N = 3 * _lib.FR_MLP_CHUNK + 5
    c = _case(51, 59, 6, N)
    mlp = DeformMLP.from_torch(c["net"], c["E"].to(dev), 59)
    cond, d_out = c["cond"].to(dev), c["d_out"].to(dev)

    def run():
        out, d_cond = torch.empty(N, 10, device=dev), torch.empty(59, device=dev)
        mlp.forward_into(cond, out)
        mlp.backward_from(d_out, cond, d_cond)
        return out.clone(), mlp.flat_grad.clone(), d_cond.clone()

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # an eager call and a graph replay
    s_out, s_dc = torch.empty(N, 10, device=dev), torch.empty(59, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mlp.forward_into(cond, s_out)
        mlp.backward_from(d_out, cond, s_dc)
    for _ in range(2):
        s_out.fill_(float("nan"))
        mlp.flat_grad.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, (s_out, mlp.flat_grad, s_dc)):
            assert torch.equal(a, b)
    # d_weights is overwritten, not accumulated into: d_out = 0 gives exact zeros
    d_cond = torch.full((59,), 3.0, device=dev)
    mlp.backward_from(torch.zeros_like(d_out), cond, d_cond)
    assert int((mlp.flat_grad != 0).sum()) == 0 and int((d_cond != 0).sum()) == 0
    # N == 0: nothing is launched, the gradients are zeros
    empty = DeformMLP(torch.zeros(0, 51, device=dev), 59)
    empty.flat_grad.fill_(float("nan"))
    d_cond.fill_(float("nan"))
    out0 = torch.empty(0, 10, device=dev)
    empty.forward_into(cond, out0)
    empty.backward_from(out0, cond, d_cond)
    torch.cuda.synchronize()
    assert int((empty.flat_grad != 0).sum()) == 0 and int((d_cond != 0).sum()) == 0


# ------------------------------------------------------------------ the step
P_STEP, RES_STEP, DC_STEP = 2048, 128, 59


def _step_setup(dev, n_frames):
    import torch
    from fateavatar_amd.mlp import embed_points
    from tests.test_gpu_flash import _targets, _template
    S = _template(dev, RES_STEP, n_frames)
    bg = torch.ones(3, device=dev)
    make, gts, _, _ = _targets(S, dev, bg, n_frames, P_STEP)
    g = torch.Generator().manual_seed(21)
    conds = [(0.3 * torch.randn(DC_STEP, generator=g)).to(dev) for _ in range(n_frames)]
    E = embed_points(make().canonical_points(S["posed"][0], S["faces"])).contiguous()

    def net():
        rng = torch.get_rng_state()
        torch.manual_seed(5)
        m = mlp_ref.RefMLP(51 + DC_STEP, 10, hidden_layers=6).to(dev)
        torch.set_rng_state(rng)
        with torch.no_grad():       # small outputs at first, as tests/test_gpu_flash.py's network
            m.output_linear.weight.mul_(0.05)
            m.output_linear.bias.zero_()
        return m
    return S, bg, make, gts, conds, E, net


def test_one_fused_step_matches_the_torch_route(gpu_device):
    """ONE eager step from identical weights: the existing route (torch MLP -> FlashStep -> deform.backward(step.d_deform)) against
    FlashStep(deformer=DeformMLP.from_torch(the same module)), both with vertex_grad."""
    import torch
    from fateavatar_amd.flash import FlashStep
    from fateavatar_amd.mlp import DeformMLP
    dev = gpu_device
    S, bg, make, gts, conds, E, net = _step_setup(dev, 3)
    lr = 1e-4
    # ---- the existing route
    torch_net, pc_t = net(), make()
    st_t = FlashStep(pc_t, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False, vertex_grad=True)
    cond_t = conds[1].clone().requires_grad_(True)
    deform = torch_net(torch.cat([E, cond_t.expand(P_STEP, DC_STEP)], dim=1))
    st_t.step(S["cams"][1], S["posed"][1], deform, gts[1])
    deform.backward(st_t.d_deform)
    want_grad = _cat([p.grad for p in torch_net.parameters()])
    # ---- the fused step
    pc_f = make()
    mlp = DeformMLP.from_torch(net(), E, DC_STEP)
    w0 = mlp.flat.detach().clone()
    st_f = FlashStep(pc_f, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False, vertex_grad=True, deformer=mlp,
                     deformer_lr=lr)
    with pytest.raises(ValueError, match="condition"):
        st_f.step(S["cams"][1], S["posed"][1], deform.detach(), gts[1])        # a `deform`-shaped third argument
    assert st_f.host_steps == 0
    loss = st_f.step(S["cams"][1], S["posed"][1], conds[1], gts[1])
    torch.cuda.synchronize()
    # (the two `deform` differ by float32 rounding, 1e-7 relative, and the loss is a mean of smooth terms of them)
    assert abs(float(loss) - float(st_t.loss)) <= 1e-4 * abs(float(st_t.loss))
    for name, got, ref in (("d_deform", st_f.d_deform, st_t.d_deform), ("flat_grad", mlp.flat_grad, want_grad),
                           ("d_cond", st_f.d_cond, cond_t.grad), ("d_verts", st_f.d_verts, st_t.d_verts)):
        err = _rel(got, ref)
        print(f"fused step against the torch route, {name}: rel-L2 {err:.3e}")
        assert float(ref.abs().max()) > 0 and err <= CEILING, (name, err)
    # the wiring of the second Adam: the weights are what torch.optim.Adam makes of the kernel's OWN gradient
    p = w0.clone().requires_grad_(True)
    p.grad = mlp.flat_grad.clone()
    torch.optim.Adam([p], lr=lr).step()
    diff = (mlp.flat.detach() - p.detach()).abs()
    assert float((mlp.flat.detach() - w0).abs().max()) > 0.5 * lr
    assert bool((diff <= 1e-6 * p.detach().abs() + 1e-6 * lr).all()), float(diff.max())
    assert st_f.deformer_adam.step_count == 1 == st_f.adam.step_count


def test_fused_step_trains_as_one_graph_and_round_trips_its_checkpoint(gpu_device):
    import torch
    from fateavatar_amd.flash import FlashGaussians, FlashStep
    from fateavatar_amd.mlp import DeformMLP
    from tests import util
    dev = gpu_device
    n_frames, steps = 6, 30
    S, bg, make, gts, conds, E, net = _step_setup(dev, n_frames)
    pc = make()
    mlp = DeformMLP.from_torch(net(), E, DC_STEP)
    w0 = mlp.flat.detach().clone()
    st = FlashStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=True, vertex_grad=True, deformer=mlp)
    losses = []
    for it in range(steps):
        f = it % n_frames
        losses.append(float(st.step(S["cams"][f], S["posed"][f], conds[f], gts[f])))
    torch.cuda.synchronize()
    st.check()
    assert st._graph is not None and st.overflows == 0
    print("loss, first and last 6 steps:", np.mean(losses[:6]), np.mean(losses[-6:]))
    assert np.mean(losses[-6:]) < np.mean(losses[:6]), (losses[:6], losses[-6:])
    applied = st.host_steps - st.skipped_steps
    assert st.host_steps == steps and st.deformer_adam.step_count == applied == st.adam.step_count
    assert float((mlp.flat.detach() - w0).abs().max()) > 0
    assert tuple(st.d_cond.shape) == (DC_STEP,) and float(st.d_cond.abs().max()) > 0 and float(st.d_verts.abs().max()) > 0
    # ---- the checkpoint carries the network under the reference's names and loads it back
    sd = st.state_dict()
    names = [k for k in sd["model"] if k.startswith("deformNet.")]
    assert names == [f"deformNet.fcs.{i}.{w}" for i in range(6) for w in ("weight", "bias")] + ["deformNet.output_linear.weight",
                                                                                             "deformNet.output_linear.bias"]
    sd["model"]["flame.shapedirs"] = torch.zeros(2)                 # (something of the reference's that stays ignored)
    other = FlashGaussians(pc.face_index.cpu(), pc.bary_coords.cpu(), -4.0, dev)
    mlp2 = DeformMLP(E, DC_STEP)
    st2 = FlashStep(other, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False, deformer=mlp2)
    assert st2.load_state_dict(sd) == ["flame.shapedirs"]
    assert torch.equal(mlp2.flat, mlp.flat) and torch.equal(st2.pc.flat, pc.flat)
    assert st2.deformer_adam.step_count == applied
    before = mlp.flat.detach().clone()
    for s in (st, st2):
        s.step(S["cams"][2], S["posed"][2], conds[2], gts[2])
    torch.cuda.synchronize()
    # the restored step goes on with the same update (the frame's gradients carry the rasterizer's float-atomic noise)
    assert _rel(mlp2.flat.detach() - before, mlp.flat.detach() - before) < 1e-2 and float((mlp.flat.detach() - before).abs().max()) > 0
    util.assert_same_trajectory(st2.pc.flat, pc.flat, "checkpoint round trip", tight=2e-3)
    assert st2.deformer_adam.step_count == applied + 1
    # without a deformer the same checkpoint loads as before: the network's entries come back as ignored keys
    plain = FlashStep(FlashGaussians(pc.face_index.cpu(), pc.bary_coords.cpu(), -4.0, dev), S["faces"], S["cams"][0].clone(), bg,
                      S["posed"][0], use_graph=False)
    assert plain.load_state_dict(sd) == sorted(names + ["flame.shapedirs"])
