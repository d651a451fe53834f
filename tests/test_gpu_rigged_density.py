"""-m gpu: GaussianAvatars past step 0 on the device — the regulariser launch (`fr_gaussian_regularise`), the step that
carries it, and the density control of the rigged set (`RiggedStep.densify_and_prune / prune / reset_opacity`).  The
reference of every comparison is the torch restatement of tests/rigged_density_ref.py (pinned on the CPU by
tests/test_rigged_density_host.py)."""
import math

import numpy as np
import pytest

from tests.rigged_density_ref import NAMES, REFERENCE, RiggedRef, draw_gate_inputs, gate_margins, regulariser_grads
from tests.test_gpu_face_local import _perturbed, _targets, _template

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24     # one float32 rounding, relative
REG_GRID_CAP = 1024 * 256   # Gaussians one sweep of k_gaussian_regularise covers at the launch's cap (kRegMaxBlocks, fr_optim.hip)


def _reg_roundings(P):
    """Roundings of a loss sum of k_gaussian_regularise behind its terms: see test_regulariser_kernel_matches_float64_autograd."""
    blocks = min(-(-P // 256), REG_GRID_CAP // 256)
    visits, per_lane = -(-P // (256 * blocks)), -(-blocks // 256)
    return 20 + (visits - 1) + max(per_lane - 2, 0)


# ------------------------------------------------------------------ 1. the kernel against float64 autograd
@pytest.mark.parametrize("P", [1, 63, 64, 65, 10_006, 100_003, REG_GRID_CAP, REG_GRID_CAP + 1, 2 * REG_GRID_CAP + 5])
def test_regulariser_kernel_matches_float64_autograd(gpu_device, P):
    """`gaussian_regularisers` with the reference's weights and thresholds against float64 autograd of
        scale_weight * relu(exp(s) - 0.6).norm(dim=1).mean() + xyz_weight * relu(xyz.norm(dim=1) - 1.0).mean()
    added to gradient arrays pre-filled with non-zero values: expected = before + weight * g.
    Inputs are drawn so that no exp(s) lies within 1 % of threshold_scale and no |xyz| within 1 % of threshold_xyz (checked
    here): no gate can flip under float32 rounding, no entry is exempt.
    Bound on every entry: |got - want| <= 1e-4 |want| + 2 x 2^-24 |want|.  The relative term is the project's standing one
    and covers the gradient's own arithmetic: expf (<= 2 roundings) goes through e - threshold, which at the 1 % margin
    amplifies it by e / (e - threshold) <= 100, i.e. <= 200 roundings = 1.2e-5, plus about ten more for the squares, the
    sum, the square root, the division and the two products.  The absolute term counts what is NOT relative to g: the
    read-modify-write addition rounds once at the magnitude of the result, and weight / P reaches the kernel rounded to
    float32 once.  The arrays are pre-filled with the gradient's own sign (and its 1 / P size), so that |want| =
    |before| + |weight g| and "the entry's magnitude" is also the magnitude of what was added up.
    Loss scalars: P non-negative terms, at most one per thread at these sizes, summed as a tree — 6 shuffle levels and 2
    across the waves in every workgroup, <= 2 partials per thread, 6 and 2 levels again in the last workgroup, the final
    multiplication by the rounded 1 / P: 20 roundings, each relative to a partial sum that is at most the total; the terms'
    own error is the relative 1e-4 as above (|xyz| - threshold amplifies the norm's three roundings by <= 100).
    Past 131 072 Gaussians a lane of the last workgroup adds up more than two partials, and past REG_GRID_CAP a thread visits
    more than one Gaussian: one rounding more per further partial and per further visit, with B = min(ceil(P / 256), 1024)
    workgroups
        N(P) = 20 + (ceil(P / 256 B) - 1) + max(ceil(B / 256) - 2, 0)         (20 up to 131 072; 22, 23, 24 at the three sizes past the cap)
    |got - want| <= (1e-4 + N(P) x 2^-24) want.
    Achieved maxima (MI355X): see profiles/r11_rigged_density.md, past the cap profiles/r18_grid_caps.md."""
    import torch
    from fateavatar_amd.loss import gaussian_regularisers, regulariser_workspace
    dev = gpu_device
    R = REFERENCE
    assert [_reg_roundings(p) for p in (1, 100_003, 131_072, REG_GRID_CAP, REG_GRID_CAP + 1, 2 * REG_GRID_CAP + 5)] == [20, 20, 20, 22, 23, 24]
    gen = torch.Generator().manual_seed(100 + P)
    scaling, xyz = draw_gate_inputs(P, gen, R["threshold_scale"], R["threshold_xyz"])
    ms, mx = gate_margins(scaling, xyz, R["threshold_scale"], R["threshold_xyz"])
    assert ms >= 0.01 and mx >= 0.01, (ms, mx)
    ls, lx, gs, gx = regulariser_grads(scaling, xyz, **R)
    if P >= 63:
        assert float(gs.abs().max()) > 0 and float(gx.abs().max()) > 0 and bool((gs == 0).any()) and bool((gx == 0).any())
    before_s = (torch.rand(P, 3, generator=gen) + 0.5) / P
    before_x = (torch.rand(P, 3, generator=gen) + 0.5) * torch.where(xyz < 0, -1.0, 1.0) * (R["xyz_weight"] / P)
    assert bool((before_s != 0).all()) and bool((before_x != 0).all())
    d_s, d_x = before_s.to(dev), before_x.to(dev)
    ws = regulariser_workspace(dev)
    out = gaussian_regularisers(scaling.to(dev), xyz.to(dev), d_s, d_x, weights=(R["scale_weight"], R["xyz_weight"]),
                                thresholds=(R["threshold_scale"], R["threshold_xyz"]), workspace=ws)
    torch.cuda.synchronize()
    assert not bool(ws.any())
    worst = {}
    for name, got, before, g in (("d_scaling", d_s, before_s, gs), ("d_xyz", d_x, before_x, gx)):
        want = before.double() + g                     # (regulariser_grads applies the weights)
        err = (got.cpu().double() - want).abs()
        bound = (1e-4 + 2 * EPS) * want.abs()
        worst[name] = float((err / want.abs()).max())
        print(f"P={P} {name}: max |got - want| / |want| = {worst[name]:.3e}, entries over the bound: {int((err > bound).sum())}")
        assert bool(torch.isfinite(got).all()) and int((err > bound).sum()) == 0, (name, worst[name])
    for name, got, want in (("scale_loss", out[0], ls), ("xyz_loss", out[1], lx)):
        rel = abs(float(got) - float(want)) / max(float(want), 1e-300) if float(want) > 0 else abs(float(got))
        print(f"P={P} {name}: got {float(got):.9g} want {float(want):.9g} rel {rel:.3e}")
        assert abs(float(got) - float(want)) <= (1e-4 + _reg_roundings(P) * EPS) * float(want), (name, float(got), float(want))


# ------------------------------------------------------------------ 2. gates and reproducibility
def test_regulariser_kernel_gates_and_reproducibility(gpu_device):
    """Thresholds 1.0 (= expf(0), exactly) and 5.0 (= |(3, 4, 0)|, exactly): components at and below the threshold, a row
    clipped to zero entirely, |xyz| at and below the threshold and xyz = 0 leave their pre-filled gradient entries
    BIT-IDENTICAL; a zero weight leaves the whole array bit-identical; NULL gradient pointers give the loss only; two
    launches, and a captured and replayed launch, give the eager bits; the workspace is zero afterwards."""
    import torch
    from fateavatar_amd.loss import gaussian_regularisers, regulariser_workspace
    dev = gpu_device
    P = 10_006
    gen = torch.Generator().manual_seed(8)
    scaling, xyz = draw_gate_inputs(P, gen, 1.0, 5.0)
    xyz = xyz * 1.5
    scaling[0] = torch.tensor([0.0, 0.0, 0.0])                  # every component AT the threshold: the row clips to zero
    scaling[1] = torch.tensor([0.0, 1.0, -1.0])                 # at, above, below
    scaling[2] = torch.tensor([-0.5, -3.0, -20.0])              # all below
    xyz[0] = torch.tensor([3.0, 4.0, 0.0])                      # |xyz| AT the threshold
    xyz[1] = torch.tensor([0.0, 0.0, 0.0])
    xyz[2] = torch.tensor([0.3, 0.4, 0.0])
    xyz[3] = torch.tensor([6.0, 8.0, 0.0])
    before_s, before_x = torch.randn(P, 3, generator=gen) + 3.0, torch.randn(P, 3, generator=gen) - 3.0
    s_d, x_d = scaling.to(dev), xyz.to(dev)
    ws = regulariser_workspace(dev)
    kw = dict(thresholds=(1.0, 5.0), workspace=ws)

    def launch(weights=(1.0, 0.5), with_s=True, with_x=True):
        d_s, d_x = before_s.to(dev), before_x.to(dev)
        out = gaussian_regularisers(s_d, x_d, d_s if with_s else None, d_x if with_x else None, weights=weights, **kw).clone()
        torch.cuda.synchronize()
        assert not bool(ws.any())
        return out, d_s, d_x

    out, d_s, d_x = launch()
    bs, bx = before_s.to(dev), before_x.to(dev)
    assert bool(torch.isfinite(d_s).all()) and bool(torch.isfinite(d_x).all()) and bool(torch.isfinite(out).all())
    assert torch.equal(d_s[0], bs[0]) and torch.equal(d_s[2], bs[2])
    assert torch.equal(d_s[1, [0, 2]], bs[1, [0, 2]]) and float(d_s[1, 1]) > float(bs[1, 1])
    assert torch.equal(d_x[:3], bx[:3]) and float(d_x[3, 0]) > float(bx[3, 0]) and float(d_x[3, 2]) == float(bx[3, 2])
    # every gated entry of the drawn rows, too
    gated_s = (torch.exp(scaling.double()) <= 1.0).to(dev)
    gated_x = (xyz.double().norm(dim=1) <= 5.0).to(dev)
    assert torch.equal(d_s[gated_s], bs[gated_s]) and torch.equal(d_x[gated_x], bx[gated_x])
    assert int((~gated_s).sum()) > 1000 and int((~gated_x).sum()) > 100
    assert float(out[0]) > 0 and float(out[1]) > 0
    # ---- zero weights
    o2, e_s, e_x = launch(weights=(0.0, 0.5))
    assert torch.equal(e_s, bs) and torch.equal(e_x, d_x) and torch.equal(o2, out)
    o3, e_s, e_x = launch(weights=(1.0, 0.0))
    assert torch.equal(e_x, bx) and torch.equal(e_s, d_s) and torch.equal(o3, out)
    # ---- NULL gradient pointers: the loss only
    o4, e_s, e_x = launch(with_s=False, with_x=False)
    assert torch.equal(o4, out) and torch.equal(e_s, bs) and torch.equal(e_x, bx)
    # ---- launch to launch
    o5, e_s, e_x = launch()
    assert torch.equal(o5, out) and torch.equal(e_s, d_s) and torch.equal(e_x, d_x)
    # ---- captured and replayed
    g_s, g_x, g_out = bs.clone(), bx.clone(), torch.zeros(2, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            gaussian_regularisers(s_d, x_d, g_s, g_x, out=g_out, weights=(1.0, 0.5), **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        g_s.copy_(bs)
        g_x.copy_(bx)
        g_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_out, out) and torch.equal(g_s, d_s) and torch.equal(g_x, d_x)
        assert not bool(ws.any())
    # ---- the wrapper's own rules
    with pytest.raises(RuntimeError):
        gaussian_regularisers(scaling, xyz, None, None)                               # no CPU path
    with pytest.raises(RuntimeError):
        gaussian_regularisers(s_d, x_d, None, None, workspace=torch.zeros(8, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------ 3. the step
def _reg_of(pc):
    """float64 regulariser gradients (weighted, reference values) and losses of a rigged set's current parameters."""
    return regulariser_grads(pc._scaling.detach().cpu(), pc._xyz.detach().cpu(), **REFERENCE)


def _step_of(S, dev, bg, seed, use_graph, regularisers):
    from fateavatar_amd.rigged import RiggedStep
    pc = _perturbed(dev, S["F"], seed=seed)
    return RiggedStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=use_graph, regularisers=regularisers)


def test_rigged_step_with_the_reference_regularisers(gpu_device, monkeypatch):
    """(a) the gradient the step hands to Adam is the image term's plus the regularisers': flat_grad minus the flat_grad of a
    twin step without regularisers on the same state, against the float64 regulariser gradient, within 8 x the backward's own
    run-to-run floor (twin-without against twin-without: the backward sums with float atomics);
    (b) six steps: after each the parameters equal torch.optim.Adam fed the step's own flat_grad (rtol 2e-6, atol 1e-7), and
    reg_loss holds the unweighted losses of the parameters the step started from;
    (c) 30 steps, graph against eager: util.assert_same_trajectory with the rigged graph test's tolerance;
    (d) regularisers=None launches nothing: reg_loss is None and `gaussian_regularisers` is never called."""
    import torch
    import fateavatar_amd.rigged as rigged
    from fateavatar_amd.rigged import REFERENCE_REGULARISERS, RIGGED_LRS
    from tests import util
    dev = gpu_device
    res, n_frames = 128, 4
    S = _template(dev, res, n_frames, seed=2)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg, n_frames)
    calls = []
    real = rigged.gaussian_regularisers
    monkeypatch.setattr(rigged, "gaussian_regularisers", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    frame = lambda st, f: st.step(S["cams"][f], S["posed"][f], gts[f])  # noqa: E731
    # ---- (a) and (d)
    st_w = _step_of(S, dev, bg, 4, False, REFERENCE_REGULARISERS)
    st_a, st_b = _step_of(S, dev, bg, 4, False, None), _step_of(S, dev, bg, 4, False, None)
    assert st_a.reg_loss is None and torch.equal(st_w.pc.flat, st_a.pc.flat)
    ls, lx, gs, gx = _reg_of(st_w.pc)
    assert float(gs.abs().max()) > 0 and float(gx.abs().max()) > 0 and bool((gs == 0).any()) and bool((gx == 0).any())
    frame(st_a, 1), frame(st_b, 1)
    torch.cuda.synchronize()
    assert calls == [] and st_a.reg_loss is None
    frame(st_w, 1)
    torch.cuda.synchronize()
    assert len(calls) == 1
    for name, g in (("_scaling", gs), ("_xyz", gx)):
        a, b, w = (s.pc.grad_view(name).double().cpu() for s in (st_a, st_b, st_w))
        floor = float((a - b).abs().max())
        err = float(((w - a) - g).abs().max())
        print(f"{name}: run-to-run floor {floor:.3e}, |(with - without) - regulariser| max {err:.3e}, max |g| {float(g.abs().max()):.3e}")
        assert floor > 0 and err <= 8 * floor, (name, err, floor)
    for name in ("_opacity", "_features_dc", "_rotation"):             # the other runs are the twin's, to the same floor
        a, b, w = (s.pc.grad_view(name).double() for s in (st_a, st_b, st_w))
        assert float((w - a).abs().max()) <= 8 * max(float((a - b).abs().max()), 1e-30), name
    assert abs(float(st_w.reg_loss[0]) - float(ls)) <= 2e-4 * float(ls) and abs(float(st_w.reg_loss[1]) - float(lx)) <= 2e-4 * float(lx)
    # ---- (b)
    st = _step_of(S, dev, bg, 6, False, REFERENCE_REGULARISERS)
    pc = st.pc
    sizes = [n for n, _ in st.adam_segments()]
    ref = [t.clone().requires_grad_() for t in torch.split(pc.flat.detach(), sizes)]
    lrs = [RIGGED_LRS[k] for k in ("xyz", "opacity", "feature_dc", "feature_rest", "rotation", "scaling")]
    topt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(ref, lrs)], lr=0.0)
    for it in range(6):
        if it == 3:
            st.update_sh_degree()
        ls, lx, _, _ = _reg_of(pc)
        loss = frame(st, it % n_frames)
        for p, g in zip(ref, torch.split(pc.flat_grad, sizes)):
            p.grad = g.clone()
        topt.step()
        want = torch.cat([p.detach() for p in ref])
        assert torch.allclose(pc.flat, want, rtol=2e-6, atol=1e-7), (it, float((pc.flat - want).abs().max()))
        assert loss is st.loss and float(loss) > 0
        assert abs(float(st.reg_loss[0]) - float(ls)) <= 2e-4 * float(ls) and abs(float(st.reg_loss[1]) - float(lx)) <= 2e-4 * float(lx)
    assert st.adam.step_count == 6
    # ---- (c)
    runs = []
    for use_graph in (False, True):
        s = _step_of(S, dev, bg, 7, use_graph, REFERENCE_REGULARISERS)
        for it in range(30):
            frame(s, it % n_frames)
        torch.cuda.synchronize()
        s.check()
        runs.append(s)
    assert runs[1]._graph is not None and runs[0]._graph is None and runs[1].overflows == 0
    assert runs[0].adam.step_count == runs[1].adam.step_count == 30
    util.assert_same_trajectory(runs[1].pc.flat, runs[0].pc.flat, "graph vs eager, regularisers on", tight=2e-2)
    assert torch.allclose(runs[1].reg_loss, runs[0].reg_loss, rtol=1e-2) and float(runs[0].reg_loss.min()) > 0
    # the regularisers act: the scale term has fallen from where the perturbed set started
    fresh = _perturbed(dev, S["F"], seed=7)
    assert float(runs[0].reg_loss[0]) < float(_reg_of(fresh)[0])


# ------------------------------------------------------------------ 4. densify_and_prune against the restatement
def _ref_of(st):
    """A RiggedRef (CPU) with the step's parameters, binding, Adam state and statistics."""
    import torch
    pc = st.pc
    ref = RiggedRef({n: getattr(pc, n).detach().cpu() for n in NAMES}, pc.binding.cpu(), st.n_faces)
    sizes = [n for n, _ in st.adam_segments()]
    for n, m, v in zip(NAMES, torch.split(st.adam.exp_avg.cpu(), sizes), torch.split(st.adam.exp_avg_sq.cpu(), sizes)):
        ref.set_moments(n, m, v, st.adam.step_count)
    ref.xyz_gradient_accum, ref.denom = st.xyz_gradient_accum.cpu().clone(), st.denom.cpu().clone()
    return ref


def _same_as_ref(st, ref, n_children):
    import torch
    pc = st.pc
    assert pc.P == ref.P
    assert torch.equal(pc.binding.cpu().long(), ref.binding)
    assert torch.equal(st.binding_counter.cpu(), ref.binding_counter) and st.binding_counter.dtype == torch.int32
    assert torch.equal(st.binding_counter.cpu().long(), torch.bincount(ref.binding, minlength=st.n_faces))
    sizes = [n for n, _ in st.adam_segments()]
    assert sum(sizes) == pc.flat.numel() == st.adam.exp_avg.numel()
    for n, m, v in zip(NAMES, torch.split(st.adam.exp_avg.cpu(), sizes), torch.split(st.adam.exp_avg_sq.cpu(), sizes)):
        got, want = getattr(pc, n).detach().cpu(), ref.p[n].detach()
        assert got.shape == want.shape, n
        if n in ("_xyz", "_scaling"):        # the split's children: 1e-6 relative (rel-L2, and of the largest entry)
            differ = int((got != want).any(dim=1).sum())
            rel = float((got.double() - want.double()).norm() / want.double().norm())
            print(f"{n}: {differ} rows differ (children: {n_children}), rel-L2 {rel:.3e}")
            assert differ <= n_children and rel <= 1e-6
            assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
        else:
            assert torch.equal(got, want), n
        rm, rv, rstep = ref.moments(n)
        assert torch.equal(m.reshape(rm.shape), rm) and torch.equal(v.reshape(rv.shape), rv), n
        assert int(rstep) == st.adam.step_count
    assert st.xyz_gradient_accum.shape == (pc.P, 1) == st.denom.shape


@pytest.mark.parametrize("case", ["all", "nothing_to_clone", "nothing_to_split", "nothing_at_all"])
def test_densify_and_prune_matches_the_restatement(gpu_device, case):
    """State built so that clone, split and the final prune each select something (statistics set directly, scalings on both
    sides of percent_dense * extent = 0.02 and well away from it, opacities on both sides of min_opacity, two Gaussians on
    most faces — the guard keeps a low-opacity Gaussian that is alone on its face, and its clones with it), product and
    restatement each with a CPU generator seeded the same.  Exact: copied fields, binding, binding_counter, moments (rows
    follow, new rows zero), the step count.  Split positions and scales: 1e-6 relative.  Statistics zero afterwards, the
    graph dropped and captured again on the following steps.  The other cases: nothing to clone, nothing to split, and
    nothing at all (the graph then stays)."""
    import torch
    dev = gpu_device
    res, n_frames = 128, 4
    S = _template(dev, res, n_frames, seed=2)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg, n_frames)
    from fateavatar_amd.rigged import RiggedGaussians, RiggedStep
    F = S["F"]
    g = torch.Generator().manual_seed(21)
    # two Gaussians on most faces: the guarded prune can only remove a Gaussian whose face keeps another one
    binding = torch.cat([torch.arange(F), torch.randint(0, F, (F,), generator=g)]).to(torch.int32)
    pc = RiggedGaussians(binding.numpy(), dev)
    F, n_faces = pc.P, F                                        # (F: rows of the state built below)
    with torch.no_grad():
        pc._xyz.copy_((0.3 * torch.randn(F, 3, generator=g)).to(dev))
        pc._rotation.add_((0.5 * torch.randn(F, 4, generator=g)).to(dev))
        pc._features_dc.copy_((torch.rand(F, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        pc._features_rest.copy_((0.3 * torch.randn(F, 15, 3, generator=g)).to(dev))
    st = RiggedStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=True)
    assert st.n_faces == n_faces and int(st.binding_counter.max()) >= 2
    small = torch.rand(F, generator=g) < 0.5
    if case == "nothing_to_clone":
        small[:] = False
    if case == "nothing_to_split":
        small[:] = True
    with torch.no_grad():
        scl = torch.where(small[:, None], -5.0 + 0.3 * torch.rand(F, 3, generator=g), -3.0 + 2.5 * torch.rand(F, 3, generator=g))
        pc._scaling.copy_(scl.to(dev))
        low = torch.rand(F, generator=g) < 0.1
        pc._opacity.copy_(torch.where(low, math.log(0.001 / 0.999), math.log(0.6 / 0.4)).reshape(F, 1).to(dev))
    for it in range(4):
        st.step(S["cams"][it % n_frames], S["posed"][it % n_frames], gts[it % n_frames])
    torch.cuda.synchronize()
    assert st._graph is not None and float(st.adam.exp_avg.abs().max()) > 0
    graph_before = st._graph
    if case == "nothing_at_all":
        st.xyz_gradient_accum.zero_()
        st.denom.zero_()
        min_opacity = 0.0
    else:
        st.xyz_gradient_accum.copy_((3e-4 * torch.rand(F, 1, generator=g)).to(dev))
        st.denom.copy_(torch.randint(0, 3, (F, 1), generator=g).float().to(dev))
        st.xyz_gradient_accum[st.denom == 0] = 0
        min_opacity = 0.005
    ref = _ref_of(st)
    steps_before, host_before = st.adam.step_count, st.host_steps
    got = st.densify_and_prune(1e-4, min_opacity, 2.0, None, torch.Generator().manual_seed(77))
    want = ref.densify_and_prune(1e-4, min_opacity, 2.0, None, torch.Generator().manual_seed(77))
    print(case, "cloned / split / pruned:", got, "P", pc.P)
    assert tuple(got) == tuple(want)
    assert (got[0] > 0) == (case in ("all", "nothing_to_split")) and (got[1] > 0) == (case in ("all", "nothing_to_clone"))
    assert (got[2] > 0) == (case != "nothing_at_all")
    _same_as_ref(st, ref, 2 * got[1])
    assert int(st.binding_counter.min()) >= 1
    assert float(st.xyz_gradient_accum.abs().max()) == 0 and float(st.denom.abs().max()) == 0
    assert st.adam.step_count == steps_before and st.host_steps == host_before
    if case == "nothing_at_all":
        assert st._graph is graph_before and pc.P == F
    else:
        assert st._graph is None and pc.P != F
    for it in range(4):
        loss = st.step(S["cams"][it % n_frames], S["posed"][it % n_frames], gts[it % n_frames])
    torch.cuda.synchronize()
    st.check()
    assert st._graph is not None and math.isfinite(float(loss)) and bool(torch.isfinite(pc.flat).all())
    assert st.adam.step_count == steps_before + 4 and float(st.denom.max()) > 0
    if case == "all":       # a second round with a world-size prune (a truthy max_screen_size)
        st.xyz_gradient_accum.zero_()
        st.denom.zero_()
        ref = _ref_of(st)
        got = st.densify_and_prune(1e-4, 0.005, 2.0, 20, torch.Generator().manual_seed(78))
        want = ref.densify_and_prune(1e-4, 0.005, 2.0, 20, torch.Generator().manual_seed(78))
        assert tuple(got) == tuple(want) and got[:2] == (0, 0) and got[2] > 0      # exp(scaling) > 0.2 somewhere
        _same_as_ref(st, ref, 0)
        assert int(st.binding_counter.min()) >= 1


# ------------------------------------------------------------------ 5. the guarded prune
def test_guarded_prune_never_empties_a_face(gpu_device):
    """Face 0 carries three Gaussians, all marked: all three stay.  Face 1 carries three, one marked: that one goes.  Face 5
    carries one, marked: it stays.  binding_counter follows and stays >= 1; moments and statistics follow the rows."""
    import torch
    from fateavatar_amd.rigged import RiggedGaussians, RiggedStep
    dev = gpu_device
    S = _template(dev, 64, 2)
    F = S["F"]
    binding = np.concatenate([np.arange(F), [0, 0, 1, 1]]).astype(np.int32)
    pc = RiggedGaussians(binding, dev)
    st = RiggedStep(pc, S["faces"], S["cams"][0].clone(), torch.ones(3, device=dev), S["posed"][0], use_graph=False)
    assert st.binding_counter[:3].tolist() == [3, 3, 1] and int(st.binding_counter.sum()) == F + 4
    st.adam.exp_avg.copy_(torch.arange(pc.flat.numel(), device=dev, dtype=torch.float32))
    st.xyz_gradient_accum.copy_(torch.arange(pc.P, device=dev, dtype=torch.float32).reshape(-1, 1))
    xyz_rows = torch.arange(pc.P * 3, device=dev, dtype=torch.float32).reshape(-1, 3)
    with torch.no_grad():
        pc._xyz.copy_(xyz_rows)
    mask = torch.zeros(pc.P, dtype=torch.bool)
    mask[[0, F, F + 1, F + 2, 5]] = True
    assert st.prune(mask) == 1 and pc.P == F + 3
    keep = torch.ones(F + 4, dtype=torch.bool, device=dev)
    keep[F + 2] = False
    assert pc.binding.tolist() == binding[keep.cpu().numpy()].tolist()
    assert st.binding_counter[:3].tolist() == [3, 2, 1] and int(st.binding_counter.min()) >= 1
    assert torch.equal(st.binding_counter.long(), torch.bincount(pc.binding.long(), minlength=F))
    assert torch.equal(pc._xyz.detach(), xyz_rows[keep])
    assert torch.equal(st.adam.exp_avg[:pc.P * 3].view(-1, 3), xyz_rows[keep])          # (the moments of the _xyz run)
    assert torch.equal(st.xyz_gradient_accum.reshape(-1), torch.arange(F + 4, device=dev, dtype=torch.float32)[keep])
    # everything marked: one Gaussian... no: NONE of a face's marked Gaussians goes when the face would be emptied
    assert st.prune(torch.ones(pc.P, dtype=torch.bool)) == 0 and pc.P == F + 3
    # prune_low_opacity is the same guard under the opacity mask
    with torch.no_grad():
        pc._opacity.fill_(-20.0)
    assert st.prune_low_opacity(0.005) == 0
    with torch.no_grad():
        pc._opacity[:F].fill_(2.0)
    assert st.prune_low_opacity(0.005) == 3 and pc.P == F and int(st.binding_counter.max()) == 1


# ------------------------------------------------------------------ 6. reset_opacity
def test_reset_opacity_is_in_place_and_the_captured_graph_follows_the_eager_step(gpu_device):
    import torch
    from tests import util
    dev = gpu_device
    res, n_frames = 128, 4
    S = _template(dev, res, n_frames, seed=2)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg, n_frames)
    runs = [_step_of(S, dev, bg, 13, use_graph, None) for use_graph in (True, False)]
    with torch.no_grad():
        for s in runs:                       # opacities on both sides of 0.01
            s.pc._opacity[::3].fill_(math.log(0.004 / 0.996))
    for s in runs:
        for it in range(6):
            s.step(S["cams"][it % n_frames], S["posed"][it % n_frames], gts[it % n_frames])
    torch.cuda.synchronize()
    st = runs[0]
    graph = st._graph
    assert graph is not None
    P = st.pc.P
    ptrs = lambda s: (s.pc.flat.data_ptr(), s.pc._opacity.data_ptr(), s.adam.exp_avg.data_ptr(), s.adam.exp_avg_sq.data_ptr())  # noqa: E731
    before_ptrs = ptrs(st)
    old = torch.sigmoid(st.pc._opacity.detach().double().cpu())
    moments_before = st.adam.exp_avg.clone()
    for s in runs:
        s.reset_opacity()
    new = torch.minimum(old, torch.full_like(old, 0.01))
    want = torch.log(new / (1 - new))
    assert bool((old < 0.01).any()) and bool((old > 0.01).any())
    assert torch.allclose(st.pc._opacity.detach().double().cpu(), want, rtol=1e-5, atol=1e-6)
    assert float(torch.sigmoid(st.pc._opacity.detach()).max()) <= 0.01 * (1 + 1e-5)
    for m in (st.adam.exp_avg, st.adam.exp_avg_sq):
        assert float(m[3 * P:4 * P].abs().max()) == 0                       # the _opacity run
    assert torch.equal(st.adam.exp_avg[:3 * P], moments_before[:3 * P]) and torch.equal(st.adam.exp_avg[4 * P:], moments_before[4 * P:])
    assert ptrs(st) == before_ptrs and st._graph is graph
    for s in runs:
        for it in range(6, 14):
            s.step(S["cams"][it % n_frames], S["posed"][it % n_frames], gts[it % n_frames])
    torch.cuda.synchronize()
    st.check()
    assert st._graph is graph and st.adam.step_count == runs[1].adam.step_count == 14
    util.assert_same_trajectory(st.pc.flat, runs[1].pc.flat, "graph vs eager across reset_opacity", tight=2e-2)


# ------------------------------------------------------------------ 7. end to end
def test_rigged_training_with_density_control_end_to_end(gpu_device):
    """120 steps at 128 x 128 from the reference's initial state with the reference's regularisers and a compressed schedule:
    densify every 20 from step 40, opacity reset at 60, SH degree up every 30.  P grows above F, every face keeps a Gaussian,
    nothing non-finite, the mean loss of the last 8 steps is below the first 8, and a checkpoint taken after a densify
    (P != F) restores into a fresh RiggedStep and continues on the same trajectory."""
    import torch
    from fateavatar_amd.rigged import REFERENCE_REGULARISERS, RiggedGaussians, RiggedStep
    from tests import util
    dev = gpu_device
    res, n_frames, steps = 128, 8, 120
    S = _template(dev, res, n_frames)
    F = S["F"]
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg, n_frames)
    pc = RiggedGaussians.one_per_face(F, dev)
    st = RiggedStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], regularisers=REFERENCE_REGULARISERS)
    gen = torch.Generator().manual_seed(3)
    losses, twin, sizes = [], None, []
    for it in range(1, steps + 1):
        f = it % n_frames
        losses.append(float(st.step(S["cams"][f], S["posed"][f], gts[f])))
        if twin is not None and twin[1] > 0:
            twin[0].step(S["cams"][f], S["posed"][f], gts[f])
            twin[1] -= 1
            if twin[1] == 0:
                torch.cuda.synchronize()
                util.assert_same_trajectory(twin[0].pc.flat, pc.flat, "checkpoint after a densify", tight=2e-3)
                assert twin[0].adam.step_count == st.adam.step_count
        if it >= 40 and it % 20 == 0:
            did = st.densify_and_prune(generator=gen)
            sizes.append(pc.P)
            print(f"step {it}: cloned / split / pruned {did}, P {pc.P}, min binding_counter {int(st.binding_counter.min())}")
            assert torch.equal(st.binding_counter.long(), torch.bincount(pc.binding.long(), minlength=F))
            assert int(st.binding_counter.min()) >= 1
        if it == 60:
            st.reset_opacity()
        if it % 30 == 0:
            st.update_sh_degree()
        if it == 45 and pc.P != F:
            sd = st.state_dict()
            fresh = RiggedStep(RiggedGaussians.one_per_face(7, dev), S["faces"], S["cams"][0].clone(), bg, S["posed"][0],
                               use_graph=False, regularisers=REFERENCE_REGULARISERS)
            assert fresh.load_state_dict(sd) == [] and fresh.pc.P == pc.P
            assert torch.equal(fresh.binding_counter, st.binding_counter)
            twin = [fresh, 2]
    torch.cuda.synchronize()
    st.check()
    print("P after each densify:", sizes, "loss first / last 8:", np.mean(losses[:8]), np.mean(losses[-8:]))
    assert pc.P > F and twin is not None and twin[1] == 0
    assert np.isfinite(losses).all() and bool(torch.isfinite(pc.flat).all()) and bool(torch.isfinite(st.reg_loss).all())
    assert pc.active_sh_degree == 3 and st.adam.step_count == steps
    assert np.mean(losses[-8:]) < np.mean(losses[:8]), (losses[:8], losses[-8:])
