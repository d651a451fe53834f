"""-m gpu: FateAvatar's scale-ratio term on the device — the launch (`fr_scale_ratio_term`) against the recorded run of the
reference's own method and against the float64 restatement of tests/fate_scale_ref.py (pinned to that run on the CPU by
tests/test_fate_scale_host.py), its autograd op, and the steps that carry it (`AvatarStep(scale_term=)`,
`AvatarBatchStep(scale_term=)`).

Bounds.  A gradient entry: |got - want| <= (1e-4 + 2 x 2^-24) |want|, the project's gradient parity bound as the sibling terms
have it (tests/test_gpu_rigged_density.py has the count: the relative term covers the arithmetic — two expf, the quotient and
two products, a dozen roundings, nothing amplified: the ratio itself is the gradient — and the absolute pair the
read-modify-write addition and the rounded weight / P).  The loss: 1e-4 relative; a row 1 % over the threshold amplifies its
ratio's few roundings a hundredfold in relu(ratio - threshold), which stays under that; from 10^5 rows on the summation's own
roundings are counted on top, `test_gpu_rigged_density._reg_roundings(P)` (the same tree, the same grid cap).  The count: exact.
All inputs are drawn with every row's ratio at least 1 % off the threshold and, over the threshold, the two largest and two
smallest activated components at least 1e-3 apart (checked where drawn): no gate or tie can flip under float32 rounding and no
row is left out."""
import functools
import math

import numpy as np
import pytest

from tests import fate_scale_ref as R
from tests.reference_runs import EPS, Case
from tests.test_gpu_avatar import _setup, _targets
from tests.test_gpu_rigged_density import REG_GRID_CAP, _reg_roundings

pytestmark = pytest.mark.gpu

GRAD_BOUND = 1e-4 + 2 * EPS
LOSS_REL = 1e-4
P_SCENE, RES, FRAMES = 3000, 64, 4
SHIFT = -2.5                 # the scenes' log-scales: exp(-2.5) x the fixture's span, 5e-5 .. 3e-2


def _say(case, name, err, what):
    print(f"{case.name} {name}: kernel {what} {err:.3e}   (reference's own float32 run {case.e32(name):.3e}, "
          f"ratio {err / max(case.e32(name), 1e-300):.2f})")


def _drawn(P, seed, thr=9.0, over=0.5, shift=0.0):
    """`shift`: added to every log-scale (a scene's Gaussians are smaller than the fixture's span; the ratios stay)."""
    import torch
    s = (R.draw_scaling(P, torch.Generator().manual_seed(seed), thr, over) + shift).float()
    gate, tie = R.margins(s, thr)
    assert gate >= 1e-2 and tie >= 1e-3, (gate, tie)
    return s


def _launch(s, dev, weight, thr, before=None):
    """(loss words, gradient buffer, workspace) of one launch on a zeroed (or the given) gradient buffer and a fresh workspace."""
    import torch
    from fateavatar_amd.loss import ScaleRatioTerm, scale_ratio_term_and_grad, scale_ratio_workspace
    d = torch.zeros_like(s, device=dev) if before is None else before.to(dev).clone()
    ws = scale_ratio_workspace(dev)
    out = scale_ratio_term_and_grad(s.to(dev), d, terms=ScaleRatioTerm(weight, thr), workspace=ws)
    torch.cuda.synchronize()
    return out.cpu(), d.cpu(), ws


def _check_against(name, s, out, d, before, want_loss, want_count, want_g, loss_bound):
    """The launch's words and buffer against float64: `want_g` the weighted gradient, `before` what the buffer held."""
    import torch
    want = before.double() + want_g
    err = (d.double() - want).abs()
    touched = want_g != 0
    worst = float((err[touched] / want[touched].abs()).max()) if bool(touched.any()) else 0.0
    over = int((err > GRAD_BOUND * want.abs()).sum())
    rel = abs(float(out[0]) - float(want_loss)) / float(want_loss) if float(want_loss) > 0 else abs(float(out[0]))
    print(f"{name}: d_scaling max |got - want| / |want| = {worst:.3e} ({over} entries over the bound); scale_loss got {float(out[0]):.9g} "
          f"want {float(want_loss):.9g} rel {rel:.3e} (bound {loss_bound:.3e}); count {int(out[1])} want {want_count}")
    assert bool(torch.isfinite(d).all()) and over == 0, (name, worst)
    assert torch.equal(d[~touched], before[~touched]), name          # nothing anywhere else: the bits it held
    assert abs(float(out[0]) - float(want_loss)) <= loss_bound * float(want_loss), (name, float(out[0]), float(want_loss))
    assert float(out[1]) == want_count, (name, float(out[1]), want_count)
    return worst, rel


# ------------------------------------------------------------------ 1. the recorded run of the reference's own method
@pytest.mark.parametrize("name", ["fatescale_mixed", "fatescale_none", "fatescale_init"])
def test_recorded_run(gpu_device, name):
    import torch
    c = Case(name)
    s, w, thr = c.inp("scaling"), c.param("scale_weight"), c.param("scale_threshold")
    want_g, want_loss = c.out("d_scaling"), float(c.out("scale_loss"))
    scale = torch.exp(s.double())
    count = int((scale.max(1).values / scale.min(1).values > thr).sum())
    P = s.shape[0]
    gen = torch.Generator().manual_seed(7)
    # a zeroed buffer, and one pre-filled with the gradient's own sign and size (|want| = |before| + |w g|)
    sign = torch.where(want_g < 0, -1.0, 1.0).float()
    filled = (torch.rand(P, 3, generator=gen) + 0.5) * sign * (w * thr / P)
    assert bool((filled != 0).all())
    for what, before in (("zeroed", torch.zeros(P, 3)), ("pre-filled", filled)):
        out, d, ws = _launch(s, gpu_device, w, thr, before)
        assert not bool(ws.any())
        worst, rel = _check_against(f"{name} {what}", s, out, d, before, want_loss, count, want_g, LOSS_REL)
        if what == "zeroed":
            _say(c, "d_scaling", worst, "worst entry, relative")
            _say(c, "scale_loss", rel, "relative difference")
        if name == "fatescale_mixed":
            assert count > 0 and float(out[0]) > 0 and int((d != before).sum()) == 2 * count
        else:
            assert float(out[0]) == 0 and float(out[1]) == 0 and torch.equal(d, before)


# ------------------------------------------------------------------ 2. the grid cap and ragged tails
@pytest.mark.parametrize("P", [1, 255, 257, REG_GRID_CAP + 257])
def test_grid_cap_and_tails(gpu_device, P):
    """One lane, one row short of a workgroup, one past it, and past kRegMaxBlocks workgroups (the grid-stride loop's second
    visit with a ragged tail), against the float64 restatement on a pre-filled buffer."""
    import torch
    w, thr = 0.1, 9.0
    s = _drawn(P, 500 + P)
    want_loss, count, want_g = R.loss_count_grad(s, w, thr)
    if P >= 255:
        assert 0.3 * P < count < 0.7 * P
    gen = torch.Generator().manual_seed(P)
    before = (torch.rand(P, 3, generator=gen) + 0.5) * torch.where(want_g < 0, -1.0, 1.0).float() * (w * thr / P)
    out, d, ws = _launch(s, gpu_device, w, thr, before)
    assert not bool(ws.any())
    bound = LOSS_REL + (_reg_roundings(P) * EPS if P >= 100_000 else 0.0)
    _check_against(f"P={P}", s, out, d, before, float(want_loss), count, want_g, bound)


# ------------------------------------------------------------------ 3. the same bits on every launch
def test_two_launches_give_the_same_bits(gpu_device):
    import torch
    from fateavatar_amd.loss import ScaleRatioTerm, scale_ratio_term_and_grad, scale_ratio_workspace
    dev = gpu_device
    P = REG_GRID_CAP + 257
    s = _drawn(P, 11).to(dev)
    ws = scale_ratio_workspace(dev)
    got = []
    for _ in range(2):
        d = torch.zeros_like(s)
        out = scale_ratio_term_and_grad(s, d, terms=ScaleRatioTerm(0.1, 9.0), workspace=ws)
        torch.cuda.synchronize()
        assert not bool(ws.any())
        got.append((out.clone(), d))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and float(got[0][0][1]) > 0
    # a zero weight and a missing buffer: the words, no gradient traffic
    d = torch.full_like(s, 3.0)
    out0 = scale_ratio_term_and_grad(s, d, terms=ScaleRatioTerm(0.0, 9.0), workspace=ws)
    out1 = scale_ratio_term_and_grad(s, None, terms=ScaleRatioTerm(0.1, 9.0), workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(out0, got[0][0]) and torch.equal(out1, got[0][0]) and bool((d == 3.0).all()) and not bool(ws.any())
    # no rows: nothing is launched, fresh words are zero
    empty = scale_ratio_term_and_grad(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), workspace=ws)
    assert empty.tolist() == [0.0, 0.0]


# ------------------------------------------------------------------ 4. ties, gates, non-finite rows
def test_ties_gates_and_non_finite_rows(gpu_device):
    import torch
    dev = gpu_device
    L = math.log
    fill = lambda P: torch.full((P, 3), 0.25)  # noqa: E731
    nan = float("nan")
    # all components equal, threshold 0.5: ratio exactly 1, the row is over the threshold by 0.5 and argmax == argmin — the
    # two contributions cancel to an exact 0 (alone, and between two rows that are dropped: loss 0.5 / P)
    out, d, _ = _launch(torch.full((1, 3), L(3e-3)), dev, 0.1, 0.5, fill(1))
    assert out.tolist() == [0.5, 1.0] and torch.equal(d, fill(1))
    s = torch.tensor([[nan, 0.0, 0.0], [L(3e-3)] * 3, [0.0, nan, 0.0]])
    out, d, _ = _launch(s, dev, 0.1, 0.5, fill(3))
    assert float(out[0]) == float(np.float32(0.5) / np.float32(3)) and float(out[1]) == 1.0 and torch.equal(d, fill(3))
    # ratio exactly AT a threshold passes nothing: exp(0) / exp(0) = 1 against 1.0, on every device
    out, d, _ = _launch(torch.zeros(2, 3), dev, 0.1, 1.0, fill(2))
    assert out.tolist() == [0.0, 0.0] and torch.equal(d, fill(2))
    # two equal largest / two equal smallest components: the FIRST takes max's / min's gradient
    s = torch.tensor([[L(2e-2), L(2e-2), L(1e-3)], [L(1e-3), L(2e-2), L(1e-3)], [L(1e-3), L(2e-2), L(2e-2)]])
    out, d, _ = _launch(s, dev, 0.3, 9.0)
    g = d.double()
    want = 0.3 / 3 * 20.0
    assert float(out[1]) == 3.0 and abs(float(out[0]) - 11.0) <= LOSS_REL * 11.0
    for row, hi, lo, none in ((0, 0, 2, 1), (1, 1, 0, 2), (2, 1, 0, 2)):
        assert float(g[row, none]) == 0.0 and float(g[row, hi]) == -float(g[row, lo]), (row, g[row])
        assert abs(float(g[row, hi]) - want) <= GRAD_BOUND * want, (row, g[row])
    # the ratio exactly at 9: log 9 is no float, so the row (x, 0, 0) is searched for over the floats x with the KERNEL's own
    # ratio — its loss word at threshold 0 and P = 1 is expf(x) / 1 — by bisection; if expf steps over 9.0 there is no such row
    lo, hi = np.float32(2.0), np.float32(2.5)
    ratio_of = lambda x: float(_launch(torch.tensor([[float(x), 0.0, 0.0]]), dev, 0.0, 0.0)[0][0])  # noqa: E731
    while np.nextafter(lo, hi) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        lo, hi = (mid, hi) if ratio_of(mid) < 9.0 else (lo, mid)
    r_lo, r_hi = ratio_of(lo), ratio_of(hi)
    print(f"ratio at the threshold: expf({float(lo)!r}) = {r_lo!r}, expf({float(hi)!r}) = {r_hi!r}")
    assert r_lo < 9.0 <= r_hi
    if r_hi == 9.0:
        out, d, _ = _launch(torch.tensor([[float(hi), 0.0, 0.0], [0.0, float(hi), 0.0]]), dev, 0.1, 9.0, fill(2))
        assert out.tolist() == [0.0, 0.0] and torch.equal(d, fill(2))
    else:
        print("no float32 x has the kernel's expf(x) == 9.0f: the sub-case is covered by the threshold 1.0 above alone")
    # a NaN, a +inf and a -200 log-scale (exp underflows to 0: the ratio is inf): nothing added, the neighbours intact
    good = _drawn(4, 3, over=0.75)
    s = torch.cat([good[0:1], torch.tensor([[L(1e-3), nan, L(1e-2)]]), good[1:2], torch.tensor([[L(1e-3), float("inf"), L(1e-3)]]),
                   good[2:3], torch.tensor([[-200.0, L(1e-2), L(1e-2)]]), good[3:4], torch.tensor([[-200.0, -200.0, -200.0]])])
    bad = torch.tensor([1, 3, 5, 7])
    keep = torch.tensor([0, 2, 4, 6])
    P = s.shape[0]
    l4, count, g4 = R.loss_count_grad(good, 0.1 * 4 / P, 9.0)        # (the mean runs over all P rows: 4 / P of the good rows' own)
    before = (torch.rand(P, 3, generator=torch.Generator().manual_seed(5)) + 0.5) * 1e-3
    out, d, ws = _launch(s, dev, 0.1, 9.0, before)
    assert count >= 1 and float(out[1]) == count and bool(torch.isfinite(out).all()) and not bool(ws.any())
    assert abs(float(out[0]) - float(l4) * 4 / P) <= LOSS_REL * float(l4) * 4 / P
    assert torch.equal(d[bad], before[bad])
    want = before[keep].double() + g4
    assert bool(((d[keep].double() - want).abs() <= GRAD_BOUND * want.abs()).all()) and not torch.equal(d[keep], before[keep])


# ------------------------------------------------------------------ 5. the autograd op
def test_autograd_op(gpu_device):
    import torch
    from fateavatar_amd.loss import scale_ratio_loss
    c = Case("fatescale_mixed")
    w, thr = c.param("scale_weight"), c.param("scale_threshold")
    want = c.out("d_scaling") / w
    for factor in (1.0, 2.5):
        s = c.inp("scaling").to(gpu_device).requires_grad_(True)
        loss = scale_ratio_loss(s, thr)
        assert loss.dim() == 0 and abs(float(loss.detach()) - float(c.out("scale_loss"))) <= LOSS_REL * float(c.out("scale_loss"))
        (factor * loss).backward()
        err = (s.grad.cpu().double() - factor * want).abs()
        assert bool((err <= GRAD_BOUND * (factor * want).abs()).all()) and int((s.grad != 0).sum()) == int((want != 0).sum())
    with torch.no_grad():                                            # the loss alone: no gradient buffer is made
        assert float(scale_ratio_loss(c.inp("scaling").to(gpu_device), thr)) == float(loss.detach())


# ------------------------------------------------------------------ 6. - 9. the steps
@functools.lru_cache(maxsize=None)
def _scene(dev_index=0):
    """A small bound scene at 64^2, a third of its log-scale rows past ratio 9, and a camera turned AWAY from the mesh: every
    Gaussian lies behind it and is culled, the image gradient is exactly zero and a step's update is the scale term's alone."""
    import torch
    from fateavatar_amd import scenes
    from fateavatar_amd.model import TorchCamera
    dev = torch.device("cuda", dev_index)
    S = _setup(dev, P_SCENE, RES, FRAMES, seed=2)
    bg = torch.ones(3, device=dev)
    centre = S["posed"][0].mean(0).cpu().numpy().astype(np.float64)
    away = TorchCamera(scenes.look_at_camera(centre + np.array([0.0, 0.0, 2.0]), centre + np.array([0.0, 0.0, 4.0]), (0, 1, 0), 0.5, 0.5,
                                             RES, RES), dev)
    scaling = _drawn(P_SCENE, 77, over=1.0 / 3.0, shift=SHIFT).to(dev)

    def make(n=None):
        pc = S["make"]()
        with torch.no_grad():
            pc._scaling.copy_(scaling)
        return pc
    return dict(S=S, bg=bg, away=away, make=make, scaling=scaling, dev=dev)


def _adam_first_step(p, g, lr):
    """float64: Adam's first step on the gradient g from zero moments (betas 0.9 / 0.999, eps 1e-8, the float32 rate), and the
    bound of tests/test_gpu_adam.py on it — half an ulp of the parameter + 16 u S — plus what the gradient's own allowance
    dg = GRAD_BOUND |g| may move the update by (that file's slope of the update in g)."""
    import torch
    from tests.test_gpu_adam import BETAS, EPS as ADAM_EPS, U, f32, half_ulp
    b1, b2 = BETAS
    lr = f32(lr)
    m, v = (1 - b1) * g, (1 - b2) * g * g
    bc1, bc2 = 1 - b1, 1 - b2
    denom = v.sqrt() / math.sqrt(bc2) + ADAM_EPS
    want = p - lr / bc1 * m / denom
    S = lr / bc1 * m.abs() / denom
    slope = (1 - b1) / denom + m.abs() * (1 - b2) * g.abs() / (v.sqrt().clamp(min=1e-300) * math.sqrt(bc2) * denom * denom)
    bound = half_ulp(torch.maximum(want.abs(), p.abs())) + 16 * U * S + lr / bc1 * slope * GRAD_BOUND * g.abs()
    return want, bound


def _culled_steps(use_graph, steps):
    """`steps` steps of AvatarStep(scale_term=REFERENCE_SCALE_TERM) on the culled scene.  Per step: the parameters before it, the
    `reg_loss` it left and the stand-alone launch's words on those parameters."""
    import torch
    from fateavatar_amd.avatar import REFERENCE_SCALE_TERM, AvatarStep
    from fateavatar_amd.loss import scale_ratio_term_and_grad
    C = _scene()
    S, dev = C["S"], C["dev"]
    pc = C["make"]()
    st = AvatarStep(pc, S["faces"], S["canon"], C["away"].clone(), C["bg"], use_graph=use_graph, scale_term=REFERENCE_SCALE_TERM)
    assert tuple(st.reg_loss.shape) == (2,) and st.scale_term == REFERENCE_SCALE_TERM
    gt = torch.ones(3, RES, RES, device=dev)
    rec = []
    for k in range(steps):
        before = pc.flat.detach().clone()
        alone = scale_ratio_term_and_grad(pc._scaling.detach().clone(), None, terms=REFERENCE_SCALE_TERM).clone()
        loss = st.step(C["away"], S["posed"][k % FRAMES], gt)
        torch.cuda.synchronize()
        assert int((st.out["radii"] > 0).sum()) == 0 and float(loss) == 0.0 and int(st._dimage.count_nonzero()) == 0
        rec.append((before, st.reg_loss.clone(), alone, pc.flat.detach().clone()))
    st.check()
    return pc, st, rec


def test_the_step_applies_the_term_alone_on_a_culled_scene(gpu_device):
    import torch
    from fateavatar_amd.avatar import FATE_LRS, REFERENCE_SCALE_TERM
    steps = 5                                          # two eager steps, then three replays of the captured one
    pc_e, st_e, rec_e = _culled_steps(False, steps)
    pc_g, st_g, rec_g = _culled_steps(True, steps)
    assert st_e._graph is None and st_g._graph is not None and st_g.overflows == 0 and st_g.adam.step_count == steps
    # `reg_loss` is the stand-alone launch's words on the step's parameters, bit for bit, and follows them from replay to replay
    for k in range(steps):
        for rec in (rec_e, rec_g):
            assert torch.equal(rec[k][1], rec[k][2]), k
        assert torch.equal(rec_g[k][1], rec_e[k][1]) and torch.equal(rec_g[k][3], rec_e[k][3]), k     # captured == eager, same bits
    words = [float(r[1][0]) for r in rec_g]
    assert all(b < a for a, b in zip(words, words[1:])) and words[0] > 0, words
    # the first step: Adam on weight x g for `_scaling`, and nothing for the other groups
    before, after = rec_e[0][0], rec_e[0][3]
    w, thr = REFERENCE_SCALE_TERM
    s0 = _scene()["scaling"].cpu()
    _, count, g = R.loss_count_grad(s0, w, thr)
    assert float(rec_e[0][1][1]) == count and abs(count - P_SCENE / 3) < 0.1 * P_SCENE
    P = pc_e.P
    off = 0
    for name, width in pc_e.FIELDS:
        a, b = before[off:off + P * width], after[off:off + P * width]
        off += P * width
        if name != "_scaling":
            assert torch.equal(a, b), name               # (a zero gradient from zero moments moves nothing)
            continue
        want, bound = _adam_first_step(a.cpu().double().view(P, 3), g, FATE_LRS["scaling"])
        err = (b.cpu().double().view(P, 3) - want).abs()
        moved = g != 0
        print(f"first Adam step on the term alone: worst error / bound {float((err / bound).max()):.3f}, moved entries {int(moved.sum())}")
        assert bool((err <= bound).all()) and torch.equal(b.cpu().view(P, 3)[~moved], a.cpu().view(P, 3)[~moved])
        assert int(moved.sum()) == 2 * count and float((b - a).abs().max()) > 0.9 * FATE_LRS["scaling"]


@pytest.mark.parametrize("chain", [True, False])
@pytest.mark.parametrize("K", [2, 4])
def test_batch_step_adds_the_term_once(gpu_device, K, chain):
    """K culled views: the term goes once into lane 0's gradient with K x weight, Adam's 1 / K gives weight — the parameters after
    one step are AvatarStep's bit for bit (K x w x g / K is exact for a power of two)."""
    import torch
    from fateavatar_amd.avatar import REFERENCE_SCALE_TERM, AvatarBatchStep
    C = _scene()
    S, dev = C["S"], C["dev"]
    _, _, rec = _culled_steps(False, 1)
    pc = C["make"]()
    st = AvatarBatchStep(pc, S["faces"], S["canon"], C["away"].clone(), C["bg"], views_per_step=K, chain=chain, use_graph=False,
                         scale_term=REFERENCE_SCALE_TERM)
    gt = torch.ones(3, RES, RES, device=dev)
    losses = st.step([C["away"]] * K, [S["posed"][0]] * K, [gt] * K)
    torch.cuda.synchronize()
    assert all(float(x) == 0.0 for x in losses)
    assert torch.equal(st.reg_loss, rec[0][1])
    assert torch.equal(pc.flat.detach(), rec[0][3]) and not torch.equal(pc.flat.detach(), rec[0][0])


def test_with_a_picture_the_term_holds_the_anisotropy_down(gpu_device):
    """The camera on the mesh, 20 steps from one state with and without the term: the unweighted scale_loss of the parameters
    falls with it and does not fall without it.  A step built with scale_term=None is the step built without the argument: no
    buffer, no workspace, and what its first step computes in front of the rasterizer's backward — the render, the loss, the
    image gradient — has the same bits (behind it the blend backward's float atomics make two runs of ANY step agree to
    rounding only, tests/test_gpu_step_ops.py)."""
    import torch
    from fateavatar_amd.avatar import REFERENCE_SCALE_TERM, AvatarStep
    from fateavatar_amd.loss import scale_ratio_term_and_grad
    C = _scene()
    S, dev, bg = C["S"], C["dev"], C["bg"]
    gts = _targets(S, dev, bg)
    measure = lambda pc: float(scale_ratio_term_and_grad(pc._scaling.detach().clone(), None, terms=REFERENCE_SCALE_TERM)[0])  # noqa: E731
    runs = {}
    for what, kw in (("with", dict(scale_term=REFERENCE_SCALE_TERM)), ("none", dict(scale_term=None)), ("absent", {})):
        pc = C["make"]()
        st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), bg, **kw)
        start = measure(pc)
        first = None
        for it in range(20 if what != "absent" else 1):
            f = it % FRAMES
            loss = st.step(S["cams"][f], S["posed"][f], gts[f])
            if first is None:
                torch.cuda.synchronize()
                first = (st.out["render"].clone(), loss.clone(), st._dimage.clone())
                assert float(loss) > 0 and int((st.out["radii"] > 0).sum()) > P_SCENE // 2
        torch.cuda.synchronize()
        st.check()
        runs[what] = (st, start, measure(pc), first)
        print(f"scale_loss over 20 steps, term {what}: {start:.6f} -> {runs[what][2]:.6f}")
    st, start, end, _ = runs["with"]
    assert end < start and float(st.reg_loss[0]) > 0 and st._graph is not None
    st, start, end, _ = runs["none"]
    assert end >= start and st.reg_loss is None and st._ratio_ws is None and st.scale_term is None
    assert runs["absent"][0].reg_loss is None and runs["absent"][0]._ratio_ws is None
    for a, b in zip(runs["none"][3], runs["absent"][3]):
        assert torch.equal(a, b)


def _recount(scaling, thr=9.0, band=1e-5):
    """(lo, hi): the rows over the threshold by a host recount in float64, leaving rows within `band` of it undecided — trained
    parameters keep no margin, and the kernel's float32 ratio is half a dozen roundings (4e-7) from the float64 one; without a
    row in the band lo == hi and the count is held exactly."""
    import torch
    scale = torch.exp(scaling.detach().cpu().double())
    ratio = scale.max(1).values / scale.min(1).values
    return int((ratio > thr * (1 + band)).sum()), int((ratio > thr * (1 - band)).sum())


def test_the_term_composes_with_the_other_options(gpu_device):
    """One step each with the mesh terms and a fused FLAME, and with the perceptual term on the narrow VGG; then across a
    densification and a checkpoint round trip: `reg_loss` is finite and its count is a host recount of the parameters the step
    read."""
    import torch
    from fateavatar_amd import flame
    from fateavatar_amd.avatar import REFERENCE_SCALE_TERM, AvatarStep
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS
    from fateavatar_amd.perceptual import Perceptual, VggFeatures
    from tests import vgg_ref
    from tests.test_gpu_flame import _step_setup
    dev = gpu_device

    def stretched(pc, seed):
        with torch.no_grad():
            pc._scaling.copy_(_drawn(pc.P, seed, over=1.0 / 3.0, shift=SHIFT).to(dev))
        return pc

    def held(st, pc, run):
        lo, hi = _recount(pc._scaling)
        run()
        torch.cuda.synchronize()
        print(f"rows over the threshold: step {float(st.reg_loss[1]):.0f}, host recount {lo} .. {hi} of {pc.P}")
        assert bool(torch.isfinite(st.reg_loss).all()) and float(st.reg_loss[0]) > 0 and 0 < lo <= float(st.reg_loss[1]) <= hi, (st.reg_loss, lo, hi)

    # ---- mesh terms + FLAME inside the step
    F = _step_setup(6)
    pc = stretched(F["make"](), 21)
    st = AvatarStep(pc, F["faces"], F["canon"], F["cams"][0].clone(), F["bg"], use_graph=False, mesh_terms=REFERENCE_MESH_TERMS,
                    flame=F["model"](), scale_term=REFERENCE_SCALE_TERM)
    held(st, pc, lambda: st.step(F["cams"][1], F["frames"][1], F["gts"][1]))
    assert bool(torch.isfinite(st.mesh_loss).all()) and float(st.loss) > 0
    # ---- the perceptual term
    C = _scene()
    S, bg = C["S"], C["bg"]
    gts = _targets(S, dev, bg)
    W, B = vgg_ref.he_weights(vgg_ref.NARROW, seed=21)
    p = Perceptual(VggFeatures(vgg_ref.NARROW, W, B, size=(24, 24), device=dev), weight=0.1)
    pc = C["make"]()
    st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), bg, use_graph=False, perceptual=p, scale_term=REFERENCE_SCALE_TERM)
    held(st, pc, lambda: st.step(S["cams"][1], S["posed"][1], gts[1]))
    assert float(st.perceptual_loss[0]) > 0
    # ---- a densification changes P: the next step's count is that of the new rows too
    pc = C["make"]()
    st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), bg, scale_term=REFERENCE_SCALE_TERM)
    for f in range(3):
        held(st, pc, lambda: st.step(S["cams"][f], S["posed"][f], gts[f]))
    assert st.uv_densify(200, generator=torch.Generator(device=dev).manual_seed(3)) == 200 and st.pc.P == P_SCENE + 200
    for f in range(4):                                 # (eager again, then captured over the new buffers)
        held(st, st.pc, lambda: st.step(S["cams"][f], S["posed"][f], gts[f]))
    # ---- the term has no state: a checkpoint is what it is without it, and the restored step goes on
    sd = st.state_dict()
    plain = AvatarStep(C["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg)
    assert sorted(plain.state_dict()) == sorted(sd)
    st2 = AvatarStep(C["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg, use_graph=False, scale_term=REFERENCE_SCALE_TERM)
    st2.load_state_dict(sd)
    assert st2.pc.P == P_SCENE + 200 and torch.equal(st2.pc.flat, st.pc.flat)
    held(st2, st2.pc, lambda: st2.step(S["cams"][0], S["posed"][0], gts[0]))
