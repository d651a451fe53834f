"""-m gpu: SplattingAvatar's objective on the device — the L1 + MSE image term (`fr_pixel_loss_grad`), the scale term
(`fr_scale_term`) and the step that carries both (`SplattingStep(image_loss=, scale_term=)`).  The reference of every comparison
is the float64 torch restatement of tests/splatting_loss_ref.py (pinned on the CPU by tests/test_splatting_loss_host.py)."""
import functools
import math

import numpy as np
import pytest

from tests import splatting_loss_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24            # one float32 rounding, relative
FACTOR = 4.0                # the kernel's error against float64 may be this many times the float32 restatement's (tests/test_gpu_mlp.py)
REF = R.REFERENCE
SHAPES = [(1, 1, 3), (3, 5, 7), (3, 64, 64), (3, 600, 600)]      # n < 4; a tail of 1; whole float4s; n / 4 > 1024 x 256: workgroups stride
WEIGHTS = [(1.0, 10.0), (1.0, 0.0), (0.0, 1.0)]
SCALE_ROWS = [1, 63, 64, 65, 257, 1025, 300_001]                 # the last: past the 1024 x 256 rows one sweep covers


def _rel(a, b):
    import torch
    return float(torch.linalg.norm(a.double().reshape(-1) - b.double().reshape(-1)) / torch.linalg.norm(b.double().reshape(-1)))


def _zeroed(ws):
    return not bool(ws.any())


# ------------------------------------------------------------------ 1. the image term
@functools.lru_cache(maxsize=None)
def _images(shape):
    """(img, gt) float32 on the CPU; every fifth value (from index 1) of gt IS img's: exactly-equal pixels."""
    import torch
    g = torch.Generator().manual_seed(1000 + shape[1] * shape[2])
    img, gt = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    gt.view(-1)[1::5] = img.view(-1)[1::5]
    return img, gt


@functools.lru_cache(maxsize=None)
def _pixel_refs(shape, weights):
    """The float64 restatement and the float32 one of the same inputs: ((loss64, grad64), (loss32, grad32))."""
    import torch
    img, gt = _images(shape)
    return R.pixel_terms(img, gt, *weights), R.pixel_terms(img, gt, *weights, dtype=torch.float32)


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_pixel_loss_matches_float64(gpu_device, shape, weights):
    """`pixel_loss_and_grad` against float64 autograd of rgb_weight * L1Loss + mse_weight * MSELoss.
    Bound (the convention of tests/test_gpu_mlp.py): the float32 restatement on the CPU has a rel-L2 error e32 against float64
    for the gradient and for the three loss words; the kernel may have at most 4 x e32 of each (another summation order, a
    multiplication by the rounded 1 / n where torch divides).  The gradient's e32 is that of up to a million entries and is
    taken as measured.  The loss words are THREE floats, two of them often the same: their e32 is a draw between nothing and a
    few roundings, not a scale — at [3,64,64] the restatement's L1 word lies 0.22 ulp from the float64 value and the kernel's,
    which the bit-equality below ties to `fr_l1_loss_grad`'s, 0.78 ulp: 3.6 x.  So for the words e32 counts as no less than
    one float32 rounding, 2^-24 relative: what a correctly rounded word may be off by.  (Measured on MI355X, kernel / e32
    before that floor: gradient 0.70 .. 1.01; words 0.03 .. 3.73 and 5.74 at [3,64,64] x (1, 10), where the kernel has 9.1e-8
    and the restatement 1.6e-8.)  Then: loss[1] is `l1_loss_and_grad`'s loss bit for bit, exactly-equal pixels get a gradient
    of exactly 0, `grad_out=False` gives the same loss bits, the workspace is left zeroed."""
    import torch
    from fateavatar_amd.loss import PixelLoss, l1_loss_and_grad, pixel_loss_and_grad, pixel_loss_workspace
    dev = gpu_device
    img, gt = _images(shape)
    (loss64, grad64), (loss32, grad32) = _pixel_refs(shape, weights)
    x, y = img.to(dev), gt.to(dev)
    ws = pixel_loss_workspace(dev)
    loss, grad = pixel_loss_and_grad(x, y, PixelLoss(*weights), workspace=ws)
    torch.cuda.synchronize()
    assert loss.shape == (3,) and grad.shape == x.shape and _zeroed(ws)
    loss_c, grad_c = loss.cpu(), grad.cpu()
    for name, got, r32, r64, floor in (("gradient", grad_c, grad32, grad64, 0.0), ("loss words", loss_c, loss32, loss64, EPS)):
        e32, err = _rel(r32, r64), _rel(got, r64)
        print(f"{shape} {weights} {name}: kernel {err:.3e}  float32 restatement {e32:.3e}  ratio {err / max(e32, 1e-300):.2f}")
        assert float(r64.abs().max()) > 0
        assert err <= FACTOR * max(e32, floor), (name, err, e32)
    print(f"{shape} {weights} words: got {loss_c.tolist()} float32 {loss32.tolist()} float64 {loss64.tolist()}")
    # the L1 word is the L1 kernel's
    l1, _ = l1_loss_and_grad(x, y)
    assert torch.equal(loss[1].reshape(()), l1.reshape(()))
    # sign(0) = 0 and 2 d = 0
    same = (img == gt)
    assert int(same.sum()) >= 1 and bool((grad_c[same] == 0).all()) and bool((grad_c[~same] != 0).all())
    # losses only
    loss_only, none = pixel_loss_and_grad(x, y, PixelLoss(*weights), grad_out=False, workspace=ws)
    torch.cuda.synchronize()
    assert none is None and torch.equal(loss_only, loss) and _zeroed(ws)


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 600, 600)])
def test_pixel_loss_is_reproducible_and_capturable(gpu_device, shape):
    """Two launches give the same bits, and so do two replays of a captured launch (buffers filled with garbage in between); [1,C,H,W]
    and the step's buffer conventions (loss_out / grad_out) are taken."""
    import torch
    from fateavatar_amd.loss import PixelLoss, pixel_loss_and_grad, pixel_loss_workspace
    dev = gpu_device
    img, gt = _images(shape)
    x, y = img.to(dev), gt.to(dev)
    w = PixelLoss(1.0, 10.0)
    ws = pixel_loss_workspace(dev)
    l1, g1 = pixel_loss_and_grad(x, y, w, workspace=ws)
    l2, g2 = pixel_loss_and_grad(x[None], y[None], w, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(g1, g2[0]) and g2.shape == (1,) + tuple(shape)
    l_out, g_out = torch.zeros(3, device=dev), torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pixel_loss_and_grad(x, y, w, loss_out=l_out, grad_out=g_out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        l_out.fill_(float("nan"))
        g_out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(l_out, l1) and torch.equal(g_out, g1) and _zeroed(ws)
    with pytest.raises(RuntimeError, match="shapes differ"):
        pixel_loss_and_grad(x, y[:, :-1], w)
    with pytest.raises(RuntimeError, match="bad output buffers"):
        pixel_loss_and_grad(x, y, w, loss_out=torch.zeros(2, device=dev))
    with pytest.raises(RuntimeError, match="pixel_loss_workspace"):
        pixel_loss_and_grad(x, y, w, workspace=torch.zeros(16, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------ 2. the scale term
@functools.lru_cache(maxsize=None)
def _scale_case(P):
    """(_scaling [P,3] float32 by the redraw rule, the float64 restatement's (loss, count, gradient, selection), a non-zero
    gradient array to add onto), all on the CPU."""
    import torch
    g = torch.Generator().manual_seed(200 + P)
    s = R.draw_scaling(P, g)
    assert not bool(R.undecided_rows(s, REF["scale_threshold"], REF["max_scaling"]).any())
    before = (torch.rand(P, 3, generator=g) + 0.5) / P
    return s, R.scale_term(s, REF["scale_weight"], REF["scale_threshold"], REF["max_scaling"]), before


def _ref_terms():
    from fateavatar_amd.loss import ScaleTerm
    return ScaleTerm(REF["scale_weight"], REF["scale_threshold"], REF["max_scaling"])


@pytest.mark.parametrize("P", SCALE_ROWS)
def test_scale_term_matches_float64_autograd(gpu_device, P):
    """`scale_term_and_grad` with the reference's weight and gates against float64 autograd of
        smax[sel].mean(),  sel = (smax > 0.008) & (smax / smin > 10),  smax / smin of exp(_scaling)
    added to a gradient array pre-filled with non-zero values: expected = before + weight * g.  Inputs by the redraw rule of
    tests/splatting_loss_ref.py (no row within 1e-4 of a gate, no two largest components within 1e-6): no selection and no
    argmax can flip under float32 rounding, so NO row is left out.  The count is exact.  Bound on the loss and on every gradient
    entry: |got - want| <= (1e-4 + 2 x 2^-24) |want|, the bound of test_regulariser_kernel_matches_float64_autograd — here the
    gradient's arithmetic is expf (<= 2 roundings), weight / count and one product, nothing is amplified by a difference; the
    loss is a tree sum of <= 300 001 non-negative terms (about twenty roundings, each relative to a partial sum) and one
    division.  Unselected rows keep their bits; the workspace is left zeroed."""
    import torch
    from fateavatar_amd.loss import scale_term_and_grad, scale_term_workspace
    dev = gpu_device
    s, (loss64, count, g64, sel), before = _scale_case(P)
    if P >= 63:
        assert 0.55 * P < count < 0.75 * P, count
    d = before.to(dev)
    ws = scale_term_workspace(dev)
    out = scale_term_and_grad(s.to(dev), d, terms=_ref_terms(), workspace=ws)
    torch.cuda.synchronize()
    assert _zeroed(ws) and out.shape == (2,)
    got_loss, got_count, got = float(out[0]), float(out[1]), d.cpu()
    print(f"P={P}: selected {count} of {P}, loss got {got_loss:.9g} want {float(loss64):.9g}")
    assert got_count == count
    assert abs(got_loss - float(loss64)) <= (1e-4 + 2 * EPS) * float(loss64)
    want = before.double() + g64
    err = (got.double() - want).abs()
    bound = (1e-4 + 2 * EPS) * want.abs()
    print(f"P={P} d_scaling: max |got - want| / |want| = {float((err / want.abs()).max()):.3e}, entries over the bound: {int((err > bound).sum())}")
    assert bool(torch.isfinite(got).all()) and int((err > bound).sum()) == 0
    assert torch.equal(got[~sel], before[~sel])                      # unselected rows: their bits
    touched = (got != before)
    assert int(touched.sum()) == count and bool((touched.sum(dim=1) <= 1).all())     # one entry per selected row, ADDED to
    assert torch.equal(touched.any(dim=1), sel)


def test_scale_term_gates_and_reproducibility(gpu_device):
    """An empty selection (all scales 1e-4): loss 0, count 0, `d_scaling` keeps its bits, nothing is divided by the empty count.
    Every row selected: the count is P.  Weight 0 and a null `d_scaling`: the same losses, no gradient traffic.  A row with a
    NaN — at its largest component or beside it — is not selected, its gradient row keeps its bits and the other rows' results
    are those without it.  Equal components (selectable only with scale_threshold < 1): the first takes the gradient.  P = 0.
    Two launches and two graph replays give the same bits; the workspace is left zeroed."""
    import torch
    from fateavatar_amd.loss import ScaleTerm, scale_term_and_grad, scale_term_workspace
    dev = gpu_device
    terms = _ref_terms()
    ws = scale_term_workspace(dev)
    P = 1025
    before = ((torch.rand(P, 3, generator=torch.Generator().manual_seed(3)) + 0.5) / P).to(dev)
    # ---- nothing selected
    s = torch.full((P, 3), math.log(1e-4), device=dev)
    d, out = before.clone(), torch.full((2,), 7.0, device=dev)
    assert scale_term_and_grad(s, d, out=out, terms=terms, workspace=ws) is out
    torch.cuda.synchronize()
    assert out.tolist() == [0.0, 0.0] and torch.equal(d, before) and _zeroed(ws)
    # ---- everything selected
    s = torch.tensor([math.log(0.1), math.log(0.001), math.log(0.002)], device=dev).repeat(P, 1).contiguous()
    d = before.clone()
    out = scale_term_and_grad(s, d, terms=terms, workspace=ws)
    torch.cuda.synchronize()
    assert float(out[1]) == P and abs(float(out[0]) - 0.1) <= 1e-6 and _zeroed(ws)
    assert torch.equal(d[:, 1:], before[:, 1:]) and bool((d[:, 0] > before[:, 0]).all())
    # ---- weight 0, null d_scaling
    s_cpu, (loss64, count, g64, sel), _ = _scale_case(P)
    s = s_cpu.to(dev)
    d = before.clone()
    full = scale_term_and_grad(s, d, terms=terms, workspace=ws)
    d0 = before.clone()
    out0 = scale_term_and_grad(s, d0, terms=ScaleTerm(0.0, terms.scale_threshold, terms.max_scaling), workspace=ws)
    outn = scale_term_and_grad(s, None, terms=terms, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(d0, before) and torch.equal(out0, full) and torch.equal(outn, full) and float(full[1]) == count and _zeroed(ws)
    # ---- NaN rows: row a's LARGEST component, row b's smallest (its largest stays a number)
    a, b = [int(i) for i in torch.nonzero(sel)[:2, 0]]
    s_nan = s_cpu.clone()
    s_nan[a, int(s_cpu[a].argmax())] = float("nan")
    s_nan[b, int(s_cpu[b].argmin())] = float("nan")
    keep = torch.ones(P, dtype=torch.bool)
    keep[[a, b]] = False
    loss_k, count_k, g_k, sel_k = R.scale_term(s_cpu[keep], terms.weight, terms.scale_threshold, terms.max_scaling)
    assert count_k == count - 2
    d_nan = before.clone()
    out_nan = scale_term_and_grad(s_nan.to(dev), d_nan, terms=terms, workspace=ws)
    torch.cuda.synchronize()
    assert float(out_nan[1]) == count_k and abs(float(out_nan[0]) - float(loss_k)) <= (1e-4 + 2 * EPS) * float(loss_k)
    assert torch.equal(d_nan[[a, b]], before[[a, b]]) and bool(torch.isfinite(d_nan).all()) and _zeroed(ws)
    want = before.cpu()[keep].double() + g_k
    assert bool(((d_nan.cpu()[keep].double() - want).abs() <= (1e-4 + 2 * EPS) * want.abs()).all())
    # ---- equal components: the FIRST index (torch.max's)
    s_eq = torch.full((5, 3), math.log(0.1), device=dev)
    d_eq = torch.zeros(5, 3, device=dev)
    out_eq = scale_term_and_grad(s_eq, d_eq, terms=ScaleTerm(1.0, 0.5, 0.008), workspace=ws)
    torch.cuda.synchronize()
    assert float(out_eq[1]) == 5 and bool((d_eq[:, 0] > 0).all()) and not bool(d_eq[:, 1:].any())
    assert abs(float(d_eq[0, 0]) - 0.1 / 5) <= 1e-6 * 0.02
    # ---- P = 0
    out_z = scale_term_and_grad(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), terms=terms, workspace=ws)
    torch.cuda.synchronize()
    assert out_z.tolist() == [0.0, 0.0] and _zeroed(ws)
    # ---- the same bits on every launch and every replay
    d2 = before.clone()
    again = scale_term_and_grad(s, d2, terms=terms, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(again, full) and torch.equal(d2, d)
    g_d, g_out = before.clone(), torch.zeros(2, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scale_term_and_grad(s, g_d, out=g_out, terms=terms, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        g_d.copy_(before)
        g_out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_out, full) and torch.equal(g_d, d) and _zeroed(ws)
    with pytest.raises(RuntimeError, match=r"\[P,3\]"):
        scale_term_and_grad(s, before[:-1].contiguous(), terms=terms)
    with pytest.raises(RuntimeError, match="2-element"):
        scale_term_and_grad(s, None, out=torch.zeros(3, device=dev), terms=terms)


# ------------------------------------------------------------------ 3. the step
from tests.test_gpu_phong import _targets, _template  # noqa: E402

N_FIRED = 64     # rows set to (0.05, 0.001, 0.002): over both gates whatever the sampled scales are


def _fired(make, dev):
    import torch
    pc = make()
    with torch.no_grad():
        pc._scaling[:N_FIRED] = torch.tensor([math.log(0.05), math.log(0.001), math.log(0.002)], device=dev)
    return pc


def _scale_of(pc):
    """The float64 restatement of the holder's present `_scaling`: (loss, count, gradient [P,3], selection)."""
    from fateavatar_amd.splatting import REFERENCE_SCALE_TERM as T
    return R.scale_term(pc._scaling.detach().cpu(), T.weight, T.scale_threshold, T.max_scaling)


def test_splatting_step_with_the_reference_objective(gpu_device, monkeypatch):
    """SplattingStep(image_loss=REFERENCE_IMAGE_LOSS, scale_term=REFERENCE_SCALE_TERM), 10 000 Gaussians at 128 x 128, 64 rows
    reshaped so that the scale term fires:
    (a) one eager step: every field's run of flat_grad against the `fold_binding=False` route back-propagating the FLOAT64
        dL/dimage of the restatement (rounded to float32 once), plus the float64 scale gradient on `_scaling`: rel-L2 <= 1e-4 —
        twice the 5e-5 tests/test_gpu_phong.py holds the folded binding to against the op; the image gradient's own float32
        arithmetic is a handful of roundings per pixel —; loss_terms against float64 to 1e-5, reg_loss against float64;
        and the scale term's share alone: flat_grad minus that of a twin WITHOUT the term, on the selected entries, against the
        float64 gradient to 1e-4 relative plus 8 x the backward's run-to-run floor (twin against twin; the backward sums with
        float atomics) plus one rounding of the largest entry;
    (b) six steps: after each the parameters equal torch.optim.Adam fed the step's own flat_grad (rtol 2e-6, atol 1e-7), and
        reg_loss holds the term of the parameters the step started from;
    (c) 30 steps, graph against eager: util.assert_same_trajectory;
    (d) a checkpoint round trip;
    (e) a default SplattingStep built beside it never reaches the new entry points, has no loss_terms / reg_loss, its first
        loss has the bits of a default step run alone, and its `flat` after three steps equals that run's — bit for bit if two
        default runs alone agree bit for bit, else within util.assert_same_trajectory (the backward's float atomics)."""
    import torch
    import fateavatar_amd.splatting as splatting
    import fateavatar_amd.train as train
    from fateavatar_amd.loss import ImageLoss, PixelLoss
    from fateavatar_amd.splatting import REFERENCE_IMAGE_LOSS, REFERENCE_SCALE_TERM, SPLATTING_LRS, SplattingGaussians, SplattingStep
    from tests import util
    dev = gpu_device
    res, n_frames, N = 128, 4, 10_000
    S = _template(dev, res, n_frames, seed=2)
    bg = torch.ones(3, device=dev)
    make, gts = _targets(S, dev, bg, n_frames, N)
    calls = []
    real_p, real_s = train.pixel_loss_and_grad, splatting.scale_term_and_grad
    monkeypatch.setattr(train, "pixel_loss_and_grad", lambda *a, **k: (calls.append("pixel"), real_p(*a, **k))[1])
    monkeypatch.setattr(splatting, "scale_term_and_grad", lambda *a, **k: (calls.append("scale"), real_s(*a, **k))[1])
    frame = lambda st, f: st.step(S["cams"][f], S["posed"][f], gts[f])  # noqa: E731

    def step_of(use_graph=False, **kw):
        return SplattingStep(_fired(make, dev), S["canonical"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=use_graph, **kw)

    both = dict(image_loss=REFERENCE_IMAGE_LOSS, scale_term=REFERENCE_SCALE_TERM)
    # ---- (e), first half: default steps alone, before anything else ran
    alone = []
    for _ in range(2):
        st = step_of()
        first = frame(st, 0).clone()
        frame(st, 1), frame(st, 2)
        torch.cuda.synchronize()
        alone.append((first, st.pc.flat.clone()))
    assert calls == [] and torch.equal(alone[0][0], alone[1][0])
    # ---- (a)
    st_w, st_i, st_j = step_of(**both), step_of(image_loss=REFERENCE_IMAGE_LOSS), step_of(image_loss=REFERENCE_IMAGE_LOSS)
    st_r = step_of(fold_binding=False)
    assert st_i.reg_loss is None and st_w.reg_loss.shape == (2,) and st_w.loss_terms.shape == (3,)
    assert isinstance(st_w.image_loss, PixelLoss) and st_w.loss.data_ptr() == st_w.loss_terms.data_ptr()
    loss64, count, g64, sel = _scale_of(st_w.pc)
    assert count >= N_FIRED and bool(sel[:N_FIRED].all())
    seen = {}

    def float64_image_gradient(image):
        terms, g = R.pixel_terms(image.detach().cpu(), st_r.gt.cpu(), *REFERENCE_IMAGE_LOSS)
        seen["terms"] = terms
        return g.float().to(dev)

    st_r._image_loss_and_grad = float64_image_gradient
    for s in (st_w, st_i, st_j, st_r):
        frame(s, 1)
    torch.cuda.synchronize()
    assert calls == ["pixel", "scale", "pixel", "pixel"]
    assert torch.allclose(st_w.loss_terms.cpu().double(), seen["terms"], rtol=1e-5, atol=0) and float(st_w.loss_terms[2]) > 0
    assert float(st_w.reg_loss[1]) == count > 0 and abs(float(st_w.reg_loss[0]) - float(loss64)) <= 2e-4 * float(loss64)
    for name, w in st_w.pc.FIELDS:
        if not w:
            continue
        got, want = st_w.pc.grad_view(name).double().cpu(), st_r.pc.grad_view(name).double().cpu()
        if name == "_scaling":
            want = want + g64
        err = util.rel_l2(got.numpy(), want.numpy())
        print(f"(a) {name}: rel-L2 against the float64 route {err:.3e}, max |want| {float(want.abs().max()):.3e}")
        assert err <= 1e-4 and (name == "_uvd" or float(want.abs().max()) > 0), (name, err)
    a, b, w = (s.pc.grad_view("_scaling").double().cpu() for s in (st_i, st_j, st_w))
    floor = float((a - b).abs().max()) + EPS * float(w.abs().max())
    err = ((w - a) - g64).abs()
    print(f"(a) scale term alone: floor {floor:.3e}, max error {float(err.max()):.3e}, max |g| {float(g64.abs().max()):.3e}")
    assert bool((err <= 1e-4 * g64.abs() + 8 * floor).all()) and float(g64.abs().max()) > 100 * floor
    # ---- (b)
    st = step_of(**both)
    pc = st.pc
    sizes = [n for n, _ in st.adam_segments()]
    ref = [t.clone().requires_grad_() for t in torch.split(pc.flat.detach(), sizes)]
    lrs = [SPLATTING_LRS[k] for k in ("uvd", "opacity", "feature_dc", "feature_rest", "rotation", "scaling")]
    topt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(ref, lrs)], lr=0.0)
    for it in range(6):
        loss64, count, _, _ = _scale_of(pc)
        loss = frame(st, it % n_frames)
        for p, g in zip(ref, torch.split(pc.flat_grad, sizes)):
            p.grad = g.clone()
        topt.step()
        want = torch.cat([p.detach() for p in ref])
        assert torch.allclose(pc.flat, want, rtol=2e-6, atol=1e-7), (it, float((pc.flat - want).abs().max()))
        assert loss is st.loss and float(loss) > 0 and float(st.loss_terms[2]) > 0
        lt = st.loss_terms.double()
        assert abs(float(lt[0]) - float(lt[1] + 10.0 * lt[2])) <= 4 * EPS * float(lt[0])
        assert float(st.reg_loss[1]) == count > 0 and abs(float(st.reg_loss[0]) - float(loss64)) <= 2e-4 * float(loss64)
    assert st.adam.step_count == 6
    # ---- (d) checkpoint: another step object restored from the state continues with the same update
    sd = st.state_dict()
    other = SplattingGaussians(torch.zeros(7, dtype=torch.int32), torch.full((7, 3), 1 / 3), -4.0, dev)
    st2 = SplattingStep(other, S["canonical"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False, **both)
    assert st2.load_state_dict(sd) == [] and st2.pc.P == pc.P
    for s in (st, st2):
        frame(s, 2)
    torch.cuda.synchronize()
    util.assert_same_trajectory(st2.pc.flat, pc.flat, "checkpoint round trip", tight=2e-3)
    assert st2.adam.step_count == 7 and torch.equal(st2.reg_loss, st.reg_loss) and torch.allclose(st2.loss_terms, st.loss_terms, rtol=1e-5)
    # ---- (c)
    runs = []
    for use_graph in (False, True):
        s = step_of(use_graph, **both)
        for it in range(30):
            frame(s, it % n_frames)
        torch.cuda.synchronize()
        s.check()
        runs.append(s)
    assert runs[1]._graph is not None and runs[0]._graph is None and runs[1].overflows == 0
    assert runs[0].adam.step_count == runs[1].adam.step_count == 30
    util.assert_same_trajectory(runs[1].pc.flat, runs[0].pc.flat, "graph vs eager, the reference objective", tight=2e-2)
    assert torch.allclose(runs[1].reg_loss, runs[0].reg_loss, rtol=1e-2) and float(runs[0].reg_loss[1]) > 0
    assert torch.allclose(runs[1].loss_terms, runs[0].loss_terms, rtol=2e-2) and float(runs[0].loss_terms[2]) > 0
    # ---- (e), second half: a default step beside all of the above
    calls.clear()
    st_d = step_of()
    first = frame(st_d, 0).clone()
    frame(st_w, 0)
    frame(st_d, 1), frame(st_d, 2)
    torch.cuda.synchronize()
    assert calls == ["pixel", "scale"] and st_d.loss_terms is None and st_d.reg_loss is None and st_d.image_loss is None
    assert torch.equal(first, alone[0][0])
    if torch.equal(alone[0][1], alone[1][1]):
        assert torch.equal(st_d.pc.flat, alone[0][1])
    else:
        util.assert_same_trajectory(st_d.pc.flat, alone[0][1], "default step beside the reference objective", tight=2e-3)
    # ---- refusals, and the generic step takes the term too
    with pytest.raises(TypeError, match=r"ImageLoss.*PixelLoss"):
        step_of(image_loss=(1.0, 10.0))
    with pytest.raises(TypeError, match="ScaleTerm"):
        step_of(scale_term=(1.0, 10.0, 0.008))
    assert isinstance(step_of(image_loss=ImageLoss(0.8, 0.2)).image_loss, ImageLoss)


def test_train_step_takes_a_pixel_loss(gpu_device):
    """TrainStep(image_loss=PixelLoss(1, 10)) on a small random scene: the step's dL/dimage and loss words are the kernel's for the
    image the step rendered, and 12 steps graph against eager."""
    import torch
    from fateavatar_amd import scenes
    from fateavatar_amd.loss import PixelLoss
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    from fateavatar_amd.render import render
    from fateavatar_amd.train import TrainStep
    from tests import util
    dev = gpu_device
    P, res = 2000, 64
    truth = scenes.head_scene(P=P, res=res, sh_degree=1, seed=3, opacity=0.6)
    cam = TorchCamera(truth.camera, dev)
    bg = torch.from_numpy(truth.bg).to(dev)
    with torch.no_grad():
        gt = render(cam, FlatGaussians(truth.means3D, truth.shs, truth.opacities, truth.scales, truth.rotations, 1, dev, fused_activations=True),
                    bg)["render"].clone()
    shs0 = (truth.shs + 0.3 * np.random.default_rng(0).standard_normal(truth.shs.shape)).astype(np.float32)

    def run(use_graph, steps):
        pc = FlatGaussians(truth.means3D, shs0, truth.opacities * 0.7, truth.scales, truth.rotations, 1, dev, fused_activations=True)
        ts = TrainStep(pc, TorchCamera(truth.camera, dev), bg, use_graph=use_graph, image_loss=PixelLoss(1.0, 10.0))
        for _ in range(steps):
            loss = ts.step(cam, gt)
        torch.cuda.synchronize()
        ts.check()
        assert loss is ts.loss and loss.data_ptr() == ts.loss_terms.data_ptr()
        return ts

    one = run(False, 1)
    terms, g = R.pixel_terms(one.out["render"].cpu(), gt.cpu(), 1.0, 10.0)
    assert torch.allclose(one.loss_terms.cpu().double(), terms, rtol=1e-5, atol=0) and float(terms[2]) > 0
    assert util.rel_l2(one._dimage.cpu().numpy(), g.numpy()) <= 1e-6
    eager, graph = run(False, 12), run(True, 12)
    assert graph._graph is not None and eager._graph is None and graph.adam.step_count == eager.adam.step_count == 12
    util.assert_same_trajectory(graph.pc.flat, eager.pc.flat, "TrainStep graph vs eager, L1 + MSE")
    assert float(eager.loss_terms[0]) < float(one.loss_terms[0])


def test_the_scale_term_survives_density_control_and_the_mesh_gradient(gpu_device):
    """The term's scratch is the step's own and does not depend on P: a captured step with both terms and `mesh_grad=True` goes
    through walk_on_triangles, densify_and_prune, prune and reset_opacity, and after each the next step's reg_loss is the float64
    term of the rows the step then has."""
    import torch
    from fateavatar_amd import scenes
    from fateavatar_amd.binding import phong_canonical
    from fateavatar_amd.model import TorchCamera
    from fateavatar_amd.splatting import REFERENCE_IMAGE_LOSS, REFERENCE_SCALE_TERM, SplattingGaussians, SplattingStep
    from tests.test_gpu_phongsurf import TET_FACES, TET_VERTS, _threshold
    dev = gpu_device
    P = 65
    s = scenes.random_scene(P, 64, 64, sh_degree=1, seed=3, tanfov=0.5, spread=0.2)
    rng = np.random.default_rng(7)
    cam, bg = TorchCamera(s.camera, dev), torch.ones(3, device=dev)
    verts, faces = torch.from_numpy(TET_VERTS).to(dev), torch.from_numpy(TET_FACES).to(dev)
    bc = rng.random((P, 3)).astype(np.float32) + 0.1
    bc /= bc.sum(1, keepdims=True)
    gt = torch.from_numpy(rng.random((3, 64, 64)).astype(np.float32)).to(dev)
    pc = SplattingGaussians((np.arange(P) % 4).astype(np.int32), bc, float(np.log(0.05)), dev)
    with torch.no_grad():
        pc._scaling[::2] = float(np.log(0.01))          # every other Gaussian below the clone / split threshold (0.02)
        pc._scaling[::3, 1:] = float(np.log(0.0005))    # every third a needle: ratio 20 or 100, over both gates
    st = SplattingStep(pc, phong_canonical(verts, faces), cam, bg, verts, use_graph=True, mesh_grad=True,
                       image_loss=REFERENCE_IMAGE_LOSS, scale_term=REFERENCE_SCALE_TERM)

    def step_and_check(what):
        loss64, count, _, _ = _scale_of(st.pc)
        st.step(cam, verts + 0.01, gt)
        torch.cuda.synchronize()
        print(f"{what}: P {st.pc.P}, selected {count}, scale_loss {float(st.reg_loss[0]):.6g}")
        assert count > 0 and float(st.reg_loss[1]) == count, what
        assert abs(float(st.reg_loss[0]) - float(loss64)) <= 2e-4 * float(loss64), what
        assert bool(torch.isfinite(st.pc.flat).all()) and float(st.loss_terms[2]) > 0 and float(st.d_verts.abs().max()) > 0, what

    for k in range(4):
        step_and_check(f"step {k}")
    assert st._graph is not None
    st.walk_on_triangles()
    step_and_check("after the walk")
    counts = st.densify_and_prune(max_grad=_threshold(st), generator=torch.Generator().manual_seed(9))
    assert counts[0] > 0 and counts[1] > 0 and st.pc.P != P
    for k in range(4):
        step_and_check(f"after densify_and_prune, step {k}")
    mask = torch.zeros(st.pc.P, dtype=torch.bool, device=dev)
    mask[[0, 7, 64]] = True
    assert st.prune(mask) == 3
    step_and_check("after prune")
    st.reset_opacity()
    step_and_check("after reset_opacity")
    st.check()
