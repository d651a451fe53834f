"""-m gpu: the fused L1 + D-SSIM image loss (`fr_image_loss_grad`: k_image_loss_maps + k_image_loss_grad) on the device — the
kernels against the float64 restatement of tests/image_loss_ref.py (pinned on the CPU by tests/test_image_loss_host.py), their
exact cases, reproducibility, the `d_ssim` autograd op, and the steps that carry the loss (`RiggedStep(image_loss=)`,
`TrainStep(image_loss=)`).

Bounds of every comparison with the restatement (ref.LOSS_ATOL, ref.GRAD_REL_L2, ref.GRAD_ENTRY): each loss scalar within
1e-5, the gradient's rel-L2 within 1e-4 (the project's parity bound), every entry within 1e-4 of max |g64|, no entry exempt.
The float32 twin of the restatement reaches <= 3e-7, <= 1.3e-5 and <= 2.5e-5 on these inputs; the achieved values and the
twin's are printed by the tests, and recorded in profiles/r12_image_loss.md."""
import pytest

from tests import image_loss_ref as ref
from tests.test_gpu_face_local import _perturbed, _targets, _template

pytestmark = pytest.mark.gpu


def _control_bytes(ws, shape):
    """The part of a workspace the kernels need zeroed: everything in front of the 12 C H W bytes of the maps."""
    C, H, W = shape
    return ws[:ws.numel() - 12 * C * H * W]


def _check(name, loss3, grad, want3, want_grad, twin3=None, twin_grad=None):
    dl, rl2, ent = ref.errors(loss3, grad, want3, want_grad)
    msg = f"{name}: loss err {dl:.3e}, grad rel-L2 {rl2:.3e}, worst entry / max|g| {ent:.3e}"
    if twin3 is not None:
        tl, t2, te = ref.errors(twin3, twin_grad, want3, want_grad)
        msg += f"   (float32 restatement: {tl:.3e}, {t2:.3e}, {te:.3e})"
    print(msg)
    import torch
    assert bool(torch.isfinite(loss3).all()) and bool(torch.isfinite(grad).all()), name
    assert dl <= ref.LOSS_ATOL and rl2 <= ref.GRAD_REL_L2 and ent <= ref.GRAD_ENTRY, msg
    return dl, rl2, ent


# ------------------------------------------------------------------ 1. parity at the smallest shapes that can go wrong
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_image_loss_matches_the_float64_restatement(gpu_device, shape, kind):
    """Shapes around the 32 x 32 tile: smaller than the window (every tap padded), the window, one tile, one pixel more and
    one less than a tile, several tiles with ragged edges, one channel; three input kinds; weights (0.8, 0.2), (0, 1), (1, 0)."""
    import torch
    from fateavatar_amd.loss import image_loss_and_grad, image_loss_workspace
    dev = gpu_device
    x, y, t64, t32 = ref.case(shape, kind)
    xd, yd = x.to(dev), y.to(dev)
    ws = image_loss_workspace(dev, *shape)
    for w in ref.WEIGHTS:
        loss3, grad = image_loss_and_grad(xd, yd, w, workspace=ws)
        torch.cuda.synchronize()
        assert loss3.shape == (3,) and grad.shape == xd.shape
        assert not bool(_control_bytes(ws, shape).any())
        _check(f"{shape} {kind} weights {w}", loss3, grad, *ref.combine(t64, w), *ref.combine(t32, w))
        assert abs(float(loss3[0]) - (w[0] * float(loss3[1]) + w[1] * float(loss3[2]))) <= 1e-6


# ------------------------------------------------------------------ 2. exact cases
@pytest.mark.parametrize("shape", [(3, 33, 47), (3, 128, 128), (1, 7, 5)], ids=lambda s: "x".join(map(str, s)))
def test_image_loss_exact_cases(gpu_device, shape):
    """Weights (1, 0): the gradient and the L1 loss are `l1_loss_and_grad`'s bits.  img == gt (random and constant): the L1
    loss and the L1 part of the gradient are exactly zero, |d_ssim| <= 1e-5.  Inputs in -0.5 .. 1.5: everything finite."""
    import torch
    from fateavatar_amd.loss import image_loss_and_grad, image_loss_workspace, l1_loss_and_grad, l1_workspace
    dev = gpu_device
    x, y, _, _ = ref.case(shape, "noise")
    xd, yd = x.to(dev), y.to(dev)
    xd.view(-1)[::7] = yd.view(-1)[::7]                      # ties: sign(0) = 0
    ws = image_loss_workspace(dev, *shape)
    l1, g1 = l1_loss_and_grad(xd, yd, workspace=l1_workspace(dev))
    loss3, g = image_loss_and_grad(xd, yd, (1.0, 0.0), workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(g, g1) and torch.equal(loss3[1], l1) and torch.equal(loss3[0], l1) and float(loss3[2]) == 0.0
    assert int((g == 0).sum()) >= xd.numel() // 7 and not bool(ws.any())
    loss3, g = image_loss_and_grad(xd, yd, (0.25, 0.0), workspace=ws)       # another weight: the same L1, the gradient scaled
    assert torch.equal(loss3[1], l1) and torch.equal(g, torch.sign(g1) * torch.tensor(0.25 / xd.numel(), dtype=torch.float32))
    # the same ties through the D-SSIM kernels: where x == y the L1 term adds an exact zero
    _, g_mix = image_loss_and_grad(xd, yd, (0.8, 0.2), workspace=ws)
    _, g_ssim = image_loss_and_grad(xd, yd, (0.0, 0.2), workspace=ws)
    tie = xd == yd
    assert torch.equal(g_mix[tie], g_ssim[tie]) and not torch.equal(g_mix[~tie], g_ssim[~tie])
    # ---- img == gt
    for same in (yd.clone(), torch.full(shape, 0.37, device=dev), torch.zeros(shape, device=dev)):
        for w in ((0.8, 0.2), (0.0, 1.0), (1.0, 0.0)):
            loss3, g = image_loss_and_grad(same, same.clone(), w, workspace=ws)
            assert float(loss3[1]) == 0.0 and abs(float(loss3[2])) <= 1e-5 and bool(torch.isfinite(g).all()), (w, loss3)
            if w[1] == 0.0:
                assert not bool(g.any())
            else:      # what is left is the D-SSIM part alone, whatever the L1 weight
                _, g0 = image_loss_and_grad(same, same.clone(), (0.0, w[1]), workspace=ws)
                assert torch.equal(g, g0)
    # ---- outside [0, 1]
    wide = (xd * 2.0 - 0.5, yd * 2.0 - 0.5)
    assert float(wide[0].min()) < 0 and float(wide[0].max()) > 1
    for w in ((0.8, 0.2), (0.0, 1.0)):
        loss3, g = image_loss_and_grad(*wide, w, workspace=ws)
        assert bool(torch.isfinite(loss3).all()) and bool(torch.isfinite(g).all())


# ------------------------------------------------------------------ 3. reproducibility and plumbing
def test_image_loss_is_bit_reproducible_and_leaves_its_workspace_ready(gpu_device, monkeypatch):
    """Two launches, and the same launch captured and replayed twice, give identical bits (no float atomics: every output has
    one owner, the sums are added in index order).  After every launch the counters and partial sums of the workspace — all of
    it in front of the maps — are zero again; the maps (12 C H W bytes) are written before they are read and take no initial
    value: a launch on a workspace whose maps hold NaN bits gives the same bits.  A None gradient entry (`image_loss_and_grad_batch`) gives the same losses and
    stores nothing.  [1,C,H,W] inputs are [C,H,W] inputs."""
    import torch
    import fateavatar_amd.loss as loss_mod
    from fateavatar_amd.loss import image_loss_and_grad, image_loss_and_grad_batch, image_loss_workspace
    dev = gpu_device
    shape = (3, 97, 130)
    x, y, _, _ = ref.case(shape, "near")
    xd, yd = x.to(dev), y.to(dev)
    ws = image_loss_workspace(dev, *shape)
    w = (0.8, 0.2)
    loss_a, grad_a = image_loss_and_grad(xd, yd, w, workspace=ws)
    loss_a, grad_a = loss_a.clone(), grad_a.clone()
    torch.cuda.synchronize()
    assert not bool(_control_bytes(ws, shape).any())
    loss_b, grad_b = image_loss_and_grad(xd, yd, w, workspace=ws)
    assert torch.equal(loss_a, loss_b) and torch.equal(grad_a, grad_b) and not bool(_control_bytes(ws, shape).any())
    # the default per-stream workspace, and 4-D inputs
    loss_c, grad_c = image_loss_and_grad(xd[None], yd[None], w)
    n_default = len([k for k in loss_mod._image_workspace if k[0] == dev.index])
    assert grad_c.shape == (1,) + shape and torch.equal(loss_a, loss_c) and torch.equal(grad_a, grad_c[0])
    # maps full of NaN bits
    ws[ws.numel() - 12 * xd.numel():] = 0xFF
    loss_n, grad_n = image_loss_and_grad(xd, yd, w, workspace=ws)
    assert torch.equal(loss_a, loss_n) and torch.equal(grad_a, grad_n)
    # losses only
    ws.zero_()
    loss_l = torch.zeros(3, device=dev)
    image_loss_and_grad_batch([xd], [yd], w, [loss_l], [None], [ws])
    assert torch.equal(loss_a, loss_l) and not bool(ws.any())
    # the default workspace is one per stream, grown to the largest shape: a smaller image reuses it
    small = image_loss_and_grad(xd[:, :40, :50].contiguous(), yd[:, :40, :50].contiguous(), w)
    again = image_loss_and_grad(xd, yd, w)
    assert len([k for k in loss_mod._image_workspace if k[0] == dev.index]) == n_default and torch.equal(again[1], grad_a)
    assert bool(torch.isfinite(small[1]).all())
    # captured and replayed
    g_loss, g_grad = torch.zeros(3, device=dev), torch.zeros_like(xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="graph capture"):
            image_loss_and_grad(xd, yd, w)                   # no workspace of this stream yet: refuses to allocate in a capture
        monkeypatch.undo()
        with pytest.raises(RuntimeError, match="workspace"):
            image_loss_and_grad_batch([xd], [yd], w, [g_loss], [g_grad], [torch.zeros(8, dtype=torch.uint8, device=dev)])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            image_loss_and_grad(xd, yd, w, loss_out=g_loss, grad_out=g_grad, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        g_loss.zero_()
        g_grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_loss, loss_a) and torch.equal(g_grad, grad_a) and not bool(_control_bytes(ws, shape).any())
    with pytest.raises(RuntimeError, match="workspace"):
        image_loss_and_grad(xd, yd, w, workspace=torch.zeros(ws.numel() - 1, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="shapes differ"):
        image_loss_and_grad(xd, yd[:, :, :-1].contiguous(), w)
    with pytest.raises(RuntimeError, match=r"\[C,H,W\]"):
        image_loss_and_grad(xd[0], yd[0], w)
    with pytest.raises(RuntimeError, match="one shape"):
        image_loss_and_grad_batch([xd, xd[:, :, :-1].contiguous()], [yd, yd], w, [g_loss, g_loss.clone()], [None, None], [ws, ws.clone()])


@pytest.mark.parametrize("w", [(0.8, 0.2), (1.0, 0.0)], ids=["dssim", "l1-only"])
def test_image_loss_batch_equals_single_calls(gpu_device, w):
    """Four different images in one launch pair equal four single calls bit for bit; a call with two leaves the other two
    images' buffers alone; a None gradient entry gives that image's losses only."""
    import torch
    from fateavatar_amd.loss import image_loss_and_grad, image_loss_and_grad_batch, image_loss_workspace
    dev = gpu_device
    shape = (3, 45, 70)
    pairs = [ref.make_inputs(shape, k, seed=s) for s, k in enumerate(("noise", "smooth", "near", "noise"))]
    xs, ys = [p[0].to(dev) for p in pairs], [p[1].to(dev) for p in pairs]
    singles = []
    for x, y in zip(xs, ys):
        l, g = image_loss_and_grad(x, y, w, workspace=image_loss_workspace(dev, *shape))
        singles.append((l.clone(), g.clone()))
    wss = [image_loss_workspace(dev, *shape) for _ in range(4)]
    losses, grads = [torch.zeros(3, device=dev) for _ in range(4)], [torch.zeros_like(x) for x in xs]
    image_loss_and_grad_batch(xs, ys, w, losses, grads, wss)
    torch.cuda.synchronize()
    for k in range(4):
        assert torch.equal(losses[k], singles[k][0]) and torch.equal(grads[k], singles[k][1]), k
        assert not bool(_control_bytes(wss[k], shape).any())
    assert not torch.equal(grads[0], grads[3])
    # two of four
    for t in losses + grads:
        t.fill_(-7.0)
    image_loss_and_grad_batch(xs[2:], ys[2:], w, losses[2:], grads[2:], wss[2:])
    torch.cuda.synchronize()
    for k in (0, 1):
        assert bool((losses[k] == -7.0).all()) and bool((grads[k] == -7.0).all())
    for k in (2, 3):
        assert torch.equal(losses[k], singles[k][0]) and torch.equal(grads[k], singles[k][1])
    # a None entry
    for t in losses + grads:
        t.fill_(-7.0)
    image_loss_and_grad_batch(xs[:3], ys[:3], w, losses[:3], [grads[0], None, grads[2]], wss[:3])
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(losses[k], singles[k][0])
    assert torch.equal(grads[0], singles[0][1]) and torch.equal(grads[2], singles[2][1]) and bool((grads[1] == -7.0).all())
    with pytest.raises(RuntimeError, match="one workspace per image"):
        image_loss_and_grad_batch(xs[:2], ys[:2], w, losses[:2], grads[:2], [wss[0], wss[0]])


# ------------------------------------------------------------------ 4. d_ssim as an autograd op
def test_d_ssim_autograd_op(gpu_device):
    """`d_ssim(x, y)` has the reference's value, returns a 0-dim tensor, scales its gradient by the incoming one and composes
    with a torch L1 term; the target takes no gradient."""
    import torch
    from fateavatar_amd.loss import d_ssim
    dev = gpu_device
    shape = (3, 64, 80)
    x, y, t64, t32 = ref.case(shape, "near")
    l1_64, ds_64, g1_64, gs_64 = t64
    xd = x.to(dev).requires_grad_()
    yd = y.to(dev)
    v = d_ssim(xd, yd)
    assert v.dim() == 0 and v.requires_grad
    (3 * v).backward()
    want3 = torch.stack([3 * ds_64, l1_64, ds_64])
    got3 = torch.stack([3 * v.detach().cpu().double(), l1_64, v.detach().cpu().double()])
    _check("3 x d_ssim", got3.float(), xd.grad, want3, 3 * gs_64)
    assert abs(float(v) - float(ds_64)) <= ref.LOSS_ATOL
    # composed with a torch L1 term, 4-D inputs
    x4 = x.to(dev)[None].clone().requires_grad_()
    loss = 0.8 * (x4 - yd[None]).abs().mean() + 0.2 * d_ssim(x4, yd[None])
    loss.backward()
    want3, want_g = ref.combine(t64, (0.8, 0.2))
    assert abs(float(loss) - float(want3[0])) <= ref.LOSS_ATOL
    _check("0.8 torch L1 + 0.2 d_ssim", want3.float(), x4.grad[0], want3, want_g)
    with torch.no_grad():
        assert not d_ssim(xd, yd).requires_grad
    with pytest.raises(RuntimeError, match="img2"):
        d_ssim(xd, yd.clone().requires_grad_())


# ------------------------------------------------------------------ 5. the steps
def _step_of(S, dev, bg, seed, use_graph, image_loss, regularisers=None):
    from fateavatar_amd.rigged import RiggedStep
    pc = _perturbed(dev, S["F"], seed=seed)
    return RiggedStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=use_graph, regularisers=regularisers,
                      image_loss=image_loss)


def _check_step_against_restatement(st, weights, name):
    """(a): the step's dL/dimage and loss words against the restatement on the step's own render and target."""
    t64 = ref.terms(st.out["render"], st.gt, __import__("torch").float64)
    t32 = ref.terms(st.out["render"], st.gt, __import__("torch").float32)
    _check(name, st.loss_terms, st._dimage, *ref.combine(t64, weights), *ref.combine(t32, weights))


def test_rigged_step_with_the_reference_image_loss(gpu_device, monkeypatch):
    """RiggedStep(image_loss=REFERENCE_IMAGE_LOSS) on the template at 128 x 128, 4 frames:
    (a) one eager step: `_dimage` and `loss_terms` against the float64 restatement on the step's render and target;
    (b) six steps: after each the parameters equal torch.optim.Adam fed the step's own flat_grad (rtol 2e-6, atol 1e-7);
    (c) 30 steps, graph against eager: util.assert_same_trajectory with the regulariser test's tolerance;
    (d) image_loss=None never calls `image_loss_and_grad` and has no `loss_terms`;
    (e) with the regularisers on as well the step runs and `reg_loss` is populated."""
    import torch
    import fateavatar_amd.train as train
    from fateavatar_amd.rigged import REFERENCE_IMAGE_LOSS, REFERENCE_REGULARISERS, RIGGED_LRS
    from tests import util
    dev = gpu_device
    res, n_frames = 128, 4
    S = _template(dev, res, n_frames, seed=2)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg, n_frames)
    calls = []
    real = train.image_loss_and_grad
    monkeypatch.setattr(train, "image_loss_and_grad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    frame = lambda st, f: st.step(S["cams"][f], S["posed"][f], gts[f])  # noqa: E731
    # ---- (d)
    st0 = _step_of(S, dev, bg, 4, False, None)
    frame(st0, 1)
    torch.cuda.synchronize()
    assert calls == [] and st0.loss_terms is None and st0.image_loss is None and float(st0.loss) > 0
    # ---- (a)
    st = _step_of(S, dev, bg, 4, False, REFERENCE_IMAGE_LOSS)
    loss = frame(st, 1)
    torch.cuda.synchronize()
    assert len(calls) == 1 and loss is st.loss and loss.data_ptr() == st.loss_terms.data_ptr() and loss.dim() == 0
    _check_step_against_restatement(st, REFERENCE_IMAGE_LOSS, "RiggedStep, one eager step")
    assert abs(float(st.loss_terms[1]) - float(st0.loss)) <= 1e-5 and float(st.loss_terms[2]) > 0
    # ---- (b)
    st = _step_of(S, dev, bg, 6, False, REFERENCE_IMAGE_LOSS)
    pc = st.pc
    sizes = [n for n, _ in st.adam_segments()]
    ref_p = [t.clone().requires_grad_() for t in torch.split(pc.flat.detach(), sizes)]
    lrs = [RIGGED_LRS[k] for k in ("xyz", "opacity", "feature_dc", "feature_rest", "rotation", "scaling")]
    topt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(ref_p, lrs)], lr=0.0)
    for it in range(6):
        if it == 3:
            st.update_sh_degree()
        loss = frame(st, it % n_frames)
        for p, g in zip(ref_p, torch.split(pc.flat_grad, sizes)):
            p.grad = g.clone()
        topt.step()
        want = torch.cat([p.detach() for p in ref_p])
        assert torch.allclose(pc.flat, want, rtol=2e-6, atol=1e-7), (it, float((pc.flat - want).abs().max()))
        assert loss is st.loss and float(loss) > 0
    assert st.adam.step_count == 6
    # ---- (c)
    runs = []
    for use_graph in (False, True):
        s = _step_of(S, dev, bg, 7, use_graph, REFERENCE_IMAGE_LOSS)
        for it in range(30):
            frame(s, it % n_frames)
        torch.cuda.synchronize()
        s.check()
        runs.append(s)
    assert runs[1]._graph is not None and runs[0]._graph is None and runs[1].overflows == 0
    assert runs[0].adam.step_count == runs[1].adam.step_count == 30
    util.assert_same_trajectory(runs[1].pc.flat, runs[0].pc.flat, "graph vs eager, D-SSIM on", tight=2e-2)
    assert torch.allclose(runs[1].loss_terms, runs[0].loss_terms, rtol=1e-2)
    _check_step_against_restatement(runs[1], REFERENCE_IMAGE_LOSS, "RiggedStep, replayed step 30")
    # ---- (e)
    st = _step_of(S, dev, bg, 8, True, REFERENCE_IMAGE_LOSS, regularisers=REFERENCE_REGULARISERS)
    for it in range(5):
        frame(st, it % n_frames)
    torch.cuda.synchronize()
    st.check()
    assert st._graph is not None and st.adam.step_count == 5
    assert float(st.reg_loss[0]) > 0 and float(st.reg_loss[1]) > 0 and float(st.loss_terms[0]) > 0


def test_train_step_with_an_image_loss(gpu_device):
    """TrainStep(image_loss=ImageLoss(0.8, 0.2)) on a small random scene: the step's dL/dimage and loss words against the
    restatement, and 24 steps graph against eager."""
    import numpy as np
    import torch
    from fateavatar_amd import scenes
    from fateavatar_amd.loss import ImageLoss
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    from fateavatar_amd.render import render
    from fateavatar_amd.train import TrainStep
    from tests import util
    dev = gpu_device
    P, res, views = 4000, 96, 4
    truth = scenes.head_scene(P=P, res=res, sh_degree=1, seed=3, opacity=0.6)
    cams = [TorchCamera(scenes.head_scene(P=8, res=res, sh_degree=1, seed=3, view=v, n_views=views).camera, dev) for v in range(views)]
    bg = torch.from_numpy(truth.bg).to(dev)
    pc_true = FlatGaussians(truth.means3D, truth.shs, truth.opacities, truth.scales, truth.rotations, 1, dev, fused_activations=True)
    with torch.no_grad():
        gts = [render(c, pc_true, bg)["render"].clone() for c in cams]
    shs0 = (truth.shs + 0.3 * np.random.default_rng(0).standard_normal(truth.shs.shape)).astype(np.float32)
    w = ImageLoss(0.8, 0.2)

    def run(use_graph, steps):
        pc = FlatGaussians(truth.means3D, shs0, truth.opacities * 0.7, truth.scales, truth.rotations, 1, dev, fused_activations=True)
        cam = TorchCamera(scenes.head_scene(P=8, res=res, sh_degree=1, seed=3, view=0, n_views=views).camera, dev)
        ts = TrainStep(pc, cam, bg, use_graph=use_graph, image_loss=w)
        for it in range(steps):
            loss = ts.step(cams[it % views], gts[it % views])
        torch.cuda.synchronize()
        ts.check()
        assert loss is ts.loss and loss.data_ptr() == ts.loss_terms.data_ptr()
        return ts

    one = run(False, 1)
    _check_step_against_restatement(one, w, "TrainStep, one eager step")
    eager, graph = run(False, 24), run(True, 24)
    assert graph._graph is not None and eager._graph is None and graph.adam.step_count == eager.adam.step_count == 24
    util.assert_same_trajectory(graph.pc.flat, eager.pc.flat, "TrainStep graph vs eager, D-SSIM on")
    assert torch.allclose(graph.loss_terms, eager.loss_terms, rtol=2e-3)
    _check_step_against_restatement(graph, w, "TrainStep, replayed step 24")
    assert float(eager.loss_terms[0]) < float(one.loss_terms[0])
    assert TrainStep(FlatGaussians(truth.means3D, shs0, truth.opacities, truth.scales, truth.rotations, 1, dev, fused_activations=True),
                     cams[0], bg).loss_terms is None
