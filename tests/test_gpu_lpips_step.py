"""-m gpu: the LPIPS term inside SplattingAvatar's and FlashAvatar's steps (SplattingStep(lpips=...), FlashStep(lpips=...,
lpips_start=...)) on small bound scenes — 64 x 64 frames, the 13-layer trunk's widths with seeded weights, no resize: what the
step's image-gradient buffer and `lpips_loss` hold after a step, eager steps against graph replays, FlashAvatar's schedule with
its one dropped graph, the schedule across a checkpoint (full, from before the start, in the reference's own layout), the
reference's whole objectives around the term, and the refusals.  Mirrors tests/test_gpu_vgg_step.py."""
import functools

import pytest

from tests import lpips_ref, vgg_ref
from tests.test_gpu_flash import _deform
from tests.test_gpu_flash import _targets as _flash_targets
from tests.test_gpu_flash import _template as _flash_template
from tests.test_gpu_phong import _targets as _splat_targets
from tests.test_gpu_phong import _template as _splat_template

pytestmark = pytest.mark.gpu

RES, N, FRAMES = 64, 3000, 5


def _lpips(dev, weight):
    from fateavatar_amd.perceptual import Lpips, VggFeatures
    W, B = vgg_ref.he_weights(lpips_ref.LPIPS13, seed=21)
    return Lpips(VggFeatures(lpips_ref.LPIPS13, W, B, size=(RES, RES), device=dev), lpips_ref.lin_weights(lpips_ref.LPIPS13, seed=22), weight)


class _Splatting:
    """SplattingStep over the 5-frame scene: step(f) runs frame f."""
    WEIGHT = 0.01

    def __init__(self, dev):
        import torch
        self.dev = dev
        self.S = _splat_template(dev, RES, FRAMES, seed=2)
        self.bg = torch.ones(3, device=dev)
        self.make, self.gts = _splat_targets(self.S, dev, self.bg, FRAMES, N)

    def lrs(self):
        from fateavatar_amd.splatting import SPLATTING_LRS
        return SPLATTING_LRS

    def build(self, lpips, use_graph=False, lrs=None, **kw):
        from fateavatar_amd.splatting import SplattingStep
        S = self.S
        return SplattingStep(self.make(), S["canonical"], S["cams"][0].clone(), self.bg, S["posed"][0], lrs=lrs, use_graph=use_graph,
                             lpips=lpips, **kw)

    def frame(self, st, f):
        return st.step(self.S["cams"][f], self.S["posed"][f], self.gts[f])

    def image_term(self, render, gt):
        from fateavatar_amd.loss import l1_loss_and_grad
        return l1_loss_and_grad(render, gt)


class _Flash(_Splatting):
    WEIGHT = 0.05

    def __init__(self, dev):
        import torch
        self.dev = dev
        self.S = _flash_template(dev, RES, FRAMES)
        self.bg = torch.ones(3, device=dev)
        self.make, self.gts, self.masks, _ = _flash_targets(self.S, dev, self.bg, FRAMES, N)
        g = torch.Generator().manual_seed(8)
        self.deforms = [_deform(N, g, dev) for _ in range(FRAMES)]

    def lrs(self):
        from fateavatar_amd.flash import FLASH_LRS
        return FLASH_LRS

    def build(self, lpips, use_graph=False, lrs=None, lpips_start=0, **kw):
        from fateavatar_amd.flash import FlashStep
        S = self.S
        return FlashStep(self.make(), S["faces"], S["cams"][0].clone(), self.bg, S["posed"][0], lrs=lrs, use_graph=use_graph, lpips=lpips,
                         lpips_start=lpips_start, **kw)

    def frame(self, st, f):
        return st.step(self.S["cams"][f], self.S["posed"][f], self.deforms[f], self.gts[f], None if st.mask is None else self.masks[f])

    def image_term(self, render, gt):
        from fateavatar_amd.loss import huber_loss_and_grad
        terms, g = huber_loss_and_grad(render, gt)
        return terms[0], g


SCENES = {"splatting": _Splatting, "flash": _Flash}


@pytest.mark.parametrize("which", list(SCENES))
def test_one_step_adds_the_weighted_gradient_to_the_image_gradient(gpu_device, which):
    import torch
    dev = gpu_device
    sc = SCENES[which](dev)
    st = sc.build(_lpips(dev, sc.WEIGHT))
    assert tuple(st.lpips_loss.shape) == (6,) and float(st.lpips_loss.abs().max()) == 0
    loss = sc.frame(st, 1)
    torch.cuda.synchronize()
    render = st.out["render"]
    base, g_base = sc.image_term(render, sc.gts[1])
    other = _lpips(dev, sc.WEIGHT)                              # (its own workspace)
    terms, g_p = other.loss_and_grad(render, sc.gts[1])
    assert float(g_p.abs().max()) > 0 and float(g_base.abs().max()) > 0
    assert torch.equal(loss, base)                              # `loss` stays the image term
    assert torch.equal(st.lpips_loss, terms) and float(terms[0]) > 0 and bool((terms[1:] > 0).all())
    assert torch.equal(st._dimage, g_base + g_p)                # (the product is rounded on its own, then added)
    assert not torch.equal(st._dimage, g_base)
    _, g_one = other.loss_and_grad(render, sc.gts[1], weight=1.0)
    assert torch.allclose(g_p, sc.WEIGHT * g_one, rtol=1e-6, atol=0)
    # a step without the term: no buffer, no launch
    plain = sc.build(None)
    assert plain.lpips is None and plain.lpips_loss is None
    sc.frame(plain, 1)
    torch.cuda.synchronize()
    assert torch.equal(plain._dimage, sc.image_term(plain.out["render"], sc.gts[1])[1])


@pytest.mark.parametrize("which", list(SCENES))
def test_one_step_of_the_full_objective_adds_the_weighted_gradient(gpu_device, which):
    """The reference's whole objectives, not the default image term: SplattingStep(image_loss=REFERENCE_IMAGE_LOSS,
    scale_term=REFERENCE_SCALE_TERM, mesh_grad=True, lpips=...) and FlashStep(mouth_mask=True, lpips=..., lpips_start=0) with a
    mask.  After one eager step the image-gradient buffer is, bit for bit, a second call of the same image-loss entry on the
    step's render plus another Lpips object's weighted gradient, and `lpips_loss` that object's terms."""
    import torch
    dev = gpu_device
    sc = SCENES[which](dev)
    if which == "splatting":
        from fateavatar_amd.loss import pixel_loss_and_grad
        from fateavatar_amd.splatting import REFERENCE_IMAGE_LOSS, REFERENCE_SCALE_TERM
        st = sc.build(_lpips(dev, sc.WEIGHT), image_loss=REFERENCE_IMAGE_LOSS, scale_term=REFERENCE_SCALE_TERM, mesh_grad=True)
        image_term = lambda render: pixel_loss_and_grad(render, sc.gts[1], REFERENCE_IMAGE_LOSS)  # noqa: E731
    else:
        from fateavatar_amd.loss import huber_loss_and_grad
        st = sc.build(_lpips(dev, sc.WEIGHT), lpips_start=0, mouth_mask=True)
        assert float(sc.masks[1].sum()) > 0
        image_term = lambda render: huber_loss_and_grad(render, sc.gts[1], st.huber, mask=sc.masks[1])  # noqa: E731
    loss = sc.frame(st, 1)
    torch.cuda.synchronize()
    render = st.out["render"]
    base_terms, g_base = image_term(render)
    other = _lpips(dev, sc.WEIGHT)
    terms, g_p = other.loss_and_grad(render, sc.gts[1])
    assert float(g_p.abs().max()) > 0 and float(g_base.abs().max()) > 0
    assert tuple(st.loss_terms.shape) == (3,) and torch.equal(st.loss_terms, base_terms) and torch.equal(loss, base_terms[0])
    assert float(base_terms[1]) > 0 and float(base_terms[2]) > 0                 # (l1, mse) / (huber, mouth)
    assert torch.equal(st.lpips_loss, terms) and float(terms[0]) > 0 and bool((terms[1:] > 0).all())
    assert torch.equal(st._dimage, g_base + g_p)
    assert not torch.equal(st._dimage, g_base)
    if which == "splatting":      # (the rest of the objective ran: the scale term's words, the mesh gradient)
        assert bool(torch.isfinite(st.reg_loss).all()) and float(st.d_verts.abs().max()) > 0 and bool(torch.isfinite(st.d_verts).all())


def _still(sc):
    return {k: 0.0 for k in sc.lrs()}


@functools.lru_cache(maxsize=None)
def _resume_runs(dev):
    """FlashStep(lpips_start=2) at learning rates 0 (a frame's render is the same bits at every step): a checkpoint after one
    step, one after four, and what the uninterrupted run's fifth step holds."""
    import torch
    sc = _Flash(dev)
    st = sc.build(_lpips(dev, 0.05), use_graph=False, lrs=_still(sc), lpips_start=2)
    sc.frame(st, 0)
    torch.cuda.synchronize()
    sd1 = st.state_dict()
    for f in (1, 2, 3):
        sc.frame(st, f)
    torch.cuda.synchronize()
    sd4 = st.state_dict()
    assert sd1["global_step"] == 1 and sd4["global_step"] == 4 and st.lpips_switches == 1
    sc.frame(st, 4)
    torch.cuda.synchronize()
    fifth = (st.lpips_loss.clone(), st._dimage.clone())
    assert float(fifth[0][0]) > 0 and not torch.equal(fifth[1], sc.image_term(st.out["render"], sc.gts[4])[1])
    return sc, sd1, sd4, fifth


def test_flash_schedule_resumes_from_a_full_checkpoint_on_either_side_of_the_start(gpu_device):
    """(a) A full checkpoint from step 4 into a fresh FlashStep(lpips_start=2, use_graph=True): the count comes back, the first
    step has the term on and holds the uninterrupted run's fifth step bit for bit, the step is captured once with the launch in
    it.  (b) A checkpoint from step 1 into that object, which is past the start and holds a graph: the term goes off and the
    graph is dropped, `lpips_loss` is zero and the image gradient the Huber term's alone for one step, then the term is back."""
    import torch
    dev = gpu_device
    sc, sd1, sd4, fifth = _resume_runs(dev)
    st = sc.build(_lpips(dev, 0.05), use_graph=True, lrs=_still(sc), lpips_start=2)
    st.load_state_dict(sd4)
    assert st.host_steps == 4 and st.adam.step_count == 4 and st.lpips_switches == 0
    sc.frame(st, 4)
    torch.cuda.synchronize()
    assert st.lpips_switches == 1 and st.host_steps == 5
    assert torch.equal(st.lpips_loss, fifth[0]) and torch.equal(st._dimage, fifth[1])
    seen = []
    for f in (0, 1, 2):
        sc.frame(st, f)
        torch.cuda.synchronize()
        seen.append((st.captures, st._graph is not None, float(st.lpips_loss[0]) > 0))
    assert seen == [(0, False, True), (1, True, True), (1, True, True)], seen
    other = _lpips(dev, 0.05)
    terms, _ = other.loss_and_grad(st.out["render"], sc.gts[2])
    assert torch.equal(st.lpips_loss, terms) and st.lpips_switches == 1
    # ---- (b)
    st.load_state_dict(sd1)
    assert st.host_steps == 1 and st._graph is None
    sc.frame(st, 1)                                                              # step 2: not past the start
    torch.cuda.synchronize()
    assert st.lpips_switches == 2 and st._graph is None and bool((st.lpips_loss == 0).all())
    assert torch.equal(st._dimage, sc.image_term(st.out["render"], sc.gts[1])[1])
    sc.frame(st, 2)                                                              # step 3: the term is back
    torch.cuda.synchronize()
    assert st.lpips_switches == 3 and st.host_steps == 3
    terms, g_p = other.loss_and_grad(st.out["render"], sc.gts[2])
    assert torch.equal(st.lpips_loss, terms) and float(terms[0]) > 0
    assert torch.equal(st._dimage, sc.image_term(st.out["render"], sc.gts[2])[1] + g_p)
    for f in (3, 4):                                                             # and the step is captured again, the launch in it
        sc.frame(st, f)
        torch.cuda.synchronize()
    assert st.captures == 2 and st._graph is not None
    terms, _ = other.loss_and_grad(st.out["render"], sc.gts[4])
    assert torch.equal(st.lpips_loss, terms) and torch.equal(st.lpips_loss, fifth[0])


def test_flash_schedule_resumes_from_a_reference_layout_checkpoint(gpu_device):
    """(c) The reference saves `global_step` and `model` and no optimizer state (train/trainer.py:396-435); its loader restores
    `global_step` (train/loader.py:102) and the loss applies `cur_step > 15000` to it (train/loss.py:250).  Such a checkpoint
    from step 4 leaves the optimizer fresh — `host_steps`, `adam.step_count` and `skipped_steps` are 0, as
    tests/test_gpu_step_resume.py holds — and the SCHEDULE at 4: the next step has the term on and holds the uninterrupted
    run's fifth step bit for bit.  (With the schedule read from `host_steps` the term stayed off for another `lpips_start`
    steps: a run resumed at step 20 000 would have trained 15 000 steps without it.)"""
    import torch
    dev = gpu_device
    sc, sd1, sd4, fifth = _resume_runs(dev)
    bare = {k: v for k, v in sd4.items() if k not in ("optimizer", "densification")}
    assert sorted(bare) == ["global_step", "model"] and bare["global_step"] == 4
    st = sc.build(_lpips(dev, 0.05), use_graph=False, lrs=_still(sc), lpips_start=2)
    assert st.load_state_dict(bare) == []
    assert st.host_steps == 0 and st.adam.step_count == 0 and st.skipped_steps == 0
    assert not st.adam.exp_avg.any() and not st.adam.exp_avg_sq.any()
    sc.frame(st, 4)
    torch.cuda.synchronize()
    assert float(st.lpips_loss[0]) > 0 and st.lpips_switches == 1, "the term is off after a resume past lpips_start"
    assert torch.equal(st.lpips_loss, fifth[0]) and torch.equal(st._dimage, fifth[1])
    assert st.host_steps == 1 and st.adam.step_count == 1 and st.schedule_steps == 5
    # a reference-layout checkpoint from BEFORE the start leaves the term off until its step comes
    st = sc.build(_lpips(dev, 0.05), use_graph=False, lrs=_still(sc), lpips_start=2)
    st.load_state_dict({k: v for k, v in sd1.items() if k not in ("optimizer", "densification")})
    seen = []
    for f in (1, 2):
        sc.frame(st, f)
        torch.cuda.synchronize()
        seen.append((st.schedule_steps, float(st.lpips_loss[0]) > 0, st.lpips_switches))
    assert seen == [(2, False, 0), (3, True, 1)], seen


def _run(sc, dev, use_graph, with_term=True, lrs=None):
    import torch
    st = sc.build(_lpips(dev, sc.WEIGHT) if with_term else None, use_graph=use_graph, lrs=lrs)
    losses, terms, grads = [], [], []
    for f in range(FRAMES):
        losses.append(sc.frame(st, f).clone())
        terms.append(None if not with_term else st.lpips_loss.clone())
        grads.append(st._dimage.clone())
    torch.cuda.synchronize()
    st.check()
    return st.pc, st, losses, terms, grads


@pytest.mark.parametrize("which", list(SCENES))
def test_two_eager_and_three_replayed_steps_are_five_eager_steps(gpu_device, which):
    """As tests/test_gpu_vgg_step.py: at learning rate 0 everything in front of the rasterizer's backward — the image loss,
    `lpips_loss`, the image gradient — is held bit for bit over five different frames; at the reference's rates two runs differ
    in the blend backward's atomic order and are held to util.assert_same_trajectory; and the term moves the parameters far
    outside that noise."""
    import torch
    from tests import util
    dev = gpu_device
    sc = SCENES[which](dev)
    still = {k: 0.0 for k in sc.lrs()}
    pc_e, st_e, loss_e, terms_e, grads_e = _run(sc, dev, False, lrs=still)
    pc_g, st_g, loss_g, terms_g, grads_g = _run(sc, dev, True, lrs=still)
    assert st_g._graph is not None and st_e._graph is None and st_g.overflows == 0 and st_g._eager_steps == 2
    assert st_g.adam.step_count == FRAMES == st_e.adam.step_count
    for k in range(FRAMES):
        assert torch.equal(loss_g[k], loss_e[k]) and torch.equal(terms_g[k], terms_e[k]) and torch.equal(grads_g[k], grads_e[k]), k
        assert float(terms_e[k][0]) > 0 and float(grads_e[k].abs().max()) > 0
    assert len({float(t[0]) for t in terms_e}) == FRAMES                      # five different frames
    assert torch.equal(pc_g.flat.detach(), pc_e.flat.detach()) and torch.equal(pc_e.flat.detach(), sc.make().flat.detach())
    # ---- at the reference's rates
    pc_e, st_e, loss_e, terms_e, _ = _run(sc, dev, False)
    pc_g, st_g, loss_g, terms_g, _ = _run(sc, dev, True)
    assert st_g._graph is not None and st_g.overflows == 0
    print("largest parameter difference, graph against eager:", float((pc_g.flat.detach() - pc_e.flat.detach()).abs().max()))
    assert torch.equal(loss_g[0], loss_e[0]) and torch.equal(terms_g[0], terms_e[0])
    for k in range(FRAMES):
        assert torch.allclose(terms_g[k], terms_e[k], rtol=1e-5, atol=0), k
    util.assert_same_trajectory(pc_g.flat.detach(), pc_e.flat.detach(), "graph vs eager with the LPIPS term", tight=2e-3)
    pc_n, st_n, _, _, _ = _run(sc, dev, False, with_term=False)
    # "Far outside that noise": the noise is what two runs of the SAME steps differ by (graph against eager, the blend backward's
    # atomic order), measured here; an entry counts as moved by the term if it differs by more than ten times the largest such
    # difference (floored at 1e-6: a float32 parameter of size <= 8 resolves 5e-7), and more entries must have moved than ten
    # times the 64 outliers util.assert_same_trajectory lets two equal runs have.  An absolute threshold (test_gpu_vgg_step.py's
    # 1e-3) cannot serve here: Adam moves an entry by about its rate per step, and five steps at SplattingAvatar's position rate
    # (1.6e-4) stay below it whatever the gradient is.
    noise = max(float((pc_g.flat.detach() - pc_e.flat.detach()).abs().max()), 1e-6)
    moved = (pc_n.flat.detach() - pc_e.flat.detach()).abs()
    n_moved = int((moved > 10 * noise).sum())
    print("without the term: largest parameter difference", float(moved.max()), "noise", noise, "entries more than 10 x noise apart", n_moved)
    assert st_n.lpips is None and st_n.lpips_loss is None
    assert n_moved > 10 * 64, (n_moved, noise)


def test_flash_schedule_switches_the_term_on_once(gpu_device):
    """FlashStep(lpips_start=2) over five frames: `lpips_loss` is zero for steps 1 and 2 and the image gradient is the Huber
    term's alone; from step 3 on the term is in; the crossing drops the step's capture state exactly once, and the step is
    captured (once) with the launch in it.  With lpips_start=3 a graph exists at the crossing: it is dropped and the step
    captured a second time — exactly one re-capture over eight steps."""
    import torch
    dev = gpu_device
    sc = _Flash(dev)
    st = sc.build(_lpips(dev, 0.05), use_graph=True, lpips_start=2)
    plain = sc.build(None, use_graph=False)
    for f in range(FRAMES):
        sc.frame(st, f)
        torch.cuda.synchronize()
        if f < 2:
            assert bool((st.lpips_loss == 0).all()), f
            assert torch.equal(st._dimage, sc.image_term(st.out["render"], sc.gts[f])[1]), f
            assert st.lpips_switches == 0
        else:
            assert float(st.lpips_loss[0]) > 0 and bool((st.lpips_loss[1:] > 0).all()), f
            assert not torch.equal(st._dimage, sc.image_term(st.out["render"], sc.gts[f])[1]), f
            assert st.lpips_switches == 1
    assert st.captures == 1 and st._graph is not None and st.adam.step_count == FRAMES     # eager 3, 4; captured at 5
    assert plain.lpips_switches == 0
    st = sc.build(_lpips(dev, 0.05), use_graph=True, lpips_start=3)
    seen = []
    for k in range(8):
        sc.frame(st, k % FRAMES)
        torch.cuda.synchronize()
        seen.append((st.captures, st._graph is not None, float(st.lpips_loss[0]) > 0))
    assert seen == [(0, False, False), (0, False, False), (1, True, False), (1, False, True), (1, False, True), (2, True, True),
                    (2, True, True), (2, True, True)], seen
    assert st.lpips_switches == 1 and st.adam.step_count == 8
    # a replayed step holds what an eager step of another object computes for the same frame
    other = _lpips(dev, 0.05)
    terms, _ = other.loss_and_grad(st.out["render"], sc.gts[7 % FRAMES])
    assert torch.equal(st.lpips_loss, terms)


@pytest.mark.parametrize("which", list(SCENES))
def test_refusals(gpu_device, which):
    import torch
    dev = gpu_device
    sc = SCENES[which](dev)
    p = _lpips(dev, sc.WEIGHT)
    with pytest.raises(TypeError, match="Lpips"):
        sc.build(p.features)
    with pytest.raises(TypeError, match="Lpips"):
        from fateavatar_amd.perceptual import Perceptual
        sc.build(Perceptual(p.features))                         # the VGG L1 term is not the LPIPS term
    # another device: one GPU here, so the object's trunk is made to SAY it lives elsewhere (nothing is launched)
    real = p.features.device
    p.features.device = torch.device("cuda", 1 if (real.index or 0) == 0 else 0)
    try:
        with pytest.raises(ValueError, match="different devices"):
            sc.build(p)
    finally:
        p.features.device = real
    if which == "flash":
        with pytest.raises(ValueError, match="lpips_start"):
            sc.build(p, lpips_start=-1)
