"""-m gpu: the perceptual term inside FateAvatar's step (AvatarStep(perceptual=...)) on a small bound scene — 64 x 64 frames,
both images resized to 24 x 24, VGG-16's widths with seeded weights: what the step's image-gradient buffer and
`perceptual_loss` hold after a step, eager steps against graph replays, and the batch step's refusal."""
import pytest

from tests import vgg_ref
from tests.test_gpu_avatar import _setup, _targets

pytestmark = pytest.mark.gpu

RES, SIZE, P, FRAMES = 64, (24, 24), 3000, 5


def _scene(dev):
    import torch
    S = _setup(dev, P, RES, FRAMES, seed=1)
    bg = torch.ones(3, device=dev)
    return S, bg, _targets(S, dev, bg)


def _perceptual(dev):
    from fateavatar_amd.perceptual import Perceptual, VggFeatures
    W, B = vgg_ref.he_weights(vgg_ref.VGG16, seed=21)
    return Perceptual(VggFeatures(vgg_ref.VGG16, W, B, size=SIZE, device=dev), weight=0.1)


def test_one_step_adds_the_weighted_gradient_to_the_l1_gradient(gpu_device):
    import torch
    from fateavatar_amd.avatar import AvatarBatchStep, AvatarStep
    from fateavatar_amd.loss import l1_loss_and_grad
    dev = gpu_device
    S, bg, gts = _scene(dev)
    p = _perceptual(dev)
    st = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg, use_graph=False, perceptual=p)
    assert tuple(st.perceptual_loss.shape) == (5,)
    loss = st.step(S["cams"][1], S["posed"][1], gts[1])
    torch.cuda.synchronize()
    render = st.out["render"]
    l1, g_l1 = l1_loss_and_grad(render, gts[1])
    other = _perceptual(dev)                                   # (its own workspace)
    terms, g_p = other.loss_and_grad(render, gts[1])
    assert float(g_p.abs().max()) > 0 and float(g_l1.abs().max()) > 0
    assert torch.equal(loss, l1)                               # `loss` stays the L1 term
    assert torch.equal(st.perceptual_loss, terms) and float(terms[0]) > 0
    assert torch.allclose(terms[0], terms[1:].sum(), rtol=1e-6)
    assert torch.allclose(st._dimage, g_l1 + g_p, rtol=1e-6, atol=0)
    assert not torch.equal(st._dimage, g_l1)
    # the batch step refuses the term, as it refuses vertex_grad
    with pytest.raises(NotImplementedError, match="perceptual"):
        AvatarBatchStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg, views_per_step=2, perceptual=p)
    with pytest.raises(TypeError, match="Perceptual"):
        AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg, perceptual=p.features)


def _run(S, bg, gts, dev, use_graph, with_term=True, lrs=None):
    """Five steps over the five frames; returns (pc, step, per-step L1 loss, per-step perceptual_loss, per-step image gradient)."""
    import torch
    from fateavatar_amd.avatar import AvatarStep
    pc = S["make"]()
    st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), bg, lrs=lrs, use_graph=use_graph,
                    perceptual=_perceptual(dev) if with_term else None)
    losses, terms, grads = [], [], []
    for f in range(FRAMES):
        losses.append(st.step(S["cams"][f], S["posed"][f], gts[f]).clone())
        terms.append(None if not with_term else st.perceptual_loss.clone())
        grads.append(st._dimage.clone())
    torch.cuda.synchronize()
    st.check()
    return pc, st, losses, terms, grads


def test_two_eager_and_three_replayed_steps_are_five_eager_steps(gpu_device):
    """Two eager plus three replayed steps against five eager steps.

    What the step computes in front of the rasterizer's backward — the render, the L1 loss, `perceptual_loss` and the image
    gradient L1 + 0.1 x VGG that the backward is handed — is deterministic and is held bit for bit, on five different frames.
    The PARAMETERS of a training run cannot be: the rasterizer's blend backward sums with float atomics (tests/test_gpu_step_ops.py:
    "two runs agree to rounding, not bit for bit"), so two runs of the same steps drift apart whatever follows the L1 launch.
    Measured on this scene with the term in the step, graph against eager at the reference's rates: perceptual_loss equal at
    step 0 and one ulp apart in one or two terms from step 1 on, parameters up to 5.0e-5 apart after five steps (4.8e-6 in a second run).  So the
    bit-for-bit runs are made at learning rate 0 (every step's frame, camera and target still differ; the parameters stay equal
    trivially), and the runs at the reference's rates are held to the project's yardstick for two runs that differ in atomic
    order (tests/util.py assert_same_trajectory) and to rtol 1e-5 on the terms."""
    import torch
    from fateavatar_amd.avatar import FATE_LRS
    from tests import util
    dev = gpu_device
    S, bg, gts = _scene(dev)
    still = {k: 0.0 for k in FATE_LRS}
    pc_e, st_e, loss_e, terms_e, grads_e = _run(S, bg, gts, dev, False, lrs=still)
    pc_g, st_g, loss_g, terms_g, grads_g = _run(S, bg, gts, dev, True, lrs=still)
    assert st_g._graph is not None and st_e._graph is None and st_g.overflows == 0 and st_g._eager_steps == 2
    assert st_g.adam.step_count == FRAMES == st_e.adam.step_count
    for k in range(FRAMES):
        assert torch.equal(loss_g[k], loss_e[k]) and torch.equal(terms_g[k], terms_e[k]) and torch.equal(grads_g[k], grads_e[k]), k
        assert float(terms_e[k][0]) > 0 and float(grads_e[k].abs().max()) > 0
    assert len({float(t[0]) for t in terms_e}) == FRAMES                      # five different frames
    assert torch.equal(pc_g.flat.detach(), pc_e.flat.detach()) and torch.equal(pc_e.flat.detach(), S["make"]().flat.detach())
    # ---- at the reference's rates
    pc_e, st_e, loss_e, terms_e, _ = _run(S, bg, gts, dev, False)
    pc_g, st_g, loss_g, terms_g, _ = _run(S, bg, gts, dev, True)
    assert st_g._graph is not None and st_g.overflows == 0
    noise = float((pc_g.flat.detach() - pc_e.flat.detach()).abs().max())
    print("largest parameter difference, graph against eager:", noise)
    assert torch.equal(loss_g[0], loss_e[0]) and torch.equal(terms_g[0], terms_e[0])
    for k in range(FRAMES):
        assert torch.allclose(terms_g[k], terms_e[k], rtol=1e-5, atol=0), k
    util.assert_same_trajectory(pc_g.flat.detach(), pc_e.flat.detach(), "graph vs eager with the perceptual term", tight=2e-3)
    # the term reaches the parameters: the same five eager steps without it end elsewhere, far outside that noise
    pc_n, st_n, _, _, _ = _run(S, bg, gts, dev, False, with_term=False)
    assert st_n.perceptual_loss is None and st_n.perceptual is None
    moved = (pc_n.flat.detach() - pc_e.flat.detach()).abs()
    print("without the term: largest parameter difference", float(moved.max()), "entries more than 1e-3 apart", int((moved > 1e-3).sum()))
    noisy = int(((pc_g.flat.detach() - pc_e.flat.detach()).abs() > 1e-3).sum())      # (at most 64, by assert_same_trajectory)
    assert int((moved > 1e-3).sum()) > 10 * max(noisy, 64), (int((moved > 1e-3).sum()), noisy)
