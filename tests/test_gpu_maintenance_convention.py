"""-m gpu: the ONE convention every step follows when its point set changes between step() calls (`TrainStep._resize`,
`CloneSplitStep`, `BoundStep.state_dict / load_state_dict`), pinned the same way over TrainStep, AvatarStep, RiggedStep and
SplattingStep: the Adam moments follow their rows, appended rows start with zero moments, the step count is kept, the
statistics follow the rows of a prune (TrainStep: restart) and restart after an append, an empty selection zeroes the
statistics but leaves the buffers and the captured step alone, and a checkpoint brings all of it back bit for bit.

Smallest shapes at which that can go wrong: the tetrahedron of tests/test_gpu_step_resume.py, 65 Gaussians (one row past a
wave), a 64 x 64 image.  The statistics and both moments are FILLED from a seeded generator, not rendered, so every
expectation is plain torch indexing of what was there before: everything is `torch.equal`, nothing has a tolerance."""
import math

import numpy as np
import pytest
import torch

from fateavatar_amd import scenes
from tests.test_gpu_step_resume import FACES, VERTS

pytestmark = pytest.mark.gpu

KINDS = ["train", "avatar", "rigged", "splatting"]
CLONE_SPLIT = ["rigged", "splatting"]
RES, COUNT = 64, 5
ROWS = [0, 7, 64]


def make(kind, dev, P=65, seed=7):
    """(a step of `kind` with P rows whose moments, statistics and step count are filled from `seed`, the arguments of a step())."""
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    s = scenes.random_scene(P, RES, RES, sh_degree=1, seed=seed, tanfov=0.5, spread=0.2)
    rng = np.random.default_rng(seed)
    cam, bg = TorchCamera(s.camera, dev), torch.ones(3, device=dev)
    verts, faces = torch.from_numpy(VERTS).to(dev), torch.from_numpy(FACES).to(dev)
    fi = (np.arange(P) % 4).astype(np.int32)
    bc = rng.random((P, 3)).astype(np.float32) + 0.1
    bc /= bc.sum(1, keepdims=True)
    gt = torch.from_numpy(rng.random((3, RES, RES)).astype(np.float32)).to(dev)
    args = (cam, verts, gt)
    if kind == "train":
        from fateavatar_amd.train import TrainStep
        st = TrainStep(FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, 1, dev, fused_activations=True), cam, bg,
                       use_graph=False)
        args = (cam, gt)
    elif kind == "avatar":
        from fateavatar_amd.avatar import AvatarGaussians, AvatarStep
        st = AvatarStep(AvatarGaussians(fi, bc, float(np.log(0.05)), dev), faces, verts, cam, bg, use_graph=False)
    elif kind == "rigged":
        from fateavatar_amd.rigged import RiggedGaussians, RiggedStep
        st = RiggedStep(RiggedGaussians(fi, dev, np.random.default_rng(seed)), faces, cam, bg, verts, use_graph=False)
    else:
        from fateavatar_amd.binding import phong_canonical
        from fateavatar_amd.splatting import SplattingGaussians, SplattingStep
        st = SplattingStep(SplattingGaussians(fi, bc, float(np.log(0.05)), dev), phong_canonical(verts, faces), cam, bg, verts,
                           use_graph=False)
    g = torch.Generator().manual_seed(seed)
    n = st.pc.flat.numel()
    with torch.no_grad():
        st.pc._opacity.fill_(0.0)                                    # sigmoid 0.5: nothing is pruned for its opacity
        st.pc._scaling.fill_(float(np.log(0.05)))                    # every other row below the clone / split threshold
        st.pc._scaling[::2] = float(np.log(0.01))                    # (percent_dense x extent = 0.02)
    st.adam.exp_avg.copy_(1e-3 * torch.randn(n, generator=g))
    st.adam.exp_avg_sq.copy_(1e-6 * (torch.rand(n, generator=g) + 0.1))
    st.xyz_gradient_accum.copy_(1e-3 * (torch.rand(P, 1, generator=g) + 0.01))
    st.denom.copy_(torch.randint(1, 4, (P, 1), generator=g).float())
    st.adam.load_state_words(torch.tensor([COUNT, 1 - 0.9 ** COUNT, 1 - 0.999 ** COUNT, 0.0]))   # (the doubles are rebuilt)
    st.host_steps = COUNT
    assert st.adam.step_count == COUNT
    return st, args


def snapshot(st):
    """Copies of everything that has one row per Gaussian: {name: [P, ...]}."""
    pc, P = st.pc, st.pc.P
    out = {name: getattr(pc, name).detach().clone() for name, _ in pc.FIELDS}
    out.update({attr: getattr(pc, attr).clone() for attr, _, _ in pc.ROW_BUFFERS})
    off = 0
    for (name, _), w in zip(pc.FIELDS, pc.widths()):
        out["m" + name] = st.adam.exp_avg[off:off + P * w].view(P, w).clone()
        out["v" + name] = st.adam.exp_avg_sq[off:off + P * w].view(P, w).clone()
        off += P * w
    assert off == st.adam.exp_avg.numel() == pc.flat.numel()
    out["acc"], out["den"] = st.xyz_gradient_accum.clone(), st.denom.clone()
    return out


def check_attached(st):
    """The optimizer and the statistics belong to the holder's present buffers."""
    pc = st.pc
    assert st.adam.param.data_ptr() == pc.flat.data_ptr() and st.adam.grad.data_ptr() == pc.flat_grad.data_ptr()
    assert st.adam.exp_avg.shape == st.adam.exp_avg_sq.shape == pc.flat.shape
    assert st.xyz_gradient_accum.shape == st.denom.shape == (pc.P, 1)
    if hasattr(st, "binding_counter"):
        assert st.binding_counter.dtype == torch.int32
        assert torch.equal(st.binding_counter.long(), torch.bincount(pc.binding.long(), minlength=st.n_faces))


def step_on(st, args):
    """(e): the changed set takes a step."""
    count = st.adam.step_count
    st.step(*args)
    torch.cuda.synchronize()
    assert st.adam.step_count == count + 1 and bool(torch.isfinite(st.pc.flat).all())


@pytest.mark.parametrize("kind", KINDS)
def test_prune_carries_rows_moments_and_statistics(gpu_device, kind):
    st, args = make(kind, gpu_device)
    P = st.pc.P
    mask = torch.zeros(P, dtype=torch.bool, device=gpu_device)
    mask[ROWS] = True
    if kind in CLONE_SPLIT:
        before = snapshot(st)
        assert st.prune(mask) == 3
    else:                                # no prune(mask) there: the same rows through their opacity
        with torch.no_grad():
            st.pc._opacity[mask] = -9.0
        before = snapshot(st)
        assert st.prune_low_opacity(0.005) == 3
    torch.cuda.synchronize()
    keep, after = ~mask, snapshot(st)
    assert st.pc.P == P - 3
    check_attached(st)
    for key, old in before.items():
        if kind == "train" and key in ("acc", "den"):           # generic 3DGS: the statistics restart
            assert after[key].shape == (P - 3, 1) and not after[key].any()
        else:
            assert torch.equal(after[key], old[keep]), key
    assert before["acc"].all() and before["m_opacity"].any()
    assert st.adam.step_count == st.host_steps == COUNT and st._graph is None and st._eager_steps == 0
    step_on(st, args)


def own_append(st, kind, dev):
    """The model's own densification.  Returns (the old rows that survive [P] bool, the number of rows appended)."""
    P = st.pc.P
    if kind == "train":
        idx = st.densify_by_gradient(10, generator=torch.Generator(device=dev).manual_seed(3))
        assert idx.shape == (10,)
        return torch.ones(P, dtype=torch.bool, device=dev), 10
    if kind == "avatar":
        assert st.uv_densify(10, generator=torch.Generator(device=dev).manual_seed(3)) == 10
        return torch.ones(P, dtype=torch.bool, device=dev), 10
    # a threshold in the widest gap between neighbouring gradient norms around the median: about half of the rows
    g = (st.xyz_gradient_accum / st.denom).norm(dim=-1)
    s = g.sort().values
    k = P // 2 - 5 + int(torch.argmax(s[P // 2 - 4:P // 2 + 6] - s[P // 2 - 5:P // 2 + 5]))
    max_grad = float((s[k].double() + s[k + 1].double()) / 2)
    large = torch.exp(st.pc._scaling.detach()).max(dim=1).values > 0.02
    clone, split = (g >= max_grad) & ~large, (g >= max_grad) & large
    counts = st.densify_and_prune(max_grad=max_grad, generator=torch.Generator().manual_seed(9))
    assert counts == (int(clone.sum()), int(split.sum()), 0) and counts[0] > 0 and counts[1] > 0
    return ~split, counts[0] + 2 * counts[1]


@pytest.mark.parametrize("kind", KINDS)
def test_append_zero_moments_statistics_restart_count_kept(gpu_device, kind):
    st, args = make(kind, gpu_device)
    before = snapshot(st)
    survive, n_new = own_append(st, kind, gpu_device)
    torch.cuda.synchronize()
    n_old = int(survive.sum())
    after = snapshot(st)
    assert st.pc.P == n_old + n_new
    check_attached(st)
    for key, old in before.items():
        if key in ("acc", "den"):
            assert after[key].shape == (st.pc.P, 1) and not after[key].any()
        else:
            assert torch.equal(after[key][:n_old], old[survive]), key          # survivors: values, row buffers, moments
            if key[0] in "mv":
                assert not after[key][n_old:].any(), key                        # appended rows: no moments
    assert st.adam.step_count == st.host_steps == COUNT and st._graph is None and st._eager_steps == 0
    step_on(st, args)


@pytest.mark.parametrize("kind", CLONE_SPLIT)
def test_empty_selection_zeroes_the_statistics_and_keeps_the_captured_step(gpu_device, kind):
    st, args = make(kind, gpu_device)
    st.use_graph = True                  # two eager steps, then the third call captures the step and replays it
    for _ in range(3):
        st.step(*args)
    torch.cuda.synchronize()
    graph = st._graph
    assert graph is not None and st.adam.step_count == COUNT + 3 and st.denom.any()
    before = snapshot(st)
    ptr = st.pc.flat.data_ptr()
    assert st.densify_and_prune(max_grad=math.inf, generator=torch.Generator().manual_seed(9)) == (0, 0, 0)
    torch.cuda.synchronize()
    after = snapshot(st)
    assert st.pc.P == 65 and st.pc.flat.data_ptr() == ptr and st._graph is graph
    for key, old in before.items():
        if key in ("acc", "den"):
            assert after[key].shape == (65, 1) and not after[key].any()
        else:
            assert torch.equal(after[key], old), key
    assert st.adam.step_count == st.host_steps == COUNT + 3
    st.step(*args)                       # the kept graph is replayed over the untouched buffers
    torch.cuda.synchronize()
    assert st._graph is graph and st.adam.step_count == COUNT + 4 and bool(torch.isfinite(st.pc.flat).all())


@pytest.mark.parametrize("kind", KINDS)
def test_checkpoint_round_trip_into_another_step(gpu_device, kind):
    st, _ = make(kind, gpu_device)
    sd = st.state_dict()
    assert sd["global_step"] == COUNT != 0
    other, _ = make(kind, gpu_device, P=37, seed=8)
    other.adam.load_state_words(torch.tensor([2.0, 1 - 0.9 ** 2, 1 - 0.999 ** 2, 0.0]))
    other.host_steps = 2
    ignored = other.load_state_dict(sd)
    torch.cuda.synchronize()
    assert ignored is None if kind == "train" else ignored == []
    assert other.pc.P == 65 and torch.equal(other.pc.flat.view(torch.int32), st.pc.flat.view(torch.int32))
    for attr, _, _ in st.pc.ROW_BUFFERS:
        a, b = getattr(other.pc, attr), getattr(st.pc, attr)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), attr
    assert torch.equal(other.adam.exp_avg, st.adam.exp_avg) and torch.equal(other.adam.exp_avg_sq, st.adam.exp_avg_sq)
    assert torch.equal(other.adam.state_words(), st.adam.state_words())
    assert torch.equal(other.xyz_gradient_accum, st.xyz_gradient_accum) and torch.equal(other.denom, st.denom) and st.denom.any()
    assert other.adam.step_count == other.host_steps == sd["global_step"] and other._graph is None
    check_attached(other)
    # ---- an old-style checkpoint (no `optimizer`, no `densification`) into a third step that stands at 2, not at the
    #      checkpoint's global_step: zero moments and statistics; TrainStep and AvatarStep go on from THAT step's count
    #      (remapped), RiggedStep and SplattingStep restart at 0 (fresh); nobody takes the checkpoint's global_step
    bare = {k: v for k, v in sd.items() if k not in ("optimizer", "densification")}
    third, _ = make(kind, gpu_device, P=37, seed=8)
    third.adam.load_state_words(torch.tensor([2.0, 1 - 0.9 ** 2, 1 - 0.999 ** 2, 0.0]))
    third.host_steps = 2
    third.load_state_dict(bare)
    assert third.pc.P == 65 and torch.equal(third.pc.flat.view(torch.int32), st.pc.flat.view(torch.int32))
    assert not third.adam.exp_avg.any() and not third.adam.exp_avg_sq.any() and not third.xyz_gradient_accum.any() and not third.denom.any()
    assert third.adam.step_count == third.host_steps == (2 if kind in ("train", "avatar") else 0)
    check_attached(third)
