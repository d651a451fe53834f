"""GPU: what `load_state_dict` leaves behind in each of the five steps, with and without the `optimizer` / `densification`
entries of the checkpoint.  This is the one place where the steps differ on purpose: TrainStep and AvatarStep REMAP the
optimizer onto the loaded buffers (the loading object's step count is kept), RiggedStep, SplattingStep and FlashStep build a
FRESH one (step count 0; FlashStep's LPIPS schedule has a count of its own, tests/test_gpu_lpips_step.py).  Everything asserted
here is exact: counts, zeros and bitwise copies.

Smallest shapes at which the step is a real one: a tetrahedron (4 faces), 65 Gaussians (one more than a wave), a 64 x 64
image, no graph.

A checkpoint without an `optimizer` entry, loaded into a step object that has not stepped yet, ends at step count 0 in all
five classes — the remapped optimizer keeps the count of the object it belongs to, and that is 0.  So the two ways to
rebind cannot be told apart there; the bare checkpoint is therefore ALSO loaded back into the object that took the three
steps, where the count stays 3 under a remap and returns to 0 under a fresh optimizer."""
import numpy as np
import pytest
import torch

from fateavatar_amd import scenes

P, RES, STEPS = 65, 64, 3
VERTS = (0.2 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) + np.array([0, 0, 1], np.float32))
FACES = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
KEEPS_COUNT = {"train": True, "avatar": True, "rigged": False, "splatting": False, "flash": False}


class Case:
    """A step of one kind on the tetrahedron scene and the arguments of its `step()`."""

    def __init__(self, kind, dev):
        from fateavatar_amd.model import FlatGaussians, TorchCamera
        s = scenes.random_scene(P, RES, RES, sh_degree=1, seed=3, tanfov=0.5, spread=0.2)
        rng = np.random.default_rng(7)
        cam, bg = TorchCamera(s.camera, dev), torch.ones(3, device=dev)
        verts, faces = torch.from_numpy(VERTS).to(dev), torch.from_numpy(FACES).to(dev)
        fi = (np.arange(P) % 4).astype(np.int32)
        bc = rng.random((P, 3)).astype(np.float32) + 0.1
        bc /= bc.sum(1, keepdims=True)
        self.gt = torch.from_numpy(rng.random((3, RES, RES)).astype(np.float32)).to(dev)
        self.args = [(cam, verts + 0.01 * k, self.gt) for k in range(STEPS)]
        if kind == "train":
            from fateavatar_amd.train import TrainStep
            pc = FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, 1, dev, fused_activations=True)
            self.st = TrainStep(pc, cam, bg, use_graph=False)
            self.args = [(cam, self.gt)] * STEPS
        elif kind == "avatar":
            from fateavatar_amd.avatar import AvatarGaussians, AvatarStep
            self.st = AvatarStep(AvatarGaussians(fi, bc, float(np.log(0.05)), dev), faces, verts, cam, bg, use_graph=False)
        elif kind == "rigged":
            from fateavatar_amd.rigged import RiggedGaussians, RiggedStep
            pc = RiggedGaussians(fi, dev)
            with torch.no_grad():
                pc._scaling.fill_(float(np.log(0.2)))
            self.st = RiggedStep(pc, faces, cam, bg, verts, use_graph=False)
        elif kind == "flash":
            from fateavatar_amd.flash import DEFORM_COLS, FlashGaussians, FlashStep
            self.st = FlashStep(FlashGaussians(fi, bc, float(np.log(0.05)), dev), faces, cam, bg, verts, use_graph=False)
            deform = torch.from_numpy((0.01 * rng.standard_normal((P, DEFORM_COLS))).astype(np.float32)).to(dev)
            self.args = [(cam, verts + 0.01 * k, deform, self.gt) for k in range(STEPS)]
        else:
            from fateavatar_amd.binding import phong_canonical
            from fateavatar_amd.splatting import SplattingGaussians, SplattingStep
            self.st = SplattingStep(SplattingGaussians(fi, bc, float(np.log(0.05)), dev), phong_canonical(verts, faces), cam, bg,
                                    verts, use_graph=False)

    def run(self):
        for a in self.args:
            self.st.step(*a)
        torch.cuda.synchronize()
        return self.st


def check_restarted(st, count, kind):
    """After loading a checkpoint without `optimizer` / `densification`: nothing carried but (perhaps) the step count."""
    assert not st.adam.exp_avg.any() and not st.adam.exp_avg_sq.any()
    assert st.adam.exp_avg.shape == st.pc.flat.shape and st.adam.param.data_ptr() == st.pc.flat.data_ptr()
    assert st.adam.grad.data_ptr() == st.pc.flat_grad.data_ptr()
    assert st.xyz_gradient_accum.shape == st.denom.shape == (P, 1)
    assert not st.xyz_gradient_accum.any() and not st.denom.any()
    assert st.adam.step_count == count, (kind, st.adam.step_count)
    assert st.host_steps == st.adam.step_count and st.skipped_steps == 0
    assert st._graph is None and st._eager_steps == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["train", "avatar", "rigged", "splatting", "flash"])
def test_resume_with_and_without_the_optimizer_entries(gpu_device, kind):
    case = Case(kind, gpu_device)
    st = case.run()
    assert st.adam.step_count == st.host_steps == STEPS
    assert st.adam.exp_avg.any() and st.adam.exp_avg_sq.any() and st.denom.any()      # there IS something to lose
    sd = st.state_dict()
    assert sd["global_step"] == STEPS
    bare = {k: v for k, v in sd.items() if k not in ("optimizer", "densification")}
    values = st.pc.flat.clone()

    # ---- the bare checkpoint into a step object that has not stepped: fresh or remapped, the count is that object's, 0
    fresh = Case(kind, gpu_device).st
    unused = fresh.load_state_dict(bare)
    assert unused is None if kind == "train" else unused == []
    assert torch.equal(fresh.pc.flat, values)
    check_restarted(fresh, 0, kind)

    # ---- the full checkpoint into another such object: the count and the moments come back bit for bit
    full = Case(kind, gpu_device).st
    full.load_state_dict(sd)
    assert torch.equal(full.pc.flat, values)
    assert full.adam.step_count == full.host_steps == STEPS and full._graph is None
    assert torch.equal(full.adam.exp_avg, sd["optimizer"]["exp_avg"]) and torch.equal(full.adam.exp_avg, st.adam.exp_avg)
    assert torch.equal(full.adam.exp_avg_sq, sd["optimizer"]["exp_avg_sq"]) and torch.equal(full.adam.exp_avg_sq, st.adam.exp_avg_sq)
    assert torch.equal(full.adam.state_words(), st.adam.state_words())
    assert torch.equal(full.xyz_gradient_accum, st.xyz_gradient_accum) and torch.equal(full.denom, st.denom)

    # ---- the bare checkpoint back into the object that took the steps: TrainStep and AvatarStep keep its count with zero
    #      moments (remapped optimizer), RiggedStep and SplattingStep start over (fresh optimizer)
    st.load_state_dict(bare)
    assert torch.equal(st.pc.flat, values)
    check_restarted(st, STEPS if KEEPS_COUNT[kind] else 0, kind)

    # ---- and the resumed object steps on
    full.step(*case.args[0])
    torch.cuda.synchronize()
    assert full.adam.step_count == full.host_steps == STEPS + 1 and bool(torch.isfinite(full.loss))
