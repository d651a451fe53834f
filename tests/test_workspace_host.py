"""(CPU) The per-stream workspace helper (fateavatar_amd/workspace.py) behind the seven `*_workspace()` makers: what it refuses,
in each op's own words."""
import pytest
import torch

from fateavatar_amd import loss, mono

# (helper, the op that resolves through it, whose device its message names)
OPS = [(loss._l1_ws, "l1_loss_and_grad", "l1_workspace() on the image's device"),
       (loss._huber_ws, "huber_loss_and_grad", "huber_workspace() on the image's device"),
       (loss._reg_ws, "gaussian_regularisers", "regulariser_workspace() on the parameters' device"),
       (loss._mesh_ws, "mesh_terms_and_grad", "mesh_terms_workspace() on the vertices' device"),
       (mono._terms_ws, "lbs_terms_and_grad", "lbs_terms_workspace() on the predictions' device"),
       (mono._pose_ws, "deform_points", "pose_workspace() on the points' device")]
MAKERS = [loss.l1_workspace, loss.huber_workspace, loss.regulariser_workspace, loss.mesh_terms_workspace, mono.lbs_terms_workspace,
          mono.pose_workspace, lambda dev: loss.image_loss_workspace(dev, 3, 8, 8)]


@pytest.mark.parametrize("helper,who,words", OPS, ids=[o[1] for o in OPS])
def test_resolve_refuses_what_is_no_workspace_of_the_op(helper, who, words):
    dev = torch.device("cuda", 0)
    need = helper.nbytes()
    assert need >= 17 * 128 + 4 and helper.maker in words
    bad = {"a CPU tensor": torch.zeros(need, dtype=torch.uint8),
           "not uint8": torch.zeros(need, dtype=torch.float32),
           "too small": torch.zeros(need - 1, dtype=torch.uint8),
           "not contiguous": torch.zeros(2 * need, dtype=torch.uint8)[::2]}
    for what, ws in bad.items():
        with pytest.raises(RuntimeError) as e:
            helper.resolve(dev, ws, who)
        assert str(e.value) == f"{who}: workspace must come from {words}", what


def test_the_image_loss_keeps_its_wording_and_its_mapping():
    h = loss._image_ws
    assert h.kept is loss._image_workspace and h.maker == "image_loss_workspace"
    assert h.nbytes(3, 8, 8) == loss._lib.lib().fr_image_loss_workspace_bytes(3, 8, 8) < h.nbytes(3, 64, 64)
    with pytest.raises(RuntimeError, match="C, H, W >= 1"):
        h.nbytes(3, 0, 8)
    with pytest.raises(RuntimeError, match="d_ssim: workspace must come from image_loss_workspace\\(\\) on the images' device"):
        h.resolve(torch.device("cuda", 0), torch.zeros(h.nbytes(3, 8, 8) - 1, dtype=torch.uint8), "d_ssim", need=(3, 8, 8))


@pytest.mark.parametrize("maker", MAKERS, ids=["l1", "huber", "regulariser", "mesh_terms", "lbs_terms", "pose", "image_loss"])
def test_fresh_refuses_what_pose_workspace_refuses(maker):
    for dev in (torch.device("cpu"), "cpu"):
        with pytest.raises(RuntimeError, match="a HIP device, not cpu \\(there is no CPU path\\)"):
            maker(dev)
    for dev, name in ((None, "NoneType"), (torch.zeros(3), "Tensor")):
        with pytest.raises(RuntimeError, match=f"_workspace: a device, not {name}"):
            maker(dev)
