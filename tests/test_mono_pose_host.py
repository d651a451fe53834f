"""CPU: the host side of MonoGaussianAvatar's pose gradients (fr_point_lbs_backward_pose, deform_points(frame_grad=True)): the
exported symbols, the argument checks that return before any launch, and what the Python wrapper accepts and refuses."""
import ctypes as C
import os

import pytest
import torch

from fateavatar_amd import _lib, mono
from tests import mono_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fr_point_lbs_pose_workspace_bytes", "fr_point_lbs_backward_pose")


def test_the_new_symbols_are_exported_and_the_workspace_has_a_size():
    header = open(os.path.join(ROOT, "include", "fr_rasterizer.h")).read()
    L = _lib.lib()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(L, sym) and sym + "(" in header
    # the wrapping counters of last_workgroup_of and at least one row of E + 108 + 12 J partial sums at the limits
    assert L.fr_point_lbs_pose_workspace_bytes() >= 17 * 32 * 4 + (64 + 108 + 96) * 4
    assert "pose_workspace" in mono.__all__


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    some = C.c_void_p(4096)         # never dereferenced: every call below returns before a launch
    assert L.fr_point_lbs_backward_pose(None, some, some, some, some, some, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "null descriptor" in _lib.last_error()
    d = _lib.fr_point_lbs()
    d.N, d.E, d.J = 0, 50, 6
    assert L.fr_point_lbs_backward_pose(C.byref(d), None, None, None, None, some, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "null pose state" in _lib.last_error()
    for st in (d.canonical, d.frame):
        st.betas = st.pose_feature = st.transforms = 4096
    d.E = 65
    assert L.fr_point_lbs_backward_pose(C.byref(d), None, None, None, None, some, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "FR_LBS_MAX_E" in _lib.last_error()
    d.E, d.J = 50, 9
    assert L.fr_point_lbs_backward_pose(C.byref(d), None, None, None, None, some, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "FR_LBS_MAX_J" in _lib.last_error()
    d.J = 6
    assert L.fr_point_lbs_backward_pose(C.byref(d), None, None, None, None, None, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "workspace" in _lib.last_error()
    d.N = 3
    d.points = d.shapedirs = d.posedirs = d.weights = 4096
    assert L.fr_point_lbs_backward_pose(C.byref(d), None, some, some, some, some, None) == _lib.FR_ERR_INVALID_ARGUMENT
    assert "g_xyz" in _lib.last_error()
    # N == 0 with everything in place: nothing is launched, nothing is touched
    d.N = 0
    assert L.fr_point_lbs_backward_pose(C.byref(d), None, some, some, some, some, None) == _lib.FR_OK


def _f32_recipe(N=8, E=5, J=3):
    p, S, P, w, c, f, _ = R.recipe(N, E, J)
    f32 = lambda t: t.float()  # noqa: E731
    return [f32(t) for t in (p, S, P, w)], mono.PoseState(*map(f32, c)), mono.PoseState(*map(f32, f))


def test_frame_grad_accepts_the_frame_state_and_still_refuses_the_canonical_one():
    x, c, f = _f32_recipe()
    leaves = mono.PoseState(*[t.clone().requires_grad_(True) for t in f])
    with pytest.raises(RuntimeError, match="frame pose state requires grad"):            # the default: as before
        mono.deform_points(*x, c, leaves)
    with pytest.raises(RuntimeError, match="no CPU path"):                                # accepted: fails only at the device
        mono.deform_points(*x, c, leaves, frame_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mono.deform_points(*x, c, f._replace(transforms=f.transforms.reshape(3, 16).clone().requires_grad_(True)), frame_grad=True)
    for k in range(3):
        bad = list(c)
        bad[k] = bad[k].clone().requires_grad_(True)
        for mode in (False, True):
            with pytest.raises(RuntimeError, match="canonical pose state requires grad"):
                mono.deform_points(*x, mono.PoseState(*bad), leaves if mode else f, frame_grad=mode)
    with pytest.raises(RuntimeError, match="frame pose state is"):                        # shapes are still checked
        mono.deform_points(*x, c, leaves._replace(betas=leaves.betas[:4]), frame_grad=True)
    with pytest.raises(RuntimeError, match="pose_workspace"):
        mono.deform_points(*x, c, leaves, frame_grad=True, workspace=1234)
    with torch.no_grad():                                                                 # nothing is recorded: nothing to refuse
        with pytest.raises(RuntimeError, match="no CPU path"):
            mono.deform_points(*x, c, leaves)


def test_pose_workspace_checks_its_argument():
    with pytest.raises(RuntimeError, match="no CPU path"):
        mono.pose_workspace(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mono.pose_workspace("cpu")
    with pytest.raises(RuntimeError, match="a device"):
        mono.pose_workspace(None)
    with pytest.raises(RuntimeError, match="a device"):
        mono.pose_workspace(torch.zeros(3))
