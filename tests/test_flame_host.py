"""Host-side tests of the fused FLAME route (fateavatar_amd/flame.py, tests/flame_ref.py): no GPU.

tests/golden/flame_lbs_small.npz was recorded on the CPU by running the reference's own `flame/lbs.py::lbs` (importable with torch
alone, `python -B`) in float64 on `flame_ref.random_model(300, 3, 7, seed=2028, dtype=float32)` — V = 300, n_shape = 3, n_exp = 7,
parents (-1, 0, 1, 1, 1) — called as FLAME.forward_with_delta_blendshape calls it: betas = (zeros [1,3], expression), the three
deltas added to `shapedirs`, `posedirs` and `v_template`.  It holds the inputs (float32 values), `verts`, `pose_feature`, `A` and
the float64 autograd gradients of sum(verts * g) to delta_shapedirs, delta_posedirs, delta_vertex, expression and pose.  Only
the data is kept here."""
import os

import numpy as np
import pytest
import torch

from tests import flame_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flame_lbs_small.npz")


def _golden():
    z = np.load(GOLDEN)
    m = {k: torch.from_numpy(z[k]) for k in z.files if z[k].ndim}
    m["n_shape"], m["n_exp"] = int(z["n_shape"]), int(z["n_exp"])
    return m


def test_restatement_reproduces_the_recorded_reference():
    m = _golden()
    assert (m["n_shape"], m["n_exp"], tuple(m["v_template"].shape)) == (3, 7, (300, 3))
    r = flame_ref.run(m, torch.float64)
    for k in ("verts", "pose_feature", "A", "d_delta_shapedirs", "d_delta_posedirs", "d_delta_vertex", "d_expression", "d_pose"):
        want = m[k]
        assert want.dtype == torch.float64 and float(want.abs().max()) > 0
        # float64 against float64, another association of the same sums: 1e-12 of the largest magnitude is 1e4 roundings
        assert float((r[k] - want).abs().max()) <= 1e-12 * float(want.abs().max()), k
    # the plain mesh (FLAME.forward) differs from the personalised one
    plain = flame_ref.run(m, torch.float64, with_deltas=False)
    assert float((plain["verts"] - m["verts"]).abs().max()) > 1e-4


def test_shape_columns_have_exactly_zero_gradient_and_adam_leaves_them_alone():
    m = _golden()
    assert int((m["d_delta_shapedirs"][:, :, :3] != 0).sum()) == 0          # the reference's own autograd, recorded
    for dtype in (torch.float32, torch.float64):
        r = flame_ref.run(m, dtype)
        assert int((r["d_delta_shapedirs"][:, :, :m["n_shape"]] != 0).sum()) == 0
        assert float(r["d_delta_shapedirs"][:, :, m["n_shape"]:].abs().max()) > 0
    # torch.optim.Adam without weight decay: zero gradient and zero moments leave the parameter bit for bit where it is
    p = m["delta_shapedirs"].clone().requires_grad_(True)
    before = p.detach().clone()
    opt = torch.optim.Adam([p], lr=1e-5)
    for _ in range(3):
        p.grad = flame_ref.run(m, torch.float32)["d_delta_shapedirs"].clone()
        opt.step()
    assert torch.equal(p.detach()[:, :, :3], before[:, :, :3])
    assert not torch.equal(p.detach()[:, :, 3:], before[:, :, 3:])


def _mesh(m, **kw):
    from fateavatar_amd.flame import FlameMesh
    return FlameMesh(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"], m["n_shape"],
                     m["n_exp"], **kw)


def test_flame_mesh_checks_its_arguments():
    from fateavatar_amd import flame
    m = _golden()
    fm = _mesh(m)
    assert (fm.V, fm.n_shape, fm.n_exp) == (300, 3, 7) and fm.flat.numel() == 300 * 3 * 7 + 36 * 900 + 900
    assert fm.flat.requires_grad and not fm.flat_grad.requires_grad and int((fm.flat != 0).sum()) == 0
    assert fm.parents.tolist() == [-1, 0, 1, 1, 1]
    bad = dict(m)
    for key, value, match in (("parents", torch.tensor([-1, 0, 2, 1, 1]), "parents"), ("parents", torch.tensor([-1, 0, 1, 1]), "5 joints"),
                              ("posedirs", m["posedirs"][:, :-3], "posedirs"), ("lbs_weights", m["lbs_weights"][:, :4], "lbs_weights"),
                              ("J_regressor", m["J_regressor"][:, :-1], "J_regressor"), ("v_template", m["v_template"][:, :2], "v_template")):
        bad = dict(m, **{key: value})
        with pytest.raises(ValueError, match=match):
            _mesh(bad)
    with pytest.raises(ValueError, match="n_exp"):
        flame.FlameMesh(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"], 10, 0)
    with pytest.raises(ValueError, match="n_exp"):
        flame.FlameMesh(m["v_template"], torch.zeros(300, 3, flame.MAX_E + 1), m["posedirs"], m["J_regressor"], m["parents"],
                        m["lbs_weights"], 0, flame.MAX_E + 1)
    with pytest.raises(ValueError, match="shapedirs"):
        flame.FlameMesh(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"], 4, 7)
    # the optimizer's groups: three (count, rate) runs in the reference's order and at its rates
    assert fm.adam_segments() == [(6300, 1e-5), (32400, 1e-5), (900, 1e-4)]
    assert fm.adam_segments({"delta_vertex": 3e-4})[2] == (900, 3e-4)
    with pytest.raises(ValueError, match="learning rates"):
        fm.adam_segments({"delta": 1e-4})
    # there is no CPU path for the kernels
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.forward_into(m["expression"], m["pose"], torch.zeros(300, 3))
    assert flame.REFERENCE_FLAME_LRS == dict(delta_shapedirs=1e-5, delta_posedirs=1e-5, delta_vertex=1e-4)


def test_checkpoint_layout_round_trips_on_the_cpu():
    m = _golden()
    fm = _mesh(m)
    sd = fm.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"delta_shapedirs": (300, 3, 10), "delta_posedirs": (36, 900),
                                                         "delta_vertex": (300, 3)}
    assert all(int((v != 0).sum()) == 0 for v in sd.values())
    flat_ptr = fm.flat.data_ptr()
    fm.load_state_dict({k: m[k] for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")})
    assert fm.flat.data_ptr() == flat_ptr                                   # in place
    assert torch.equal(fm.delta_exp, m["delta_shapedirs"][:, :, 3:]) and torch.equal(fm.delta_shape_columns, m["delta_shapedirs"][:, :, :3])
    assert torch.equal(fm.delta_posedirs, m["delta_posedirs"]) and torch.equal(fm.delta_vertex, m["delta_vertex"])
    back = fm.state_dict()
    for k in back:                                                          # the shape columns come back as they were loaded
        assert torch.equal(back[k], m[k]), k
    other = _mesh(m)
    other.load_state_dict(back)
    assert torch.equal(other.flat, fm.flat)
    with pytest.raises(KeyError, match="delta_vertex"):
        fm.load_state_dict({k: v for k, v in back.items() if k != "delta_vertex"})
    with pytest.raises(ValueError, match="delta_shapedirs"):
        fm.load_state_dict(dict(back, delta_shapedirs=back["delta_shapedirs"][:, :, 1:]))
    assert torch.equal(fm.state_dict()["delta_vertex"], m["delta_vertex"])  # a refused load changes nothing


def test_from_state_dict_reads_the_reference_keys():
    from fateavatar_amd.flame import FlameMesh
    m = _golden()
    sd = {"flame." + k: m[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")}
    sd["flame.parents"] = m["parents"].long()
    sd["flame.faces_tensor"] = torch.zeros(4, 3, dtype=torch.long)          # (buffers of the reference's that are not needed)
    sd["_opacity"] = torch.zeros(5, 1)
    fm = FlameMesh.from_state_dict(sd, n_exp=7)
    assert (fm.V, fm.n_shape, fm.n_exp) == (300, 3, 7) and torch.equal(fm.shapedirs, m["shapedirs"])
    assert int((fm.flat != 0).sum()) == 0
    sd.update({k: m[k] for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")})
    fm = FlameMesh.from_state_dict(sd, n_exp=7, n_shape=3)
    assert torch.equal(fm.delta_vertex, m["delta_vertex"]) and torch.equal(fm.delta_exp, m["delta_shapedirs"][:, :, 3:])
    with pytest.raises(KeyError, match="flame.posedirs"):
        FlameMesh.from_state_dict({k: v for k, v in sd.items() if k != "flame.posedirs"}, n_exp=7)


def test_synthetic_flame_is_a_smooth_valid_model():
    from fateavatar_amd import flame, scenes
    verts, _, _ = scenes.head_geometry()
    fm = flame.synthetic_flame(verts, seed=3, n_shape=2, n_exp=5)
    again = flame.synthetic_flame(verts, seed=3, n_shape=2, n_exp=5)
    assert fm.V == len(verts) and torch.equal(fm.shapedirs, again.shapedirs) and torch.equal(fm.posedirs, again.posedirs)
    assert torch.allclose(fm.lbs_weights.sum(1), torch.ones(fm.V), atol=1e-5)
    assert torch.allclose(fm.J_regressor.sum(1), torch.ones(5), atol=1e-5)
    # posing it with the restatement gives a finite head that moves with the jaw
    e, p = torch.zeros(5), torch.zeros(15)
    rest = flame_ref.lbs(e, p, fm.v_template, fm.shapedirs, fm.posedirs, fm.J_regressor, fm.parents, fm.lbs_weights, 2)[0]
    p2 = p.clone()
    p2[6] = 0.2
    moved = flame_ref.lbs(e, p2, fm.v_template, fm.shapedirs, fm.posedirs, fm.J_regressor, fm.parents, fm.lbs_weights, 2)[0]
    assert bool(torch.isfinite(moved).all()) and float((rest - fm.v_template).abs().max()) < 1e-6
    assert 1e-4 < float((moved - rest).abs().max()) < 0.1
