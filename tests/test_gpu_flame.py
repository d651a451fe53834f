"""-m gpu: the fused FLAME kernels (csrc/fr_flame.hip, fateavatar_amd/flame.py) on the device — forward and backward against the
float64 restatement of tests/flame_ref.py with a bound MEASURED on the float32 restatement, the same bits on every launch and
graph replay, the autograd op, and AvatarStep(flame=...) against the existing route (torch FLAME outside the step).

The bound (as tests/test_gpu_mlp.py): the float32 restatement on the CPU has a rel-L2 error e32 against float64 for each output;
the kernels may have at most FACTOR x e32 (another summation order) and never more than the project's gradient ceiling 1e-4."""
import ctypes
import functools

import numpy as np
import pytest

from tests import flame_ref

pytestmark = pytest.mark.gpu

FACTOR, CEILING = 4.0, 1e-4
# (V, n_shape, n_exp): one vertex, an odd size below one skinning tile, the golden file's, a ragged size at the widest expression,
# FLAME's own vertex count, and one vertex past each grid cap (256 workgroups of 16 and of 64 vertices) at n_exp = 1
SHAPES = [(1, 0, 1), (63, 0, 5), (300, 3, 7), (257, 2, 128), (5023, 100, 50), (4097, 0, 1), (16385, 0, 1)]
OUTPUTS = ("verts", "verts_orig", "pose_feature", "A", "d_delta_exp", "d_delta_posedirs", "d_delta_vertex", "d_expression", "d_pose")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _case(V, NS, NE):
    """One model and its inputs on the CPU from a seed of the shape, with the float64 and the float32 restatement's results
    (computed once, shared, never modified)."""
    import torch
    m = flame_ref.random_model(V, NS, NE, seed=1000 * NE + 10 * NS + V, dtype=torch.float32)
    out = {}
    for name, dtype in (("r64", torch.float64), ("r32", torch.float32)):
        r = flame_ref.run(m, dtype)
        r["d_delta_exp"] = r.pop("d_delta_shapedirs")[:, :, NS:].contiguous()
        r["verts_orig"] = flame_ref.run(m, dtype, with_deltas=False)["verts"]
        out[name] = r
    return dict(m=m, **out)


def _mesh(m, dev):
    from fateavatar_amd.flame import FlameMesh
    fm = FlameMesh(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"], m["n_shape"],
                   m["n_exp"], device=dev)
    fm.load_state_dict({k: m[k] for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")})
    return fm


def _run(fm, m, dev, orig=True, poison=float("nan")):
    """One forward and one backward through the raw entry points into poisoned outputs: a dict of device tensors."""
    import torch
    full = lambda *s: torch.full(s, poison, device=dev)  # noqa: E731
    e, p, g = m["expression"].to(dev), m["pose"].to(dev), m["g"].to(dev)
    o = dict(verts=full(fm.V, 3), verts_orig=full(fm.V, 3) if orig else None, pose_feature=full(36), A=full(5, 4, 4),
             d_expression=full(fm.n_exp), d_pose=full(15))
    fm.flat_grad.fill_(poison)
    fm.forward_into(e, p, o["verts"], o["verts_orig"], o["pose_feature"], o["A"])
    fm.backward_from(g, e, p, o["d_expression"], o["d_pose"])
    o.update(d_delta_exp=fm.grad_delta_exp.clone(), d_delta_posedirs=fm.grad_delta_posedirs.clone(),
             d_delta_vertex=fm.grad_delta_vertex.clone())
    return o


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_against_float64(gpu_device, shape):
    import torch
    dev = gpu_device
    c = _case(*shape)
    m, r64, r32 = c["m"], c["r64"], c["r32"]
    fm = _mesh(m, dev)
    got = _run(fm, m, dev)
    torch.cuda.synchronize()
    assert int(fm.workspace_zeroed_part().count_nonzero()) == 0
    for name in OUTPUTS:
        v, ref64, ref32 = got[name].cpu().reshape(-1), r64[name].reshape(-1), r32[name].reshape(-1)
        assert bool(torch.isfinite(v).all()), name
        e32, err = _rel(ref32, ref64), _rel(v, ref64)
        print(f"V={shape[0]} NS={shape[1]} NE={shape[2]} {name}: kernel {err:.3e}  float32 restatement {e32:.3e}  "
              f"ratio {err / max(e32, 1e-300):.2f}")
        assert float(ref64.abs().max()) > 0
        assert err <= FACTOR * e32, (name, err, e32)
        assert err <= CEILING, (name, err)
    # without verts_orig, and with some outputs NULL: what the others receive are the same bits
    alone = _run(fm, m, dev, orig=False)
    for name in OUTPUTS:
        if name != "verts_orig":
            assert torch.equal(alone[name], got[name]), name
    e, p, g = m["expression"].to(dev), m["pose"].to(dev), m["g"].to(dev)
    d_pose = torch.full((15,), float("nan"), device=dev)
    fm.flat_grad.fill_(7.0)
    fm.backward_from(g, e, p, None, d_pose, deltas=False)
    assert torch.equal(d_pose, got["d_pose"]) and bool((fm.flat_grad == 7.0).all())
    d_e = torch.full((fm.n_exp,), float("nan"), device=dev)
    fm.backward_from(g, e, p, d_e, None)
    assert torch.equal(d_e, got["d_expression"]) and torch.equal(fm.grad_delta_posedirs, got["d_delta_posedirs"])
    torch.cuda.synchronize()
    assert int(fm.workspace_zeroed_part().count_nonzero()) == 0


def test_same_bits_on_every_launch_and_replay_and_outputs_are_overwritten(gpu_device):
    import torch
    from fateavatar_amd import _lib
    from fateavatar_amd.flame import FlameMesh
    dev = gpu_device
    c = _case(5023, 100, 50)
    m = c["m"]
    fm = _mesh(m, dev)
    first, second = _run(fm, m, dev, poison=float("nan")), _run(fm, m, dev, poison=-3.0e30)
    for name in OUTPUTS:
        assert torch.equal(first[name], second[name]), name
    # an eager call and a graph replay, into poisoned static outputs
    e, p, g = m["expression"].to(dev), m["pose"].to(dev), m["g"].to(dev)
    s = dict(verts=torch.empty(fm.V, 3, device=dev), verts_orig=torch.empty(fm.V, 3, device=dev), pose_feature=torch.empty(36, device=dev),
             A=torch.empty(5, 4, 4, device=dev), d_expression=torch.empty(50, device=dev), d_pose=torch.empty(15, device=dev))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fm.forward_into(e, p, s["verts"], s["verts_orig"], s["pose_feature"], s["A"])
        fm.backward_from(g, e, p, s["d_expression"], s["d_pose"])
    for _ in range(2):
        for t in s.values():
            t.fill_(float("nan"))
        fm.flat_grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for name, t in s.items():
            assert torch.equal(t, first[name]), name
        assert torch.equal(fm.grad_delta_exp, first["d_delta_exp"]) and torch.equal(fm.grad_delta_posedirs, first["d_delta_posedirs"])
        assert torch.equal(fm.grad_delta_vertex, first["d_delta_vertex"])
        assert int(fm.workspace_zeroed_part().count_nonzero()) == 0
    # stored, not accumulated: g = 0 gives exact zeros over the poison
    zero = _run(fm, m | {"g": torch.zeros_like(m["g"])}, dev, poison=5.0)
    for name in ("d_delta_exp", "d_delta_posedirs", "d_delta_vertex", "d_expression", "d_pose"):
        assert int(zero[name].count_nonzero()) == 0, name
    # V = 0 launches nothing; sizes outside the limits are refused by the entry points themselves
    empty = FlameMesh(torch.zeros(0, 3), torch.zeros(0, 3, 4), torch.zeros(36, 0), torch.zeros(5, 0), [-1, 0, 1, 1, 1], torch.zeros(0, 5),
                      1, 3, device=dev)
    d_e = torch.full((3,), float("nan"), device=dev)
    empty.forward_into(torch.zeros(3, device=dev), torch.zeros(15, device=dev), torch.empty(0, 3, device=dev))
    empty.backward_from(torch.empty(0, 3, device=dev), torch.zeros(3, device=dev), torch.zeros(15, device=dev), d_e)
    assert int(d_e.count_nonzero()) == 0
    d = fm._desc(e, p)
    d.NE = _lib.FR_FLAME_MAX_E + 1
    with pytest.raises(RuntimeError, match="FR_FLAME_MAX_E"):
        _lib.launch("fr_flame_forward", dev, ctypes.byref(d), s["verts"].data_ptr(), None, None, None, fm._workspace.data_ptr())
    d.NE, d.pose = 50, None
    with pytest.raises(RuntimeError, match="null parents, expression or pose"):
        _lib.launch("fr_flame_backward", dev, ctypes.byref(d), g.data_ptr(), None, None, None, None, None, fm._workspace.data_ptr())


def test_autograd_op_hands_out_the_same_gradients(gpu_device):
    import torch
    dev = gpu_device
    c = _case(300, 3, 7)
    m = c["m"]
    fm = _mesh(m, dev)
    raw = _run(fm, m, dev)
    e, p = m["expression"].to(dev).requires_grad_(True), m["pose"].to(dev).requires_grad_(True)
    verts, phi, A = fm(e, p)
    assert verts.requires_grad and not phi.requires_grad and not A.requires_grad
    assert torch.equal(verts.detach(), raw["verts"]) and torch.equal(phi, raw["pose_feature"]) and torch.equal(A, raw["A"])
    # another frame goes through the same FlameMesh before the backward: the op restores its own frame's state
    fm(torch.zeros_like(e), torch.zeros_like(p))
    verts.backward(m["g"].to(dev))
    assert torch.equal(fm.flat.grad, fm.flat_grad) and fm.flat.grad.data_ptr() != fm.flat_grad.data_ptr()
    assert torch.equal(fm.grad_delta_exp, raw["d_delta_exp"]) and torch.equal(fm.grad_delta_vertex, raw["d_delta_vertex"])
    assert torch.equal(e.grad, raw["d_expression"]) and torch.equal(p.grad, raw["d_pose"])
    assert _rel(p.grad.cpu(), c["r64"]["d_pose"]) <= CEILING
    with pytest.raises(ValueError, match=r"contiguous \[7\]"):
        fm(torch.zeros(6, device=dev), p)
    with pytest.raises(TypeError, match="float32"):
        fm(e.detach(), torch.zeros(15, device=dev, dtype=torch.float64))


# ------------------------------------------------------------------ the step
P_STEP, RES_STEP, NS_STEP, NE_STEP = 2000, 128, 4, 10


@functools.lru_cache(maxsize=None)
def _step_setup(n_frames):
    """The head template centred on the origin (as FLAME's own template is), a synthetic FLAME over it with small non-zero
    deltas, `n_frames` frames of (camera, expression, pose) and target images of a hidden avatar on the float64-posed mesh."""
    import torch
    from fateavatar_amd import flame, mesh_sampling, scenes
    from fateavatar_amd.avatar import AvatarGaussians, AvatarStep, _BoundFrame
    from fateavatar_amd.binding import bind_gaussians
    from fateavatar_amd.knn import init_scale_by_knn
    from fateavatar_amd.model import TorchCamera
    from fateavatar_amd.render import render
    dev = torch.device("cuda:0")
    verts, faces, _ = scenes.head_geometry()
    verts = (verts - verts.mean(0)).astype(np.float32)
    rng = np.random.default_rng(4)
    fi, bc = mesh_sampling.random_sampling_barycoords(P_STEP, verts, faces, rng)
    pts = (verts[faces[fi]] * bc[:, :, None]).sum(1).astype(np.float32)
    scale_init = float(init_scale_by_knn(torch.from_numpy(pts).to(dev))[2])
    make = lambda: AvatarGaussians(fi, bc, scale_init, dev)  # noqa: E731
    g = torch.Generator().manual_seed(12)
    V, L = len(verts), NS_STEP + NE_STEP
    deltas = dict(delta_shapedirs=5e-4 * torch.randn(V, 3, L, generator=g), delta_posedirs=5e-4 * torch.randn(36, 3 * V, generator=g),
                  delta_vertex=2e-3 * torch.randn(V, 3, generator=g))

    def model():
        fm = flame.synthetic_flame(verts, seed=1, n_shape=NS_STEP, n_exp=NE_STEP, device=dev)
        fm.load_state_dict(deltas)
        return fm
    fm = model()
    frames = [flame.FlameFrame((0.5 * torch.randn(NE_STEP, generator=g)).to(dev), (0.1 * torch.randn(15, generator=g)).to(dev))
              for _ in range(n_frames)]
    cams = []
    for _ in range(n_frames):
        eye = np.array([0.25 * rng.uniform(-1, 1), 0.15 * rng.uniform(-1, 1), 0.8 + 0.1 * rng.uniform(-1, 1)], np.float32)
        cams.append(TorchCamera(scenes.look_at_camera(eye, np.zeros(3), (0, 1, 0), 0.5, 0.5, RES_STEP, RES_STEP), dev))
    faces_t, canon, bg = torch.from_numpy(faces).to(dev), torch.from_numpy(verts).to(dev), torch.ones(3, device=dev)
    gt = make()
    with torch.no_grad():
        gt._features_dc.copy_((torch.rand(gt.P, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
    ref = AvatarStep(gt, faces_t, canon, cams[0].clone(), bg, use_graph=False)
    gts = []
    with torch.no_grad():
        for f in range(n_frames):
            shown = _posed(fm, frames[f], torch.float64)[0].float().contiguous()
            xyz, rot, scl = bind_gaussians(shown, ref.faces, gt.face_index, gt.bary_coords, ref.face_scale_canonical, gt._offset,
                                           gt._rotation, gt._scaling, ref.shell_len, True)
            gts.append(render(cams[f], _BoundFrame(xyz, gt, rot, scl, None), bg)["render"].clone())
    return dict(dev=dev, make=make, model=model, frames=frames, cams=cams, faces=faces_t, canon=canon, bg=bg, gts=gts, deltas=deltas)


def _posed(fm, frame, dtype, leaves=None):
    """(verts, verts_orig) of the torch restatement on the FlameMesh's own tables, on its device, in `dtype`; `leaves`: the
    (delta_shapedirs, delta_posedirs, delta_vertex, expression, pose) to differentiate through, else the mesh's values."""
    c = lambda t: t.detach().to(dtype)  # noqa: E731
    sd = fm.state_dict()
    dS, dP, dV, e, p = leaves if leaves is not None else (c(sd["delta_shapedirs"]), c(sd["delta_posedirs"]), c(sd["delta_vertex"]),
                                                          c(frame.expression), c(frame.pose))
    tables = (c(fm.v_template), c(fm.shapedirs), c(fm.posedirs), c(fm.J_regressor), fm.parents.cpu(), c(fm.lbs_weights), fm.n_shape)
    verts = flame_ref.lbs(e, p, *tables, dS, dP, dV)[0]
    orig = flame_ref.lbs(e.detach(), p.detach(), *tables)[0]
    return verts, orig


def test_one_fused_step_matches_the_torch_route(gpu_device):
    """ONE eager step from identical state: the existing route (float32 torch FLAME on the device -> AvatarStep(mesh_terms) ->
    posed.backward(step.d_verts)) against AvatarStep(flame=..., mesh_terms=...)."""
    import torch
    from fateavatar_amd.avatar import AvatarBatchStep, AvatarStep
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS
    S = _step_setup(6)
    dev, f = S["dev"], 1
    frame, cam, gt = S["frames"][f], S["cams"][f], S["gts"][f]
    # ---- the existing route
    fm_t = S["model"]()
    sd = fm_t.state_dict()
    leaves = [sd[k].clone().requires_grad_(True) for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")] + \
             [frame.expression.clone().requires_grad_(True), frame.pose.clone().requires_grad_(True)]
    posed, orig = _posed(fm_t, frame, torch.float32, leaves)
    st_t = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=False, mesh_terms=REFERENCE_MESH_TERMS)
    st_t.step(cam, posed, gt, verts_orig=orig.detach())
    posed.backward(st_t.d_verts)
    assert int(leaves[0].grad[:, :, :NS_STEP].count_nonzero()) == 0
    want_flat = torch.cat([leaves[0].grad[:, :, NS_STEP:].reshape(-1), leaves[1].grad.reshape(-1), leaves[2].grad.reshape(-1)])
    # ---- the fused step
    fm = S["model"]()
    w0 = fm.flat.detach().clone()
    st_f = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=False, mesh_terms=REFERENCE_MESH_TERMS,
                      flame=fm)
    assert st_f.vertex_grad
    with pytest.raises(ValueError, match="FlameFrame"):
        st_f.step(cam, posed.detach(), gt)                                   # a vertex tensor
    with pytest.raises(ValueError, match="FlameFrame"):
        st_f.step(cam, frame, gt, verts_orig=orig.detach())
    assert st_f.host_steps == 0
    with pytest.raises(NotImplementedError, match="flame"):
        AvatarBatchStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], views_per_step=2, flame=fm)
    loss = st_f.step(cam, frame, gt)
    torch.cuda.synchronize()
    # (the two posed meshes differ by float32 rounding, and the loss is a mean of smooth terms of them)
    assert abs(float(loss) - float(st_t.loss)) <= 1e-4 * abs(float(st_t.loss))
    assert _rel(st_f.verts, posed.detach()) <= 1e-6 and _rel(st_f.verts_orig, orig.detach()) <= 1e-6
    for name, got, ref in (("d_verts", st_f.d_verts, st_t.d_verts), ("flat_grad", fm.flat_grad, want_flat),
                           ("d_expression", st_f.d_expression, leaves[3].grad), ("d_pose", st_f.d_pose, leaves[4].grad)):
        err = _rel(got, ref)
        print(f"fused step against the torch route, {name}: rel-L2 {err:.3e}")
        assert float(ref.abs().max()) > 0 and err <= CEILING, (name, err)
    # the wiring of the second Adam: the deltas are what torch.optim.Adam makes of the kernel's OWN gradient, group by group
    a, b, _ = fm.counts
    parts = [w0[:a].clone().requires_grad_(True), w0[a:a + b].clone().requires_grad_(True), w0[a + b:].clone().requires_grad_(True)]
    for q, gq in zip(parts, (fm.flat_grad[:a], fm.flat_grad[a:a + b], fm.flat_grad[a + b:])):
        q.grad = gq.clone()
    lrs = (1e-5, 1e-5, 1e-4)
    torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(parts, lrs)], lr=0.0).step()
    want = torch.cat([q.detach() for q in parts])
    rate = torch.cat([torch.full_like(q.detach(), lr) for q, lr in zip(parts, lrs)])
    diff = (fm.flat.detach() - want).abs()
    assert float((fm.flat.detach() - w0).abs().max()) > 0.5 * 1e-4
    assert bool((diff <= 1e-6 * want.abs() + 1e-6 * rate).all()), float(diff.max())
    assert st_f.flame_adam.step_count == 1 == st_f.adam.step_count


def test_fused_step_trains_as_one_graph_and_round_trips_its_checkpoint(gpu_device):
    import torch
    from fateavatar_amd.avatar import AvatarStep
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS
    from tests import util
    n_frames, steps = 6, 30
    S = _step_setup(n_frames)
    dev = S["dev"]
    fm, pc = S["model"](), S["make"]()
    w0 = fm.flat.detach().clone()
    st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=True, mesh_terms=REFERENCE_MESH_TERMS, flame=fm)
    losses = []
    for it in range(steps):
        f = it % n_frames
        losses.append(float(st.step(S["cams"][f], S["frames"][f], S["gts"][f])))
    torch.cuda.synchronize()
    st.check()
    assert st._graph is not None and st.overflows == 0
    print("loss, first and last 6 steps:", np.mean(losses[:6]), np.mean(losses[-6:]))
    assert np.mean(losses[-6:]) < np.mean(losses[:6]), (losses[:6], losses[-6:])
    applied = st.host_steps - st.skipped_steps
    assert st.host_steps == steps and st.flame_adam.step_count == applied == st.adam.step_count
    assert float((fm.flat.detach() - w0).abs().max()) > 0
    assert tuple(st.d_expression.shape) == (NE_STEP,) and float(st.d_expression.abs().max()) > 0 and float(st.d_pose.abs().max()) > 0
    assert torch.equal(fm.delta_shape_columns, S["deltas"]["delta_shapedirs"][:, :, :NS_STEP].to(dev))     # never trained
    # ---- the checkpoint carries the deltas in the reference's shapes and loads them back
    sd = st.state_dict()
    V = fm.V
    assert {k: tuple(sd["model"][k].shape) for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")} == \
        {"delta_shapedirs": (V, 3, NS_STEP + NE_STEP), "delta_posedirs": (36, 3 * V), "delta_vertex": (V, 3)}
    sd["model"]["flame.shapedirs"] = torch.zeros(2)                 # (something of the reference's that stays ignored)
    fm2 = S["model"]()
    st2 = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=False,
                     mesh_terms=REFERENCE_MESH_TERMS, flame=fm2)
    assert st2.load_state_dict(sd) == ["flame.shapedirs"]
    assert torch.equal(fm2.flat, fm.flat) and torch.equal(st2.pc.flat, pc.flat)
    assert st2.flame_adam.step_count == applied == st2.adam.step_count
    before = fm.flat.detach().clone()
    for s in (st, st2):
        s.step(S["cams"][2], S["frames"][2], S["gts"][2])
    torch.cuda.synchronize()
    # the restored step goes on with the same update (the frame's gradients carry the rasterizer's float-atomic noise)
    assert _rel(fm2.flat.detach() - before, fm.flat.detach() - before) < 1e-2 and float((fm.flat.detach() - before).abs().max()) > 0
    util.assert_same_trajectory(st2.pc.flat, pc.flat, "checkpoint round trip", tight=2e-3)
    assert st2.flame_adam.step_count == applied + 1
    # without a FLAME model the same checkpoint loads as before: the deltas come back as ignored keys
    plain = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=False)
    assert plain.load_state_dict(sd) == sorted(["delta_shapedirs", "delta_posedirs", "delta_vertex", "flame.shapedirs"])
