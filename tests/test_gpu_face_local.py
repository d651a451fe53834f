"""-m gpu: GaussianAvatars' face-local binding (model/baseline/gaussianavatars.py:144-171) on the device — the stand-alone
op, the binding inside the rasterizer's per-Gaussian kernels, the whole path against the CPU oracle, the fused
optimisation step, and the shell binding left as it was.  The reference of every comparison is the torch restatement of
tests/face_local_ref.py (pinned on the CPU by tests/test_face_local_host.py)."""
import numpy as np
import pytest

from tests.face_local_ref import face_local_bind, quaternion_candidates

pytestmark = pytest.mark.gpu


def _template(dev, res, n_frames, seed=0):
    """The head template (10 006 faces) posed by the synthetic INSTA sequence, one Gaussian per face."""
    import torch
    from fateavatar_amd import insta
    from fateavatar_amd.model import TorchCamera
    transform, posed, faces = insta.synthetic_sequence(n_frames, res, seed)
    arrays = insta.camera_arrays(transform)
    return dict(posed=torch.from_numpy(posed).to(dev), faces=torch.from_numpy(faces).to(dev).to(torch.int32).contiguous(),
                cams=[TorchCamera(c, dev) for c in arrays], cam_arrays=arrays, F=int(faces.shape[0]))


def _perturbed(dev, F, seed, sh_scale=0.3):
    """A rigged set away from its symmetric initial state: off-face positions, anisotropic rotated splats, colour in every SH
    band, opacity 0.6."""
    import torch
    from fateavatar_amd.rigged import RiggedGaussians
    pc = RiggedGaussians.one_per_face(F, dev)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        pc._xyz.copy_((0.5 * torch.randn(F, 3, generator=g)).to(dev))
        pc._scaling.add_((0.4 * torch.randn(F, 3, generator=g)).to(dev))
        pc._rotation.add_((0.5 * torch.randn(F, 4, generator=g)).to(dev))
        pc._features_dc.copy_((torch.rand(F, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        pc._features_rest.copy_((sh_scale * torch.randn(F, 15, 3, generator=g)).to(dev))
        pc._opacity.fill_(float(np.log(0.6 / 0.4)))
    return pc


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ------------------------------------------------------------------ 1. the stand-alone op
def _awkward_mesh(seed):
    """A seeded random mesh whose first faces are degenerate (a repeated vertex: every length clamps) and clamped (three
    collinear vertices, exactly: the second axis clamps), and whose faces use all four quaternion candidates."""
    rng = np.random.default_rng(seed)
    V, F, N = 400, 700, 5000
    verts = rng.normal(size=(V, 3)).astype(np.float32)
    verts[0], verts[1], verts[2] = (0, 0, 0), (1, 2, 2), (2, 4, 4)     # collinear, and exactly so in float32
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    faces[0] = (5, 5, 9)
    faces[1] = (0, 1, 2)
    binding = np.concatenate([np.arange(F), rng.integers(0, F, N - F)]).astype(np.int32)
    return verts, faces, binding, rng


@pytest.mark.parametrize("mesh", ["head_template", "awkward"])
def test_face_local_op_matches_the_torch_restatement(gpu_device, mesh):
    """`bind_gaussians_face_local` against the float32 restatement: forward within 1e-5 + 1e-5 |ref|, gradients w.r.t. verts,
    local_xyz, rotation and scaling within rel-L2 2e-4 of torch autograd (the bound the shell binding is held to)."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_face_local
    dev = gpu_device
    if mesh == "head_template":
        S = _template(dev, 64, 4)
        verts, faces = S["posed"][2].cpu().numpy(), S["faces"].cpu().numpy()
        rng = np.random.default_rng(7)
        binding = np.concatenate([np.arange(S["F"]), rng.integers(0, S["F"], 20000)]).astype(np.int32)
    else:
        verts, faces, binding, rng = _awkward_mesh(5)
    used = np.bincount(quaternion_candidates(torch.from_numpy(verts), torch.from_numpy(faces)).numpy(), minlength=4)
    assert (used > 0).all(), used
    N = binding.shape[0]
    local = rng.normal(size=(N, 3)).astype(np.float32)
    rot = rng.normal(size=(N, 4)).astype(np.float32)
    scl = rng.normal(size=(N, 3)).astype(np.float32)
    w = [rng.normal(size=s).astype(np.float32) for s in ((N, 3), (N, 4), (N, 3))]

    def run(fn, device):
        x = [torch.from_numpy(a).to(device).requires_grad_(True) for a in (verts, local, rot, scl)]
        out = fn(x[0], torch.from_numpy(faces).to(device), torch.from_numpy(binding).to(device), x[1], x[2], x[3])
        torch.autograd.backward(list(out), [torch.from_numpy(a).to(device) for a in w])
        return [o.detach().cpu() for o in out], [t.grad.cpu() for t in x]

    ref_out, ref_grad = run(face_local_bind, "cpu")
    got_out, got_grad = run(bind_gaussians_face_local, dev)
    for name, g, r in zip(("xyz", "rotation", "scaling"), got_out, ref_out):
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(g).all()), name
        err = float(((g - r).abs() - 1e-5 * r.abs()).max())
        print(f"{mesh} forward {name}: max (|d| - 1e-5 |ref|) {err:.3e}")
        assert err <= 1e-5, (name, err)
    for name, g, r in zip(("verts", "local_xyz", "rotation", "scaling"), got_grad, ref_grad):
        assert bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0, name
        err = _rel(g, r)
        print(f"{mesh} gradient {name}: rel-L2 {err:.3e}")
        assert err <= 2e-4, (name, err)


# ------------------------------------------------------------------ 2. folded against unfolded
@pytest.mark.parametrize("depth_alpha", [False, True])
@pytest.mark.parametrize("degree", [0, 3])
@pytest.mark.parametrize("K", [1, 4])
def test_face_local_binding_inside_the_kernels_equals_the_op(gpu_device, K, degree, depth_alpha):
    """`render_bound_batch` with a FaceLocalBinding against `bind_gaussians_face_local` + `render_batch`: image, radii and
    out["bound"] the same BITS, gradients within 5e-5 rel-L2, densification counts equal — with gradients and under
    no_grad (the forward-only kernels)."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_face_local
    from fateavatar_amd.bound import FaceLocalBinding, render_bound_batch
    from fateavatar_amd.render import render_batch
    from fateavatar_amd.rigged import _RiggedFrame
    dev = gpu_device
    S = _template(dev, 128, 4, seed=3)
    bg = torch.ones(3, device=dev)
    base = _perturbed(dev, S["F"], seed=4)
    base.active_sh_degree = degree
    gen = torch.Generator().manual_seed(9)
    gts = [torch.rand(3, 128, 128, generator=gen).to(dev) for _ in range(K)]
    wd = [torch.randn(1, 128, 128, generator=gen).to(dev) / 128 ** 2 for _ in range(K)]
    names = [n for n, _ in base.FIELDS]

    class Holder:
        max_sh_degree = 3

        def __init__(self, leaves):
            self.active_sh_degree = degree
            for n, t in leaves.items():
                setattr(self, n, t)
            self.binding = base.binding

        @property
        def get_features(self):
            return torch.cat((self._features_dc, self._features_rest), dim=1)

    def run(folded, grad=True):
        leaves = [{n: getattr(base, n).detach().clone().requires_grad_(grad) for n in names} for _ in range(K)]
        verts = [S["posed"][k].clone().requires_grad_(grad) for k in range(K)]
        stats = [(torch.zeros(base.P, 1, device=dev), torch.zeros(base.P, 1, device=dev)) for _ in range(K)]
        pcs = [Holder(l) for l in leaves]
        cams = S["cams"][:K]
        if folded:
            outs = render_bound_batch(cams, [_RiggedFrame(pc, st) for pc, st in zip(pcs, stats)], verts,
                                      FaceLocalBinding(S["faces"], base.binding), bg, depth_alpha=depth_alpha)
            bound = [o["bound"] for o in outs]
        else:
            frames, bound = [], []
            for k in range(K):
                b = bind_gaussians_face_local(verts[k], S["faces"], base.binding, leaves[k]["_xyz"], leaves[k]["_rotation"],
                                              leaves[k]["_scaling"])
                frames.append(_RiggedFrame(pcs[k], stats[k], b))
                bound.append(tuple(t.detach() for t in b))
            outs = render_batch(cams, frames, bg, depth_alpha=depth_alpha)
        if grad:
            loss = sum(torch.nn.functional.l1_loss(o["render"], gts[k]) for k, o in enumerate(outs))
            if depth_alpha:
                loss = loss + sum((o["depth"] * wd[k]).sum() + (o["alpha"] * wd[k].flip(1)).sum() for k, o in enumerate(outs))
            loss.backward()
        torch.cuda.synchronize()
        return outs, bound, leaves, verts, stats

    def same_frames(o_f, b_f, o_u, b_u):
        for k in range(K):
            assert torch.equal(o_f[k]["render"], o_u[k]["render"]) and torch.equal(o_f[k]["radii"], o_u[k]["radii"])
            assert torch.equal(o_f[k]["visibility_filter"], o_u[k]["visibility_filter"])
            assert int((o_f[k]["radii"] > 0).sum()) > 1000
            if depth_alpha:
                assert torch.equal(o_f[k]["depth"], o_u[k]["depth"]) and torch.equal(o_f[k]["alpha"], o_u[k]["alpha"])
            for a, b in zip(b_f[k], b_u[k]):
                assert torch.equal(a, b) and not a.requires_grad

    o_f, b_f, l_f, v_f, s_f = run(True)
    o_u, b_u, l_u, v_u, s_u = run(False)
    same_frames(o_f, b_f, o_u, b_u)
    for k in range(K):
        for n in names:
            a, b = l_f[k][n].grad, l_u[k][n].grad
            if n == "_features_rest" and degree == 0:      # (bands above the active degree get no gradient)
                assert a is None or float(a.abs().max()) == 0
                continue
            assert a is not None and b is not None and a.shape == b.shape, n
            err = _rel(a, b)
            assert err < 5e-5 and float(b.abs().max()) > 0, (n, err)
        assert _rel(v_f[k].grad, v_u[k].grad) < 5e-5 and float(v_u[k].grad.abs().max()) > 0
        assert _rel(o_f[k]["viewspace_points"].grad, o_u[k]["viewspace_points"].grad) < 5e-5
        assert torch.equal(s_f[k][1], s_u[k][1]) and float(s_u[k][1].max()) > 0
        assert float((s_f[k][0] - s_u[k][0]).abs().max()) <= 1e-4 * float(s_u[k][0].abs().max())
    # forward-only kernels: the same frame under no_grad, bit for bit the frame above
    with torch.no_grad():
        n_f, nb_f, _, _, _ = run(True, grad=False)
        n_u, nb_u, _, _, _ = run(False, grad=False)
    same_frames(n_f, nb_f, n_u, nb_u)
    same_frames(n_f, nb_f, o_f, b_f)


# ------------------------------------------------------------------ 3. the whole path against the CPU oracle
def test_face_local_frame_against_the_cpu_oracle(gpu_device):
    """Bind with the torch restatement, render with the CPU oracle; the device renders the same Gaussians straight from their
    binding.  Image: |d| <= 1e-5 + 1e-4 |ref| on >= 99.99 % of the values, every pixel outside explained as a threshold flip
    (util.explain_pixel).  Gradients (flip pixels masked out of dL/dpixel, no row exempt): |d| <= 1e-4 |ref| + 5e-6 max|ref|
    on >= 99.9 % of the entries and rel-L2 <= 1e-4 — tests/test_gpu_parity.py's bounds — for verts, local_xyz, rotation,
    scaling, opacity and the SH coefficients.  10 006 Gaussians, SH degree 3, 160 x 160."""
    import torch
    from fateavatar_amd.bound import FaceLocalBinding, render_bound_batch
    from fateavatar_amd.rigged import _RiggedFrame
    from oracle import oracle
    from tests import util
    dev = gpu_device
    res = 160
    S = _template(dev, res, 4, seed=1)
    assert S["F"] >= 10_000
    pc = _perturbed(dev, S["F"], seed=6)
    pc.active_sh_degree = 3
    f = 1
    cam, c = S["cams"][f], S["cam_arrays"][f]
    bg = np.array([0.2, 0.5, 0.9], np.float32)
    # ---- reference: restatement (float32, CPU) -> activations -> oracle
    names = [n for n, _ in pc.FIELDS]
    ref = {n: getattr(pc, n).detach().cpu().clone().requires_grad_(True) for n in names}
    verts_r = S["posed"][f].cpu().clone().requires_grad_(True)
    xyz, rot_b, scl_b = face_local_bind(verts_r, S["faces"].cpu(), pc.binding.cpu(), ref["_xyz"], ref["_rotation"], ref["_scaling"])
    act = dict(scales=torch.exp(scl_b), rotations=torch.nn.functional.normalize(rot_b), opacities=torch.sigmoid(ref["_opacity"]))
    shs = torch.cat((ref["_features_dc"], ref["_features_rest"]), dim=1)
    npy = lambda t: np.ascontiguousarray(t.detach().numpy())  # noqa: E731
    o = oracle.forward(bg=bg, means3D=npy(xyz), opacities=npy(act["opacities"]), viewmatrix=c.world_view_transform,
                       projmatrix=c.full_proj_transform, campos=c.camera_center, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
                       H=res, W=res, shs=npy(shs), sh_degree=3, scales=npy(act["scales"]), rotations=npy(act["rotations"]))
    # ---- device: the frame straight from its binding
    verts_d = S["posed"][f].clone().requires_grad_(True)
    out = render_bound_batch([cam], [_RiggedFrame(pc, None)], [verts_d], FaceLocalBinding(S["faces"], pc.binding),
                             torch.from_numpy(bg).to(dev))[0]
    col = out["render"].detach().cpu().numpy()
    # (the bound values reach the two rasterizers from two evaluations of the binding, float rounding apart: a radius,
    # ceil(3 sigma), may differ by one on a rare Gaussian — test_fused_activations_match_torch_activations' bound)
    radii = out["radii"].cpu().numpy()
    assert np.mean(radii == o.radii) > 0.999 and np.abs(radii - o.radii).max() <= 1
    assert int((o.radii > 0).sum()) > 3000
    fc = util.frac_close(col, o.color, 1e-4, 1e-5)
    bad = (np.abs(col - o.color) > 1e-5 + 1e-4 * np.abs(o.color)).any(0)
    print(f"image: {fc:.6f} of the values within tolerance, {int(bad.sum())} pixel(s) outside")
    assert fc >= 0.9999 and np.isfinite(col).all()
    ys, xs = np.nonzero(bad)
    unexplained = [(x, y) for x, y in zip(xs.tolist(), ys.tolist()) if not util.explain_pixel(o, x, y) <= 1.0]
    assert not unexplained, unexplained[:5]
    assert np.abs(col - o.color).max() < 0.05
    # ---- gradients
    dpix = (np.random.default_rng(11).uniform(-1, 1, (3, res, res)) / (res * res)).astype(np.float32)
    dpix[:, bad] = 0.0
    ob = oracle.backward(o, dpix)
    t = torch.from_numpy
    torch.autograd.backward([xyz, act["scales"], act["rotations"], act["opacities"], shs],
                            [t(ob.dL_dmeans3D), t(ob.dL_dscales), t(ob.dL_drotations), t(ob.dL_dopacity).reshape(-1, 1), t(ob.dL_dsh)])
    out["render"].backward(t(dpix).to(dev))
    got = {n: getattr(pc, n).grad.detach().cpu().numpy() for n in names}
    got["verts"] = verts_d.grad.cpu().numpy()
    want = {n: ref[n].grad.numpy() for n in names}
    want["verts"] = verts_r.grad.numpy()
    for n in got:
        g, r = got[n], want[n]
        scale = np.abs(r).max()
        assert g.shape == r.shape and np.isfinite(g).all() and scale > 0, n
        fr, rl = util.frac_close(g, r, 1e-4, 5e-6 * scale), util.rel_l2(g, r)
        print(f"gradient {n}: rel-L2 {rl:.2e}, {fr:.5f} of the entries within tolerance")
        assert (fr >= 0.999 or round((1.0 - fr) * g.size) <= 3) and rl <= 1e-4, (n, fr, rl)


# ------------------------------------------------------------------ 4. the step
def _targets(S, dev, bg, n_frames):
    """Images of a hidden rigged avatar: the same binding, coloured / opaque / placed differently."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_face_local
    from fateavatar_amd.render import render
    from fateavatar_amd.rigged import _RiggedFrame
    gt = _perturbed(dev, S["F"], seed=5, sh_scale=0.1)
    gt.active_sh_degree = 3
    with torch.no_grad():
        gt._xyz.mul_(0.3)
    imgs = []
    for f in range(n_frames):
        with torch.no_grad():
            b = bind_gaussians_face_local(S["posed"][f], S["faces"], gt.binding, gt._xyz, gt._rotation, gt._scaling)
            imgs.append(render(S["cams"][f], _RiggedFrame(gt, None, b), bg)["render"].clone())
    return imgs


def test_rigged_step_graph_follows_eager_across_an_sh_degree_update(gpu_device):
    """60 steps of RiggedStep on the template's 10 006 faces at 256 x 256 over an 8-frame sequence, `update_sh_degree()` after
    step 30: the replayed HIP graph follows the eager step (util.assert_same_trajectory), the loss falls (mean of the last
    8 steps — one pass over the 8 frames — below the mean of the first 8), the stand-alone op (`fold_binding=False`) gives the
    same losses to rtol 2e-2."""
    import torch
    from fateavatar_amd.rigged import RIGGED_LRS, RiggedGaussians, RiggedStep
    from tests import util
    dev = gpu_device
    res, n_frames, steps = 256, 8, 60
    S = _template(dev, res, n_frames)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg, n_frames)

    def run(use_graph, fold=True):
        pc = RiggedGaussians.one_per_face(S["F"], dev)
        st = RiggedStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=use_graph, fold_binding=fold)
        assert st.adam_segments() == [(pc.P * 3, RIGGED_LRS["xyz"]), (pc.P, RIGGED_LRS["opacity"]), (pc.P * 3, RIGGED_LRS["feature_dc"]),
                                      (pc.P * 45, RIGGED_LRS["feature_dc"] / 20), (pc.P * 4, RIGGED_LRS["rotation"]),
                                      (pc.P * 3, RIGGED_LRS["scaling"])]
        losses, captures = [], 0
        for it in range(steps):
            if it == 30:
                assert st.update_sh_degree() == 1 and st._graph is None
            had = st._graph is not None
            losses.append(float(st.step(S["cams"][it % n_frames], S["posed"][it % n_frames], gts[it % n_frames])))
            captures += int(st._graph is not None and not had)
        torch.cuda.synchronize()
        st.check()
        return pc, losses, st, captures

    pc_e, loss_e, st_e, cap_e = run(False)
    pc_g, loss_g, st_g, cap_g = run(True)
    assert st_g._graph is not None and st_e._graph is None and st_g.overflows == 0
    assert cap_e == 0 and cap_g == 2                                  # captured, and captured again after the degree changed
    assert pc_g.active_sh_degree == pc_e.active_sh_degree == 1
    assert st_g.adam.step_count == steps == st_e.adam.step_count
    print("loss, first and last 8 steps:", np.mean(loss_e[:8]), np.mean(loss_e[-8:]))
    assert np.mean(loss_e[-8:]) < np.mean(loss_e[:8]), (loss_e[:8], loss_e[-8:])
    assert np.allclose(loss_g, loss_e, rtol=2e-2), (loss_g[-4:], loss_e[-4:])
    assert torch.equal(st_g.denom, st_e.denom) and float(st_e.denom.max()) > 0
    util.assert_same_trajectory(pc_g.flat, pc_e.flat, "graph vs eager", tight=2e-2)
    fresh = RiggedGaussians.one_per_face(S["F"], dev)
    for name, _ in pc_e.FIELDS:                                       # every group moved, the higher SH bands too
        assert float((getattr(pc_e, name).detach() - getattr(fresh, name).detach()).abs().max()) > 0, name
    # the stand-alone op as the A/B
    pc_u, loss_u, st_u, _ = run(False, fold=False)
    assert np.allclose(loss_u, loss_e, rtol=2e-2), (loss_u[-4:], loss_e[-4:])
    assert torch.equal(st_u.denom, st_e.denom)


def test_rigged_step_parameters_follow_torch_adam_on_the_same_gradients(gpu_device):
    """Six steps (one degree update in between): after every step the flat parameter buffer equals torch.optim.Adam over the
    reference's six groups (train/optim.py:73-80) fed the gradients the step left in its flat gradient buffer, within
    test_fused_adam_matches_torch_adam's bound (rtol 2e-6, atol 1e-7).  And a checkpoint round trip restores the step."""
    import torch
    from fateavatar_amd.rigged import RIGGED_LRS, RiggedGaussians, RiggedStep
    dev = gpu_device
    res, n_frames = 128, 4
    S = _template(dev, res, n_frames, seed=2)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg, n_frames)
    pc = RiggedGaussians.one_per_face(S["F"], dev)
    st = RiggedStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False)
    sizes = [n for n, _ in st.adam_segments()]
    ref = [t.clone().requires_grad_() for t in torch.split(pc.flat.detach(), sizes)]
    lrs = [RIGGED_LRS[k] for k in ("xyz", "opacity", "feature_dc", "feature_rest", "rotation", "scaling")]
    topt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(ref, lrs)], lr=0.0)
    for it in range(6):
        if it == 3:
            st.update_sh_degree()
        st.step(S["cams"][it % n_frames], S["posed"][it % n_frames], gts[it % n_frames])
        for p, g in zip(ref, torch.split(pc.flat_grad, sizes)):
            p.grad = g.clone()
        assert float(pc.flat_grad.abs().max()) > 0
        topt.step()
        want = torch.cat([p.detach() for p in ref])
        assert torch.allclose(pc.flat, want, rtol=2e-6, atol=1e-7), (it, float((pc.flat - want).abs().max()))
    assert st.adam.step_count == 6
    # checkpoint: another step object restored from the state continues with the same update
    sd = st.state_dict()
    assert list(sd["model"]) == ["_xyz", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "binding"]
    st2 = RiggedStep(RiggedGaussians.one_per_face(7, dev), S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False)
    assert st2.load_state_dict(sd) == [] and st2.pc.P == pc.P and st2.pc.active_sh_degree == 1
    for s in (st, st2):
        s.step(S["cams"][2], S["posed"][2], gts[2])
    torch.cuda.synchronize()
    from tests import util
    util.assert_same_trajectory(st2.pc.flat, pc.flat, "checkpoint round trip", tight=2e-3)
    assert st2.adam.step_count == 7


# ------------------------------------------------------------------ 5. the shell binding is what it was
def test_zeroed_mode_field_is_the_shell_binding(gpu_device):
    """A descriptor built as callers built it before the field existed (zero-initialised, `mode` never written) and the same
    descriptor with `mode = FR_BIND_SHELL` written: bit-identical frames — and the frame of `bind_gaussians` + `render`."""
    import torch
    from fateavatar_amd import _lib, mesh_sampling, rasterizer, scenes
    from fateavatar_amd.avatar import AvatarGaussians, _BoundFrame
    from fateavatar_amd.binding import SHELL, _describe, bind_gaussians, face_scale
    from fateavatar_amd.render import _screenspace_points, _settings, render
    dev = gpu_device
    S = _template(dev, 128, 2)
    verts0, faces_np, _ = scenes.head_geometry()
    fi, bc = mesh_sampling.random_sampling_barycoords(20_000, verts0, faces_np, np.random.default_rng(1))
    pc = AvatarGaussians(fi, bc, float(np.log(2e-3)), dev)
    with torch.no_grad():
        pc._features_dc.add_(0.3)
        pc._offset.add_(0.2)
        pc._opacity.add_(2.0)
    canon = face_scale(torch.from_numpy(verts0).to(dev), S["faces"])
    verts, cam, bg = S["posed"][1].contiguous(), S["cams"][1], torch.ones(3, device=dev)
    rs = _settings(cam, pc, bg, 1.0)
    empty = torch.Tensor([])

    def frame(write_mode):
        b = _describe(SHELL, verts, S["faces"], pc.face_index, pc._offset.detach(), pc._rotation.detach(), pc._scaling.detach(),
                      pc.bary_coords, canon, 0.05, True)
        if write_mode:
            b.mode = _lib.FR_BIND_SHELL
        assert b.mode == 0 and not b.local_xyz
        xyz, rot, scl = (torch.empty((pc.P, k), device=dev) for k in (3, 4, 3))
        sp = _screenspace_points(xyz, pc)
        args = rasterizer._forward_args(rs, xyz, sp, pc._features_dc.detach(), empty, pc._opacity.detach(), scl, rot, empty)
        res = rasterizer.rasterize_gaussians_batch([args], raw=True, bindings=[b])[0]
        torch.cuda.synchronize()
        return res[1].clone(), res[2].clone(), xyz, rot, scl

    a, b = frame(False), frame(True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int((a[1] > 0).sum()) > 1000
    with torch.no_grad():
        bound = bind_gaussians(verts, S["faces"], pc.face_index, pc.bary_coords, canon, pc._offset, pc._rotation, pc._scaling, 0.05, True)
        ref = render(cam, _BoundFrame(bound[0], pc, bound[1], bound[2], None), bg)
    assert torch.equal(ref["render"], a[0]) and torch.equal(ref["radii"], a[1])
    for x, y in zip(bound, a[2:]):
        assert torch.equal(x, y)
