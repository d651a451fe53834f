"""-m gpu: SplattingAvatar's Phong-surface binding (model/baseline/splattingavatar.py:203-246) on the device — the per-frame
mesh pass, the stand-alone op, the binding inside the rasterizer's per-Gaussian kernels, the whole path against the CPU oracle,
the fused optimisation step, and the two other modes left as they were.  The reference of every comparison is the torch
restatement of tests/phong_ref.py (pinned on the CPU by tests/test_phong_host.py)."""
import numpy as np
import pytest

from tests import phong_ref as P

pytestmark = pytest.mark.gpu


def _template(dev, res, n_frames, seed=0):
    """The head template posed by the synthetic INSTA sequence; frame 0 is the canonical mesh."""
    import torch
    from fateavatar_amd import insta
    from fateavatar_amd.binding import phong_canonical
    from fateavatar_amd.model import TorchCamera
    transform, posed, faces = insta.synthetic_sequence(n_frames, res, seed)
    arrays = insta.camera_arrays(transform)
    posed_t, faces_t = torch.from_numpy(posed).to(dev), torch.from_numpy(faces).to(dev).to(torch.int32).contiguous()
    return dict(posed=posed_t, faces=faces_t, cams=[TorchCamera(c, dev) for c in arrays], cam_arrays=arrays, F=int(faces.shape[0]),
                canonical=phong_canonical(posed_t[0], faces_t))


def _perturbed(S, dev, N, seed):
    """N Gaussians sampled on the canonical template, away from the initial state: off the surface, anisotropic rotated splats,
    coloured, opacity 0.6."""
    import torch
    from fateavatar_amd.splatting import SplattingGaussians
    g = torch.Generator().manual_seed(seed)
    pc = SplattingGaussians.sample(S["posed"][0], S["faces"], N, g)
    with torch.no_grad():
        pc._uvd.copy_((0.01 * torch.randn(N, 3, generator=g)).to(dev))
        pc._scaling.add_((0.3 * torch.randn(N, 3, generator=g)).to(dev))
        pc._rotation.add_((0.5 * torch.randn(N, 4, generator=g)).to(dev))
        pc._features_dc.copy_((torch.rand(N, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        pc._opacity.fill_(float(np.log(0.6 / 0.4)))
    return pc


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _meshes(name):
    """(cano_verts, verts, faces, face_index, bary, rng) as numpy: the head template (frame 2) or the turned mesh."""
    if name == "head_template":
        import torch
        posed, faces = P.head_template()
        rng = np.random.default_rng(7)
        F, N = faces.shape[0], 30_001
        fi = np.concatenate([np.arange(F), rng.integers(0, F, N - F)]).astype(np.int32)
        _, bary = P.sample_bary_on_triangles(F, N, torch.Generator().manual_seed(7))
        return posed[0], posed[2], faces.astype(np.int32), fi, bary.numpy(), rng
    cano, verts, faces, fi, bary = P.turned_mesh()
    P.assert_turned_mesh_is_well_posed(cano, verts, faces)     # on the float64 reference, before anything is compared
    return cano, verts, faces, fi, bary, np.random.default_rng(5)


# ------------------------------------------------------------------ 1. the mesh pass
@pytest.mark.parametrize("mesh", ["head_template", "turned"])
def test_mesh_frame_matches_the_torch_restatement(gpu_device, mesh):
    """`phong_frame` against the float32 restatement (torch.inverse, index_add): |d| <= 1e-5 + 1e-5 |ref| for vert_normals,
    vert_quats and face_ratio — the bound the other bindings' forward is held to; and two calls give identical bits."""
    import torch
    from fateavatar_amd.binding import phong_canonical, phong_frame
    dev = gpu_device
    cano, verts, faces, _, _, _ = _meshes(mesh)
    t = torch.from_numpy
    ref = P.mesh_frame(t(cano), t(faces), t(verts))
    c = phong_canonical(t(cano).to(dev), t(faces).to(dev))
    got = phong_frame(c, t(verts).to(dev))
    again = phong_frame(c, t(verts).to(dev))
    torch.cuda.synchronize()
    for name, g, a, r in zip(("vert_normals", "vert_quats", "face_ratio"), got, again, ref):
        assert g.shape == r.shape and bool(torch.isfinite(r).all()) and bool(torch.isfinite(g).all()), name
        err = float(((g.cpu() - r).abs() - 1e-5 * r.abs()).max())
        print(f"{mesh} {name}: max (|d| - 1e-5 |ref|) {err:.3e}")
        assert err <= 1e-5, (name, err)
        assert torch.equal(g, a), name


# ------------------------------------------------------------------ 2. the stand-alone op
@pytest.mark.parametrize("mesh", ["head_template", "turned"])
def test_phong_op_matches_the_torch_restatement(gpu_device, mesh):
    """`bind_gaussians_phong` (on `phong_frame`'s arrays) against the float32 restatement end to end: forward within
    1e-5 + 1e-5 |ref|, gradients w.r.t. uvd, rotation and scaling within rel-L2 2e-4 of torch autograd; the u, v columns of
    d_uvd are exactly 0; a vertex gradient is refused."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_phong, phong_canonical, phong_frame
    dev = gpu_device
    cano, verts, faces, fi, bary, rng = _meshes(mesh)
    N = fi.shape[0]
    uvd = (0.05 * rng.normal(size=(N, 3))).astype(np.float32)
    rot = rng.normal(size=(N, 4)).astype(np.float32)
    scl = rng.normal(size=(N, 3)).astype(np.float32)
    w = [rng.normal(size=s).astype(np.float32) for s in ((N, 3), (N, 4), (N, 3))]
    t = torch.from_numpy

    def run(device):
        x = [t(a).to(device).requires_grad_(True) for a in (uvd, rot, scl)]
        c, v, f = t(cano).to(device), t(verts).to(device), t(faces).to(device)
        if device == "cpu":
            out = P.phong_bind(v, f, t(fi), t(bary), P.mesh_frame(c, f, v), *x)
        else:
            out = bind_gaussians_phong(v, f, t(fi).to(device), t(bary).to(device), phong_frame(phong_canonical(c, f), v), *x)
        torch.autograd.backward(list(out), [t(a).to(device) for a in w])
        return [o.detach().cpu() for o in out], [a.grad.cpu() for a in x]

    ref_out, ref_grad = run("cpu")
    got_out, got_grad = run(dev)
    for name, g, r in zip(("xyz", "rotation", "scaling"), got_out, ref_out):
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(g).all()), name
        err = float(((g - r).abs() - 1e-5 * r.abs()).max())
        print(f"{mesh} forward {name}: max (|d| - 1e-5 |ref|) {err:.3e}")
        assert err <= 1e-5, (name, err)
    for name, g, r in zip(("uvd", "rotation", "scaling"), got_grad, ref_grad):
        assert bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0, name
        err = _rel(g, r)
        print(f"{mesh} gradient {name}: rel-L2 {err:.3e}")
        assert err <= 2e-4, (name, err)
    assert float(got_grad[0][:, :2].abs().max()) == 0.0 and float(ref_grad[0][:, :2].abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="no vertex gradient"):
        bind_gaussians_phong(t(verts).to(dev).requires_grad_(True), None, None, None, (None, None, None), None, None, None)


# ------------------------------------------------------------------ 3. folded against unfolded
@pytest.mark.parametrize("depth_alpha", [False, True])
@pytest.mark.parametrize("K", [1, 4])
def test_phong_binding_inside_the_kernels_equals_the_op(gpu_device, K, depth_alpha):
    """`render_bound_batch` with a PhongBinding against `bind_gaussians_phong` + `render_batch`: image, radii, visibility and
    out["bound"] the same BITS, gradients within 5e-5 rel-L2, densification counts equal — with gradients and under no_grad
    (the forward-only kernels).  The conditions of test_face_local_binding_inside_the_kernels_equals_the_op."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_phong, phong_frame
    from fateavatar_amd.bound import PhongBinding, render_bound_batch
    from fateavatar_amd.render import render_batch
    from fateavatar_amd.splatting import _SplattingFrame
    dev = gpu_device
    S = _template(dev, 128, 5, seed=3)
    bg = torch.ones(3, device=dev)
    N = 20_003
    base = _perturbed(S, dev, N, seed=4)
    gen = torch.Generator().manual_seed(9)
    gts = [torch.rand(3, 128, 128, generator=gen).to(dev) for _ in range(K)]
    wd = [torch.randn(1, 128, 128, generator=gen).to(dev) / 128 ** 2 for _ in range(K)]
    names = [n for n, _ in base.FIELDS]
    pb = PhongBinding(S["faces"], base.face_index, base.bary_coords, S["canonical"])

    class Holder:
        max_sh_degree = 0

        def __init__(self, leaves):
            for n, t in leaves.items():
                setattr(self, n, t)

        @property
        def get_features(self):
            return torch.cat((self._features_dc, self._features_rest), dim=1)

    def run(folded, grad=True):
        leaves = [{n: getattr(base, n).detach().clone().requires_grad_(grad) for n in names} for _ in range(K)]
        verts = [S["posed"][k + 1].clone() for k in range(K)]            # (frames 1 .. K: frame 0 is the canonical mesh)
        stats = [(torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev)) for _ in range(K)]
        pcs = [Holder(l) for l in leaves]
        cams = S["cams"][1:K + 1]
        if folded:
            outs = render_bound_batch(cams, [_SplattingFrame(pc, st) for pc, st in zip(pcs, stats)], verts, pb, bg,
                                      depth_alpha=depth_alpha)
            bound = [o["bound"] for o in outs]
        else:
            frames, bound = [], []
            for k in range(K):
                b = bind_gaussians_phong(verts[k], S["faces"], base.face_index, base.bary_coords,
                                         phong_frame(S["canonical"], verts[k]), leaves[k]["_uvd"], leaves[k]["_rotation"],
                                         leaves[k]["_scaling"])
                frames.append(_SplattingFrame(pcs[k], stats[k], b))
                bound.append(tuple(t.detach() for t in b))
            outs = render_batch(cams, frames, bg, depth_alpha=depth_alpha)
        if grad:
            loss = sum(torch.nn.functional.l1_loss(o["render"], gts[k]) for k, o in enumerate(outs))
            if depth_alpha:
                loss = loss + sum((o["depth"] * wd[k]).sum() + (o["alpha"] * wd[k].flip(1)).sum() for k, o in enumerate(outs))
            loss.backward()
        torch.cuda.synchronize()
        return outs, bound, leaves, stats

    def same_frames(o_f, b_f, o_u, b_u):
        for k in range(K):
            assert torch.equal(o_f[k]["render"], o_u[k]["render"]) and torch.equal(o_f[k]["radii"], o_u[k]["radii"])
            assert torch.equal(o_f[k]["visibility_filter"], o_u[k]["visibility_filter"])
            assert int((o_f[k]["radii"] > 0).sum()) > 1000
            if depth_alpha:
                assert torch.equal(o_f[k]["depth"], o_u[k]["depth"]) and torch.equal(o_f[k]["alpha"], o_u[k]["alpha"])
            for a, b in zip(b_f[k], b_u[k]):
                assert torch.equal(a, b) and not a.requires_grad

    o_f, b_f, l_f, s_f = run(True)
    o_u, b_u, l_u, s_u = run(False)
    same_frames(o_f, b_f, o_u, b_u)
    for k in range(K):
        for n in names:
            a, b = l_f[k][n].grad, l_u[k][n].grad
            if n == "_features_rest":                     # [N,0,3] at SH degree 0
                assert a is None or a.numel() == 0
                continue
            assert a is not None and b is not None and a.shape == b.shape, n
            err = _rel(a, b)
            assert err < 5e-5 and float(b.abs().max()) > 0, (n, err)
        assert float(l_f[k]["_uvd"].grad[:, :2].abs().max()) == 0.0
        assert _rel(o_f[k]["viewspace_points"].grad, o_u[k]["viewspace_points"].grad) < 5e-5
        assert torch.equal(s_f[k][1], s_u[k][1]) and float(s_u[k][1].max()) > 0
        assert float((s_f[k][0] - s_u[k][0]).abs().max()) <= 1e-4 * float(s_u[k][0].abs().max())
    # forward-only kernels: the same frame under no_grad, bit for bit the frame above
    with torch.no_grad():
        n_f, nb_f, _, _ = run(True, grad=False)
        n_u, nb_u, _, _ = run(False, grad=False)
    same_frames(n_f, nb_f, n_u, nb_u)
    same_frames(n_f, nb_f, o_f, b_f)
    # no vertex gradient in this mode
    with pytest.raises(RuntimeError, match="no vertex gradient"):
        render_bound_batch(S["cams"][1:2], [_SplattingFrame(base, None)], [S["posed"][1].clone().requires_grad_(True)], pb, bg)


# ------------------------------------------------------------------ 4. the whole path against the CPU oracle
def test_phong_frame_against_the_cpu_oracle(gpu_device):
    """Mesh pass and binding by the torch restatement, render with the CPU oracle; the device renders the same Gaussians straight
    from their binding.  Image: |d| <= 1e-5 + 1e-4 |ref| on >= 99.99 % of the values, every pixel outside explained as a
    threshold flip (util.explain_pixel).  Gradients (flip pixels masked out of dL/dpixel, no row exempt): |d| <= 1e-4 |ref| +
    5e-6 max|ref| on >= 99.9 % of the entries and rel-L2 <= 1e-4 — test_face_local_frame_against_the_cpu_oracle's bounds — for
    uvd, rotation, scaling, opacity and the colour.  10 000 Gaussians, SH degree 0, 160 x 160."""
    import torch
    from fateavatar_amd.bound import PhongBinding, render_bound_batch
    from fateavatar_amd.splatting import _SplattingFrame
    from oracle import oracle
    from tests import util
    dev = gpu_device
    res = 160
    S = _template(dev, res, 4, seed=1)
    pc = _perturbed(S, dev, 10_000, seed=6)
    with torch.no_grad():                       # splats large enough to cover the 160 x 160 head
        pc._scaling.add_(0.5)
    f = 2
    cam, c = S["cams"][f], S["cam_arrays"][f]
    bg = np.array([0.2, 0.5, 0.9], np.float32)
    # ---- reference: restatement (float32, CPU) -> activations -> oracle
    names = [n for n, _ in pc.FIELDS if n != "_features_rest"]
    ref = {n: getattr(pc, n).detach().cpu().clone().requires_grad_(True) for n in names}
    cano, verts, faces = S["posed"][0].cpu(), S["posed"][f].cpu(), S["faces"].cpu()
    xyz, rot_b, scl_b = P.phong_bind(verts, faces, pc.face_index.cpu(), pc.bary_coords.cpu(), P.mesh_frame(cano, faces, verts),
                                     ref["_uvd"], ref["_rotation"], ref["_scaling"])
    act = dict(scales=torch.exp(scl_b), rotations=torch.nn.functional.normalize(rot_b), opacities=torch.sigmoid(ref["_opacity"]))
    shs = ref["_features_dc"]
    npy = lambda t: np.ascontiguousarray(t.detach().numpy())  # noqa: E731
    o = oracle.forward(bg=bg, means3D=npy(xyz), opacities=npy(act["opacities"]), viewmatrix=c.world_view_transform,
                       projmatrix=c.full_proj_transform, campos=c.camera_center, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
                       H=res, W=res, shs=npy(shs), sh_degree=0, scales=npy(act["scales"]), rotations=npy(act["rotations"]))
    # ---- device: the frame straight from its binding
    out = render_bound_batch([cam], [_SplattingFrame(pc, None)], [S["posed"][f]],
                             PhongBinding(S["faces"], pc.face_index, pc.bary_coords, S["canonical"]), torch.from_numpy(bg).to(dev))[0]
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
    for n in names:
        g, r = getattr(pc, n).grad.detach().cpu().numpy(), ref[n].grad.numpy()
        if n == "_uvd":
            assert np.abs(g[:, :2]).max() == 0 and np.abs(r[:, :2]).max() == 0
        scale = np.abs(r).max()
        assert g.shape == r.shape and np.isfinite(g).all() and scale > 0, n
        fr, rl = util.frac_close(g, r, 1e-4, 5e-6 * scale), util.rel_l2(g, r)
        print(f"gradient {n}: rel-L2 {rl:.2e}, {fr:.5f} of the entries within tolerance")
        assert (fr >= 0.999 or round((1.0 - fr) * g.size) <= 3) and rl <= 1e-4, (n, fr, rl)


# ------------------------------------------------------------------ 5. the step
def _targets(S, dev, bg, n_frames, N):
    """(set to train, images of a hidden avatar of the same embedding: coloured / opaque / placed / shaped differently)."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_phong, phong_frame
    from fateavatar_amd.render import render
    from fateavatar_amd.splatting import SplattingGaussians, _SplattingFrame
    make = lambda: SplattingGaussians.sample(S["posed"][0], S["faces"], N, torch.Generator().manual_seed(2))  # noqa: E731
    gt = make()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        gt._features_dc.copy_((torch.rand(N, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
        gt._uvd[:, 2].copy_((0.003 * torch.randn(N, generator=g)).to(dev))
        gt._rotation.add_((0.3 * torch.randn(N, 4, generator=g)).to(dev))
        gt._scaling.add_((0.3 * torch.randn(N, 3, generator=g)).to(dev))
    imgs = []
    with torch.no_grad():
        for f in range(n_frames):
            b = bind_gaussians_phong(S["posed"][f], S["faces"], gt.face_index, gt.bary_coords, phong_frame(S["canonical"], S["posed"][f]),
                                     gt._uvd, gt._rotation, gt._scaling)
            imgs.append(render(S["cams"][f], _SplattingFrame(gt, None, b), bg)["render"].clone())
    return make, imgs


def test_splatting_step_graph_follows_eager(gpu_device):
    """40 steps of SplattingStep, the reference's 10 000 Gaussians at 128 x 128 over an 8-frame sequence: the replayed HIP graph
    (mesh pass included) follows the eager step — losses to rtol 2e-2, util.assert_same_trajectory —, the loss falls, the
    stand-alone op (`fold_binding=False`) gives the same losses to rtol 2e-2, every non-empty group moved and the u, v columns
    of `_uvd` did not."""
    import torch
    from fateavatar_amd.splatting import SPLATTING_LRS, SplattingStep
    from tests import util
    dev = gpu_device
    res, n_frames, steps, N = 128, 8, 40, 10_000
    S = _template(dev, res, n_frames)
    bg = torch.ones(3, device=dev)
    make, gts = _targets(S, dev, bg, n_frames, N)

    def run(use_graph, fold=True):
        pc = make()
        st = SplattingStep(pc, S["canonical"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=use_graph, fold_binding=fold)
        assert st.adam_segments() == [(N * 3, SPLATTING_LRS["uvd"]), (N, SPLATTING_LRS["opacity"]), (N * 3, SPLATTING_LRS["feature_dc"]),
                                      (0, SPLATTING_LRS["feature_dc"] / 20), (N * 4, SPLATTING_LRS["rotation"]),
                                      (N * 3, SPLATTING_LRS["scaling"])]
        losses = [float(st.step(S["cams"][it % n_frames], S["posed"][it % n_frames], gts[it % n_frames])) for it in range(steps)]
        torch.cuda.synchronize()
        st.check()
        return pc, losses, st

    pc_e, loss_e, st_e = run(False)
    pc_g, loss_g, st_g = run(True)
    assert st_g._graph is not None and st_e._graph is None and st_g.overflows == 0
    assert st_g.adam.step_count == steps == st_e.adam.step_count
    print("loss, first and last 8 steps:", np.mean(loss_e[:8]), np.mean(loss_e[-8:]))
    assert np.mean(loss_e[-8:]) < np.mean(loss_e[:8]), (loss_e[:8], loss_e[-8:])
    assert np.allclose(loss_g, loss_e, rtol=2e-2), (loss_g[-4:], loss_e[-4:])
    assert torch.equal(st_g.denom, st_e.denom) and float(st_e.denom.max()) > 0
    util.assert_same_trajectory(pc_g.flat, pc_e.flat, "graph vs eager", tight=2e-2)
    fresh = make()
    for name, w in pc_e.FIELDS:
        if w:
            assert float((getattr(pc_e, name).detach() - getattr(fresh, name).detach()).abs().max()) > 0, name
    assert float(pc_e._uvd.detach()[:, :2].abs().max()) == 0.0            # zero gradient: Adam leaves them where they were
    pc_u, loss_u, st_u = run(False, fold=False)
    assert np.allclose(loss_u, loss_e, rtol=2e-2), (loss_u[-4:], loss_e[-4:])
    assert torch.equal(st_u.denom, st_e.denom)


def test_splatting_step_parameters_follow_torch_adam_on_the_same_gradients(gpu_device):
    """Six steps: after every step the flat parameter buffer equals torch.optim.Adam over the reference's six groups
    (train/optim.py:106-117) fed the gradients the step left in its flat gradient buffer, within
    test_fused_adam_matches_torch_adam's bound (rtol 2e-6, atol 1e-7).  And a checkpoint round trip restores the step."""
    import torch
    from fateavatar_amd.splatting import SPLATTING_LRS, SplattingGaussians, SplattingStep
    from tests import util
    dev = gpu_device
    res, n_frames, N = 128, 4, 10_000
    S = _template(dev, res, n_frames, seed=2)
    bg = torch.ones(3, device=dev)
    make, gts = _targets(S, dev, bg, n_frames, N)
    pc = make()
    st = SplattingStep(pc, S["canonical"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False)
    sizes = [n for n, _ in st.adam_segments()]
    ref = [t.clone().requires_grad_() for t in torch.split(pc.flat.detach(), sizes)]
    lrs = [SPLATTING_LRS[k] for k in ("uvd", "opacity", "feature_dc", "feature_rest", "rotation", "scaling")]
    topt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(ref, lrs)], lr=0.0)
    for it in range(6):
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
    assert list(sd["model"]) == ["_uvd", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "sample_fidxs",
                                 "sample_bary"]
    other = SplattingGaussians(torch.zeros(7, dtype=torch.int32), torch.full((7, 3), 1 / 3), -4.0, dev)
    st2 = SplattingStep(other, S["canonical"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False)
    assert st2.load_state_dict(sd) == [] and st2.pc.P == pc.P
    for s in (st, st2):
        s.step(S["cams"][2], S["posed"][2], gts[2])
    torch.cuda.synchronize()
    util.assert_same_trajectory(st2.pc.flat, pc.flat, "checkpoint round trip", tight=2e-3)
    assert st2.adam.step_count == 7


# ------------------------------------------------------------------ 6. the other modes are what they were
def test_plain_descriptor_is_the_shell_binding_and_face_local_frames_keep_their_bits(gpu_device):
    """A shell descriptor built as callers built it before the Phong mode existed (plain fr_binding, `mode` never written) renders the frame of
    `bind_gaussians` + `render`; and a face-local frame rendered before and after a Phong frame on the same handle is the
    same bits."""
    import torch
    from fateavatar_amd import _lib, mesh_sampling, rasterizer, scenes
    from fateavatar_amd.avatar import AvatarGaussians, _BoundFrame
    from fateavatar_amd.binding import SHELL, _describe, bind_gaussians, face_scale
    from fateavatar_amd.bound import FaceLocalBinding, PhongBinding, render_bound_batch
    from fateavatar_amd.render import _screenspace_points, _settings, render
    from fateavatar_amd.rigged import RiggedGaussians, _RiggedFrame
    from fateavatar_amd.splatting import _SplattingFrame
    dev = gpu_device
    S = _template(dev, 128, 3)
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
    b = _describe(SHELL, verts, S["faces"], pc.face_index, pc._offset.detach(), pc._rotation.detach(), pc._scaling.detach(),
                  pc.bary_coords, canon, 0.05, True)
    assert type(b) is _lib.fr_binding and b.mode == _lib.FR_BIND_SHELL and not b.local_xyz      # no Phong tail at all
    xyz, rot, scl = (torch.empty((pc.P, k), device=dev) for k in (3, 4, 3))
    sp = _screenspace_points(xyz, pc)
    args = rasterizer._forward_args(rs, xyz, sp, pc._features_dc.detach(), empty, pc._opacity.detach(), scl, rot, empty)
    res = rasterizer.rasterize_gaussians_batch([args], raw=True, bindings=[b])[0]
    torch.cuda.synchronize()
    assert int((res[2] > 0).sum()) > 1000
    with torch.no_grad():
        bound = bind_gaussians(verts, S["faces"], pc.face_index, pc.bary_coords, canon, pc._offset, pc._rotation, pc._scaling, 0.05, True)
        ref = render(cam, _BoundFrame(bound[0], pc, bound[1], bound[2], None), bg)
    assert torch.equal(ref["render"], res[1]) and torch.equal(ref["radii"], res[2])
    for x, y in zip(bound, (xyz, rot, scl)):
        assert torch.equal(x, y)
    # ---- face-local, Phong, face-local again on the same handle
    rg = RiggedGaussians.one_per_face(S["F"], dev)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        rg._xyz.copy_((0.5 * torch.randn(S["F"], 3, generator=g)).to(dev))
        rg._features_dc.copy_(torch.rand(S["F"], 1, 3, generator=g).to(dev))
        rg._opacity.fill_(1.0)
    ph = _perturbed(S, dev, 12_345, seed=8)

    def face_local():
        with torch.no_grad():
            o = render_bound_batch([cam], [_RiggedFrame(rg, None)], [verts], FaceLocalBinding(S["faces"], rg.binding), bg)[0]
        torch.cuda.synchronize()
        return [o["render"].clone(), o["radii"].clone(), *[t.clone() for t in o["bound"]]]

    before = face_local()
    with torch.no_grad():
        o = render_bound_batch([cam], [_SplattingFrame(ph, None)], [verts],
                               PhongBinding(S["faces"], ph.face_index, ph.bary_coords, S["canonical"]), bg)[0]
    torch.cuda.synchronize()
    assert int((o["radii"] > 0).sum()) > 1000
    after = face_local()
    assert int((before[1] > 0).sum()) > 1000
    for x, y in zip(before, after):
        assert torch.equal(x, y)
