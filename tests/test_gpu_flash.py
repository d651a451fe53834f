"""-m gpu: FlashAvatar's MLP-deformed binding (model/baseline/flashavatar.py:242-276) and Huber term (train/loss.py:217-239) on the
device — the stand-alone op, the binding inside the rasterizer's per-Gaussian kernels, the whole path against the CPU oracle,
the Huber launch, the fused optimisation step and its seam to the caller's MLP, and the three other modes left as they were.
The reference of every comparison is the torch restatement of tests/flash_ref.py (pinned on the CPU by tests/test_flash_host.py)."""
import numpy as np
import pytest

from tests import flash_ref as R

pytestmark = pytest.mark.gpu


def _template(dev, res, n_frames, seed=0):
    """The head template posed by the synthetic INSTA sequence; frame 0 is the canonical mesh."""
    import torch
    from fateavatar_amd import insta
    from fateavatar_amd.model import TorchCamera
    transform, posed, faces = insta.synthetic_sequence(n_frames, res, seed)
    arrays = insta.camera_arrays(transform)
    posed_t, faces_t = torch.from_numpy(posed).to(dev), torch.from_numpy(faces).to(dev).to(torch.int32).contiguous()
    return dict(posed=posed_t, faces=faces_t, cams=[TorchCamera(c, dev) for c in arrays], cam_arrays=arrays, F=int(faces.shape[0]))


def _gaussians(S, dev, N, seed, perturb=True):
    """N Gaussians at random barycentric points of the template, log-scale from the knn estimate of the canonical points; with
    `perturb` away from the initial state: anisotropic rotated splats, coloured, opacity 0.6."""
    import torch
    from fateavatar_amd.flash import FlashGaussians
    from fateavatar_amd.knn import init_scale_by_knn
    from fateavatar_amd.splatting import sample_bary_on_triangles
    g = torch.Generator().manual_seed(seed)
    fi, bary = sample_bary_on_triangles(S["F"], N, g)
    pts = torch.einsum("nij,ni->nj", S["posed"][0][S["faces"].long()][fi.to(dev)], bary.to(dev)).contiguous()
    pc = FlashGaussians(fi, bary, float(init_scale_by_knn(pts)[2]), dev)
    if perturb:
        with torch.no_grad():
            pc._scaling.add_((0.3 * torch.randn(N, 3, generator=g)).to(dev))
            pc._rotation.add_((0.5 * torch.randn(N, 4, generator=g)).to(dev))
            pc._features_dc.copy_((torch.rand(N, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
            pc._opacity.fill_(float(np.log(0.6 / 0.4)))
    return pc


def _deform(N, g, dev=None):
    """MLP outputs of a plausible size: positions move by about a splat, rotations turn visibly, and the scale columns are
    small because the binding MULTIPLIES the raw log-scale (about -5.5 here) by exp(tanh(.)): 0.05 moves it by +-0.3, the
    spread the sibling modes' tests give their splats (0.3 would stretch them by a factor of seven, up to half the image)."""
    import torch
    d = torch.randn(N, 10, generator=g) * torch.tensor([0.01] * 3 + [0.5] * 4 + [0.05] * 3)
    return d.to(dev) if dev is not None else d


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _meshes(name):
    """(verts, faces, face_index, bary, rng) as numpy: the head template at frame 2 of the synthetic sequence with every face
    used at least once, or a hand mesh of 4 faces."""
    import torch
    from fateavatar_amd.splatting import sample_bary_on_triangles
    if name == "head_template":
        from tests import phong_ref
        posed, faces = phong_ref.head_template()
        rng = np.random.default_rng(7)
        F, N = faces.shape[0], 30_001
        fi = np.concatenate([np.arange(F), rng.integers(0, F, N - F)]).astype(np.int32)
        _, bary = sample_bary_on_triangles(F, N, torch.Generator().manual_seed(7))
        return posed[2], faces.astype(np.int32), fi, bary.numpy(), rng
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0.5], [-0.5, 0.3, 0.8]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [1, 4, 2], [3, 5, 0]], np.int32)
    fi = np.array([0, 1, 2, 3, 3, 1, 0], np.int32)
    _, bary = sample_bary_on_triangles(4, 7, torch.Generator().manual_seed(3))
    return verts, faces, fi, bary.numpy(), np.random.default_rng(5)


# ------------------------------------------------------------------ 1. the stand-alone op
@pytest.mark.parametrize("mesh", ["head_template", "hand"])
def test_deform_op_matches_the_torch_restatement(gpu_device, mesh):
    """`bind_gaussians_deform` against the float32 restatement on the CPU: forward within 1e-5 + 1e-5 |ref|, gradients w.r.t.
    deform, rotation, scaling and verts within rel-L2 2e-4 of torch autograd (test_phong_op_matches_the_torch_restatement's
    bounds; the vertex bound as the shell op's).  deform ~ 1.5 N(0,1): tanh runs into saturation; the rotations are unnormalised
    and some products have a negative real part, which stays."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_deform
    dev = gpu_device
    verts, faces, fi, bary, rng = _meshes(mesh)
    N = fi.shape[0]
    deform = (1.5 * rng.normal(size=(N, 10))).astype(np.float32)
    deform[0] = 4.0 * np.sign(deform[0])                          # (seven rows alone need not reach saturation)
    rot = rng.normal(size=(N, 4)).astype(np.float32)
    scl = rng.normal(size=(N, 3)).astype(np.float32)
    w = [rng.normal(size=s).astype(np.float32) for s in ((N, 3), (N, 4), (N, 3))]
    t = torch.from_numpy

    def run(device):
        x = [t(a).to(device).requires_grad_(True) for a in (verts, deform, rot, scl)]
        f, i, b = t(faces).to(device), t(fi).to(device), t(bary).to(device)
        out = R.deform_bind(x[0], f, i, b, *x[1:]) if device == "cpu" else bind_gaussians_deform(x[0], f, i, b, *x[1:])
        torch.autograd.backward(list(out), [t(a).to(device) for a in w])
        return [o.detach().cpu() for o in out], [a.grad.cpu() for a in x]

    ref_out, ref_grad = run("cpu")
    got_out, got_grad = run(dev)
    assert int((ref_out[1][:, 0] < 0).sum()) >= 1 and float(np.abs(np.tanh(deform)).max()) > 0.999
    neg = ref_out[1][:, 0] < -1e-3
    assert bool((got_out[1][neg, 0] < 0).all())                                   # the sign is kept, not standardised
    for name, g, r in zip(("xyz", "rotation", "scaling"), got_out, ref_out):
        assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(g).all()), name
        err = float(((g - r).abs() - 1e-5 * r.abs()).max())
        print(f"{mesh} forward {name}: max (|d| - 1e-5 |ref|) {err:.3e}")
        assert err <= 1e-5, (name, err)
    for name, g, r in zip(("verts", "deform", "rotation", "scaling"), got_grad, ref_grad):
        assert g.shape == r.shape and bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0, name
        err = _rel(g, r)
        print(f"{mesh} gradient {name}: rel-L2 {err:.3e}")
        assert err <= 2e-4, (name, err)


# ------------------------------------------------------------------ 2. folded against unfolded
@pytest.mark.parametrize("depth_alpha", [False, True])
@pytest.mark.parametrize("K", [1, 4])
def test_deform_binding_inside_the_kernels_equals_the_op(gpu_device, K, depth_alpha):
    """`render_bound_batch` with a DeformBinding against `bind_gaussians_deform` + `render_batch`, 128 x 128, N = 16 387, a
    different deform per view: image, radii, visibility, planes and out["bound"] the same BITS, gradients of all raw parameters,
    deform, verts and viewspace_points within 5e-5 rel-L2, densification counts equal — with gradients and under no_grad (the
    forward-only kernels).  150 Gaussians of every view sit on a triangle behind that view's camera: culled, and their ten
    d_deform words are exactly 0 in a buffer pre-filled with 7.0.  The conditions of
    test_phong_binding_inside_the_kernels_equals_the_op."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_deform
    from fateavatar_amd.bound import DeformBinding, render_bound_batch
    from fateavatar_amd.flash import _FlashFrame
    from fateavatar_amd.rasterizer import GradOut
    from fateavatar_amd.render import render_batch
    dev = gpu_device
    S = _template(dev, 128, 5, seed=3)
    bg = torch.ones(3, device=dev)
    N, n_behind = 16_387, 150
    base = _gaussians(S, dev, N, seed=4)
    V, F = int(S["posed"].shape[1]), S["F"]
    # one more face: a small triangle BEHIND each view's camera (on the far side of it from the head), with the last rows on it
    faces = torch.cat([S["faces"], torch.tensor([[V, V + 1, V + 2]], dtype=torch.int32, device=dev)])
    face_index = base.face_index.clone()
    face_index[N - n_behind:] = F
    tri = torch.tensor([[0.0, 0, 0], [0.01, 0, 0], [0, 0.01, 0]])
    views = []
    for k in range(K):
        c = torch.from_numpy(np.asarray(S["cam_arrays"][k + 1].camera_center, np.float32).reshape(3))
        behind = c + (c - S["posed"][k + 1].mean(0).cpu())
        views.append(torch.cat([S["posed"][k + 1], (behind + tri).to(dev)]).contiguous())
    gen = torch.Generator().manual_seed(9)
    gts = [torch.rand(3, 128, 128, generator=gen).to(dev) for _ in range(K)]
    wd = [torch.randn(1, 128, 128, generator=gen).to(dev) / 128 ** 2 for _ in range(K)]
    deforms = [_deform(N, gen, dev) for _ in range(K)]
    names = ["_opacity", "_features_dc", "_rotation", "_scaling"]
    db = DeformBinding(faces, face_index, base.bary_coords)

    class Holder:
        max_sh_degree = 0

        def __init__(self, leaves):
            for n, t in leaves.items():
                setattr(self, n, t)

    def run(folded, grad=True):
        leaves = [{n: getattr(base, n).detach().clone().requires_grad_(grad) for n in names} for _ in range(K)]
        dfs = [d.clone().requires_grad_(grad) for d in deforms]
        bufs = [torch.full((N, 10), 7.0, device=dev) for _ in range(K)]
        if folded and grad:
            for d, b in zip(dfs, bufs):
                d._fr_grad_out = GradOut(b)                                   # the kernel writes d_deform into this buffer
        verts = [v.clone().requires_grad_(grad) for v in views]
        stats = [(torch.zeros(N, 1, device=dev), torch.zeros(N, 1, device=dev)) for _ in range(K)]
        pcs = [Holder(l) for l in leaves]
        cams = S["cams"][1:K + 1]
        if folded:
            outs = render_bound_batch(cams, [_FlashFrame(pc, st, deform=d) for pc, st, d in zip(pcs, stats, dfs)], verts, db, bg,
                                      depth_alpha=depth_alpha)
            bound = [o["bound"] for o in outs]
        else:
            frames, bound = [], []
            for k in range(K):
                b = bind_gaussians_deform(verts[k], faces, face_index, base.bary_coords, dfs[k], leaves[k]["_rotation"],
                                          leaves[k]["_scaling"])
                frames.append(_FlashFrame(pcs[k], stats[k], bound=b))
                bound.append(tuple(t.detach() for t in b))
            outs = render_batch(cams, frames, bg, depth_alpha=depth_alpha)
        if grad:
            loss = sum(torch.nn.functional.l1_loss(o["render"], gts[k]) for k, o in enumerate(outs))
            if depth_alpha:
                loss = loss + sum((o["depth"] * wd[k]).sum() + (o["alpha"] * wd[k].flip(1)).sum() for k, o in enumerate(outs))
            loss.backward()
        torch.cuda.synchronize()
        return outs, bound, leaves, stats, dfs, verts, bufs

    def same_frames(o_f, b_f, o_u, b_u):
        for k in range(K):
            assert torch.equal(o_f[k]["render"], o_u[k]["render"]) and torch.equal(o_f[k]["radii"], o_u[k]["radii"])
            assert torch.equal(o_f[k]["visibility_filter"], o_u[k]["visibility_filter"])
            assert int((o_f[k]["radii"] > 0).sum()) > 1000
            if depth_alpha:
                assert torch.equal(o_f[k]["depth"], o_u[k]["depth"]) and torch.equal(o_f[k]["alpha"], o_u[k]["alpha"])
            for a, b in zip(b_f[k], b_u[k]):
                assert torch.equal(a, b) and not a.requires_grad

    o_f, b_f, l_f, s_f, d_f, v_f, bufs = run(True)
    o_u, b_u, l_u, s_u, d_u, v_u, _ = run(False)
    same_frames(o_f, b_f, o_u, b_u)
    for k in range(K):
        for n in names:
            a, b = l_f[k][n].grad, l_u[k][n].grad
            assert a is not None and b is not None and a.shape == b.shape, n
            err = _rel(a, b)
            assert err < 5e-5 and float(b.abs().max()) > 0, (n, err)
        for what, a, b in (("deform", d_f[k].grad, d_u[k].grad), ("verts", v_f[k].grad, v_u[k].grad),
                           ("viewspace_points", o_f[k]["viewspace_points"].grad, o_u[k]["viewspace_points"].grad)):
            assert a is not None and b is not None and a.shape == b.shape, what
            err = _rel(a, b)
            assert err < 5e-5 and float(b.abs().max()) > 0, (what, err)
        assert torch.equal(s_f[k][1], s_u[k][1]) and float(s_u[k][1].max()) > 0
        assert float((s_f[k][0] - s_u[k][0]).abs().max()) <= 1e-4 * float(s_u[k][0].abs().max())
        # culled Gaussians: all ten gradient words written, as zeros, into the buffer that held 7.0
        culled = o_f[k]["radii"] == 0
        assert int(culled.sum()) >= 100 and bool(culled[N - n_behind:].all())
        assert d_f[k].grad.data_ptr() == bufs[k].data_ptr()
        assert float(bufs[k][culled].abs().max()) == 0.0 and not bool((bufs[k] == 7.0).any())
        assert float(d_u[k].grad[culled].abs().max()) == 0.0
        assert float(v_f[k].grad[V:].abs().max()) == 0.0                     # nothing reaches the triangle behind the camera
    # forward-only kernels: the same frame under no_grad, bit for bit the frame above
    with torch.no_grad():
        n_f, nb_f = run(True, grad=False)[:2]
        n_u, nb_u = run(False, grad=False)[:2]
    same_frames(n_f, nb_f, n_u, nb_u)
    same_frames(n_f, nb_f, o_f, b_f)


# ------------------------------------------------------------------ 3. the whole path against the CPU oracle
def test_deform_frame_against_the_cpu_oracle(gpu_device):
    """Binding by the torch restatement, render with the CPU oracle; the device renders the same Gaussians straight from their
    binding.  Image: |d| <= 1e-5 + 1e-4 |ref| on >= 99.99 % of the values, every pixel outside explained as a threshold flip
    (util.explain_pixel).  Gradients (flip pixels masked out of dL/dpixel, no row exempt): |d| <= 1e-4 |ref| + 5e-6 max|ref| on
    >= 99.9 % of the entries and rel-L2 <= 1e-4 — test_phong_frame_against_the_cpu_oracle's bounds and flip handling — for
    deform, rotation, scaling, opacity and the colour.  10 000 Gaussians, SH degree 0, 160 x 160."""
    import torch
    from fateavatar_amd.bound import DeformBinding, render_bound_batch
    from fateavatar_amd.flash import _FlashFrame
    from oracle import oracle
    from tests import util
    dev = gpu_device
    res, N = 160, 10_000
    S = _template(dev, res, 4, seed=1)
    pc = _gaussians(S, dev, N, seed=6)
    with torch.no_grad():                       # splats large enough to cover the 160 x 160 head (the log-scale is negative)
        pc._scaling.add_(0.5)
    f = 2
    cam, c = S["cams"][f], S["cam_arrays"][f]
    bg = np.array([0.2, 0.5, 0.9], np.float32)
    deform = _deform(N, torch.Generator().manual_seed(12))
    # ---- reference: restatement (float32, CPU) -> activations -> oracle
    names = ["_opacity", "_features_dc", "_rotation", "_scaling"]
    ref = {n: getattr(pc, n).detach().cpu().clone().requires_grad_(True) for n in names}
    ref["deform"] = deform.clone().requires_grad_(True)
    verts, faces = S["posed"][f].cpu(), S["faces"].cpu()
    xyz, rot_b, scl_b = R.deform_bind(verts, faces, pc.face_index.cpu(), pc.bary_coords.cpu(), ref["deform"], ref["_rotation"],
                                      ref["_scaling"])
    act = dict(scales=torch.exp(scl_b), rotations=torch.nn.functional.normalize(rot_b), opacities=torch.sigmoid(ref["_opacity"]))
    shs = ref["_features_dc"]
    npy = lambda t: np.ascontiguousarray(t.detach().numpy())  # noqa: E731
    o = oracle.forward(bg=bg, means3D=npy(xyz), opacities=npy(act["opacities"]), viewmatrix=c.world_view_transform,
                       projmatrix=c.full_proj_transform, campos=c.camera_center, tanfovx=c.tanfovx, tanfovy=c.tanfovy,
                       H=res, W=res, shs=npy(shs), sh_degree=0, scales=npy(act["scales"]), rotations=npy(act["rotations"]))
    # ---- device: the frame straight from its binding
    dev_deform = deform.to(dev).requires_grad_(True)
    out = render_bound_batch([cam], [_FlashFrame(pc, None, deform=dev_deform)], [S["posed"][f]],
                             DeformBinding(S["faces"], pc.face_index, pc.bary_coords), torch.from_numpy(bg).to(dev))[0]
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
    assert pc._features_rest.grad is None
    for n in names + ["deform"]:
        g = (dev_deform.grad if n == "deform" else getattr(pc, n).grad).detach().cpu().numpy()
        r = ref[n].grad.numpy()
        scale = np.abs(r).max()
        assert g.shape == r.shape and np.isfinite(g).all() and scale > 0, n
        fr, rl = util.frac_close(g, r, 1e-4, 5e-6 * scale), util.rel_l2(g, r)
        print(f"gradient {n}: rel-L2 {rl:.2e}, {fr:.5f} of the entries within tolerance")
        assert (fr >= 0.999 or round((1.0 - fr) * g.size) <= 3) and rl <= 1e-4, (n, fr, rl)


# ------------------------------------------------------------------ 4. the Huber launch
def _huber_case(shape, seed):
    """(img, gt, mask) float32 CPU tensors: differences on both sides of alpha, some exactly +-alpha, some exactly 0."""
    import torch
    g = torch.Generator().manual_seed(seed)
    C, H, W = shape
    gt = torch.rand(C, H, W, generator=g)
    img = (gt + 0.15 * torch.randn(C, H, W, generator=g)).contiguous()
    flat_i, flat_g = img.view(-1), gt.view(-1)
    a = torch.tensor(R.ALPHA, dtype=torch.float32)
    n = flat_i.numel()
    flat_g[0:n:97] = 0.0
    flat_i[0:n:97] = a                           # d = +alpha exactly (float32)
    flat_g[1:n:101] = 0.0
    flat_i[1:n:101] = -a                         # d = -alpha
    flat_i[2:n:89] = flat_g[2:n:89]              # d = 0
    mask = torch.rand(1, H, W, generator=g)
    mask.view(-1)[0:H * W:7] = 1.0
    mask.view(-1)[3:H * W:11] = 0.0
    d = img - gt
    assert int((d == a).sum()) > 0 and int((d == -a).sum()) > 0 and int((d == 0).sum()) > 0
    return img, gt, mask


HUBER_GRID_CAP = 1024 * 256 * 4    # floats one trip of k_huber_loss_grad's float4 sweep covers at the launch's cap (kL1MaxBlocks, fr_optim.hip)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", [(3, 37, 41), (3, 128, 128), (3, 512, 512), (3, 593, 591), (4, 512, 512), (4, 65, 4033)])
def test_huber_loss_and_grad_matches_the_restatement(gpu_device, shape, masked):
    """(3 x 593 x 591 = 1 051 389 floats: past HUBER_GRID_CAP, so some lanes make a second trip; n % 4 = 1, so there is a scalar
    tail; H W is odd, so float4 pieces straddle the channel boundary of the mask's broadcast.  4 x 512 x 512 is HUBER_GRID_CAP exactly:
    every lane of the capped grid makes one trip; 4 x 65 x 4033 is one float4 more: one lane makes a second.)
    The three loss words within 1e-6 relative of the float64 restatement (test_l1_loss_and_grad_matches_autograd's bound), the
    gradient within rtol 1e-6 of the float32 restatement's autograd (a handful of roundings of same-signed terms, no
    cancellation; exactly 0 where d = 0); three repeated calls give identical bits (the workspace comes back zeroed, the sums
    are reproducible); without a gradient buffer the loss is still written."""
    import torch
    from fateavatar_amd.loss import huber_loss_and_grad, huber_workspace
    dev = gpu_device
    img, gt, mask = _huber_case(shape, seed=shape[1])
    if shape[1] > 512:
        assert img.numel() > HUBER_GRID_CAP and img.numel() % 4 == 1 and (shape[1] * shape[2]) % 4 != 0
    if shape[0] == 4:
        assert img.numel() == HUBER_GRID_CAP + (0 if shape[1] == 512 else 4)
    m = mask if masked else None
    want = [float(x) for x in R.huber_loss(img.double(), gt.double(), None if m is None else m.double())]
    leaf = img.clone().requires_grad_(True)
    R.huber_loss(leaf, gt, m)[0].backward()
    ws = huber_workspace(dev)
    dm = None if m is None else m.to(dev)
    runs = [huber_loss_and_grad(img.to(dev), gt.to(dev), mask=dm, workspace=ws) for _ in range(3)]
    torch.cuda.synchronize()
    loss, grad = runs[0][0].cpu(), runs[0][1].cpu()
    for k, name in enumerate(("total", "huber", "mouth")):
        print(f"{shape} masked={masked} {name}: {float(loss[k]):.9g} against {want[k]:.9g}")
        assert abs(float(loss[k]) - want[k]) <= 1e-6 * abs(want[k]), (name, float(loss[k]), want[k])
    if not masked:
        assert float(loss[2]) == 0.0 and float(loss[0]) == float(loss[1])
    rel = ((grad - leaf.grad).abs() / leaf.grad.abs().clamp_min(1e-30)).max()
    print(f"{shape} masked={masked} gradient: max relative difference {float(rel):.3e}")
    assert torch.allclose(grad, leaf.grad, rtol=1e-6, atol=0.0)
    assert float(grad[(img - gt) == 0].abs().max()) == 0.0
    for l, g in runs[1:]:
        assert torch.equal(l.cpu(), loss) and torch.equal(g.cpu(), grad)
    assert int(ws.count_nonzero()) == 0
    only, none = huber_loss_and_grad(img.to(dev), gt.to(dev), mask=dm, grad_out=False, workspace=ws)
    assert none is None and torch.equal(only.cpu(), loss)


def test_huber_launches_on_three_streams_do_not_mix(gpu_device):
    """Launches that overlap on three streams, each with its own workspace and its own images: every result is the bits of the
    same launch made alone, 20 times over."""
    import torch
    from fateavatar_amd.loss import huber_loss_and_grad, huber_workspace
    dev = gpu_device
    cases = [[t.to(dev) for t in _huber_case((3, 128, 128), seed=20 + k)] for k in range(3)]
    alone = [huber_loss_and_grad(i, g, mask=m, workspace=huber_workspace(dev)) for i, g, m in cases]
    alone = [(l.clone(), g.clone()) for l, g in alone]
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    spaces = [huber_workspace(dev) for _ in range(3)]
    outs = [(torch.zeros(3, device=dev), torch.zeros(3, 128, 128, device=dev)) for _ in range(3)]
    torch.cuda.synchronize()
    for _ in range(20):
        for s, (i, g, m), ws, (l, gr) in zip(streams, cases, spaces, outs):
            with torch.cuda.stream(s):
                huber_loss_and_grad(i, g, mask=m, loss_out=l, grad_out=gr, workspace=ws)
        torch.cuda.synchronize()
        for (l, gr), (wl, wg) in zip(outs, alone):
            assert torch.equal(l, wl) and torch.equal(gr, wg)
    assert len({float(l[0]) for l, _ in alone}) == 3


# ------------------------------------------------------------------ 5. the seam to the caller's MLP
@pytest.mark.parametrize("fold", [True, False])
def test_step_hands_the_mlp_and_the_mesh_their_gradients(gpu_device, fold):
    """One eager FlashStep.step at 128 x 128, N = 16 384, with a mouth mask: `d_deform` and `d_verts` agree within 5e-5 rel-L2
    with autograd through `bind_gaussians_deform` -> `render` fed the same dL/dimage (the fused Huber's), and `loss_terms` is
    `huber_loss_and_grad` of the kept render."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_deform
    from fateavatar_amd.flash import FlashStep, _FlashFrame
    from fateavatar_amd.loss import huber_loss_and_grad
    from fateavatar_amd.render import render
    dev = gpu_device
    res, N = 128, 16_384
    S = _template(dev, res, 3, seed=2)
    bg = torch.ones(3, device=dev)
    pc, twin = _gaussians(S, dev, N, seed=3), _gaussians(S, dev, N, seed=3)
    assert torch.equal(pc.flat, twin.flat)
    gen = torch.Generator().manual_seed(4)
    gt = torch.rand(3, res, res, generator=gen).to(dev)
    mask = (torch.rand(1, res, res, generator=gen) > 0.7).float().to(dev)
    deform = _deform(N, gen, dev)
    st = FlashStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False, fold_binding=fold, mouth_mask=True,
                   vertex_grad=True)
    with pytest.raises(ValueError, match="mouth_mask"):
        st.step(S["cams"][1], S["posed"][1], deform, gt)
    loss = st.step(S["cams"][1], S["posed"][1], deform.clone().requires_grad_(True), gt, mask)
    torch.cuda.synchronize()
    assert tuple(st.d_deform.shape) == (N, 10) and tuple(st.d_verts.shape) == tuple(S["posed"][1].shape)
    assert loss.data_ptr() == st.loss_terms.data_ptr() and float(loss) == float(st.loss_terms[0])
    want, _ = huber_loss_and_grad(st.out["render"], gt, mask=mask)
    assert torch.equal(want, st.loss_terms) and float(st.loss_terms[2]) > 0
    # ---- autograd through the stand-alone op on the parameters as they were before the update
    verts = S["posed"][1].clone().requires_grad_(True)
    d = deform.clone().requires_grad_(True)
    b = bind_gaussians_deform(verts, S["faces"], twin.face_index, twin.bary_coords, d, twin._rotation, twin._scaling)
    out = render(S["cams"][1], _FlashFrame(twin, None, bound=b), bg)
    assert torch.equal(out["render"], st.out["render"])
    out["render"].backward(st._dimage)
    for name, got, ref in (("d_deform", st.d_deform, d.grad), ("d_verts", st.d_verts, verts.grad)):
        err = _rel(got, ref)
        print(f"fold={fold} {name}: rel-L2 {err:.3e}")
        assert err < 5e-5 and float(ref.abs().max()) > 0, (name, err)
    no_mask = FlashStep(twin, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False)
    with pytest.raises(ValueError, match="mouth_mask"):
        no_mask.step(S["cams"][1], S["posed"][1], deform, gt, mask)
    assert no_mask.d_verts is None and no_mask.mask is None


# ------------------------------------------------------------------ 6. the step
def _mlp(dev, seed):
    """A small deformation network: canonical point and a per-frame condition in, the ten raw outputs out (small at first)."""
    import torch
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(3 + 4, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                              torch.nn.Linear(64, 10)).to(dev)
    with torch.no_grad():
        net[-1].weight.mul_(0.05)
        net[-1].bias.zero_()
    return net


def _targets(S, dev, bg, n_frames, N):
    """(set to train, images of a hidden avatar at the same places: coloured / opaque / shaped differently and deformed per frame,
    per-frame mouth masks, per-frame conditions)."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_deform
    from fateavatar_amd.flash import _FlashFrame
    from fateavatar_amd.render import render
    make = lambda: _gaussians(S, dev, N, seed=2, perturb=False)  # noqa: E731
    gt = make()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        gt._features_dc.copy_((torch.rand(N, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        gt._opacity.fill_(float(np.log(0.6 / 0.4)))
        gt._rotation.add_((0.3 * torch.randn(N, 4, generator=g)).to(dev))
        gt._scaling.add_((0.3 * torch.randn(N, 3, generator=g)).to(dev))
    res = S["cams"][0].image_height
    imgs, masks, conds = [], [], []
    yy, xx = torch.meshgrid(torch.arange(res), torch.arange(res), indexing="ij")
    with torch.no_grad():
        for f in range(n_frames):
            b = bind_gaussians_deform(S["posed"][f], S["faces"], gt.face_index, gt.bary_coords, _deform(N, g, dev), gt._rotation,
                                      gt._scaling)
            imgs.append(render(S["cams"][f], _FlashFrame(gt, None, bound=b), bg)["render"].clone())
            masks.append((((yy - 0.62 * res) / (0.10 * res)) ** 2 + ((xx - 0.5 * res) / (0.16 * res)) ** 2 < 1).float()[None].to(dev))
            conds.append(torch.tensor([np.sin(f), np.cos(f), f / n_frames, 1.0], dtype=torch.float32, device=dev))
    return make, imgs, masks, conds


def test_flash_step_graph_follows_eager(gpu_device):
    """40 steps of FlashStep with a mouth mask, 16 384 Gaussians at 128 x 128 over an 8-frame sequence, a small torch MLP trained
    through `d_deform` from a fixed seed: the replayed HIP graph follows the eager step — losses to rtol 2e-2,
    util.assert_same_trajectory —, the loss falls, the stand-alone op (`fold_binding=False`) gives the same losses to rtol 2e-2,
    every group but `_features_rest` moved, `_features_rest` is still exactly 0, and the MLP's weights moved.  Mirrors
    test_splatting_step_graph_follows_eager."""
    import torch
    from fateavatar_amd.flash import FLASH_LRS, FlashStep
    from tests import util
    dev = gpu_device
    res, n_frames, steps, N = 128, 8, 40, 16_384
    S = _template(dev, res, n_frames)
    bg = torch.ones(3, device=dev)
    make, gts, masks, conds = _targets(S, dev, bg, n_frames, N)

    def run(use_graph, fold=True):
        pc = make()
        net = _mlp(dev, seed=1)
        first = [p.detach().clone() for p in net.parameters()]
        # the reference's deformer rate (config/flashavatar.yaml: deformer_lr 1e-4).  Adam moves every weight by about its rate
        # per step whatever the gradient's size: at 1e-3 the 64-wide last layer shifts the outputs by O(1) within these 40
        # steps, tanh saturates, the Gaussians fly up to a metre off the head and out of the frame, and the two trajectories
        # differ in WHICH Gaussians are culled (measured at 1e-3: equal losses to 2e-2, but one opacity three rates apart)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        pts = pc.canonical_points(S["posed"][0], S["faces"])
        st = FlashStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=use_graph, fold_binding=fold, mouth_mask=True)
        assert st.adam_segments() == [(N, FLASH_LRS["opacity"]), (N * 3, FLASH_LRS["feature_dc"]), (N * 45, FLASH_LRS["feature_dc"] / 20),
                                      (N * 4, FLASH_LRS["rotation"]), (N * 3, FLASH_LRS["scaling"])]
        losses = []
        for it in range(steps):
            f = it % n_frames
            deform = net(torch.cat([pts, conds[f].expand(N, 4)], dim=1))
            losses.append(st.step(S["cams"][f], S["posed"][f], deform, gts[f], masks[f]))
            opt.zero_grad(set_to_none=True)
            deform.backward(st.d_deform)
            opt.step()
            losses[-1] = float(losses[-1])
        torch.cuda.synchronize()
        st.check()
        moved = [float((p.detach() - q).abs().max()) for p, q in zip(net.parameters(), first)]
        return pc, losses, st, moved

    pc_e, loss_e, st_e, moved_e = run(False)
    pc_g, loss_g, st_g, _ = run(True)
    assert st_g._graph is not None and st_e._graph is None and st_g.overflows == 0
    assert st_g.adam.step_count == steps == st_e.adam.step_count
    print("loss, first and last 8 steps:", np.mean(loss_e[:8]), np.mean(loss_e[-8:]))
    assert np.mean(loss_e[-8:]) < np.mean(loss_e[:8]), (loss_e[:8], loss_e[-8:])
    assert np.allclose(loss_g, loss_e, rtol=2e-2), (loss_g[-4:], loss_e[-4:])
    # (the counts need not be equal bit for bit as in the sibling test: the MLP moves the Gaussians, and a splat at the edge of
    # visibility may flip on float noise between the two trajectories)
    assert float(st_e.denom.max()) > 0 and float(st_g.denom.max()) > 0
    util.assert_same_trajectory(pc_g.flat, pc_e.flat, "graph vs eager", tight=2e-2)
    fresh = make()
    for name, _ in pc_e.FIELDS:
        d = float((getattr(pc_e, name).detach() - getattr(fresh, name).detach()).abs().max())
        assert (d == 0.0) if name == "_features_rest" else (d > 0), (name, d)
    assert float(pc_e._features_rest.detach().abs().max()) == 0.0 and float(pc_g._features_rest.detach().abs().max()) == 0.0
    assert min(moved_e) > 0, moved_e
    pc_u, loss_u, st_u, _ = run(False, fold=False)
    assert np.allclose(loss_u, loss_e, rtol=2e-2), (loss_u[-4:], loss_e[-4:])


# ------------------------------------------------------------------ 7. Adam and the checkpoint
def test_flash_step_parameters_follow_torch_adam_on_the_same_gradients(gpu_device):
    """Six steps: after every step the flat parameter buffer equals torch.optim.Adam over the reference's five groups
    (train/optim.py:45-51) fed the gradients the step left in its flat gradient buffer, within
    test_fused_adam_matches_torch_adam's bound (rtol 2e-6, atol 1e-7).  And a checkpoint round trip restores the step."""
    import torch
    from fateavatar_amd.flash import FLASH_LRS, FlashGaussians, FlashStep
    from tests import util
    dev = gpu_device
    res, n_frames, N = 128, 4, 16_384
    S = _template(dev, res, n_frames, seed=2)
    bg = torch.ones(3, device=dev)
    make, gts, masks, _ = _targets(S, dev, bg, n_frames, N)
    g = torch.Generator().manual_seed(8)
    deforms = [_deform(N, g, dev) for _ in range(n_frames)]
    pc = make()
    st = FlashStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False)
    sizes = [n for n, _ in st.adam_segments()]
    ref = [t.clone().requires_grad_() for t in torch.split(pc.flat.detach(), sizes)]
    lrs = [FLASH_LRS[k] for k in ("opacity", "feature_dc", "feature_rest", "rotation", "scaling")]
    topt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(ref, lrs)], lr=0.0)
    for it in range(6):
        f = it % n_frames
        st.step(S["cams"][f], S["posed"][f], deforms[f], gts[f])
        for p, gr in zip(ref, torch.split(pc.flat_grad, sizes)):
            p.grad = gr.clone()
        assert float(pc.flat_grad.abs().max()) > 0 and float(pc.grad_view("_features_rest").abs().max()) == 0.0
        topt.step()
        want = torch.cat([p.detach() for p in ref])
        assert torch.allclose(pc.flat, want, rtol=2e-6, atol=1e-7), (it, float((pc.flat - want).abs().max()))
    assert st.adam.step_count == 6
    # checkpoint: another step object restored from the state continues with the same update
    sd = st.state_dict()
    assert list(sd["model"]) == ["_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling", "face_index", "bary_coords"]
    assert tuple(sd["model"]["_features_rest"].shape) == (N, 15, 3)
    sd["model"]["deformNet.0.weight"] = torch.zeros(2, 2)          # the reference's checkpoint holds the MLP too: ignored here
    other = FlashGaussians(torch.zeros(7, dtype=torch.int32), torch.full((7, 3), 1 / 3), -4.0, dev)
    st2 = FlashStep(other, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], use_graph=False)
    assert st2.load_state_dict(sd) == ["deformNet.0.weight"] and st2.pc.P == pc.P and tuple(st2.deform.shape) == (N, 10)
    for s in (st, st2):
        s.step(S["cams"][2], S["posed"][2], deforms[2], gts[2])
    torch.cuda.synchronize()
    util.assert_same_trajectory(st2.pc.flat, pc.flat, "checkpoint round trip", tight=2e-3)
    assert st2.adam.step_count == 7


# ------------------------------------------------------------------ 8. the other modes are what they were
def test_the_other_modes_keep_their_bits_around_a_deform_frame(gpu_device):
    """A shell, a face-local and a Phong frame rendered before and after a deform frame on the same handle are the same bits; and a
    shell descriptor whose `mode` member is written explicitly (FR_BIND_SHELL) renders what the zero-filled one renders."""
    import ctypes as C
    import torch
    from fateavatar_amd import _lib, mesh_sampling, rasterizer, scenes
    from fateavatar_amd.avatar import AvatarGaussians, _RawFrame
    from fateavatar_amd.binding import SHELL, _describe, face_scale, phong_canonical
    from fateavatar_amd.bound import DeformBinding, FaceLocalBinding, MeshBinding, PhongBinding, render_bound_batch
    from fateavatar_amd.flash import _FlashFrame
    from fateavatar_amd.render import _screenspace_points, _settings
    from fateavatar_amd.rigged import RiggedGaussians, _RiggedFrame
    from fateavatar_amd.splatting import SplattingGaussians, _SplattingFrame
    dev = gpu_device
    S = _template(dev, 128, 3)
    verts0, faces_np, _ = scenes.head_geometry()
    fi, bc = mesh_sampling.random_sampling_barycoords(20_000, verts0, faces_np, np.random.default_rng(1))
    av = AvatarGaussians(fi, bc, float(np.log(2e-3)), dev)
    with torch.no_grad():
        av._features_dc.add_(0.3)
        av._offset.add_(0.2)
        av._opacity.add_(2.0)
    canon = face_scale(torch.from_numpy(verts0).to(dev), S["faces"])
    verts, cam, bg = S["posed"][1].contiguous(), S["cams"][1], torch.ones(3, device=dev)
    g = torch.Generator().manual_seed(3)
    rg = RiggedGaussians.one_per_face(S["F"], dev)
    with torch.no_grad():
        rg._xyz.copy_((0.5 * torch.randn(S["F"], 3, generator=g)).to(dev))
        rg._features_dc.copy_(torch.rand(S["F"], 1, 3, generator=g).to(dev))
        rg._opacity.fill_(1.0)
    canonical = phong_canonical(S["posed"][0], S["faces"])
    ph = SplattingGaussians.sample(S["posed"][0], S["faces"], 12_345, g)
    with torch.no_grad():
        ph._features_dc.copy_(torch.rand(12_345, 1, 3, generator=g).to(dev))
        ph._opacity.fill_(1.0)
    fl = _gaussians(S, dev, 16_387, seed=8)

    def frames():
        res = []
        with torch.no_grad():
            for holder, binding in ((_RawFrame(av, None), MeshBinding(S["faces"], av.face_index, av.bary_coords, canon, 0.05, True)),
                                    (_RiggedFrame(rg, None), FaceLocalBinding(S["faces"], rg.binding)),
                                    (_SplattingFrame(ph, None), PhongBinding(S["faces"], ph.face_index, ph.bary_coords, canonical))):
                o = render_bound_batch([cam], [holder], [verts], binding, bg)[0]
                torch.cuda.synchronize()
                assert int((o["radii"] > 0).sum()) > 1000
                res += [o["render"].clone(), o["radii"].clone(), *[t.clone() for t in o["bound"]]]
        return res

    before = frames()
    with torch.no_grad():
        o = render_bound_batch([cam], [_FlashFrame(fl, None, deform=_deform(16_387, g, dev))], [verts],
                               DeformBinding(S["faces"], fl.face_index, fl.bary_coords), bg)[0]
    torch.cuda.synchronize()
    assert int((o["radii"] > 0).sum()) > 1000
    for x, y in zip(before, frames()):
        assert torch.equal(x, y)
    # ---- the shell descriptor: `mode` written explicitly against a zero-filled member
    rs = _settings(cam, av, bg, 1.0)
    empty = torch.Tensor([])
    wrote = _describe(SHELL, verts, S["faces"], av.face_index, av._offset.detach(), av._rotation.detach(), av._scaling.detach(),
                      av.bary_coords, canon, 0.05, True)
    plain = _lib.fr_binding()
    for name, _ in _lib.fr_binding._fields_:
        if name not in ("mode", "local_xyz"):
            setattr(plain, name, getattr(wrote, name))
    wrote.mode = _lib.FR_BIND_SHELL
    assert bytes(memoryview(wrote)) == bytes(memoryview(plain)) and C.sizeof(plain) == C.sizeof(wrote)
    got = []
    for b in (wrote, plain):
        xyz, rot, scl = (torch.empty((av.P, k), device=dev) for k in (3, 4, 3))
        sp = _screenspace_points(xyz, av)
        args = rasterizer._forward_args(rs, xyz, sp, av._features_dc.detach(), empty, av._opacity.detach(), scl, rot, empty)
        res = rasterizer.rasterize_gaussians_batch([args], raw=True, bindings=[b])[0]
        torch.cuda.synchronize()
        got.append((res[1].clone(), res[2].clone(), xyz, rot, scl))
    assert int((got[0][1] > 0).sum()) > 1000
    for x, y in zip(*got):
        assert torch.equal(x, y)
    assert torch.equal(got[0][0], before[0])                 # ... which is the shell frame above
