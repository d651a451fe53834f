"""GPU: MonoGaussianAvatar's fused per-point calls (fateavatar_amd/mono.py over csrc/fr_point_lbs.hip) against the plain-torch
restatement (tests/mono_ref.py)."""
import functools

import pytest

from tests import mono_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(50, 6), (7, 5)]
NAMES = ("points", "shapedirs", "posedirs", "lbs_weights")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _reference(N, E, J):
    """The recipe's inputs (rounded to float32 once: all runs read the same values) and, on the CPU, the float64 restatement's
    output and gradients and the float32 restatement's error against them."""
    import torch
    p, S, P, w, c, f, g = R.recipe(N, E, J)
    r32 = lambda t: t.float()  # noqa: E731
    x32, c32, f32, g32 = [r32(t) for t in (p, S, P, w)], tuple(map(r32, c)), tuple(map(r32, f)), r32(g)

    def run(dtype):
        leaves = [t.to(dtype).requires_grad_(True) for t in x32]
        xyz = R.deform_points(*leaves, tuple(t.to(dtype) for t in c32), tuple(t.to(dtype) for t in f32))
        return xyz.detach(), torch.autograd.grad(xyz, leaves, g32.to(dtype))

    xyz64, grad64 = run(torch.float64)
    xyz32, grad32 = run(torch.float32)
    err32 = (float((xyz32.double() - xyz64).abs().max()), [_rel(a, b) for a, b in zip(grad32, grad64)])
    return x32, c32, f32, g32, xyz64, grad64, err32


def _on(dev, x32, c32, f32, g32):
    from fateavatar_amd.mono import PoseState
    return [t.to(dev) for t in x32], PoseState(*[t.to(dev) for t in c32]), PoseState(*[t.to(dev) for t in f32]), g32.to(dev)


@pytest.mark.parametrize("E,J", SHAPES)
@pytest.mark.parametrize("N", [1, 63, 65, 4099])
def test_deform_points_matches_the_float64_restatement(gpu_device, N, E, J):
    """Forward within 1e-5 + 1e-5 |ref| and each gradient within rel-L2 2e-4 of the float64 restatement (the sibling ops' bounds,
    test_deform_op_matches_the_torch_restatement): about 50x and 1000x the float32 restatement's own error on this recipe."""
    import torch
    from fateavatar_amd.mono import deform_points
    x32, c32, f32, g32, xyz64, grad64, err32 = _reference(N, E, J)
    x, c, f, g = _on(gpu_device, x32, c32, f32, g32)
    leaves = [t.requires_grad_(True) for t in x]
    xyz = deform_points(*leaves, c, f)
    grads = torch.autograd.grad(xyz, leaves, g)
    got = xyz.detach().cpu().double()
    assert bool(torch.isfinite(got).all())
    err = float(((got - xyz64).abs() - 1e-5 * xyz64.abs()).max())
    raw = float((got - xyz64).abs().max())
    print(f"N={N} E={E} J={J} forward: max |d| {raw:.3e} (float32 restatement {err32[0]:.3e}, ratio {raw / max(err32[0], 1e-30):.2f}); "
          f"max (|d| - 1e-5 |ref|) {err:.3e}")
    assert err <= 1e-5, err
    for name, gg, r, e32 in zip(NAMES, grads, grad64, err32[1]):
        gg = gg.cpu()
        assert gg.shape == r.shape and bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0 and float(r.abs().max()) > 0, name
        e = _rel(gg, r)
        print(f"N={N} E={E} J={J} gradient {name}: rel-L2 {e:.3e} (float32 restatement {e32:.3e}, ratio {e / max(e32, 1e-30):.2f})")
        assert e <= 2e-4, (name, e)


@pytest.mark.parametrize("E,J", SHAPES)
def test_each_gradient_alone_is_the_full_call_and_two_runs_agree(gpu_device, E, J):
    """A backward with only one gradient requested (the other pointers NULL) writes the bits of the full call; a second full
    run writes the same bits again."""
    import torch
    from fateavatar_amd.mono import deform_points
    x32, c32, f32, g32, *_ = _reference(4099, E, J)
    x, c, f, g = _on(gpu_device, x32, c32, f32, g32)

    def run(which):
        leaves = [t.detach().clone().requires_grad_(k in which) for k, t in enumerate(x)]
        xyz = deform_points(*leaves, c, f)
        return xyz.detach(), torch.autograd.grad(xyz, [leaves[k] for k in which], g)

    xyz, full = run((0, 1, 2, 3))
    xyz2, again = run((0, 1, 2, 3))
    assert torch.equal(xyz, xyz2)
    for name, a, b in zip(NAMES, full, again):
        assert torch.equal(a, b), name
    for k, name in enumerate(NAMES):
        xyz1, (alone,) = run((k,))
        assert torch.equal(xyz1, xyz) and torch.equal(alone, full[k]), name


def test_graph_replay_with_new_pose_states_is_the_eager_result(gpu_device):
    """Forward + backward captured once; new pose states are copied into the static buffers between replays."""
    import torch
    from fateavatar_amd.mono import PoseState, deform_points
    dev = gpu_device
    N, E, J = 4099, 50, 6
    x32, c32, f32, g32, *_ = _reference(N, E, J)
    x, c, f, g = _on(dev, x32, c32, f32, g32)
    poses = [(c, f)]
    for seed in (5, 6):
        _, _, _, _, c2, f2, _ = R.recipe(1, E, J, seed=seed)
        poses.append((PoseState(*[t.float().to(dev) for t in c2]), PoseState(*[t.float().to(dev) for t in f2])))

    def eager(c, f):
        leaves = [t.detach().clone().requires_grad_(True) for t in x]
        xyz = deform_points(*leaves, c, f)
        return [xyz.detach().clone()] + [t.clone() for t in torch.autograd.grad(xyz, leaves, g)]

    want = [eager(*p) for p in poses]
    assert not torch.equal(want[0][0], want[1][0])
    sc, sf = PoseState(*[t.clone() for t in c]), PoseState(*[t.clone() for t in f])
    leaves = [t.detach().clone().requires_grad_(True) for t in x]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xyz = deform_points(*leaves, sc, sf)
        grads = torch.autograd.grad(xyz, leaves, g)
    for (pc, pf), w in list(zip(poses, want))[::-1] + [(poses[1], want[1])]:
        for dst, src in zip(tuple(sc) + tuple(sf), tuple(pc) + tuple(pf)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("xyz",) + NAMES, [xyz, *grads], w):
            assert torch.equal(a, b), name


@functools.lru_cache(maxsize=None)
def _grid_case(V, N=4099):
    """Vertices and points on the grid of multiples of 1/64 resp. 1/128 in [-1, 1]^3 (differences, squares and their sums are
    exact in float32, so equal distances are equal bits): the last vertex duplicates vertex 0, the first points sit exactly
    midway between two vertices or on the duplicated vertex, the rest are random grid points."""
    import torch
    gen = torch.Generator().manual_seed(V)
    verts = torch.randint(-64, 65, (V, 3), generator=gen).float() / 64
    if V > 1:
        verts[V - 1] = verts[0]
    pts = torch.randint(-128, 129, (N, 3), generator=gen).float() / 128
    a, b = torch.randint(0, V, (512,), generator=gen), torch.randint(0, V, (512,), generator=gen)
    pts[:512] = (verts[a] + verts[b]) / 2
    pts[512:520] = verts[0]
    return verts, pts


@pytest.mark.parametrize("V", [1, 5, 5023])
def test_nearest_vertex_is_the_float32_restatement_exactly(gpu_device, V):
    import torch
    from fateavatar_amd.mono import nearest_vertex
    verts, pts = (t.to(gpu_device) for t in _grid_case(V))
    idx, d2 = nearest_vertex(pts, verts)
    ref_idx, ref_d2 = R.nearest_vertex(pts, verts)
    assert idx.dtype == torch.int32 and torch.equal(idx.long(), ref_idx)
    assert torch.equal(d2.view(torch.int32), ref_d2.view(torch.int32))
    if V > 1:
        # rows in which more than one vertex attains the minimum: the lowest of them was taken
        rows = torch.arange(0, 520, device=gpu_device)
        d = ((pts[rows, None, :] - verts[None]) ** 2)
        d = (d[..., 0] + d[..., 1]) + d[..., 2]
        attain = d == d.min(dim=1, keepdim=True).values
        tied = attain.sum(1) > 1
        assert int(tied.sum()) >= 8
        lowest = attain.to(torch.int8).argmax(dim=1)
        assert torch.equal(idx[rows][tied].long(), lowest[tied])
        assert bool((idx[512:520] == 0).all())                      # on the duplicated vertex: index 0, not V - 1
    # a general cloud, too (no grid)
    gen = torch.Generator().manual_seed(1)
    p2, v2 = torch.randn((777, 3), generator=gen).to(gpu_device), torch.randn((V, 3), generator=gen).to(gpu_device)
    i2, dd2 = nearest_vertex(p2, v2)
    r2, rd2 = R.nearest_vertex(p2, v2)
    assert torch.equal(i2.long(), r2) and torch.equal(dd2.view(torch.int32), rd2.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _terms_case(N, V, E, J, seed=0):
    import torch
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    index = torch.randint(0, V, (N,), generator=gen, dtype=torch.int32)
    index[0], index[1] = 0, V - 1
    gt = [torch.softmax(rn(V, J), 1), 0.01 * rn(V, 36, 3), 0.01 * rn(V, 3, E)]
    pred = [torch.softmax(rn(N, J), 1), 0.01 * rn(N, 36, 3), 0.01 * rn(N, 3, E)]
    return index, pred, gt


# typical size of pred - gt per term on _terms_case (softmax rows of 6: ~0.2; two 0.01 N(0,1): 0.014)
_TERM_SIGMA = (0.2, 0.014, 0.014)


@pytest.mark.parametrize("E,J", SHAPES)
def test_lbs_terms_losses_and_added_gradients(gpu_device, E, J):
    """Losses within 1e-6 relative of the float64 restatement; what the kernel ADDED to pre-filled buffers within rel-L2 1e-6
    of float64 autograd's weight_k * d loss_k / d pred_k.  The buffers are pre-filled with values of the gradient's own size
    (weight_k * 2 sigma_k / count_k, from the inputs' spread), so that the sum's rounding (2^-24 of the sum) stays below the
    bound on the added part; a zero weight leaves its array's bits alone."""
    import torch
    from fateavatar_amd.mono import LbsWeights, lbs_terms_and_grad
    dev = gpu_device
    N, V = 1027, 97
    index, pred, gt = _terms_case(N, V, E, J)
    terms = LbsWeights(1.0, 1e4, 250.0)
    leaves = [t.double().requires_grad_(True) for t in pred]
    loss64 = R.lbs_terms(index, *leaves, *[t.double() for t in gt])
    grad64 = torch.autograd.grad((loss64 * torch.tensor(terms, dtype=torch.float64)).sum(), leaves)
    gen = torch.Generator().manual_seed(9)
    pre = [torch.randn(t.shape, generator=gen) * (wk * 2 * s / t.numel()) for t, wk, s in zip(pred, terms, _TERM_SIGMA)]
    bufs = [t.clone().to(dev) for t in pre]
    d_pred, d_gt = [t.to(dev) for t in pred], [t.to(dev) for t in gt]
    loss = lbs_terms_and_grad(index.to(dev), *d_pred, *d_gt, terms, *bufs)
    for k, name in enumerate(("weights", "posedirs", "shapedirs")):
        e = abs(float(loss[k]) - float(loss64[k].detach())) / float(loss64[k].detach())
        added = bufs[k].cpu().double() - pre[k].double()
        ge = _rel(added, grad64[k])
        print(f"E={E} J={J} {name}: loss {float(loss[k]):.9e} rel err {e:.3e}; added gradient rel-L2 {ge:.3e}; "
              f"|pre| / |grad| {float(pre[k].norm() / grad64[k].norm()):.2f}")
        assert e <= 1e-6, (name, e)
        assert ge <= 1e-6, (name, ge)
    # losses only, and a zero weight: bits unchanged
    again = [t.clone().to(dev) for t in pre]
    loss2 = lbs_terms_and_grad(index.to(dev), *d_pred, *d_gt, LbsWeights(1.0, 0.0, 250.0), again[0], again[1], again[2])
    assert torch.equal(loss2, loss)
    assert torch.equal(again[1].cpu().view(torch.int32), pre[1].view(torch.int32))
    assert torch.equal(again[0], bufs[0]) and torch.equal(again[2], bufs[2])
    loss3 = lbs_terms_and_grad(index.to(dev), *d_pred, *d_gt)
    assert torch.equal(loss3, loss)


def test_lbs_terms_without_points_launch_nothing(gpu_device):
    """N == 0: a caller's `out` keeps its content; without `out` the result is zeros, not uninitialised memory."""
    import torch
    from fateavatar_amd.mono import LbsWeights, lbs_terms_and_grad
    dev = gpu_device
    _, _, gt = _terms_case(4, 9, 7, 5)
    gt = [t.to(dev) for t in gt]
    empty = [torch.zeros((0, 5), device=dev), torch.zeros((0, 36, 3), device=dev), torch.zeros((0, 3, 7), device=dev)]
    index = torch.zeros((0,), dtype=torch.int32, device=dev)
    assert lbs_terms_and_grad(index, *empty, *gt, LbsWeights(1.0, 1.0, 1.0)).tolist() == [0.0, 0.0, 0.0]
    out = torch.tensor([1.0, 2.0, 3.0], device=dev)
    assert lbs_terms_and_grad(index, *empty, *gt, out=out) is out and out.tolist() == [1.0, 2.0, 3.0]


def test_lbs_terms_on_three_streams_do_not_mix(gpu_device):
    """Three launches in flight on three streams, each with a workspace of its own, give what each gives alone."""
    import torch
    from fateavatar_amd.mono import LbsWeights, lbs_terms_and_grad, lbs_terms_workspace
    dev = gpu_device
    N, V, E, J = 4099, 97, 50, 6
    terms = LbsWeights(0.5, 2.0, 3.0)
    cases = []
    for seed in (1, 2, 3):
        index, pred, gt = _terms_case(N, V, E, J, seed=seed)
        cases.append((index.to(dev), [t.to(dev) for t in pred], [t.to(dev) for t in gt]))

    def run(case, ws):
        index, pred, gt = case
        bufs = [torch.zeros_like(t) for t in pred]
        out = torch.empty(3, device=dev)
        lbs_terms_and_grad(index, *pred, *gt, terms, *bufs, out=out, workspace=ws)
        return out, bufs

    alone = [run(c, lbs_terms_workspace(dev)) for c in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in cases]
    spaces = [lbs_terms_workspace(dev) for _ in cases]
    torch.cuda.synchronize()
    together = []
    for _ in range(3):                      # (a workspace is left zeroed: it serves again)
        together = []
        for c, s, ws in zip(cases, streams, spaces):
            with torch.cuda.stream(s):
                together.append(run(c, ws))
    torch.cuda.synchronize()
    assert len({float(a[0][2]) for a in alone}) == 3
    for (la, ga), (lt, gt_) in zip(alone, together):
        assert torch.equal(la, lt)
        for a, b in zip(ga, gt_):
            assert torch.equal(a, b)
    for ws in spaces:
        assert int(ws.count_nonzero()) == 0


def test_image_loss_gradient_through_the_chain_matches_the_restatement(gpu_device):
    """dL1/d(points, shapedirs, posedirs, lbs_weights) through deform_points -> splat_attributes -> render_points at 64x64 with
    N = 2048, against the same chain with the restatement on the same device: rel-L2 <= 2e-4."""
    import numpy as np
    import torch
    from fateavatar_amd import scenes
    from fateavatar_amd.model import TorchCamera
    from fateavatar_amd.mono import PoseState, deform_points, render_points, splat_attributes
    dev = gpu_device
    N, E, J = 2048, 50, 6
    s = scenes.head_scene(P=N, res=64, sh_degree=0, seed=0)
    cam = TorchCamera(s.camera, dev)
    bg = torch.zeros(3, device=dev)
    gen = torch.Generator().manual_seed(0)
    rn = lambda *sh: torch.randn(sh, generator=gen)  # noqa: E731
    points = torch.from_numpy(np.asarray(s.means3D, np.float32))
    centre = points.mean(0).double()

    def bones(angle):                       # rigid motions about the head's centre; bone 0 the identity
        A = R.rigid_bones(J, angle, gen)
        A[:, :3, 3] = 0.05 * A[:, :3, 3] + centre - A[:, :3, :3] @ centre
        A[0] = torch.eye(4, dtype=torch.float64)
        return A.float()

    x = [points, 0.002 * rn(N, 3, E), 0.002 * rn(N, 36, 3), torch.softmax(2 * rn(N, J), 1)]
    c = PoseState(rn(E), 0.3 * rn(36), bones(0.05))
    f = PoseState(rn(E), 0.3 * rn(36), bones(0.15))
    feats, offs, target = rn(N, 11), 0.1 * rn(N, 11), torch.rand((3, 64, 64), generator=gen)
    x, feats, offs, target = [t.to(dev) for t in x], feats.to(dev), offs.to(dev), target.to(dev)
    c, f = PoseState(*[t.to(dev) for t in c]), PoseState(*[t.to(dev) for t in f])

    def run(op):
        leaves = [t.detach().clone().requires_grad_(True) for t in x]
        xyz = op(*leaves, c, f)
        rgb, opacity, scales, rotations = splat_attributes(feats, offs, radius=0.002, scene_scale=4.0)
        image, radii = render_points(cam, xyz, rgb, opacity, scales, rotations, bg)
        loss = (image - target).abs().mean()
        return image.detach(), radii, torch.autograd.grad(loss, leaves)

    img_a, radii, got = run(deform_points)
    img_b, _, want = run(R.deform_points)
    assert int((radii > 0).sum()) > N // 2 and float(img_a.max()) > 0.05
    assert float((img_a - img_b).abs().max()) < 1e-3
    for name, a, b in zip(NAMES, got, want):
        assert bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0, name
        e = _rel(a, b)
        print(f"end to end, gradient {name}: rel-L2 {e:.3e}")
        assert e <= 2e-4, (name, e)
