"""GPU: the gradients of MonoGaussianAvatar's point deformation to the frame's pose state (deform_points(frame_grad=True) over
k_point_lbs_pose_bwd, csrc/fr_point_lbs.hip) against the plain-torch restatement (tests/mono_ref.py) with autograd."""
import functools

import pytest

from tests import mono_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("betas", "pose_feature", "transforms")
POINT_NAMES = ("points", "shapedirs", "posedirs", "lbs_weights")
POSE_GRID_CAP = 256 * 64     # points one sweep of k_point_lbs_pose_bwd covers: kPoseMaxBlocks x (kPoseThreads / kLbsGroup)
# the shapes of test_gpu_mono.py's DEFORM_CASES with this kernel's cap: below it at the two everyday shapes; one exactly full
# sweep, one point in a second sweep and a partial third sweep; the declared limits and an E on either side of the stride
POSE_CASES = [(N, E, J) for E, J in ((50, 6), (7, 5)) for N in (1, 63, 65, 4099)] \
    + [(POSE_GRID_CAP, 50, 6), (POSE_GRID_CAP + 1, 50, 6), (2 * POSE_GRID_CAP + 17, 50, 6)] \
    + [(4099, 1, 1), (4099, 15, 8), (4099, 16, 1), (4099, 17, 8), (4099, 64, 8)]
ELEMENT_FACTOR = 16          # test_gpu_mono.py's ROW_FACTOR and its rule, per element of a summed gradient


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _element_metric(got, ref64):
    """m_k = |got_k - ref_k| / (|ref_k| + rms(ref)) per element k of a summed gradient."""
    a, r = got.double().reshape(-1), ref64.double().reshape(-1)
    return (a - r).abs() / (r.abs() + r.pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def _reference(N, E, J):
    """The recipe's inputs (rounded to float32 once) and, on the CPU, the float64 restatement's gradients to the frame state
    and the float32 restatement's error against them (rel-L2 and the worst element)."""
    import torch
    p, S, P, w, c, f, g = R.recipe(N, E, J)
    r32 = lambda t: t.float()  # noqa: E731
    x32, c32, f32, g32 = [r32(t) for t in (p, S, P, w)], tuple(map(r32, c)), tuple(map(r32, f)), r32(g)

    def run(dtype):
        frame = [t.to(dtype).clone().requires_grad_(True) for t in f32]      # (a copy: `to` hands float32 back as it is)
        xyz = R.deform_points(*[t.to(dtype) for t in x32], tuple(t.to(dtype) for t in c32), tuple(frame))
        return torch.autograd.grad(xyz, frame, g32.to(dtype))

    grad64, grad32 = run(torch.float64), run(torch.float32)
    err32 = ([_rel(a, b) for a, b in zip(grad32, grad64)], [float(_element_metric(a, b).max()) for a, b in zip(grad32, grad64)])
    return x32, c32, f32, g32, grad64, err32


def _on(dev, x32, c32, f32, g32):
    from fateavatar_amd.mono import PoseState
    return [t.to(dev) for t in x32], PoseState(*[t.to(dev) for t in c32]), PoseState(*[t.to(dev) for t in f32]), g32.to(dev)


def _pose_grads(x, c, f, g, which=(0, 1, 2), points_too=False, workspace=None, flat=False):
    """deform_points(frame_grad=True) and its backward: (xyz, gradients of the frame state's entries `which`[, the four
    per-point gradients])."""
    import torch
    from fateavatar_amd.mono import PoseState, deform_points
    frame = [t.detach().clone() for t in f]
    if flat:
        frame[2] = frame[2].reshape(-1, 16)
    frame = [t.requires_grad_(k in which) for k, t in enumerate(frame)]
    leaves = [t.detach().clone().requires_grad_(points_too) for t in x]
    xyz = deform_points(*leaves, c, PoseState(*frame), frame_grad=True, workspace=workspace)
    grads = torch.autograd.grad(xyz, [frame[k] for k in which] + (leaves if points_too else []), g)
    return xyz.detach(), grads[:len(which)], grads[len(which):]


@pytest.mark.parametrize("N,E,J", POSE_CASES)
def test_pose_gradients_match_the_float64_restatement(gpu_device, N, E, J):
    """Each of the three gradients within rel-L2 2e-4 of float64 autograd through the restatement (the sibling ops' gross
    bound), and every ELEMENT held as well: the maximum of m_k = |got_k - ref_k| / (|ref_k| + rms(ref)) is at most
    ELEMENT_FACTOR = 16 times the maximum the float32 plain-torch restatement reaches against float64 on the same inputs,
    computed on the CPU and never from the kernel (test_gpu_mono.py's ROW_FACTOR and its rule: below N = 4 099 a maximum over
    a handful of summands is no yardstick, so the shape's N = 4 099 value is used).  That yardstick is asserted to lie in
    (0, 2e-5]; it depends on the order in which the host's torch sums (threads, vector width): 1.4e-6 / 6.7e-7 / 6.5e-7 (betas,
    pose_feature, transforms) at (4 099, 50, 6) on one host, 2.6e-6 / 3.0e-6 / 1.2e-6 on another.  The last row of every
    bone's gradient is exactly 0.  Achieved ratios (MI355X): profiles/r19_mono_pose.md."""
    import torch
    x32, c32, f32, g32, grad64, err32 = _reference(N, E, J)
    elem32 = err32[1] if N >= 4099 else _reference(4099, E, J)[5][1]
    x, c, f, g = _on(gpu_device, x32, c32, f32, g32)
    _, grads, _ = _pose_grads(x, c, f, g)
    for name, gg, like, r, e32, m32 in zip(NAMES, grads, f32, grad64, err32[0], elem32):
        gg = gg.cpu()
        assert gg.shape == like.shape == r.shape and bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0 \
            and float(r.abs().max()) > 0, name
        e = _rel(gg, r)
        m = _element_metric(gg, r)
        worst = int(m.argmax())
        print(f"N={N} E={E} J={J} gradient {name}: rel-L2 {e:.3e} (float32 restatement {e32:.3e}, ratio {e / max(e32, 1e-30):.2f}); "
              f"worst element {worst}: {float(m[worst]):.3e} (float32 restatement's worst {m32:.3e}, ratio "
              f"{float(m[worst]) / max(m32, 1e-30):.2f} of the {ELEMENT_FACTOR} allowed)")
        assert e <= 2e-4, (name, e)
        assert 0 < m32 <= 2e-5, (name, m32)
        assert float(m[worst]) <= ELEMENT_FACTOR * m32, (name, worst, float(m[worst]), m32)
    assert bool((grads[2][:, 3, :] == 0).all())


@pytest.mark.parametrize("N", [4099, 2 * POSE_GRID_CAP + 17])
def test_each_pose_gradient_alone_is_the_full_call_and_the_point_gradients_keep_their_bits(gpu_device, N):
    """A pose gradient requested alone (the other output pointers NULL) has the bits of the full call, [J,16] transforms get the
    [J,4,4] gradient's bits in their own shape, a second run repeats them, the workspace is all zero after every launch, and
    xyz and the four per-point gradients are those of the call without frame_grad."""
    import torch
    from fateavatar_amd.mono import deform_points, pose_workspace
    E, J = 50, 6
    x32, c32, f32, g32, *_ = _reference(N, E, J)
    x, c, f, g = _on(gpu_device, x32, c32, f32, g32)
    ws = pose_workspace(gpu_device)
    xyz, full, points = _pose_grads(x, c, f, g, points_too=True, workspace=ws)
    torch.cuda.synchronize()
    assert int(ws.count_nonzero()) == 0
    xyz2, again, points2 = _pose_grads(x, c, f, g, points_too=True, workspace=ws)
    torch.cuda.synchronize()
    assert int(ws.count_nonzero()) == 0 and torch.equal(xyz, xyz2)
    for name, a, b in zip(NAMES + POINT_NAMES, full + points, again + points2):
        assert torch.equal(a, b), name
    for k, name in enumerate(NAMES):
        xyz1, (alone,), _ = _pose_grads(x, c, f, g, which=(k,), workspace=ws)
        assert torch.equal(xyz1, xyz) and torch.equal(alone, full[k]), name
    _, (flat,), _ = _pose_grads(x, c, f, g, which=(2,), workspace=ws, flat=True)
    assert flat.shape == (J, 16) and torch.equal(flat.reshape(J, 4, 4), full[2])
    _, default_ws, _ = _pose_grads(x, c, f, g)                         # the workspace kept for the stream
    for name, a, b in zip(NAMES, full, default_ws):
        assert torch.equal(a, b), name
    torch.cuda.synchronize()
    assert int(ws.count_nonzero()) == 0
    # without frame_grad: the forward and the four per-point gradients, bit for bit
    leaves = [t.detach().clone().requires_grad_(True) for t in x]
    plain = deform_points(*leaves, c, f)
    assert torch.equal(plain.detach(), xyz)
    for name, a, b in zip(POINT_NAMES, torch.autograd.grad(plain, leaves, g), points):
        assert torch.equal(a, b), name


def test_no_points_give_zero_pose_gradients(gpu_device):
    import torch
    x32, c32, f32, _, *_ = _reference(1, 7, 5)
    x, c, f, _ = _on(gpu_device, x32, c32, f32, torch.zeros(1, 3))
    x = [t[:0] for t in x]
    xyz, grads, _ = _pose_grads(x, c, f, torch.zeros((0, 3), device=gpu_device))
    assert xyz.shape == (0, 3)
    for name, gg, like in zip(NAMES, grads, f):
        assert gg.shape == like.shape and int(gg.count_nonzero()) == 0, name


def test_graph_replay_with_new_pose_states_gives_the_eager_pose_gradients(gpu_device):
    """Forward + backward with pose gradients captured once; new pose states are copied into the static buffers between
    replays, and each replay equals the eager result (test_graph_replay_with_new_pose_states_is_the_eager_result's manner)."""
    import torch
    from fateavatar_amd.mono import PoseState, deform_points, pose_workspace
    dev = gpu_device
    N, E, J = 4099, 50, 6
    x32, c32, f32, g32, *_ = _reference(N, E, J)
    x, c, f, g = _on(dev, x32, c32, f32, g32)
    poses = [(c, f)]
    for seed in (5, 6):
        _, _, _, _, c2, f2, _ = R.recipe(1, E, J, seed=seed)
        poses.append((PoseState(*[t.float().to(dev) for t in c2]), PoseState(*[t.float().to(dev) for t in f2])))

    def eager(c, f):
        xyz, grads, points = _pose_grads(x, c, f, g, points_too=True)
        return [xyz.clone()] + [t.clone() for t in grads + points]

    want = [eager(*p) for p in poses]
    assert not torch.equal(want[0][1], want[1][1])
    sc = PoseState(*[t.clone() for t in c])
    sf = [t.clone().requires_grad_(True) for t in f]
    leaves = [t.detach().clone().requires_grad_(True) for t in x]
    ws = pose_workspace(dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xyz = deform_points(*leaves, sc, PoseState(*sf), frame_grad=True, workspace=ws)
        grads = torch.autograd.grad(xyz, sf + leaves, g)
    for (pc, pf), w in list(zip(poses, want))[::-1] + [(poses[1], want[1])]:
        with torch.no_grad():
            for dst, src in zip(tuple(sc) + tuple(sf), tuple(pc) + tuple(pf)):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("xyz",) + NAMES + POINT_NAMES, [xyz, *grads], w):
            assert torch.equal(a, b), name
        assert int(ws.count_nonzero()) == 0


def test_pose_gradients_on_three_streams_do_not_mix(gpu_device):
    """Three backward launches in flight on three streams, each with a workspace of its own, give what each gives alone."""
    import torch
    from fateavatar_amd.mono import PoseState, pose_workspace
    dev = gpu_device
    N, E, J = 4099, 50, 6
    cases = []
    for seed in (1, 2, 3):
        p, S, P, w, c, f, g = R.recipe(N, E, J, seed=seed)
        cases.append(([t.float().to(dev) for t in (p, S, P, w)], PoseState(*[t.float().to(dev) for t in c]),
                      PoseState(*[t.float().to(dev) for t in f]), g.float().to(dev)))
    alone = [_pose_grads(*case, workspace=pose_workspace(dev))[1] for case in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in cases]
    spaces = [pose_workspace(dev) for _ in cases]
    torch.cuda.synchronize()
    together = []
    for _ in range(3):                      # (a workspace is left zeroed: it serves again)
        together = []
        for case, s, ws in zip(cases, streams, spaces):
            with torch.cuda.stream(s):
                together.append(_pose_grads(*case, workspace=ws)[1])
    torch.cuda.synchronize()
    assert len({float(a[0][0]) for a in alone}) == 3
    for a, t in zip(alone, together):
        for name, u, v in zip(NAMES, a, t):
            assert torch.equal(u, v), name
    for ws in spaces:
        assert int(ws.count_nonzero()) == 0


def test_image_loss_gradient_to_the_frame_state_through_the_chain_matches_the_restatement(gpu_device):
    """dL1/d(frame betas, pose_feature, transforms) through deform_points -> splat_attributes -> render_points at 64x64 with
    N = 2048, against the same chain with the restatement on the same device: rel-L2 <= 2e-4 (the existing chain test's bound
    and scene, test_image_loss_gradient_through_the_chain_matches_the_restatement)."""
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
        frame = [t.detach().clone().requires_grad_(True) for t in f]
        xyz = op(*x, c, PoseState(*frame))
        rgb, opacity, scales, rotations = splat_attributes(feats, offs, radius=0.002, scene_scale=4.0)
        image, radii = render_points(cam, xyz, rgb, opacity, scales, rotations, bg)
        loss = (image - target).abs().mean()
        return image.detach(), radii, torch.autograd.grad(loss, frame)

    img_a, radii, got = run(lambda *a: deform_points(*a, frame_grad=True))
    img_b, _, want = run(R.deform_points)
    assert int((radii > 0).sum()) > N // 2 and float(img_a.max()) > 0.05
    assert float((img_a - img_b).abs().max()) < 1e-3
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0, name
        e = _rel(a, b)
        print(f"end to end, gradient {name}: rel-L2 {e:.3e}")
        assert e <= 2e-4, (name, e)
