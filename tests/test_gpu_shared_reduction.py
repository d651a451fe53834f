"""A launch's sums across its workgroups have ONE protocol in two helpers (csrc/fr_common.hpp): per-workgroup partials, added up
by the workgroup that finishes last, which leaves the workspace as it found it.  sum_over_workgroups adds a few scalars (every
fused loss kernel ends with it), sum_rows_over_workgroups a whole row of sums (FLAME's three reducing kernels, the point
deformation's backward to the frame's pose).  Every user of either is run here at the workgroup counts where that tail changes
its path: 1, 15, 16 and 17 (last_workgroup_of's counter groups fill up at 16; the pose backward's fifteen runs of rows go from
one row each to two, with empty trailing runs), the op's grid cap (1024: four partials per thread of the scalar helper's last
workgroup; 256 for the row helper's users) and one past it (the grid stays at the cap and sweeps twice).  Everything asserted is
exact: equal bits from launch to launch and from a fresh workspace, and a zero workspace afterwards.  The values against
float64 are held by the ops' own tests."""
import pytest

pytestmark = pytest.mark.gpu

CAP = 1024                      # kL1MaxBlocks = kRegMaxBlocks = kMeshMaxBlocks = kTermsMaxBlocks
COUNTS = (1, 15, 16, 17, CAP, CAP + 1)
ROW_CAP = 256                   # kFlMaxBlocks = kPoseMaxBlocks: the grid cap of sum_rows_over_workgroups' users
ROW_COUNTS = (1, 15, 16, 17, ROW_CAP, ROW_CAP + 1)
COUNTER_BYTES = 17 * 128        # (kDoneGroups + 1) counters, one 128-byte line each
# [C,H,W] -> C x ceil(H / 32) x ceil(W / 32) workgroups; the image loss has no cap
IMAGE_SHAPES = {1: (1, 32, 32), 15: (3, 32, 160), 16: (1, 128, 128), 17: (1, 32, 544)}


def _rand(gen, *shape):
    import torch
    return torch.rand(*shape, generator=gen, dtype=torch.float32)


def _l1(b, dev, gen):
    from fateavatar_amd.loss import l1_loss_and_grad, l1_workspace
    n = 1024 * b + 3
    x, y = _rand(gen, n).to(dev), _rand(gen, n).to(dev)
    return (lambda ws: list(l1_loss_and_grad(x, y, workspace=ws))), (lambda: l1_workspace(dev))


def _l1_batch(b, dev, gen):
    """Two images in one launch (grid (b, 2)), a workspace each: both are checked."""
    import torch
    from fateavatar_amd.loss import l1_loss_and_grad_batch, l1_workspace
    n = 1024 * b + 3
    xs, ys = [_rand(gen, n).to(dev) for _ in range(2)], [_rand(gen, n).to(dev) for _ in range(2)]

    def run(wss):
        losses, grads = [torch.empty((), dtype=torch.float32, device=dev) for _ in xs], [torch.empty_like(x) for x in xs]
        l1_loss_and_grad_batch(xs, ys, losses, grads, list(wss))
        return losses + grads
    return run, (lambda: (l1_workspace(dev), l1_workspace(dev)))


def _l1_terms(b, dev, gen):
    """fr_image_loss_grad with a D-SSIM weight of 0: the L1 kernel's instance that zeroes its partials.  1024 b + 2 floats as
    two rows (the entry point takes rows of up to 2^20 pixels): b workgroups and a tail of two."""
    from fateavatar_amd.loss import image_loss_and_grad, image_loss_workspace
    shape = (1, 2, 512 * b + 1)
    x, y = _rand(gen, *shape).to(dev), _rand(gen, *shape).to(dev)
    return (lambda ws: list(image_loss_and_grad(x, y, (0.8, 0.0), workspace=ws))), (lambda: image_loss_workspace(dev, *shape))


def _huber(b, dev, gen):
    from fateavatar_amd.loss import huber_loss_and_grad, huber_workspace
    n = 1024 * b + 3
    x, y, m = _rand(gen, 1, 1, n).to(dev), _rand(gen, 1, 1, n).to(dev), _rand(gen, 1, n).to(dev)
    return (lambda ws: list(huber_loss_and_grad(x, y, mask=m, workspace=ws))), (lambda: huber_workspace(dev))


def _pixel(b, dev, gen):
    from fateavatar_amd.loss import pixel_loss_and_grad, pixel_loss_workspace
    n = 1024 * b + 3
    x, y = _rand(gen, 1, 1, n).to(dev), _rand(gen, 1, 1, n).to(dev)
    return (lambda ws: list(pixel_loss_and_grad(x, y, workspace=ws))), (lambda: pixel_loss_workspace(dev))


def _scale_term(b, dev, gen):
    """The reference's gates on rows drawn around them (tests/splatting_loss_ref.py): in float64, here on the CPU, rows lie on
    both sides of both gates and the selection is neither empty nor everything, so the loss word is a sum of positive terms."""
    import torch
    from fateavatar_amd.loss import ScaleTerm, scale_term_and_grad, scale_term_workspace
    from tests import splatting_loss_ref as R
    P = 256 * b
    ref = R.REFERENCE
    cpu = R.draw_scaling(P, gen)
    scale = torch.exp(cpu.double())
    smax, smin = scale.max(dim=1).values, scale.min(dim=1).values
    for gate in (smax > ref["max_scaling"], smax / smin > ref["scale_threshold"]):
        assert bool(gate.any()) and not bool(gate.all())
    count = R.scale_term(cpu, ref["scale_weight"], ref["scale_threshold"], ref["max_scaling"])[1]
    assert 0 < count < P, count
    scaling = cpu.to(dev)

    def run(ws):
        d = torch.zeros_like(scaling)
        terms = ScaleTerm(ref["scale_weight"], ref["scale_threshold"], ref["max_scaling"])
        return [scale_term_and_grad(scaling, d, terms=terms, workspace=ws).clone(), d]
    return run, (lambda: scale_term_workspace(dev))


def _regulariser(b, dev, gen):
    import torch
    from fateavatar_amd.loss import gaussian_regularisers, regulariser_workspace
    P = 256 * b
    scaling, xyz = (_rand(gen, P, 3) - 0.7).to(dev), (2.0 * _rand(gen, P, 3)).to(dev)      # both sides of both thresholds

    def run(ws):
        d_s, d_x = torch.zeros_like(scaling), torch.zeros_like(xyz)
        return [gaussian_regularisers(scaling, xyz, d_s, d_x, workspace=ws).clone(), d_s, d_x]
    return run, (lambda: regulariser_workspace(dev))


def _mesh(b, dev, gen):
    import torch
    from fateavatar_amd.binding import mesh_laplacian
    from fateavatar_amd.loss import MeshTerms, mesh_terms_and_grad, mesh_terms_workspace
    V = 32 * b
    i = torch.arange(V)
    lap = mesh_laplacian(torch.stack([i, (i + 1) % V, (i + 2) % V], dim=1).to(dev), V)     # a closed ring: neighbours i +- 1, i +- 2
    verts, orig = _rand(gen, V, 3).to(dev), _rand(gen, V, 3).to(dev)

    def run(ws):
        d = torch.zeros_like(verts)
        return [mesh_terms_and_grad(verts, orig, lap, MeshTerms(1e3, 0.3), d_verts=d, workspace=ws).clone(), d]
    return run, (lambda: mesh_terms_workspace(dev))


def _lbs(b, dev, gen):
    import torch
    from fateavatar_amd.mono import LbsWeights, lbs_terms_and_grad, lbs_terms_workspace
    N, V, E, J = 16 * b, 5, 1, 1
    index = torch.randint(0, V, (N,), generator=gen, dtype=torch.int32).to(dev)
    pred = [_rand(gen, N, J).to(dev), _rand(gen, N, 36, 3).to(dev), _rand(gen, N, 3, E).to(dev)]
    gt = [_rand(gen, V, J).to(dev), _rand(gen, V, 36, 3).to(dev), _rand(gen, V, 3, E).to(dev)]

    def run(ws):
        bufs = [torch.zeros_like(t) for t in pred]
        return [lbs_terms_and_grad(index, *pred, *gt, LbsWeights(0.5, 2.0, 3.0), *bufs, workspace=ws).clone()] + bufs
    return run, (lambda: lbs_terms_workspace(dev))


def _image(b, dev, gen):
    from fateavatar_amd.loss import image_loss_and_grad, image_loss_workspace
    shape = IMAGE_SHAPES[b]
    x, y = _rand(gen, *shape).to(dev), _rand(gen, *shape).to(dev)
    return (lambda ws: list(image_loss_and_grad(x, y, (0.8, 0.2), workspace=ws))), (lambda: image_loss_workspace(dev, *shape))


def _mono_pose(b, dev, gen):
    """deform_points' backward to the frame's pose state: a workgroup of 1024 threads takes 64 points, a row is 272 sums."""
    import torch
    from fateavatar_amd.mono import PoseState, deform_points, pose_workspace
    from tests import mono_ref
    p, S, P, w, c, f, g = mono_ref.recipe(64 * b, 3, 2, seed=int(gen.initial_seed()))
    x = [t.float().to(dev).contiguous() for t in (p, S, P, w)]
    c, f, g = PoseState(*(t.float().to(dev) for t in c)), [t.float().to(dev) for t in f], g.float().to(dev)

    def run(ws):
        frame = [t.clone().requires_grad_(True) for t in f]
        xyz = deform_points(*x, c, PoseState(*frame), frame_grad=True, workspace=ws)
        return list(torch.autograd.grad(xyz, frame, g))                  # d_betas, d_pose_feature, d_transforms
    return run, (lambda: pose_workspace(dev))


class _FlameWorkspace:
    """A FlameMesh owns its workspace: a fresh one is a fresh mesh over the same tables."""

    def __init__(self, make):
        self.fm = make()
        self.zeroed = self.fm.workspace_zeroed_part()
        assert self.zeroed.numel() == COUNTER_BYTES + 4 * ROW_CAP * 128       # (the promise covers all of it)


def _flame(b, dev, gen):
    """FLAME forward and backward on two meshes, a workspace each: V = 16 b (the two sixteen-lanes-per-vertex kernels run b
    workgroups) and V = 64 b (the two 64-vertices-per-workgroup kernels do).  Rows of 32, 128 and 128 sums."""
    import torch
    from fateavatar_amd.flame import synthetic_flame
    cases = []
    for V in (16 * b, 64 * b):
        template = _rand(gen, V, 3).numpy()
        deltas = 1e-3 * (_rand(gen, V * 3 * 3 + 36 * 3 * V + 3 * V) - 0.5)
        e, p, g = (_rand(gen, 3) - 0.5).to(dev), (0.2 * (_rand(gen, 15) - 0.5)).to(dev), (_rand(gen, V, 3) - 0.5).to(dev)

        def make(template=template, deltas=deltas):
            fm = synthetic_flame(template, seed=1, n_shape=1, n_exp=3, device=dev)
            with torch.no_grad():
                fm.flat.copy_(deltas)
            return fm
        cases.append((make, e, p, g))

    def run(wss):
        outs = []
        for (_, e, p, g), ws in zip(cases, wss):
            fm = ws.fm
            verts, orig = torch.empty_like(g), torch.empty_like(g)
            phi, A = torch.empty(36, device=dev), torch.empty(5, 4, 4, device=dev)
            d_e, d_p = torch.empty_like(e), torch.empty_like(p)
            fm.forward_into(e, p, verts, orig, phi, A)
            fm.backward_from(g, e, p, d_e, d_p)
            outs += [verts, orig, phi, A, fm.flat_grad, d_e, d_p]
        return outs
    return run, (lambda: tuple(_FlameWorkspace(make) for make, *_ in cases))


# op -> (case builder, partial floats the kernel promises to leave zeroed (None: no promise), the counts it is run at)
OPS = {"l1": (_l1, None, COUNTS), "l1_batch": (_l1_batch, None, COUNTS), "l1_terms": (_l1_terms, CAP, COUNTS),
       "huber": (_huber, 2 * CAP, COUNTS), "pixel": (_pixel, 2 * CAP, COUNTS), "scale_term": (_scale_term, 2 * CAP, COUNTS),
       "regulariser": (_regulariser, 2 * CAP, COUNTS), "mesh": (_mesh, 2 * CAP, COUNTS), "lbs": (_lbs, 3 * CAP, COUNTS),
       "image": (_image, 0, tuple(IMAGE_SHAPES)), "mono_pose": (_mono_pose, ROW_CAP * 272, ROW_COUNTS),
       "flame": (_flame, ROW_CAP * 128, ROW_COUNTS)}
CASES = [(op, b) for op, (_, _, counts) in OPS.items() for b in counts]


@pytest.mark.parametrize("op,b", CASES, ids=[f"{op}-{b}" for op, b in CASES])
def test_same_bits_on_every_launch_and_the_workspace_left_zeroed(gpu_device, op, b):
    import torch
    dev = gpu_device
    build, partial_floats, _ = OPS[op]
    run, fresh = build(b, dev, torch.Generator().manual_seed(1000 + b))
    if op == "image":
        partial_floats = 2 * b

    def launch(ws):
        outs = run(ws)
        torch.cuda.synchronize()
        for w in (ws if isinstance(ws, tuple) else (ws,)):     # (l1_batch: one workspace per image; flame: one per mesh)
            w = w.zeroed if isinstance(w, _FlameWorkspace) else w
            assert int(w[:COUNTER_BYTES].count_nonzero()) == 0, "counters"
            if partial_floats is not None:
                assert int(w[COUNTER_BYTES:COUNTER_BYTES + 4 * partial_floats].count_nonzero()) == 0, "partials"
        return [o.clone() for o in outs]

    ws = fresh()
    first, second, other = launch(ws), launch(ws), launch(fresh())
    assert float(first[0].abs().max()) > 0                     # (the sums saw data)
    for a, s, o in zip(first, second, other):
        assert torch.equal(a.view(torch.int32), s.view(torch.int32)) and torch.equal(a.view(torch.int32), o.view(torch.int32))
