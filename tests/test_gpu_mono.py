"""GPU: MonoGaussianAvatar's fused per-point calls (fateavatar_amd/mono.py over csrc/fr_point_lbs.hip) against the plain-torch
restatement (tests/mono_ref.py)."""
import functools

import pytest

from tests import mono_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(50, 6), (7, 5)]
NAMES = ("points", "shapedirs", "posedirs", "lbs_weights")
LBS_GRID_CAP = 2048 * 16     # points one sweep of k_point_lbs_fwd / _bwd covers: kLbsMaxBlocks x (kLbsThreads / kLbsGroup), fr_point_lbs.hip
TERMS_GRID_CAP = 1024 * 16   # points one sweep of k_lbs_terms covers: kTermsMaxBlocks x (kLbsThreads / kLbsGroup)
NV_CHUNK, NV_MAX_V = 4096, 8192   # vertices k_nearest_vertex holds in LDS at a time (kNvChunk) and FR_NEAREST_MAX_V
# the shapes of test_deform_points_matches_the_float64_restatement: the sizes below the cap at the two everyday shapes; one
# exactly full sweep, one point in a second sweep and a partial third sweep; the declared limits (E = 64, J = 8, E = 1, J = 1)
# and an E on either side of the sixteen-lane stride
DEFORM_CASES = [(N, E, J) for E, J in SHAPES for N in (1, 63, 65, 4099)] \
    + [(LBS_GRID_CAP, 50, 6), (LBS_GRID_CAP + 1, 50, 6), (2 * LBS_GRID_CAP + 17, 50, 6), (LBS_GRID_CAP + 1, 64, 8)] \
    + [(4099, 1, 1), (4099, 15, 8), (4099, 16, 1), (4099, 17, 8), (4099, 64, 8)]
ROW_FACTOR = 16              # a row of a gradient may miss float64 by this many times the float32 restatement's own worst row


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _row_metric(got, ref64):
    """m_i = |got_i - ref_i| / (|ref_i| + s) per point i (a row = everything the array holds for the point), s the RMS row norm
    of the float64 gradient: one wrong row shows at its full size, and a row whose gradient happens to be small is not held
    to more than the array's typical row allows."""
    a, r = got.reshape(got.shape[0], -1).double(), ref64.reshape(ref64.shape[0], -1).double()
    n = r.norm(dim=1)
    return (a - r).norm(dim=1) / (n + n.pow(2).mean().sqrt())


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
    err32 = (float((xyz32.double() - xyz64).abs().max()), [_rel(a, b) for a, b in zip(grad32, grad64)],
             [float(_row_metric(a, b).max()) for a, b in zip(grad32, grad64)])
    return x32, c32, f32, g32, xyz64, grad64, err32


def _on(dev, x32, c32, f32, g32):
    from fateavatar_amd.mono import PoseState
    return [t.to(dev) for t in x32], PoseState(*[t.to(dev) for t in c32]), PoseState(*[t.to(dev) for t in f32]), g32.to(dev)


@pytest.mark.parametrize("N,E,J", DEFORM_CASES)
def test_deform_points_matches_the_float64_restatement(gpu_device, N, E, J):
    """Forward within 1e-5 + 1e-5 |ref| and each gradient within rel-L2 2e-4 of the float64 restatement (the sibling ops' bounds,
    test_deform_op_matches_the_torch_restatement): about 50x and 1000x the float32 restatement's own error on this recipe.
    Over a whole array that lets single rows be wrong (at N = 4 099 one row may be off by over 1 %), and the rows most likely
    to be wrong are single ones: the last row of a partly dead wave, the first row of a second sweep.  So every ROW is held to
    float64 as well, by `_row_metric`: its maximum is at most ROW_FACTOR = 16 times the maximum the float32 plain-torch
    restatement (tests/mono_ref.py, autograd) reaches against float64 on the same inputs, computed on the CPU — never from the
    kernel.  That yardstick is 2.2e-7, 1.3e-7, 1.4e-7, 5.8e-7 (points, shapedirs, posedirs, lbs_weights) at (65 553, 50, 6), the
    same within 20 % at (32 769, 64, 8) and (4 099, 17, 8), and the float32 transcription of the kernels' closed forms lies
    within 1.2x of it: the factor is room for another order of the same float32 sums and nothing more.  A maximum over a few
    rows is no yardstick (it can be 0: a one-hot row of bone 0 is exact), so below N = 4 099 the shape's N = 4 099 value is
    used; it is asserted to be <= 2e-6 (if a new shape breaks that, the inputs change, not the factor).
    Achieved ratios (MI355X): profiles/r18_grid_caps.md."""
    import torch
    from fateavatar_amd.mono import deform_points
    x32, c32, f32, g32, xyz64, grad64, err32 = _reference(N, E, J)
    row32 = err32[2] if N >= 4099 else _reference(4099, E, J)[6][2]
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
    for name, gg, r, e32, m32 in zip(NAMES, grads, grad64, err32[1], row32):
        gg = gg.cpu()
        assert gg.shape == r.shape and bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0 and float(r.abs().max()) > 0, name
        e = _rel(gg, r)
        m = _row_metric(gg, r)
        worst = int(m.argmax())
        print(f"N={N} E={E} J={J} gradient {name}: rel-L2 {e:.3e} (float32 restatement {e32:.3e}, ratio {e / max(e32, 1e-30):.2f}); "
              f"worst row {worst}: {float(m[worst]):.3e} (float32 restatement's worst {m32:.3e}, ratio {float(m[worst]) / m32:.2f} "
              f"of the {ROW_FACTOR} allowed)")
        assert e <= 2e-4, (name, e)
        assert 0 < m32 <= 2e-6, (name, m32)
        assert float(m[worst]) <= ROW_FACTOR * m32, (name, worst, float(m[worst]), m32)


@pytest.mark.parametrize("N,E,J", [pytest.param(4099, 50, 6, id="50-6"), pytest.param(4099, 7, 5, id="7-5"),
                                   pytest.param(2 * LBS_GRID_CAP + 17, 50, 6, id="65553-50-6")])
def test_each_gradient_alone_is_the_full_call_and_two_runs_agree(gpu_device, N, E, J):
    """A backward with only one gradient requested (the other pointers NULL) writes the bits of the full call; a second full
    run writes the same bits again.  Below the grid's cap and with a partial third sweep."""
    import torch
    from fateavatar_amd.mono import deform_points
    x32, c32, f32, g32, *_ = _reference(N, E, J)
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


N_SPECIAL = 592             # rows of _grid_case that are placed by hand


@functools.lru_cache(maxsize=None)
def _grid_case(V, N=4099):
    """Vertices and points on the grid of multiples of 1/64 resp. 1/128 in [-1, 1]^3 (differences, squares and their sums are
    exact in float32, so equal distances are equal bits).  The last vertex duplicates vertex 0, and vertex NV_CHUNK (the first
    of the second chunk in LDS), where there is one, duplicates vertex 7 (at V = NV_CHUNK + 1 the two are one vertex: it
    duplicates 7).  Points 0 .. 511 sit exactly midway between two vertices, 512 .. 519 on vertex 0, 520 .. 527 on vertex 7 and
    528 .. 591, where the second chunk has that many, on vertices of the second chunk whose position no other vertex shares;
    the rest are random grid points.  N < 4099: rows 512 .. 512 + N of that cloud (the rows on the duplicated vertices first).
    -> (verts, points, second-chunk vertices of rows 528 .. 591 or None)."""
    import torch
    gen = torch.Generator().manual_seed(V)
    verts = torch.randint(-64, 65, (V, 3), generator=gen).float() / 64
    if V > 1:
        verts[V - 1] = verts[0]
    if V > NV_CHUNK:
        verts[NV_CHUNK] = verts[7]
    pts = torch.randint(-128, 129, (4099, 3), generator=gen).float() / 128
    a, b = torch.randint(0, V, (512,), generator=gen), torch.randint(0, V, (512,), generator=gen)
    pts[:512] = (verts[a] + verts[b]) / 2
    pts[512:520] = verts[0]
    alone = None
    if V > NV_CHUNK:
        pts[520:528] = verts[7]
        key = ((verts[:, 0] * 64 + 64) * 129 + (verts[:, 1] * 64 + 64)) * 129 + (verts[:, 2] * 64 + 64)
        _, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
        single = torch.nonzero(counts[inverse][NV_CHUNK:] == 1).flatten() + NV_CHUNK
        if single.numel() >= 64:
            alone = single[torch.linspace(0, single.numel() - 1, 64).long()]      # spread over the chunk, its last vertices included
            pts[528:592] = verts[alone]
    return verts, (pts if N == 4099 else pts[512:512 + N].clone()), alone


@pytest.mark.parametrize("V", [1, 5, 5023, NV_CHUNK - 1, NV_CHUNK, NV_CHUNK + 1, NV_MAX_V - 1, NV_MAX_V])
def test_nearest_vertex_is_the_float32_restatement_exactly(gpu_device, V):
    """Index and squared distance are the restatement's bits, below, at and past one chunk of vertices in LDS and at the
    declared limit; a tie keeps the lowest index, across the chunk boundary too."""
    import torch
    from fateavatar_amd.mono import nearest_vertex
    verts, pts, alone = _grid_case(V)
    verts, pts = verts.to(gpu_device), pts.to(gpu_device)
    idx, d2 = nearest_vertex(pts, verts)
    ref_idx, ref_d2 = R.nearest_vertex(pts, verts)
    assert idx.dtype == torch.int32 and torch.equal(idx.long(), ref_idx)
    assert torch.equal(d2.view(torch.int32), ref_d2.view(torch.int32))
    if V > 1:
        # rows in which more than one vertex attains the minimum: the lowest of them was taken
        rows = torch.arange(0, N_SPECIAL, device=gpu_device)
        d = ((pts[rows, None, :] - verts[None]) ** 2)
        d = (d[..., 0] + d[..., 1]) + d[..., 2]
        attain = d == d.min(dim=1, keepdim=True).values
        tied = attain.sum(1) > 1
        assert int(tied.sum()) >= 8
        lowest = attain.to(torch.int8).argmax(dim=1)
        assert torch.equal(idx[rows][tied].long(), lowest[tied])
        assert bool((idx[512:520] == 0).all())                      # on the duplicated vertex: index 0, not V - 1
    if V > NV_CHUNK:
        assert bool(tied[520:528].all()) and bool((idx[520:528] == 7).all()) and bool((d2[520:528] == 0).all())   # 7, not NV_CHUNK
        # a tie between the two chunks among the midpoints as well
        both = attain[:512, :NV_CHUNK].any(1) & attain[:512, NV_CHUNK:].any(1)
        assert V < NV_MAX_V - 1 or int(both.sum()) >= 8
    assert (alone is not None) == (V > NV_CHUNK + 1)
    if alone is not None:
        assert int(alone.min()) > NV_CHUNK and int(alone.max()) >= V - 64
        assert torch.equal(idx[528:592].long().cpu(), alone) and bool((d2[528:592] == 0).all())
    # a general cloud, too (no grid)
    gen = torch.Generator().manual_seed(1)
    p2, v2 = torch.randn((777, 3), generator=gen).to(gpu_device), torch.randn((V, 3), generator=gen).to(gpu_device)
    i2, dd2 = nearest_vertex(p2, v2)
    r2, rd2 = R.nearest_vertex(p2, v2)
    assert torch.equal(i2.long(), r2) and torch.equal(dd2.view(torch.int32), rd2.view(torch.int32))


@pytest.mark.parametrize("V", [NV_CHUNK - 1, NV_CHUNK, NV_CHUNK + 1, NV_MAX_V - 1, NV_MAX_V])
@pytest.mark.parametrize("N", [1, 255, 257])
def test_nearest_vertex_with_part_workgroups_at_the_chunk_sizes(gpu_device, N, V):
    """One point, one lane short of a workgroup and one lane into a second one (dead lanes load chunks with the live ones):
    the restatement's bits, and the rows on the duplicated vertices keep the lower index."""
    import torch
    from fateavatar_amd.mono import nearest_vertex
    verts, pts, _ = _grid_case(V, N)
    verts, pts = verts.to(gpu_device), pts.to(gpu_device)
    assert pts.shape == (N, 3)
    idx, d2 = nearest_vertex(pts, verts)
    ref_idx, ref_d2 = R.nearest_vertex(pts, verts)
    assert torch.equal(idx.long(), ref_idx) and torch.equal(d2.view(torch.int32), ref_d2.view(torch.int32))
    assert bool((idx[:8] == 0).all()) and bool((d2[:8] == 0).all())              # vertex 0, not its duplicate V - 1
    if V > NV_CHUNK and N > 16:
        assert bool((idx[8:16] == 7).all()) and bool((d2[8:16] == 0).all())      # vertex 7, not its duplicate NV_CHUNK


@functools.lru_cache(maxsize=None)
def _terms_case(N, V, E, J, seed=0):
    import torch
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    # (J = 1: a softmax over one bone is the constant 1 and the term 0; a sigmoid keeps the weights in (0, 1) and apart)
    unit = (lambda t: torch.softmax(t, 1)) if J > 1 else torch.sigmoid
    index = torch.randint(0, V, (N,), generator=gen, dtype=torch.int32)
    index[0], index[1] = 0, V - 1
    gt = [unit(rn(V, J)), 0.01 * rn(V, 36, 3), 0.01 * rn(V, 3, E)]
    pred = [unit(rn(N, J)), 0.01 * rn(N, 36, 3), 0.01 * rn(N, 3, E)]
    return index, pred, gt


@functools.lru_cache(maxsize=None)
def _terms_truth(N, V, E, J, terms):
    """Float64 on the CPU, once per case: the three losses and weight_k * d loss_k / d pred_k."""
    import torch
    index, pred, gt = _terms_case(N, V, E, J)
    leaves = [t.double().requires_grad_(True) for t in pred]
    loss64 = R.lbs_terms(index, *leaves, *[t.double() for t in gt])
    grad64 = torch.autograd.grad((loss64 * torch.tensor(terms, dtype=torch.float64)).sum(), leaves)
    return loss64.detach(), grad64


# typical size of pred - gt per term on _terms_case (softmax rows of 6: ~0.2; two 0.01 N(0,1): 0.014)
_TERM_SIGMA = (0.2, 0.014, 0.014)
EPS = 2.0 ** -24             # one float32 rounding, relative


def _terms_roundings(N, E, J):
    """R per term (weights, posedirs, shapedirs): see test_lbs_terms_losses_and_added_gradients."""
    blocks = min(-(-N // 16), TERMS_GRID_CAP // 16)
    visits, per_lane = -(-N // (16 * blocks)), -(-blocks // 256)
    return [-(-length // 16) + visits + per_lane + 18 for length in (J, 108, 3 * E)]


@pytest.mark.parametrize("N,E,J", [pytest.param(1027, 50, 6, id="50-6"), pytest.param(1027, 7, 5, id="7-5"), (1027, 1, 1),
                                   (TERMS_GRID_CAP, 50, 6), (TERMS_GRID_CAP + 1, 50, 6), (3 * TERMS_GRID_CAP + 5, 50, 6),
                                   (TERMS_GRID_CAP + 1, 64, 8)])
def test_lbs_terms_losses_and_added_gradients(gpu_device, N, E, J):
    """Losses against the float64 restatement within a COUNTED bound, R x 2^-24 x loss.  A term is a sum of squares (pred - gt)^2:
    nothing cancels, so every rounding on the way from an element to the result costs at most 2^-24 of the result, and R is the
    number of roundings on the longest such way through k_lbs_terms (fr_point_lbs.hip, built without FMA contraction), for a row
    of `len` floats (J, 108, 3 E), B = min(ceil(N / 16), 1024) workgroups:
        the element: the difference 1 (it enters squared: 2), the square 1                                    3
        a lane's ceil(len / 16) elements of a row, added one after the other (the first to 0: exact)           ceil(len / 16) - 1
        the group's ceil(N / 16 B) visits, a row's sum added per visit (the first to 0)                        visits - 1
        the wave's shuffle tree 6, the workgroup's four waves 2                                                8
        in the last workgroup ceil(B / 256) partials per lane (the first to 0), tree and waves again           ceil(B / 256) - 1 + 8
        1 / count, rounded on the host, and the product                                                        2
        R = ceil(len / 16) + ceil(N / 16 B) + ceil(B / 256) + 18
    = 30 for shapedirs at (1 027, 50), 36 at (49 157, 50).  At the sizes this test ran before the count (N = 1 027) that is
    looser than the 1e-6 it asserted, which therefore stays beside it there.
    What the kernel ADDED to pre-filled buffers is within rel-L2 1e-6 of float64 autograd's weight_k * d loss_k / d pred_k, and
    every entry of the buffer after the launch within 4 x 2^-24 (|pre| + |g64|) of pre + g64: one rounding for the difference, one
    for the coefficient (rounded on the host), one for the product, one for the read-modify-write.  The buffers are pre-filled
    with values of the gradient's own size (weight_k * 2 sigma_k / count_k, from the inputs' spread), so that the sum's
    rounding (2^-24 of the sum) stays below the bound on the added part; a zero weight leaves its array's bits alone.
    Achieved maxima (MI355X): profiles/r18_grid_caps.md."""
    import torch
    from fateavatar_amd.mono import LbsWeights, lbs_terms_and_grad
    dev = gpu_device
    V = 97
    index, pred, gt = _terms_case(N, V, E, J)
    terms = LbsWeights(1.0, 1e4, 250.0)
    loss64, grad64 = _terms_truth(N, V, E, J, terms)
    gen = torch.Generator().manual_seed(9)
    pre = [torch.randn(t.shape, generator=gen) * (wk * 2 * s / t.numel()) for t, wk, s in zip(pred, terms, _TERM_SIGMA)]
    bufs = [t.clone().to(dev) for t in pre]
    d_pred, d_gt = [t.to(dev) for t in pred], [t.to(dev) for t in gt]
    loss = lbs_terms_and_grad(index.to(dev), *d_pred, *d_gt, terms, *bufs)
    counted = _terms_roundings(N, E, J)
    for k, name in enumerate(("weights", "posedirs", "shapedirs")):
        assert float(loss64[k]) > 0, name
        e = abs(float(loss[k]) - float(loss64[k])) / float(loss64[k])
        after = bufs[k].cpu().double()
        added = after - pre[k].double()
        ge = _rel(added, grad64[k])
        entry = (after - (pre[k].double() + grad64[k])).abs() / (pre[k].double().abs() + grad64[k].abs()).clamp_min(1e-300)
        print(f"N={N} E={E} J={J} {name}: loss {float(loss[k]):.9e} rel err {e:.3e} = {e / EPS:.2f} of the R = {counted[k]} roundings "
              f"allowed; added gradient rel-L2 {ge:.3e}, worst entry {float(entry.max()) / EPS:.2f} of the 4 roundings allowed; "
              f"|pre| / |grad| {float(pre[k].norm() / grad64[k].norm()):.2f}")
        assert e <= counted[k] * EPS, (name, e)
        if N == 1027:
            assert e <= 1e-6, (name, e)
        assert ge <= 1e-6, (name, ge)
        assert float(entry.max()) <= 4 * EPS, (name, float(entry.max()))
    # losses only, and a zero weight: bits unchanged
    again = [t.clone().to(dev) for t in pre]
    loss2 = lbs_terms_and_grad(index.to(dev), *d_pred, *d_gt, LbsWeights(1.0, 0.0, 250.0), again[0], again[1], again[2])
    assert torch.equal(loss2, loss)
    assert torch.equal(again[1].cpu().view(torch.int32), pre[1].view(torch.int32))
    assert torch.equal(again[0], bufs[0]) and torch.equal(again[2], bufs[2])
    loss3 = lbs_terms_and_grad(index.to(dev), *d_pred, *d_gt)
    assert torch.equal(loss3, loss)


def test_lbs_terms_clamp_indices_outside_the_table(gpu_device):
    """Rows whose index is -7, V or 2^31 - 1 give the bits (losses and added gradients) of the same call with those indices set
    to 0, V - 1 and V - 1: the kernel clamps an index before any use of it (k_lbs_terms, fr_point_lbs.hip)."""
    import torch
    from fateavatar_amd.mono import LbsWeights, lbs_terms_and_grad
    dev = gpu_device
    N, V, E, J = TERMS_GRID_CAP + 1, 97, 50, 6
    index, pred, gt = _terms_case(N, V, E, J)
    outside, clamped = index.clone(), index.clone()
    rows = [0, 1, 2, 15, 16, 4098, TERMS_GRID_CAP - 1, TERMS_GRID_CAP, 777]      # (TERMS_GRID_CAP: the second sweep's only point)
    for r, (bad, good) in zip(rows, [(-7, 0), (V, V - 1), (2 ** 31 - 1, V - 1)] * 3):
        outside[r], clamped[r] = bad, good
    d_pred, d_gt = [t.to(dev) for t in pred], [t.to(dev) for t in gt]
    terms = LbsWeights(1.0, 1e4, 250.0)

    def run(idx):
        bufs = [torch.zeros_like(t) for t in d_pred]
        return lbs_terms_and_grad(idx.to(dev), *d_pred, *d_gt, terms, *bufs).clone(), bufs

    (la, ga), (lb, gb) = run(outside), run(clamped)
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    for a, b in zip(ga, gb):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and float(a[rows].abs().max()) > 0
    lc, _ = run(index)
    assert not torch.equal(lc, la)                                                 # (the nine rows do matter)


def test_lbs_terms_past_the_cap_repeat_their_bits_and_zero_the_workspace(gpu_device):
    """N = 49 157 (a partial fourth sweep, four partials per lane of the last workgroup): two runs give equal bits, the workspace
    is all zero after each, and a losses-only call gives the same three words."""
    import torch
    from fateavatar_amd.mono import LbsWeights, lbs_terms_and_grad, lbs_terms_workspace
    dev = gpu_device
    N, V, E, J = 3 * TERMS_GRID_CAP + 5, 97, 50, 6
    index, pred, gt = _terms_case(N, V, E, J)
    index, d_pred, d_gt = index.to(dev), [t.to(dev) for t in pred], [t.to(dev) for t in gt]
    ws = lbs_terms_workspace(dev)
    runs = []
    for _ in range(2):
        bufs = [torch.zeros_like(t) for t in d_pred]
        loss = lbs_terms_and_grad(index, *d_pred, *d_gt, LbsWeights(1.0, 1e4, 250.0), *bufs, workspace=ws).clone()
        torch.cuda.synchronize()
        assert int(ws.count_nonzero()) == 0
        runs.append((loss, bufs))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and float(runs[0][0].min()) > 0
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    only = lbs_terms_and_grad(index, *d_pred, *d_gt, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(only.view(torch.int32), runs[0][0].view(torch.int32)) and int(ws.count_nonzero()) == 0


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
