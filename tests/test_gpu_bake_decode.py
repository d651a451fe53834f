"""GPU: the neural-baking decode (`texture.decode_attributes`: fr_bake_decode / fr_bake_decode_backward) and the rotation term
(`loss.rot_term_and_grad`: fr_rot_term), csrc/fr_bake.hip.

The oracle is tests/bake_ref.py on the CPU in float64: activate every slice of the decoder output — rotation through
`rotation_activation` — then F.grid_sample(.., "bilinear", "border", align_corners=True), and its autograd.

Tolerances: the "four floors" rule of tests/test_gpu_texture.py.  Per output and per gradient slice the test measures the
FLOOR on its own inputs — the same restatement in float32 torch against float64 — prints it, and holds the HIP result to
4 x that floor in max-abs and in rel-L2.  Where the floor is a draw and not a statistic (N < 1000: it can be 0) the bound is
the larger of 4 x floor and an a-priori one, that file's, restated for this kernel:
    forward   the sample position carries <= 4 ulp of (size - 1) per axis, which moves the value by at most that times the
              largest texel-to-texel difference (<= 2 max|act|), plus 8 ulp of the activation's ARGUMENT scale for its own
              roundings — max|act| for the 1 -> 1 activations, 2 pi sqrt(3) for rotation, whose components are sin / cos of
              theta / 2 with theta <= 2 pi sqrt(3) and carry theta's roundings (tanh, x 2 pi, the norm) at a slope <= 1 / 2 .. 1;
    gradient  a texel's gradient is a sum of n <= (its list's length) terms weight x d_out x act': the position error times
              n max|d_out| max|act'|, plus 8 ulp of that for the sum and the Jacobian.  max|act'| of rotation is bounded by
              4 x 1.5 x 2 pi (four components, |d q_j / d a_i| <= |s| + |cos / 2 - s| <= 1.5, d a / d t <= 2 pi).
The mistakes these tests exist for — a wrong slice, the shuffle, a Jacobian's sign, the Taylor branch — show at >= 1e-2."""
import math

import numpy as np
import pytest

from tests import bake_ref as R

pytestmark = pytest.mark.gpu

MEAN_S, MAX_S = -5.0, -4.5           # a scaling prior's mean and mean + std (uv_decoder.py:298-301), log-scale units
ULP = 2.0 ** -24
SHAPES = [(1, 7), (5, 1), (37, 53), (512, 512)]
COUNTS = [1, 257, 100003]


@pytest.fixture(autouse=True)
def _needs_a_device(gpu_device):
    """Without a device every test skips."""


def _uniform(gen, *shape):
    import torch
    return torch.rand(*shape, generator=gen) * 2 - 1


_CASES = {}


def _case(H, W, N):
    """A decoder output, a UV set and upstream gradients (CPU, float32), with what the kernels can go wrong on:
    texture   uniform(-1, 1); about a tenth of the texels have all three ROTATION channels exactly 0 (the Taylor branch,
              forward and backward), another tenth +-5 (tanh saturated, tanh' about 0) — at least one texel of each;
    uv        uniform in [-0.1, 1.1] x [-0.1, 0.7] (part of it clipped to the border; the rows below 0.7 (H - 1) + 1 get no
              random point), and from the front: points exactly ON texels, points on the last column (u = 1) and on the last
              row (v = 1, at u = 0, 0.5, 1), and a cluster of N / 8 points inside ONE texel cell."""
    import torch
    key = (H, W, N)
    if key in _CASES:
        return _CASES[key]
    gen = torch.Generator().manual_seed(1000 * H + 10 * W + N % 7)
    tex = _uniform(gen, 1, 11, H, W)
    pick = torch.randperm(H * W, generator=gen)
    n_special = max(1, H * W // 10)
    zero, sat = pick[:n_special], pick[n_special:2 * n_special]
    rot = tex[0, 7:10].reshape(3, -1)
    rot[:, zero] = 0.0
    rot[:, sat] = 5.0 * torch.sign(_uniform(gen, 3, len(sat)) + 1e-3)
    uv = torch.rand(N, 2, generator=gen) * torch.tensor([1.2, 0.8]) - 0.1
    if N >= 257:
        k = N // 8
        xs = torch.randint(0, W, (k,), generator=gen).float() / max(W - 1, 1)
        ys = torch.randint(0, int(0.7 * (H - 1)) + 1, (k,), generator=gen).float() / max(H - 1, 1)   # (rows the random points reach)
        uv[:k] = torch.stack([xs, ys], 1)                                                   # exactly on texels
        uv[k:k + 8, 0] = 1.0                                                                # the last column
        uv[k + 8:k + 11] = torch.tensor([[0.0, 1.0], [0.5, 1.0], [1.0, 1.0]])              # the last row
        cell = torch.tensor([(W // 3) / max(W - 1, 1), (H // 3) / max(H - 1, 1)])
        size = torch.tensor([1.0 / max(W - 1, 1), 1.0 / max(H - 1, 1)])
        uv[k + 11:2 * k + 11] = cell + torch.rand(k, 2, generator=gen) * size * 0.999       # many points in one texel cell
    d_values = {n: _uniform(gen, N, w) for n, w in R.WIDTHS.items()}
    _CASES[key] = dict(tex=tex, uv=uv, d_values=d_values, zero=zero, sat=sat)
    return _CASES[key]


_REFS = {}


def _refs(H, W, N):
    """The float64 and float32 restatements of a case: computed once, shared, never written to."""
    import torch
    key = (H, W, N)
    if key not in _REFS:
        c = _case(H, W, N)
        _REFS[key] = (R.decode_with_grad(c["tex"], c["uv"], MEAN_S, MAX_S, c["d_values"], torch.float64),
                      R.decode_with_grad(c["tex"], c["uv"], MEAN_S, MAX_S, c["d_values"], torch.float32))
    return _REFS[key]


def _err(a, ref):
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    return float((a - ref).abs().max()), float((a - ref).norm() / max(float(ref.norm()), 1e-300))


def _hip(c, H, W):
    import torch
    from fateavatar_amd import texture
    dev = torch.device("cuda:0")
    plan = texture.TexturePlan(c["uv"].to(dev), H, W)
    tex = c["tex"].to(dev).requires_grad_(True)
    texture_dict, values = texture.decode_attributes(tex, plan, MEAN_S, MAX_S)
    assert list(values) == list(R.NAMES) and list(texture_dict) == list(R.NAMES)
    (grad,) = torch.autograd.grad([values[n] for n in R.NAMES], [tex], [c["d_values"][n].to(dev) for n in R.NAMES])
    torch.cuda.synchronize()
    return {n: v.detach().cpu() for n, v in values.items()}, grad.cpu(), plan, texture_dict


def _act_scale(name, tex_slice):
    """(max |act|, the activation's argument scale, max |act'|) of a slice, float64."""
    t = tex_slice.double().requires_grad_(True)
    a = R.activate(name, t, MEAN_S, MAX_S)
    amax = float(a.detach().abs().max())
    if name == "rotation":
        return amax, 2 * math.pi * math.sqrt(3.0), 4 * 1.5 * 2 * math.pi
    a.sum().backward()
    return amax, amax, float(t.grad.abs().max())


@pytest.mark.parametrize("N", COUNTS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_decode_and_its_backward_within_four_floors(H, W, N):
    import torch
    c = _case(H, W, N)
    (ref_v, ref_g), (f32_v, f32_g) = _refs(H, W, N)
    hip_v, hip_g, plan, texture_dict = _hip(c, H, W)
    row_start, _ = plan.csr()
    longest = int((row_start[1:] - row_start[:-1]).max())
    small = N < 1000
    pos = 4 * ULP * ((W - 1) + (H - 1))
    assert hip_g.shape == c["tex"].shape and bool(torch.isfinite(hip_g).all())
    for name, (lo, hi) in zip(R.NAMES, ((0, 3), (3, 4), (4, 7), (7, 10), (10, 11))):
        assert hip_v[name].shape == (N, R.WIDTHS[name]) and tuple(texture_dict[name].shape) == (1, hi - lo, H, W)
        amax, arg, dmax = _act_scale(name, c["tex"][:, lo:hi])
        dout = float(c["d_values"][name].abs().max())
        for what, hip, f32, ref in (("forward", hip_v[name], f32_v[name], ref_v[name]),
                                    ("gradient", hip_g[:, lo:hi], f32_g[:, lo:hi], ref_g[:, lo:hi])):
            floor, got = _err(f32, ref), _err(hip, ref)
            bound = [4 * floor[0], 4 * floor[1]]
            if small:
                gmax = longest * dout * dmax
                apriori = pos * 2 * amax + 8 * ULP * arg if what == "forward" else pos * gmax + 8 * ULP * gmax
                bound[0] = max(bound[0], apriori)
                bound[1] = max(bound[1], apriori * ref.numel() ** 0.5 / max(float(ref.double().norm()), 1e-300))
            print(f"decode {H}x{W} N={N} {name} {what}: floor max-abs {floor[0]:.3e} rel-L2 {floor[1]:.3e} | HIP max-abs {got[0]:.3e} "
                  f"rel-L2 {got[1]:.3e} | bound {bound[0]:.3e} / {bound[1]:.3e}")
            assert np.isfinite(got[0]) and got[0] <= bound[0] and got[1] <= bound[1], (name, what, floor, got, bound)
    # the special rotation texels were sampled: a point sits exactly on a zero texel / the Taylor branch is hit backward
    counts = (row_start[1:] - row_start[:-1]).cpu()
    if N >= 257:
        assert int(counts[c["zero"]].sum()) > 0 and int(counts[c["sat"]].sum()) > 0
    # texels no point touches: the stored gradient is exactly 0
    untouched = (counts == 0).reshape(H, W)
    if (H, W) in ((37, 53), (512, 512)):
        assert int(untouched.sum()) > H * W // 8
    assert bool((hip_g[0][:, untouched] == 0).all())


@pytest.mark.parametrize("H,W,N", [(37, 53, 100003), (512, 512, 100003), (1, 7, 257)])
def test_four_attributes_are_gather_attributes_rows_and_the_backward_repeats_its_bits(H, W, N):
    """Colour, opacity, scaling and offset use the look-up's expressions in its order: bit-equal rows (and gradient slices:
    the same list order and the same act').  Two backward launches into NaN-filled buffers give identical bits, every texel
    written; a NULL gradient array stands for zeros."""
    import torch
    from fateavatar_amd import _lib, texture
    dev = torch.device("cuda:0")
    c = _case(H, W, N)
    plan = texture.TexturePlan(c["uv"].to(dev), H, W)
    tex = c["tex"].to(dev)
    leaf_a, leaf_b = tex.clone().requires_grad_(True), tex.clone().requires_grad_(True)
    _, va = texture.decode_attributes(leaf_a, plan, MEAN_S, MAX_S)
    _, vb = texture.gather_attributes(leaf_b, plan, MEAN_S, MAX_S)
    same = ("color", "opacity", "scaling", "offset")
    for n in same:
        assert torch.equal(va[n], vb[n]), n
    d = {n: g.to(dev) for n, g in c["d_values"].items()}
    torch.autograd.backward([va[n] for n in same], [d[n] for n in same])
    torch.autograd.backward([vb[n] for n in same], [d[n] for n in same])
    torch.cuda.synchronize()
    for lo, hi in ((0, 3), (3, 4), (4, 7), (10, 11)):
        assert torch.equal(leaf_a.grad[:, lo:hi], leaf_b.grad[:, lo:hi]), (lo, hi)
    assert bool((leaf_a.grad[:, 7:10] == 0).all())                   # (rotation got no upstream gradient: NULL, stored zeros)
    # the C ABI, twice, into NaN
    row_start, entries = plan.csr()
    runs = []
    for _ in range(2):
        out = torch.full_like(tex, float("nan"))
        rc = _lib.lib().fr_bake_decode_backward(plan.N, plan.uv.data_ptr(), H, W, row_start.data_ptr(), entries.data_ptr(), tex.data_ptr(),
                                                MEAN_S, MAX_S, *[d[n].data_ptr() for n in R.NAMES], out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.FR_OK, _lib.last_error()
        torch.cuda.synchronize()
        runs.append(out)
    assert bool(torch.isfinite(runs[0]).all()) and torch.equal(runs[0], runs[1])
    leaf = tex.clone().requires_grad_(True)
    _, v = texture.decode_attributes(leaf, plan, MEAN_S, MAX_S)
    torch.autograd.backward([v[n] for n in R.NAMES], [d[n] for n in R.NAMES])
    assert torch.equal(leaf.grad, runs[0])                            # the autograd route gives those bits
    # a plan of another (larger) UV set: entries past N are skipped, nothing is read out of bounds
    keep = N // 2
    half = texture.TexturePlan(c["uv"][:keep].to(dev), H, W)
    out = torch.full_like(tex, float("nan"))
    texture.decode_backward_into(half, tex, MEAN_S, MAX_S, [d[n][:keep].contiguous() for n in R.NAMES], out)
    guarded = torch.full_like(tex, float("nan"))
    rc = _lib.lib().fr_bake_decode_backward(keep, plan.uv.data_ptr(), H, W, row_start.data_ptr(), entries.data_ptr(), tex.data_ptr(),
                                            MEAN_S, MAX_S, *[d[n].data_ptr() for n in R.NAMES], guarded.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.FR_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, guarded)


def test_zero_rotation_texels_take_the_taylor_branch():
    """An all-zero rotation slice: every row is the identity's image (0, 1, 0, 0) exactly, and the gradient is pi x the
    upstream (x, y, z) components' interpolation adjoint — finite, nothing divided by theta."""
    import torch
    from fateavatar_amd import texture
    dev = torch.device("cuda:0")
    H, W, N = 9, 6, 500
    gen = torch.Generator().manual_seed(3)
    tex = _uniform(gen, 1, 11, H, W)
    tex[:, 7:10] = 0.0
    uv = torch.rand(N, 2, generator=gen)
    plan = texture.TexturePlan(uv.to(dev), H, W)
    leaf = tex.to(dev).requires_grad_(True)
    _, v = texture.decode_attributes(leaf, plan, MEAN_S, MAX_S)
    rot = v["rotation"].detach().cpu()
    # (the four weights sum to 1 within their own roundings: four products and three additions)
    assert bool((rot[:, [0, 2, 3]] == 0).all()) and float((rot[:, 1] - 1).abs().max()) <= 8 * ULP
    d_rot = _uniform(gen, N, 4)
    v["rotation"].backward(d_rot.to(dev))
    torch.cuda.synchronize()
    got = leaf.grad[0, 7:10].cpu()
    # the adjoint of the interpolation for the emitted components 2, 3, 0 (= x, y, z), in float64, times pi
    x = torch.zeros(1, 3, H, W, dtype=torch.float64, requires_grad=True)
    o = torch.nn.functional.grid_sample(x, (2 * uv.double() - 1)[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    o[0, :, 0, :].t().backward(d_rot[:, [2, 3, 0]].double())
    want = x.grad[0] * math.pi
    x.grad = None
    o = torch.nn.functional.grid_sample(x, (2 * uv.double() - 1)[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    o[0, :, 0, :].t().backward(d_rot[:, [2, 3, 0]].double().abs())
    scale = float(x.grad.abs().max()) * math.pi                       # the largest sum of |terms| of a texel
    row_start, _ = plan.csr()
    longest = int((row_start[1:] - row_start[:-1]).max())
    assert bool(torch.isfinite(got).all())
    err = float((got.double() - want).abs().max())
    print(f"zero texels: gradient max-abs error {err:.3e}, largest sum of |terms| {scale:.3e}, longest list {longest}")
    # a sequential float32 sum of n terms: <= n ulp of the sum of their magnitudes; 16 more for the weights (the position's
    # 4 ulp x (H + W - 2) of a texel), the product with float32(pi) and the Jacobian's own roundings
    assert err <= (longest + 16 + 4 * (H + W - 2)) * ULP * scale


def test_forward_and_backward_replayed_as_a_graph_match_eager():
    import torch
    from fateavatar_amd import texture
    dev = torch.device("cuda:0")
    H, W, N = 37, 53, 100003
    c = _case(H, W, N)
    plan = texture.TexturePlan(c["uv"].to(dev), H, W)
    plan.csr()                                                       # (the plan is built eagerly: it sorts and synchronises)
    tex = c["tex"].to(dev).requires_grad_(True)
    d = [c["d_values"][n].to(dev) for n in R.NAMES]
    run = lambda t: texture.decode_attributes(t, plan, MEAN_S, MAX_S)[1]  # noqa: E731
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                    # warm the allocator on the capture stream
        v = run(tex)
        torch.autograd.grad([v[n] for n in R.NAMES], [tex], d)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        v = run(tex)
        outs = [v[n] for n in R.NAMES]
        grads = torch.autograd.grad(outs, [tex], d)
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(77)
    for rep in range(2):
        with torch.no_grad():
            tex.copy_(_uniform(gen, *tex.shape).to(dev))             # new contents in the captured buffers
            for t in d:
                t.copy_(_uniform(gen, *t.shape).to(dev))
            for o in list(outs) + list(grads):
                o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        leaf = tex.detach().clone().requires_grad_(True)
        ev = run(leaf)
        e_outs = [ev[n] for n in R.NAMES]
        e_grads = torch.autograd.grad(e_outs, [leaf], d)
        torch.cuda.synchronize()
        for a, b in zip(list(outs) + list(grads), list(e_outs) + list(e_grads)):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), rep


# ------------------------------------------------------------------ the rotation term
def _rot_rows(N, seed):
    """[N,4] uniform(-1, 1) rows.  A row within atan(0.5) of a half angle of pi (negative real part, a short vector part) is
    flipped to its positive real part: there float32 loses the leading digits of sin(half), the floor becomes one row's
    accident, and the term's value AT half = pi is pinned by the row (-1, 0, 0, 0) below.  From 300 rows on, rows 0 .. 2 are
    (1,0,0,0), (0,0,0,0) and (-1,0,0,0): no vector part, no gradient."""
    import torch
    q = _uniform(torch.Generator().manual_seed(seed), N, 4)
    n = q[:, 1:].norm(dim=1)
    flip = (q[:, 0] < 0) & (n < 0.5 * q[:, 0].abs())
    q[flip, 0] = q[flip, 0].abs()
    if N >= 300:
        q[:3] = torch.tensor([[1.0, 0, 0, 0], [0.0, 0, 0, 0], [-1.0, 0, 0, 0]])
    return q


@pytest.mark.parametrize("N", [1, 300, 70001])
def test_rot_term_within_four_floors_adds_and_repeats_its_bits(N):
    """One workgroup, two, and past the grid cap (256 workgroups of 256 rows).  The loss word and the ADDED gradient against
    the float64 restatement within 4 x the float32 torch floor — a scalar's floor counts as no less than one float32
    rounding, and so does the single row's gradient (N = 1: one draw)."""
    import torch
    from fateavatar_amd.loss import rot_loss, rot_term_and_grad, rot_term_workspace
    dev = torch.device("cuda:0")
    weight = 0.1
    q = _rot_rows(N, 40 + N % 11)
    ref_l, ref_g = R.rot_loss_and_grad(q, torch.float64)
    f32_l, f32_g = R.rot_loss_and_grad(q, torch.float32)
    scale = float(ref_g.abs().max())
    before = _uniform(torch.Generator().manual_seed(9), N, 4) * (weight * scale)     # (a non-zero buffer at the gradient's own scale)
    ws = rot_term_workspace(dev)
    runs = []
    for _ in range(2):
        d = before.to(dev)
        out = rot_term_and_grad(q.to(dev), d, weight=weight, workspace=ws)
        torch.cuda.synchronize()
        runs.append((out.cpu(), d.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and not bool(ws.any())
    loss, d = runs[0]
    rel = lambda a: abs(float(a) - float(ref_l)) / max(abs(float(ref_l)), 1e-300)  # noqa: E731
    floor_l = max(rel(f32_l), ULP)
    print(f"rot term N={N}: loss {float(loss[0])!r} (float64 {float(ref_l)!r}) relative error {rel(loss[0]):.3e}, floor {floor_l:.3e}")
    assert rel(loss[0]) <= 4 * floor_l
    added = (d.double() - before.double()) / weight
    floor, got = _err(f32_g, ref_g), _err(added, ref_g)
    # the kernel's sum before + weight x g rounds at the sum's scale (<= 2 weight x scale): 4 ulp of `scale` on top of the floors
    slack = 4 * ULP * scale
    floor = (max(floor[0], ULP * scale), max(floor[1], ULP)) if N == 1 else floor
    print(f"rot term N={N}: gradient floor max-abs {floor[0]:.3e} rel-L2 {floor[1]:.3e} | HIP max-abs {got[0]:.3e} rel-L2 {got[1]:.3e}")
    assert got[0] <= 4 * floor[0] + slack and got[1] <= 4 * floor[1] + slack * added.numel() ** 0.5 / max(float(ref_g.norm()), 1e-300)
    if N >= 300:
        assert torch.equal(d[:3], before[:3])                        # rows without a vector part: nothing added
        assert int((d[3:] != before[3:]).any(dim=1).sum()) == N - 3
    # the autograd op: the same loss word, the gradient with weight 1 scaled by the incoming one
    leaf = q.to(dev).requires_grad_(True)
    l = rot_loss(leaf)
    assert l.dim() == 0 and float(l.detach()) == float(loss[0])
    (2.5 * l).backward()
    torch.cuda.synchronize()
    got = _err(leaf.grad.cpu() / 2.5, ref_g)
    assert got[0] <= 4 * floor[0] + 4 * ULP * scale and got[1] <= 4 * floor[1] + 4 * ULP
    # the loss alone, and a zero weight: the gradient array is not touched
    d0 = before.to(dev)
    assert float(rot_term_and_grad(q.to(dev), d0, weight=0.0, workspace=ws)[0]) == float(loss[0]) and torch.equal(d0.cpu(), before)
    assert float(rot_term_and_grad(q.to(dev), None, workspace=ws)[0]) == float(loss[0])
