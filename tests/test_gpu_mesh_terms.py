"""-m gpu: FateAvatar's mesh terms on the device — the launch (`fr_mesh_terms` through `loss.mesh_terms_and_grad`) against
float64, its gates and bits, `laplacian_smoothing_loss` as an autograd op, and the steps that hand their caller
dLoss/dposed_verts (`vertex_grad`, `mesh_terms`).

reference: FateAvatarLoss.get_laplacian_smoothing_loss / flame_loss (train/loss.py:112-121,166-180,192-197) with the weights
of config/fateavatar.yaml:23; the restatement the kernel is held to is tests/mesh_terms_ref.py."""
import numpy as np
import pytest

from tests.mesh_terms_ref import (displaced, flame_distance, float64_terms, float64_terms_sparse, laplacian_dense, laplacian_smoothing,
                                  random_mesh, random_mesh_drawn_at_once)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
N_RED = 21     # roundings of a loss sum behind its terms up to 8 192 vertices: see test_mesh_terms_kernel_matches_float64
MESH_GRID_CAP = 1024 * 32   # vertices one sweep of k_mesh_terms covers: kMeshMaxBlocks x (kMeshThreads / kMeshGroup), fr_mesh_terms.hip
SIZES = [1, 3, 4, 63, 64, 65, 257]
# past the cap (an exactly full sweep, one vertex in a second sweep, a partial third sweep): meshes drawn at once, held to the
# sparse float64 restatement (V x V doubles would be 8.6 GB and more)
BIG_SIZES = [MESH_GRID_CAP, MESH_GRID_CAP + 1, 2 * MESH_GRID_CAP + 9]
SEED = {1: 101, 3: 103, 4: 104, 63: 115, 64: 105, 65: 101, 257: 102}   # (63 .. 257: draws that leave a vertex without a face)
SEED.update({V: 200 + k for k, V in enumerate(BIG_SIZES)})
_cache = {}


def _mesh(V):
    """(verts_orig, verts, faces) of a case, float32 / int64 numpy: a drawn mesh, or the head template."""
    if V not in _cache:
        if V == "template":
            from fateavatar_amd import scenes
            vo, faces, _ = scenes.head_geometry()
            vo, faces, seed = np.ascontiguousarray(vo, dtype=np.float32), np.asarray(faces, dtype=np.int64), 7
        else:
            vo, faces = (random_mesh_drawn_at_once if V in BIG_SIZES else random_mesh)(V, SEED[V])
            seed = SEED[V]
        _cache[V] = (vo, displaced(vo, seed), faces)
    return _cache[V]


def _truth(V, weights):
    """float64_terms of a case (past the cap: its sparse form), computed once per (case, weights) and left unchanged."""
    import torch
    key = (V, tuple(weights))
    if key not in _cache:
        vo, v, faces = _mesh(V)
        terms = float64_terms_sparse if V in BIG_SIZES else float64_terms
        _cache[key] = terms(faces, vo.shape[0], torch.from_numpy(vo), torch.from_numpy(v), *weights)
    return _cache[key]


def _n_red(V):
    """N_RED, plus one rounding per further partial a lane of the last workgroup adds up (past 8 192 vertices) and one per
    further vertex a group of lanes visits (past MESH_GRID_CAP), as csrc/fr_mesh_terms.hip's header spells out."""
    blocks = min(-(-V // 32), MESH_GRID_CAP // 32)
    return N_RED + (-(-blocks // 256) - 1) + (-(-V // (32 * blocks)) - 1)


def _grad_bound(t, weights, V, want):
    """|got - want| per entry of d_verts after the launch: (2 deg_max + 10) eps x (the magnitude of what was added up) +
    eps |want| for the read-modify-write."""
    mag = weights[0] * t["Mg"] + weights[1] * (2.0 / (3.0 * V)) * t["d"].abs()
    return (2 * int(t["deg"].max()) + 10) * EPS * mag + EPS * want.abs()


def _loss_bounds(t, V):
    r_err = (t["deg"][:, None].double() + 3.0) * EPS * t["Mr"]
    lap = float((2.0 * t["r"].abs() * r_err).sum()) / V + _n_red(V) * EPS * t["lap"]
    flame = float((2.0 * t["d"].abs() * EPS * t["d"].abs()).sum()) / (3.0 * V) + _n_red(V) * EPS * t["flame"]
    return lap, flame


def _lap_of(faces, V, dev):
    import torch
    from fateavatar_amd.binding import MeshLaplacian, mesh_laplacian
    lap = mesh_laplacian(torch.from_numpy(faces), V)
    return MeshLaplacian(lap.row_ptr.to(dev), lap.col.to(dev), V)


def test_drawn_meshes_have_empty_rows():
    """The draws of `random_mesh` include a vertex no face uses on either side of the wave boundary and beyond one workgroup
    (next to V = 1, which has no face at all)."""
    empty = {V: int((_truth(V, (1e5, 0.0))["deg"] == 0).sum()) for V in SIZES}
    assert empty[1] == 1 and min(empty[63], empty[64], empty[65], empty[257]) >= 1 and empty[3] == empty[4] == 0, empty
    assert int(_truth(257, (1e5, 0.0))["deg"].max()) > int(_truth(257, (1e5, 0.0))["deg"].min()) + 4      # irregular degrees
    for V in BIG_SIZES:
        deg = _truth(V, (1e5, 0.0))["deg"]
        assert deg.shape == (V,) and int((deg == 0).sum()) >= 8 and int(deg.max()) > int(deg.min()) + 16, V
    assert [_n_red(V) for V in (1, 5023, 8192, 8193, MESH_GRID_CAP, MESH_GRID_CAP + 1, 2 * MESH_GRID_CAP + 9)] == [21, 21, 21, 22, 24, 25, 26]


# ------------------------------------------------------------------ 4. the kernel against float64
@pytest.mark.parametrize("weights", [(1e5, 0.0), (1e5, 0.3)])
@pytest.mark.parametrize("V", SIZES + ["template"] + BIG_SIZES)
def test_mesh_terms_kernel_matches_float64(gpu_device, V, weights):
    """`mesh_terms_and_grad` against float64 autograd of w_lap x laplacian + w_flame x flame on the dense restatement, added
    to a gradient array pre-filled with the gradient's own sign: expected = before + grad, no entry exempt.  eps = 2^-24.
    The kernel as written (csrc/fr_mesh_terms.hip, no FMA contraction), first order:
      d_j = verts_j - orig_j                                  1 rounding
      r_k = (sum_j d_j) * (1 / deg_k) - d_k                   d_j 1, deg_k - 1 additions, 1 / deg 1, product 1, subtraction 1
                                                              -> |dr_k| <= (deg_k + 3) eps M^r_k,   M^r = |L| |d|
      g_i = -r_i + sum_j r_j * (1 / deg_j)                    r_j deg_j + 3, 1 / deg_j and product 2, <= deg_i additions of
                                                              two non-zero terms (eight lanes' sums, then a shuffle tree)
      added_i = c_lap g_i + c_flame d_i                       c_lap (rounded on the host) and product 2; c_flame, product,
                                                              addition 3 -> deg_i + deg_j + 10 <= 2 deg_max + 10 roundings
                                                              of w M^g_i (+ w_flame (2/3V) |d_i|),   M^g = (2/V) |L|^T M^r
      d_verts_i += added_i                                    1 rounding of the result: eps |want_i|
    Loss scalars: |dloss| <= sum_i 2 |r_i| bound(r_i) / V + N_RED eps loss (flame: d, bound eps |d|, 3 V) with N_RED = 21: the
    squares and the row's two additions 3, the wave's shuffle tree 6, the workgroup's four waves 2, in the last workgroup
    its shuffle tree 6 and four waves 2 (one partial per lane: 157 workgroups of 32 vertices on the template), the rounded
    1 / V and the product 2; a group of lanes visits one vertex up to 32 768 vertices.  Past 8 192 vertices a lane of the last
    workgroup adds up ceil(B / 256) partials (B = min(ceil(V / 32), 1024) workgroups) and past MESH_GRID_CAP a group visits
    ceil(V / 32 B) vertices, a rounding more for each further one (`_n_red`): 24, 25, 26 at BIG_SIZES, whose meshes are drawn at
    once and held to the SPARSE float64 restatement (tests/test_mesh_terms_host.py pins it to the dense one).
    Achieved maxima (MI355X): see profiles/r15_mesh_terms.md, past the cap profiles/r18_grid_caps.md."""
    import torch
    from fateavatar_amd.loss import MeshTerms, mesh_terms_and_grad, mesh_terms_workspace
    dev = gpu_device
    vo, v, faces = _mesh(V)
    n = vo.shape[0]
    t = _truth(V, weights)
    lap = _lap_of(faces, n, dev)
    g = t["grad"]
    gen = torch.Generator().manual_seed(11)
    scale = float(g.abs().mean())
    before = ((torch.rand(n, 3, generator=gen) + 0.5) * torch.where(g < 0, -1.0, 1.0) * scale).float()
    assert scale > 0 and bool((before != 0).all())
    d_verts = before.to(dev)
    ws = mesh_terms_workspace(dev)
    out = mesh_terms_and_grad(torch.from_numpy(v).to(dev), torch.from_numpy(vo).to(dev), lap, MeshTerms(*weights), d_verts=d_verts,
                              workspace=ws)
    torch.cuda.synchronize()
    assert not bool(ws.any())
    want = before.double() + g
    err = (d_verts.cpu().double() - want).abs()
    bound = _grad_bound(t, weights, n, want)
    unit = (err - EPS * want.abs()).clamp_min(0) / (EPS * (weights[0] * t["Mg"]).clamp_min(1e-300))
    print(f"V={V} weights={weights}: max |got - want| / bound = {float((err / bound).max()):.3f}, beyond the read-modify-write "
          f"{float(unit.max()):.2f} eps w M^g, entries over the bound: {int((err > bound).sum())}")
    assert bool(torch.isfinite(d_verts).all()) and int((err > bound).sum()) == 0
    b_lap, b_flame = _loss_bounds(t, n)
    for name, got, want_l, b in (("laplacian", float(out[0]), t["lap"], b_lap), ("flame", float(out[1]), t["flame"], b_flame)):
        print(f"V={V} {name}: got {got:.9g} want {want_l:.9g} |d| {abs(got - want_l):.3e} bound {b:.3e}")
        assert want_l > 0 and abs(got - want_l) <= b, (name, got, want_l, b)


# ------------------------------------------------------------------ 5. gates and bits
def test_mesh_terms_kernel_gates_and_reproducibility(gpu_device):
    """Weights (0, 0) leave `d_verts` bit-identical; weight 0 for one term equals the other term alone; NULL `d_verts` gives
    the losses only; verts == verts_orig gives both losses exactly 0 and `d_verts` bit-identical; two launches, and a
    captured and replayed launch, give the eager bits; the workspace is zero afterwards; V == 0 launches nothing."""
    import torch
    from fateavatar_amd.binding import mesh_laplacian
    from fateavatar_amd.loss import MeshTerms, mesh_terms_and_grad, mesh_terms_workspace
    dev = gpu_device
    vo, v, faces = _mesh("template")
    n = vo.shape[0]
    lap = _lap_of(faces, n, dev)
    v_d, vo_d = torch.from_numpy(v).to(dev), torch.from_numpy(vo).to(dev)
    before = (torch.randn(n, 3, generator=torch.Generator().manual_seed(3)) + 3.0).to(dev)
    before[0, 0] = -0.0
    ws = mesh_terms_workspace(dev)

    def launch(weights, with_grad=True, verts=v_d, zero=False):
        d = torch.zeros_like(before) if zero else before.clone()
        out = mesh_terms_and_grad(verts, vo_d, lap, MeshTerms(*weights), d_verts=d if with_grad else None, workspace=ws).clone()
        torch.cuda.synchronize()
        assert not bool(ws.any())
        return out, d

    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731
    out, d = launch((1e5, 0.3))
    assert bool(torch.isfinite(d).all()) and float(out[0]) > 0 and float(out[1]) > 0 and not torch.equal(d, before)
    o0, d0 = launch((0.0, 0.0))
    assert bits(d0, before) and bits(o0, out)
    # one weight 0: the other term alone — into zeros, so that the sum of the two single launches is the pair's arithmetic
    _, only_l = launch((1e5, 0.0), zero=True)
    _, only_f = launch((0.0, 0.3), zero=True)
    _, pair = launch((1e5, 0.3), zero=True)
    assert bits(pair, only_l + only_f) and float(only_f.abs().max()) > 0 and float(only_l.abs().max()) > 0
    t = _truth("template", (1e5, 0.0))
    assert float((only_l.cpu().double() - t["grad"]).abs().max()) <= float(_grad_bound(t, (1e5, 0.0), n, t["grad"]).max())
    o1, d1 = launch((1e5, 0.3), with_grad=False)
    assert bits(o1, out) and bits(d1, before)
    o2, d2 = launch((1e5, 0.3), verts=vo_d)
    assert float(o2[0]) == 0.0 and float(o2[1]) == 0.0 and bits(d2, before)
    o3, d3 = launch((1e5, 0.3))
    assert bits(o3, out) and bits(d3, d)
    # ---- captured and replayed
    g_d, g_out = before.clone(), torch.zeros(2, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mesh_terms_and_grad(v_d, vo_d, lap, MeshTerms(1e5, 0.3), d_verts=g_d, out=g_out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        g_d.copy_(before)
        g_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert bits(g_out, out) and bits(g_d, d) and not bool(ws.any())
    # ---- V == 0: nothing is launched, `loss` stays
    empty = mesh_laplacian(torch.zeros((0, 3), dtype=torch.int64, device=dev), 0)
    keep = torch.full((2,), 7.0, device=dev)
    mesh_terms_and_grad(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), empty, out=keep, workspace=ws)
    torch.cuda.synchronize()
    assert keep.tolist() == [7.0, 7.0]
    # ---- the wrapper's own rules
    with pytest.raises(RuntimeError):
        mesh_terms_and_grad(torch.from_numpy(v), torch.from_numpy(vo), lap)                  # no CPU path
    with pytest.raises(RuntimeError):
        mesh_terms_and_grad(v_d, vo_d, lap, workspace=torch.zeros(8, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError):
        mesh_terms_and_grad(v_d[:-1].contiguous(), vo_d[:-1].contiguous(), lap)              # another mesh's Laplacian


# ------------------------------------------------------------------ 6. the autograd op
@pytest.mark.parametrize("batched", [False, True])
def test_laplacian_smoothing_loss_matches_float64_autograd(gpu_device, batched):
    """`laplacian_smoothing_loss(verts_orig, verts, lap)` on [V,3] and [1,V,3] against float64 autograd of the literal expression:
    value and `verts.grad` within the bounds of test_mesh_terms_kernel_matches_float64 at weights (1, 0) (the gradient lands
    in zeros and is multiplied by an incoming 1: both exact); `verts_orig.grad` stays None."""
    import torch
    from fateavatar_amd.loss import laplacian_smoothing_loss
    dev = gpu_device
    V = 257
    vo, v, faces = _mesh(V)
    t = _truth(V, (1.0, 0.0))
    lap = _lap_of(faces, V, dev)
    shape = (1, V, 3) if batched else (V, 3)
    verts = torch.from_numpy(v).to(dev).reshape(shape).requires_grad_(True)
    orig = torch.from_numpy(vo).to(dev).reshape(shape).requires_grad_(True)
    loss = laplacian_smoothing_loss(orig, verts, lap)
    assert loss.dim() == 0
    loss.backward()
    torch.cuda.synchronize()
    assert orig.grad is None and verts.grad.shape == shape
    assert abs(loss.item() - t["lap"]) <= _loss_bounds(t, V)[0]
    got = verts.grad.reshape(V, 3).cpu().double()
    err = (got - t["grad"]).abs()
    assert int((err > _grad_bound(t, (1.0, 0.0), V, t["grad"])).sum()) == 0 and float(t["grad"].abs().max()) > 0
    with torch.no_grad():                                            # the loss alone
        assert laplacian_smoothing_loss(orig, verts, lap).item() == loss.item()
    with pytest.raises(RuntimeError):
        laplacian_smoothing_loss(orig.reshape(-1), verts.reshape(-1), lap)


# ------------------------------------------------------------------ 7. the steps
def _displace(posed, seed):
    """The step tests' displaced mesh: `displaced` plus 3 mm of noise.  The float32 restatement applies the dense L to verts
    and to verts_orig separately, at positions around 1.5 (the template's height): that difference loses about
    eps |L| |v| / |L d| — 2.9e-5 rel-L2 of the gradient (CPU, against float64) with `displaced` alone, which would use up most of
    the 5e-5 the comparison allows for the order of float atomics; with the rougher mesh it is 9e-6."""
    import torch
    p = posed.cpu().numpy()
    rough = 0.003 * np.random.default_rng(seed + 50).standard_normal(p.shape)
    return torch.from_numpy((displaced(p, seed) + rough).astype(np.float32)).to(posed.device)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def test_avatar_step_hands_over_the_vertex_gradient(gpu_device):
    """`AvatarStep(vertex_grad=True)` without mesh terms, and with REFERENCE_MESH_TERMS on a displaced mesh, folded and with the
    stand-alone binding op: `step.d_verts` after step 1 and 2 (eager) and after the first replayed step (3) against an
    independent autograd evaluation at the parameters the step started from — verts leaf -> bind_gaussians -> render ->
    F.l1_loss + weights x the float32 restatement — rel-L2 < 5e-5 (the bound test_binding_inside_the_rasterizer_kernels_equals_
    the_binding_op holds dL/dverts to: the order of float atomics).  Every step is compared on its own: a `d_verts` that
    accumulated over steps would be the sum of two.  `mesh_loss` against float64 within the kernel test's loss bounds."""
    import torch
    from fateavatar_amd.avatar import AvatarStep, _BoundFrame
    from fateavatar_amd.binding import bind_gaussians
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS
    from fateavatar_amd.render import render
    from tests.test_gpu_avatar import _setup, _targets
    dev = gpu_device
    S = _setup(dev, 20_000, 128, 4, seed=3)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg)
    faces_np = S["faces"].cpu().numpy()
    V = int(S["canon"].shape[0])
    L32 = laplacian_dense(faces_np, V, torch.float32).to(dev)
    moved = [_displace(S["posed"][f], f) for f in range(4)]

    def make():
        g = torch.Generator().manual_seed(4)
        pc = S["make"]()
        with torch.no_grad():
            pc._features_dc.add_(0.2)
            pc._offset.add_((0.2 * torch.randn(pc.P, 1, generator=g)).to(dev))
            pc._scaling.add_((0.5 * torch.randn(pc.P, 3, generator=g)).to(dev))
            pc._rotation.add_((0.5 * torch.randn(pc.P, 4, generator=g)).to(dev))
            pc._opacity.add_(2.0)
        return pc

    class Holder:
        pass

    def reference(st, pc, f, verts, orig, terms):
        h = Holder()
        for n, _ in pc.FIELDS:
            setattr(h, n, getattr(pc, n).detach().clone().requires_grad_(True))
        v = verts.clone().requires_grad_(True)
        xyz, rot, scl = bind_gaussians(v, st.faces, pc.face_index, pc.bary_coords, st.face_scale_canonical, h._offset, h._rotation,
                                       h._scaling, st.shell_len, st.resize_scale)
        out = render(S["cams"][f], _BoundFrame(xyz, h, rot, scl, None), bg)
        loss = torch.nn.functional.l1_loss(out["render"], gts[f])
        if terms is not None:
            loss = loss + terms[0] * laplacian_smoothing(L32, orig, v) + terms[1] * flame_distance(orig, v)
        loss.backward()
        return v.grad

    for terms in (None, REFERENCE_MESH_TERMS):
        for fold in (True, False):
            pc = make()
            st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), bg, fold_binding=fold, vertex_grad=True, mesh_terms=terms)
            for it in range(3):
                f = it + 1
                verts, orig = (moved[f], S["posed"][f]) if terms is not None else (S["posed"][f], None)
                want = reference(st, pc, f, verts, orig, terms)            # (before the step moves the parameters)
                st.step(S["cams"][f], verts, gts[f], verts_orig=orig)
                torch.cuda.synchronize()
                assert (st._graph is not None) == (it == 2)
                got = st.d_verts
                rel = _rel(got, want)
                print(f"mesh_terms={terms is not None} fold={fold} step {it + 1}: rel-L2 {rel:.3e}, max |want| {float(want.abs().max()):.3e}")
                assert got.shape == (V, 3) and float(want.abs().max()) > 0 and rel < 5e-5, (terms, fold, it, rel)
                if terms is None:
                    assert st.mesh_loss is None
                else:
                    t = float64_terms(faces_np, V, orig.cpu(), verts.cpu(), *terms)
                    b_lap, b_flame = _loss_bounds(t, V)
                    assert abs(float(st.mesh_loss[0]) - t["lap"]) <= b_lap and abs(float(st.mesh_loss[1]) - t["flame"]) <= b_flame
                    assert t["lap"] > 0 and float(st.loss) > 0
            st.check()
            replayed = st.d_verts
            st.step(S["cams"][0], moved[0] if terms is not None else S["posed"][0], gts[0],
                    verts_orig=S["posed"][0] if terms is not None else None)
            assert st.d_verts.data_ptr() == replayed.data_ptr()            # one storage across the replays


def test_rigged_step_hands_over_the_vertex_gradient(gpu_device):
    """`RiggedStep(vertex_grad=True)`: `d_verts` after an eager step and after the first replayed one against autograd through
    `bind_gaussians_face_local` + render + L1 at the parameters the step started from, rel-L2 < 5e-5."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_face_local
    from fateavatar_amd.render import render
    from fateavatar_amd.rigged import RiggedStep, _RiggedFrame
    from tests.test_gpu_face_local import _perturbed, _targets, _template
    dev = gpu_device
    S = _template(dev, 128, 4)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg, 4)
    pc = _perturbed(dev, S["F"], seed=9)
    st = RiggedStep(pc, S["faces"], S["cams"][0].clone(), bg, S["posed"][0], vertex_grad=True)

    class Holder:
        pass

    for it in range(3):
        f = it + 1
        h = Holder()
        h.active_sh_degree, h.binding = pc.active_sh_degree, pc.binding
        leaves = {n: getattr(pc, n).detach().clone().requires_grad_(True) for n, _ in pc.FIELDS}
        for n, t in leaves.items():
            setattr(h, n, t)
        h.get_features = torch.cat((h._features_dc, h._features_rest), dim=1)
        v = S["posed"][f].clone().requires_grad_(True)
        b = bind_gaussians_face_local(v, S["faces"], pc.binding, h._xyz, h._rotation, h._scaling)
        torch.nn.functional.l1_loss(render(S["cams"][f], _RiggedFrame(h, None, b), bg)["render"], gts[f]).backward()
        st.step(S["cams"][f], S["posed"][f], gts[f])
        torch.cuda.synchronize()
        assert (st._graph is not None) == (it == 2)
        rel = _rel(st.d_verts, v.grad)
        print(f"rigged step {it + 1}: rel-L2 {rel:.3e}, max |want| {float(v.grad.abs().max()):.3e}")
        assert float(v.grad.abs().max()) > 0 and rel < 5e-5, (it, rel)
    st.check()


# ------------------------------------------------------------------ 8. the rest of the contract
def test_options_are_refused_where_they_are_not_built_and_defaults_change_nothing(gpu_device):
    import torch
    from fateavatar_amd.avatar import AvatarBatchStep, AvatarStep
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS, MeshTerms
    from fateavatar_amd.splatting import SplattingGaussians, SplattingStep
    from fateavatar_amd.binding import phong_canonical
    from tests import util
    from tests.test_gpu_avatar import _setup, _targets
    dev = gpu_device
    assert REFERENCE_MESH_TERMS == MeshTerms(1e5, 0.0) == MeshTerms()
    S = _setup(dev, 20_000, 128, 4, seed=3)
    bg = torch.ones(3, device=dev)
    gts = _targets(S, dev, bg)
    faces = S["faces"].to(torch.int32).contiguous()
    spc = SplattingGaussians.sample(S["canon"], faces, 2000, torch.Generator().manual_seed(1))
    with pytest.raises(NotImplementedError, match="vertex"):
        SplattingStep(spc, phong_canonical(S["canon"], faces), S["cams"][0].clone(), bg, S["posed"][0], vertex_grad=True)
    with pytest.raises(NotImplementedError, match="vertex_grad"):
        AvatarBatchStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg, views_per_step=2, vertex_grad=True)
    with pytest.raises(NotImplementedError, match="mesh_terms"):
        AvatarBatchStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg, views_per_step=2, mesh_terms=REFERENCE_MESH_TERMS)
    st = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg, mesh_terms=REFERENCE_MESH_TERMS)
    assert st.vertex_grad
    with pytest.raises(ValueError, match="verts_orig"):
        st.step(S["cams"][0], S["posed"][0], gts[0])
    plain = AvatarStep(S["make"](), S["faces"], S["canon"], S["cams"][0].clone(), bg)
    with pytest.raises(ValueError, match="verts_orig"):
        plain.step(S["cams"][0], S["posed"][0], gts[0], verts_orig=S["posed"][0])
    # the option does not touch the Gaussians' update, and the default step has no vertex-gradient buffer at any time
    runs = []
    for vg in (False, True):
        pc = S["make"]()
        s = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), bg, vertex_grad=vg)
        for it in range(12):
            s.step(S["cams"][it % 4], S["posed"][it % 4], gts[it % 4])
            assert (s.d_verts is not None) == vg
        torch.cuda.synchronize()
        s.check()
        assert s._graph is not None and s.mesh_loss is None and s.verts_orig is None
        assert (s._vertex_leaf(s.verts) is s.verts) == (not vg)
        runs.append(pc)
    # (two runs that differ in the order of float atomics only: the tolerance test_fateavatar_step_with_and_without_the_
    # folded_binding holds such a pair to)
    util.assert_same_trajectory(runs[1].flat, runs[0].flat, "vertex_grad on against off", tight=2e-2)
