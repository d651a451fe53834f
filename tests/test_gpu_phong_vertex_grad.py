"""-m gpu: the vertex gradient of SplattingAvatar's Phong-surface binding (model/baseline/splattingavatar.py:203-246) on the
device — the mesh pass's backward alone, the per-Gaussian scatter alone, the two differentiable ops end to end, the folded frame
with a `PosedPhongBinding`, and `SplattingStep(mesh_grad=True)`.

Every comparison is against tests/phong_ref.py in float64 under torch autograd (`mesh_frame` + `phong_bind`, `verts` the leaf;
pinned against central differences by tests/test_phong_vertex_grad_host.py).  The measure is the rel-L2 of
tests/test_gpu_phong.py::_rel per gradient array and the bound is 2e-4, the bound this project holds every binding gradient to
(test_gpu_phong.py:122).  The float32 restatement alone sits at 6.0e-7 (turned mesh) and 1.7 - 1.8e-7 (head template) for
d_verts against float64; every test prints what it achieved.  No row or element is exempted anywhere."""
import numpy as np
import pytest

from tests import phong_ref as P
from tests.test_gpu_phong import _meshes, _rel, _template

pytestmark = pytest.mark.gpu

BOUND = 2e-4


def _mesh(name):
    """(cano_verts, verts, faces) as numpy float32 / int32."""
    if name == "triangle":
        return (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 0.1, 0], [1, 0, 0.2], [0.1, 1, 0]], np.float32),
                np.array([[0, 1, 2]], np.int32))
    cano, verts, faces = _meshes("head_template" if name == "head_template" else "turned")[:3]
    if name == "turned_plus_unused":     # one vertex appended that belongs to no face
        cano = np.concatenate([cano, np.array([[9, 9, 9]], np.float32)])
        verts = np.concatenate([verts, np.array([[8, 8, 8]], np.float32)])
    return cano, verts, faces


def _check(name, got, ref):
    import torch
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()), name
    assert float(ref.abs().max()) > 0, name
    err = _rel(got, ref)
    print(f"{name}: rel-L2 {err:.3e}")
    assert err <= BOUND, (name, err)


# ------------------------------------------------------------------ 1. the mesh pass's backward alone
@pytest.mark.parametrize("mesh", ["turned", "head_template", "triangle", "turned_plus_unused"])
def test_mesh_pass_backward_matches_float64_autograd(gpu_device, mesh):
    """`fr_phong_frame_backward` with random upstream (d_vn, d_vq, d_ratio) against float64 autograd of `mesh_frame`; two calls
    give identical bits, and captured in a graph and replayed twice it gives those bits again; a vertex without a face keeps an
    exactly zero row and everything is finite."""
    import torch
    from fateavatar_amd.binding import phong_canonical, phong_frame_backward, phong_frame_backward_workspace_bytes
    dev = gpu_device
    cano, verts, faces = _mesh(mesh)
    V, F = verts.shape[0], faces.shape[0]
    rng = np.random.default_rng(3)
    ups = [rng.normal(size=s).astype(np.float32) for s in ((V, 3), (V, 4), (F,))]
    t = torch.from_numpy
    v64 = t(verts).double().requires_grad_(True)
    torch.autograd.backward(list(P.mesh_frame(t(cano).double(), t(faces), v64)), [t(u).double() for u in ups])
    c = phong_canonical(t(cano).to(dev), t(faces).to(dev))
    vd, ud = t(verts).to(dev), [t(u).to(dev) for u in ups]
    ws = torch.empty(max(phong_frame_backward_workspace_bytes(V, F), 1), dtype=torch.uint8, device=dev)
    assert phong_frame_backward_workspace_bytes(V, F) == 28 * V

    def call(out):
        out.zero_()
        return phong_frame_backward(c, vd, *ud, out, ws)

    first = call(torch.empty(V, 3, device=dev)).clone()
    second = call(torch.empty(V, 3, device=dev)).clone()
    torch.cuda.synchronize()
    _check(f"{mesh} d_verts", first, v64.grad)
    assert torch.equal(first, second)
    if mesh == "turned_plus_unused":
        assert float(first[-1].abs().max()) == 0.0 and float(v64.grad[-1].abs().max()) == 0.0
    # it ADDS: onto a d_verts that holds something already
    base = t(rng.normal(size=(V, 3)).astype(np.float32)).to(dev)
    added = phong_frame_backward(c, vd, *ud, base.clone(), ws)
    assert torch.equal(added, base + first)
    # upstream gradients that are not given are zeros
    only_n = phong_frame_backward(c, vd, ud[0], None, None, torch.zeros(V, 3, device=dev), ws).clone()
    zeros = phong_frame_backward(c, vd, ud[0], torch.zeros_like(ud[1]), torch.zeros_like(ud[2]), torch.zeros(V, 3, device=dev), ws)
    assert torch.equal(only_n, zeros)
    # captured and replayed
    static = torch.empty(V, 3, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(static)
    for _ in range(2):
        static.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, first)


# ------------------------------------------------------------------ 2. the per-Gaussian scatter alone
@pytest.mark.parametrize("case", ["turned", "one_face"])
def test_scatter_matches_float64_autograd(gpu_device, case):
    """`fr_bind_backward_phong_frame` against float64 autograd of `phong_bind` with the frame arrays as independent leaves: the
    turned mesh's 5 000 Gaussians (no multiple of 64), and 4 096 Gaussians all on face 0 (every add hits the same addresses);
    with every upstream gradient NULL the outputs stay zero; each output NULL in turn leaves the others within the bound."""
    import torch
    from fateavatar_amd.binding import phong_canonical, phong_frame, phong_scatter_frame_grads
    dev = gpu_device
    cano, verts, faces, fi, bary, _ = _meshes("turned")
    rng = np.random.default_rng(11)
    if case == "one_face":
        N = 4096
        fi = np.zeros(N, np.int32)
        _, b = P.sample_bary_on_triangles(1, N, torch.Generator().manual_seed(3))
        bary = b.numpy()
    N, V, F = fi.shape[0], verts.shape[0], faces.shape[0]
    assert N % 64 != 0 or case == "one_face"
    uvd = (0.05 * rng.normal(size=(N, 3))).astype(np.float32)
    rot = rng.normal(size=(N, 4)).astype(np.float32)
    scl = rng.normal(size=(N, 3)).astype(np.float32)
    w = [rng.normal(size=s).astype(np.float32) for s in ((N, 3), (N, 4), (N, 3))]
    t = torch.from_numpy
    d = lambda a: t(a).double()  # noqa: E731
    # ---- reference: verts and the three frame arrays as four independent float64 leaves
    v64 = d(verts).requires_grad_(True)
    frame64 = [x.detach().requires_grad_(True) for x in P.mesh_frame(d(cano), t(faces), d(verts))]
    out = P.phong_bind(v64, t(faces), t(fi), d(bary), frame64, d(uvd), d(rot), d(scl))
    torch.autograd.backward(list(out), [d(a) for a in w])
    ref = [v64.grad, *[x.grad for x in frame64]]
    # ---- device
    vd, fd = t(verts).to(dev), t(faces).to(dev)
    frame = phong_frame(phong_canonical(t(cano).to(dev), fd), vd)
    args = (vd, fd, t(fi).to(dev), t(bary).to(dev), frame, t(uvd).to(dev), t(rot).to(dev), t(scl).to(dev))
    wd = [t(a).to(dev) for a in w]
    shapes = ((V, 3), (V, 3), (V, 4), (F,))
    names = ("d_verts", "d_vert_normals", "d_vert_quats", "d_face_ratio")
    outs = [torch.zeros(s, device=dev) for s in shapes]
    phong_scatter_frame_grads(*args, *wd, *outs)
    torch.cuda.synchronize()
    for n, g, r in zip(names, outs, ref):
        _check(f"{case} {n}", g, r)
    # all upstream gradients NULL: nothing is added
    outs = [torch.zeros(s, device=dev) for s in shapes]
    phong_scatter_frame_grads(*args, None, None, None, *outs)
    torch.cuda.synchronize()
    assert all(float(o.abs().max()) == 0.0 for o in outs)
    # one upstream gradient at a time: the sum of the three is the whole
    parts = []
    for k in range(3):
        outs = [torch.zeros(s, device=dev) for s in shapes]
        phong_scatter_frame_grads(*args, *[wd[j] if j == k else None for j in range(3)], *outs)
        parts.append(outs)
    for i, (n, r) in enumerate(zip(names, ref)):
        _check(f"{case} {n} from one upstream array at a time", sum(p[i].double() for p in parts), r)
    # each output NULL in turn
    for skip in range(4):
        outs = [None if i == skip else torch.zeros(s, device=dev) for i, s in enumerate(shapes)]
        phong_scatter_frame_grads(*args, *wd, *outs)
        torch.cuda.synchronize()
        for i, (n, r) in enumerate(zip(names, ref)):
            if i != skip:
                _check(f"{case} {n} without {names[skip]}", outs[i], r)


# ------------------------------------------------------------------ 3. the two ops end to end
@pytest.mark.parametrize("mesh", ["head_template", "turned"])
def test_differentiable_ops_end_to_end(gpu_device, mesh):
    """`phong_frame(differentiable=True)` -> `bind_gaussians_phong` -> backward at the sizes of test_gpu_phong.py::_meshes:
    verts.grad within the bound of float64 autograd; the gradients of uvd / rotation / scaling are the detached call's bits;
    the default `phong_frame` is today's function and its outputs are detached."""
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
    d = lambda a: t(a).double()  # noqa: E731
    v64 = d(verts).requires_grad_(True)
    out = P.phong_bind(v64, t(faces), t(fi), d(bary), P.mesh_frame(d(cano), t(faces), v64), d(uvd), d(rot), d(scl))
    torch.autograd.backward(list(out), [d(a) for a in w])
    c = phong_canonical(t(cano).to(dev), t(faces).to(dev))

    def run(differentiable):
        x = [t(a).to(dev).requires_grad_(True) for a in (uvd, rot, scl)]
        v = t(verts).to(dev).requires_grad_(differentiable)
        frame = phong_frame(c, v, differentiable=differentiable)
        assert all(f.requires_grad == differentiable for f in frame)
        o = bind_gaussians_phong(v, t(faces).to(dev), t(fi).to(dev), t(bary).to(dev), frame, *x)
        torch.autograd.backward(list(o), [t(a).to(dev) for a in w])
        torch.cuda.synchronize()
        return [a.detach() for a in o], [a.grad for a in x], v.grad, [f.detach() for f in frame]

    o_d, g_d, gv, f_d = run(True)
    o_p, g_p, none, f_p = run(False)
    assert none is None
    _check(f"{mesh} verts.grad", gv, v64.grad)
    for a, b in zip(o_d + g_d + f_d, o_p + g_p + f_p):
        assert torch.equal(a, b)
    assert float(g_d[0][:, :2].abs().max()) == 0.0
    # a default call is positional-compatible and detached even for a leaf that requires grad
    again = phong_frame(c, t(verts).to(dev).requires_grad_(True))
    assert all(not f.requires_grad and torch.equal(f, g) for f, g in zip(again, f_p))
    # with a detached frame a `verts` that requires grad is refused exactly as before
    with pytest.raises(RuntimeError, match="no vertex gradient"):
        bind_gaussians_phong(t(verts).to(dev).requires_grad_(True), t(faces).to(dev), t(fi).to(dev), t(bary).to(dev), f_p,
                             *[t(a).to(dev) for a in (uvd, rot, scl)])


# ------------------------------------------------------------------ 4. the folded frame
def _small_avatar(S, dev, N, seed, single_pixel=False):
    """N Gaussians on the canonical template without the k-NN initialisation: off the surface, anisotropic rotated splats large
    enough to cover a 64 x 64 head, coloured, opacity 0.6.  `single_pixel`: the scenes of tests/test_gpu_camera_grad.py's
    bit-for-bit checks instead — log-scale -9 and opacity 0.005, an alpha >= 1/255 footprint of less than half a pixel: every
    Gaussian reaches at most one pixel, so the blend backward's float atomics add once per Gaussian and the whole backward is
    deterministic (three Adam steps at the reference's rates keep the opacity below 0.0058)."""
    import torch
    from fateavatar_amd.splatting import SplattingGaussians, sample_bary_on_triangles
    g = torch.Generator().manual_seed(seed)
    fidx, bary = sample_bary_on_triangles(S["F"], N, g)
    pc = SplattingGaussians(fidx, bary, float(np.log(0.012)), dev)
    with torch.no_grad():
        pc._uvd.copy_((0.01 * torch.randn(N, 3, generator=g)).to(dev))
        pc._scaling.add_((0.3 * torch.randn(N, 3, generator=g)).to(dev))
        pc._rotation.add_((0.5 * torch.randn(N, 4, generator=g)).to(dev))
        pc._features_dc.copy_((torch.rand(N, 1, 3, generator=g) * 2.0 - 1.0).to(dev))
        pc._opacity.fill_(float(np.log(0.6 / 0.4)))
        if single_pixel:
            pc._scaling.fill_(-9.0)
            pc._opacity.fill_(float(np.log(0.0050 / 0.9950)))
    return pc


@pytest.mark.parametrize("scene", ["single_pixel", "covering"])
def test_posed_phong_binding_returns_the_vertex_gradient(gpu_device, scene):
    """`render_bound_batch` with a `PosedPhongBinding`: 64 x 64, 2 000 Gaussians, K = 3 views of which two share one posed mesh.
    Images and the `bound` triple are `PhongBinding`'s bits, and so is every parameter gradient on the single-pixel scene (where
    the blend backward adds once per Gaussian: `_small_avatar`); on the covering scene, whose Gaussians reach many tiles, two
    runs of the SAME frame differ in the last bits of those sums, and the parameter gradients are held to the 5e-5 rel-L2 of
    test_gpu_phong.py's test 3.  dLoss/dverts of both meshes is within the bound of the unfolded route (differentiable ops in
    front of render()) and of the CPU route of test_gpu_phong.py's test 4 (float32 restatement -> activations -> oracle) with
    `verts` as one more leaf.  Pixels on which the device and the oracle disagree beyond test 4's image tolerance (threshold
    flips) are masked out of dL/dpixel on every route."""
    import torch
    from fateavatar_amd.binding import bind_gaussians_phong, phong_frame
    from fateavatar_amd.bound import PhongBinding, PosedPhongBinding, render_bound_batch
    from fateavatar_amd.render import render_batch
    from fateavatar_amd.splatting import _SplattingFrame
    from oracle import oracle
    dev = gpu_device
    res, N, K = 64, 2000, 3
    S = _template(dev, res, 4, seed=1)
    pc = _small_avatar(S, dev, N, seed=6, single_pixel=scene == "single_pixel")
    names = [n for n, _ in pc.FIELDS if n != "_features_rest"]
    bg_np = np.array([0.2, 0.5, 0.9], np.float32)
    bg = torch.from_numpy(bg_np).to(dev)
    view_mesh, view_cam = [1, 1, 3], [1, 2, 3]          # views 0 and 1 share the posed mesh of frame 1
    cams = [S["cams"][k] for k in view_cam]
    faces_c, cano_c = S["faces"].cpu(), S["posed"][0].cpu()
    t = torch.from_numpy

    # ---- the CPU route, forward: restatement (float32) -> activations -> oracle, per view
    ref = {n: getattr(pc, n).detach().cpu().clone().requires_grad_(True) for n in names}
    ref_verts = {m: S["posed"][m].cpu().clone().requires_grad_(True) for m in set(view_mesh)}
    npy = lambda x: np.ascontiguousarray(x.detach().numpy())  # noqa: E731
    cpu_views = []
    for m, ci in zip(view_mesh, view_cam):
        c = S["cam_arrays"][ci]
        xyz, rot_b, scl_b = P.phong_bind(ref_verts[m], faces_c, pc.face_index.cpu(), pc.bary_coords.cpu(),
                                         P.mesh_frame(cano_c, faces_c, ref_verts[m]), ref["_uvd"], ref["_rotation"], ref["_scaling"])
        act = [xyz, torch.exp(scl_b), torch.nn.functional.normalize(rot_b), torch.sigmoid(ref["_opacity"]), ref["_features_dc"]]
        o = oracle.forward(bg=bg_np, means3D=npy(act[0]), opacities=npy(act[3]), viewmatrix=c.world_view_transform,
                           projmatrix=c.full_proj_transform, campos=c.camera_center, tanfovx=c.tanfovx, tanfovy=c.tanfovy, H=res,
                           W=res, shs=npy(act[4]), sh_degree=0, scales=npy(act[1]), rotations=npy(act[2]))
        assert int((o.radii > 0).sum()) > 500
        cpu_views.append((o, act))

    def run(binding_cls, leaves_require_grad, dpix=None):
        """The folded frame; dpix None: images only."""
        for n in names:
            getattr(pc, n).grad = None
        leaves = {m: S["posed"][m].clone().requires_grad_(leaves_require_grad) for m in set(view_mesh)}
        outs = render_bound_batch(cams, [_SplattingFrame(pc, None)] * K, [leaves[m] for m in view_mesh],
                                  binding_cls(S["faces"], pc.face_index, pc.bary_coords, S["canonical"]), bg)
        if dpix is not None:
            torch.autograd.backward([o["render"] for o in outs], dpix)
        torch.cuda.synchronize()
        return outs, {n: getattr(pc, n).grad.clone() for n in names} if dpix is not None else None, leaves

    with torch.no_grad():
        plain_fwd, _, _ = run(PhongBinding, False)
    rng = np.random.default_rng(11)
    dpix = []
    for k, (o, _) in enumerate(cpu_views):
        col = plain_fwd[k]["render"].cpu().numpy()
        bad = (np.abs(col - o.color) > 1e-5 + 1e-4 * np.abs(o.color)).any(0)
        print(f"view {k}: {int(bad.sum())} pixel(s) masked, {int((o.radii > 0).sum())} Gaussians visible")
        assert bad.mean() < 0.01
        g = (rng.uniform(-1, 1, (3, res, res)) / (res * res)).astype(np.float32)
        g[:, bad] = 0.0
        dpix.append(g)
    dpix_d = [t(g).to(dev) for g in dpix]

    # ---- PhongBinding (detached verts) against PosedPhongBinding (leaves)
    o_plain, g_plain, _ = run(PhongBinding, False, dpix_d)
    o_posed, g_posed, leaves = run(PosedPhongBinding, True, dpix_d)
    for k in range(K):
        assert torch.equal(o_posed[k]["render"], o_plain[k]["render"]) and torch.equal(o_posed[k]["radii"], o_plain[k]["radii"])
        for a, b in zip(o_posed[k]["bound"], o_plain[k]["bound"]):
            assert torch.equal(a, b) and not a.requires_grad
    for n in names:
        assert float(g_plain[n].abs().max()) > 0, n
        if scene == "single_pixel":
            assert torch.equal(g_posed[n], g_plain[n]), n
        else:
            assert _rel(g_posed[n], g_plain[n]) < 5e-5, n
    got = {m: leaves[m].grad.clone() for m in leaves}
    assert all(g is not None and g.shape == S["posed"][0].shape for g in got.values())
    # under no_grad, and with vertices that do not require grad, it is PhongBinding
    o_same, g_same, _ = run(PosedPhongBinding, False, dpix_d)
    for n in names:
        assert torch.equal(g_same[n], g_plain[n]) if scene == "single_pixel" else _rel(g_same[n], g_plain[n]) < 5e-5, n

    # ---- the unfolded route: the differentiable ops in front of render()
    for n in names:
        getattr(pc, n).grad = None
    un = {m: S["posed"][m].clone().requires_grad_(True) for m in leaves}
    frames_of = {m: phong_frame(S["canonical"], un[m], differentiable=True) for m in un}
    frames = []
    for m in view_mesh:
        b = bind_gaussians_phong(un[m], S["faces"], pc.face_index, pc.bary_coords, frames_of[m], pc._uvd, pc._rotation, pc._scaling)
        frames.append(_SplattingFrame(pc, None, b))
    outs = render_batch(cams, frames, bg)
    torch.autograd.backward([o["render"] for o in outs], dpix_d)
    torch.cuda.synchronize()
    for m in sorted(un):
        _check(f"mesh of frame {m}: folded d_verts against the unfolded route", got[m], un[m].grad)

    # ---- the CPU route, backward
    heads, grads = [], []
    for (o, act), g in zip(cpu_views, dpix):
        ob = oracle.backward(o, g)
        heads += act
        grads += [t(ob.dL_dmeans3D), t(ob.dL_dscales), t(ob.dL_drotations), t(ob.dL_dopacity).reshape(-1, 1), t(ob.dL_dsh)]
    torch.autograd.backward(heads, grads)
    for m in sorted(ref_verts):
        _check(f"mesh of frame {m}: folded d_verts against the CPU oracle route", got[m], ref_verts[m].grad)
    assert _rel(got[1], got[3]) > 1e-2              # two meshes, two gradients


# ------------------------------------------------------------------ 5. the step
def test_splatting_step_mesh_grad(gpu_device):
    """`SplattingStep(mesh_grad=True)`, 64 x 64, 2 000 single-pixel Gaussians (`_small_avatar`: the step's backward is
    deterministic there), three steps over three different poses: parameters and both Adam moments are the bits of a
    `SplattingStep()` without it; `d_verts` differs from step to step, is one preallocated
    buffer, agrees between the replayed graph and the eager step and between `fold_binding` True and False within the bound;
    `vertex_grad=True` still raises and names `mesh_grad`."""
    import torch
    from fateavatar_amd.splatting import SplattingStep
    dev = gpu_device
    res, N, steps = 64, 2000, 3
    S = _template(dev, res, 4, seed=2)
    bg = torch.ones(3, device=dev)
    gts = [torch.rand(3, res, res, generator=torch.Generator().manual_seed(20 + k)).to(dev) for k in range(steps)]

    def run(**kw):
        pc = _small_avatar(S, dev, N, seed=8, single_pixel=True)
        st = SplattingStep(pc, S["canonical"], S["cams"][0].clone(), bg, S["posed"][0], **kw)
        ptr = st.d_verts.data_ptr() if st.mesh_grad else None
        grads = []
        for it in range(steps):
            verts = S["posed"][it + 1].clone().requires_grad_(st.mesh_grad)     # (a mesh that hangs on autograd, as a caller's would)
            st.step(S["cams"][it + 1], verts, gts[it])
            torch.cuda.synchronize()
            if st.mesh_grad:
                assert st.d_verts.data_ptr() == ptr and st.d_verts.shape == verts.shape and not st.verts.requires_grad
                grads.append(st.d_verts.clone())
        st.check()
        return pc, st, grads

    pc_0, st_0, _ = run(use_graph=False)
    pc_e, st_e, g_e = run(use_graph=False, mesh_grad=True)
    pc_g, st_g, g_g = run(use_graph=True, mesh_grad=True)
    pc_u, st_u, g_u = run(use_graph=False, mesh_grad=True, fold_binding=False)
    assert st_0.d_verts is None and not st_0.mesh_grad
    assert st_g._graph is not None and st_e._graph is None, "step 3 of the third run is a graph replay"
    assert torch.equal(pc_e.flat, pc_0.flat), "mesh_grad changes no parameter"
    assert torch.equal(st_e.adam.exp_avg, st_0.adam.exp_avg) and torch.equal(st_e.adam.exp_avg_sq, st_0.adam.exp_avg_sq)
    assert float((pc_0.flat - _small_avatar(S, dev, N, seed=8, single_pixel=True).flat).abs().max()) > 0
    for it in range(steps):
        assert bool(torch.isfinite(g_e[it]).all()) and float(g_e[it].abs().max()) > 0
        _check(f"step {it}: d_verts, graph against eager", g_g[it], g_e[it])
        _check(f"step {it}: d_verts, stand-alone ops against the folded binding", g_u[it], g_e[it])
    assert _rel(g_e[1], g_e[0]) > 1e-2 and _rel(g_e[2], g_e[1]) > 1e-2
    with pytest.raises(NotImplementedError, match="mesh_grad"):
        SplattingStep(_small_avatar(S, dev, 16, seed=1), S["canonical"], S["cams"][0].clone(), bg, S["posed"][0], vertex_grad=True)
