"""-m gpu: FateAvatar's WHOLE step as one step — AvatarStep(flame=, mesh_terms=, perceptual=, camera_grad=True): FLAME forward
(both meshes) -> the bound frame -> L1 -> the VGG term -> the rasterizer's backward with vertex and camera gradients -> the mesh
terms -> FLAME backward -> the Gaussians' Adam -> the mesh's Adam.  tests/test_gpu_flame.py runs the step with FLAME and the
mesh terms, tests/test_gpu_vgg_step.py with the perceptual term, tests/test_gpu_camera_grad.py with camera gradients; here all
of them share one captured body, and the point set is resized while the mesh's optimizer is alive.

The scene is tests/test_gpu_flame._step_setup (2 000 Gaussians on the head template, 128 x 128, a synthetic FLAME with
n_exp = 10); the perceptual term is built as in tests/test_gpu_vgg_step.py (VGG-16's widths, seeded weights, both images
resized to 24 x 24, weight 0.1)."""
import pytest

from tests import vgg_ref
from tests.test_gpu_flame import CEILING, FACTOR, _posed, _rel, _step_setup

pytestmark = pytest.mark.gpu

SIZE, FRAMES = (24, 24), 5


def _perceptual(dev):
    from fateavatar_amd.perceptual import Perceptual, VggFeatures
    W, B = vgg_ref.he_weights(vgg_ref.VGG16, seed=21)
    return Perceptual(VggFeatures(vgg_ref.VGG16, W, B, size=SIZE, device=dev), weight=0.1)


def _full_step(S, fm, use_graph, **kw):
    from fateavatar_amd.avatar import AvatarStep
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS
    pc = S["make"]()
    st = AvatarStep(pc, S["faces"], S["canon"], S["cams"][0].clone(), S["bg"], use_graph=use_graph, mesh_terms=REFERENCE_MESH_TERMS,
                    flame=fm, perceptual=_perceptual(S["dev"]), camera_grad=True, **kw)
    return pc, st


def _second_mesh(S, fm_state, frame):
    """(FlameMesh, verts, verts_orig): another FlameMesh with the deltas `fm_state`, posed for `frame` by its own launches."""
    import torch
    fm2 = S["model"]()
    fm2.load_state_dict(fm_state)
    v, vo = torch.full((fm2.V, 3), float("nan"), device=S["dev"]), torch.full((fm2.V, 3), float("nan"), device=S["dev"])
    fm2.forward_into(frame.expression, frame.pose, v, vo)
    return fm2, v, vo


def test_one_eager_step_is_its_stages_run_alone(gpu_device):
    """ONE eager step against its own stages run alone on the step's buffers."""
    import torch
    from fateavatar_amd.loss import REFERENCE_MESH_TERMS, l1_loss_and_grad, mesh_terms_and_grad, mesh_terms_workspace
    S = _step_setup(6)
    dev, f = S["dev"], 1
    frame, cam, gt = S["frames"][f], S["cams"][f], S["gts"][f]
    fm = S["model"]()
    before = fm.state_dict()
    pc, st = _full_step(S, fm, use_graph=False)
    loss = st.step(cam, frame, gt)
    torch.cuda.synchronize()
    st.check()
    assert st.overflows == 0 and st.flame_adam.step_count == 1 == st.adam.step_count
    # ---- FLAME forward: a second FlameMesh with the deltas the step started from
    fm2, v2, vo2 = _second_mesh(S, before, frame)
    assert torch.equal(st.verts, v2) and torch.equal(st.verts_orig, vo2) and not torch.equal(v2, vo2)
    # ---- the image terms on the step's render
    render = st.out["render"]
    l1, g_l1 = l1_loss_and_grad(render, gt)
    terms, g_p = _perceptual(dev).loss_and_grad(render, gt)                  # (a second Perceptual: its own workspace)
    assert torch.equal(loss, l1) and torch.equal(st.loss, l1) and float(l1) > 0
    assert torch.equal(st.perceptual_loss, terms) and float(terms[0]) > 0
    assert float(g_p.abs().max()) > 0 and float(g_l1.abs().max()) > 0
    assert torch.allclose(st._dimage, g_l1 + g_p, rtol=1e-6, atol=0) and not torch.equal(st._dimage, g_l1)
    # ---- the mesh terms on the step's two meshes
    alone = mesh_terms_and_grad(st.verts, st.verts_orig, st.laplacian, REFERENCE_MESH_TERMS, d_verts=torch.zeros_like(st.d_verts),
                                workspace=mesh_terms_workspace(dev))
    assert torch.equal(st.mesh_loss, alone) and float(alone[0]) > 0
    # ---- FLAME backward from the step's d_verts: the second FlameMesh, bit for bit, and float64 autograd of the restatement
    d_e, d_p = torch.full((fm.n_exp,), float("nan"), device=dev), torch.full((15,), float("nan"), device=dev)
    fm2.flat_grad.fill_(float("nan"))
    fm2.backward_from(st.d_verts, frame.expression, frame.pose, d_e, d_p)
    torch.cuda.synchronize()
    assert float(st.d_verts.abs().max()) > 0 and bool(torch.isfinite(st.d_verts).all())
    assert torch.equal(fm.flat_grad, fm2.flat_grad) and torch.equal(st.d_expression, d_e) and torch.equal(st.d_pose, d_p)
    leaves = [before[k].double().clone().requires_grad_(True) for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex")] + \
             [frame.expression.double().clone().requires_grad_(True), frame.pose.double().clone().requires_grad_(True)]
    posed, _ = _posed(fm2, frame, torch.float64, leaves)
    assert _rel(st.verts, posed.detach()) <= 1e-6
    posed.backward(st.d_verts.double())
    ns = fm.n_shape
    assert int(leaves[0].grad[:, :, :ns].count_nonzero()) == 0
    want_flat = torch.cat([leaves[0].grad[:, :, ns:].reshape(-1), leaves[1].grad.reshape(-1), leaves[2].grad.reshape(-1)])
    for name, got, ref in (("flat_grad", fm.flat_grad, want_flat), ("d_expression", st.d_expression, leaves[3].grad),
                           ("d_pose", st.d_pose, leaves[4].grad)):
        err = _rel(got, ref)
        print(f"whole step against float64 autograd fed the step's d_verts, {name}: rel-L2 {err:.3e}")
        assert float(ref.abs().max()) > 0 and bool(torch.isfinite(got).all()) and err <= CEILING, (name, err)
    # ---- the camera gradients of the same backward.  (FateAvatar renders SH degree 0 — AvatarGaussians.max_sh_degree — and the
    # camera centre enters a frame through the SH view direction alone: d_campos is exactly zero, not merely small)
    for name in ("d_view", "d_proj"):
        t = getattr(st, name)
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, name
    assert tuple(st.d_campos.shape) == (3,) and int(st.d_campos.count_nonzero()) == 0 and pc.max_sh_degree == 0
    # (the mesh's Adam ran behind all of it)
    assert not torch.equal(fm.flat.detach(), torch.cat([before["delta_shapedirs"][:, :, ns:].reshape(-1),
                                                        before["delta_posedirs"].reshape(-1), before["delta_vertex"].reshape(-1)]))


EXACT = ("loss", "perceptual_loss", "_dimage", "verts", "verts_orig", "mesh_loss")
ATOMIC = ("d_verts", "flat_grad", "d_expression", "d_pose")       # behind the rasterizer's float-atomic sums


def _five_steps(S, use_graph):
    """Five steps over five frames with every parameter held bitwise in place: rate 0 for the Gaussians; the mesh's segments
    refuse 0, so 1e-30 (an update of at most 1e-30 against deltas of 1e-4 and more).  Per step, copies of what the step holds."""
    import torch
    from fateavatar_amd.avatar import FATE_LRS
    from fateavatar_amd.flame import REFERENCE_FLAME_LRS
    fm = S["model"]()
    with torch.no_grad():
        # (the scene's seeded deltas hold a couple of EXACT zeros, which an update of 1e-30 would move: they start at 1e-12 here,
        # in every run alike — seven orders below the deltas' scale — so that "in place" can be asserted of every entry)
        fm.flat[fm.flat == 0] = 1e-12
    flat0 = fm.flat.detach().clone()
    pc, st = _full_step(S, fm, use_graph, lrs={k: 0.0 for k in FATE_LRS}, flame_lrs={k: 1e-30 for k in REFERENCE_FLAME_LRS})
    pc0 = pc.flat.detach().clone()
    kept = []
    for f in range(FRAMES):
        st.step(S["cams"][f], S["frames"][f], S["gts"][f])
        row = {n: getattr(st, n).clone() for n in EXACT + ATOMIC[:1] + ATOMIC[2:]}
        row["flat_grad"] = fm.flat_grad.clone()
        kept.append(row)
    torch.cuda.synchronize()
    st.check()
    assert int(flat0.count_nonzero()) == flat0.numel()
    assert torch.equal(fm.flat.detach(), flat0) and torch.equal(pc.flat.detach(), pc0)
    assert st.overflows == 0 and st.flame_adam.step_count == FRAMES == st.adam.step_count
    return st, kept


def test_two_eager_and_three_replayed_steps_are_five_eager_steps(gpu_device):
    """What lies in front of the rasterizer's backward, and the meshes and their terms, bit for bit; what lies behind its atomic
    sums within FACTOR x what two EAGER runs of the same steps show against each other (another order of the same float32 sums),
    measured here on three eager runs, and never above CEILING."""
    import torch
    S = _step_setup(6)
    st_a, a = _five_steps(S, False)
    st_b, b = _five_steps(S, False)
    st_c, c = _five_steps(S, False)
    st_g, g = _five_steps(S, True)
    assert st_g._graph is not None and st_a._graph is None and st_g._eager_steps == 2 and st_g.overflows == 0
    for k in range(FRAMES):
        for n in EXACT:
            assert torch.equal(g[k][n], a[k][n]) and torch.equal(b[k][n], a[k][n]) and torch.equal(c[k][n], a[k][n]), (k, n)
        assert float(a[k]["perceptual_loss"][0]) > 0 and float(a[k]["mesh_loss"][0]) > 0
    assert len({float(r["loss"]) for r in a}) == FRAMES                          # five different frames
    for n in ATOMIC:
        # (three eager runs, the largest difference any two of them show on any step: one pair of runs is one draw)
        noise = max(_rel(x[k][n], y[k][n]) for x, y in ((b, a), (c, a), (c, b)) for k in range(FRAMES))
        err = max(_rel(g[k][n], a[k][n]) for k in range(FRAMES))
        print(f"{n}: graph against eager rel-L2 {err:.3e}; eager against eager {noise:.3e} (allowed: {FACTOR:g} x that, at most {CEILING:g})")
        assert all(float(r[n].abs().max()) > 0 and bool(torch.isfinite(r[n]).all()) for r in g), n
        assert err <= min(FACTOR * noise, CEILING), (n, err, noise)


def test_resizes_keep_the_live_mesh_optimizer(gpu_device):
    """Six captured steps at the reference's rates, a densification and a prune, six more: the mesh's Adam is made once and goes
    on (AvatarStep._make_adam / _buffers_moved) while the Gaussians' is remapped."""
    import torch
    S = _step_setup(6)
    dev = S["dev"]
    fm = S["model"]()
    pc, st = _full_step(S, fm, use_graph=True)
    for it in range(6):
        st.step(S["cams"][it % 6], S["frames"][it % 6], S["gts"][it % 6])
    torch.cuda.synchronize()
    st.check()
    assert st._graph is not None and st.overflows == 0
    adam = st.flame_adam
    applied = st.host_steps - st.skipped_steps
    assert st.host_steps == 6 and adam.step_count == applied == st.adam.step_count
    m, v, flat = adam.exp_avg.clone(), adam.exp_avg_sq.clone(), fm.flat.detach().clone()
    assert float(m.abs().max()) > 0 and float(v.abs().max()) > 0
    P0 = pc.P
    assert st.uv_densify(200, torch.Generator(device=dev).manual_seed(8)) == 200
    with torch.no_grad():
        pc._opacity[:37] = -20.0                                                 # (something for the prune to take)
    pruned = st.prune_low_opacity()
    torch.cuda.synchronize()
    assert pruned >= 37 and st.pc.P == P0 + 200 - pruned
    assert st.flame_adam is adam and adam.param.data_ptr() == fm.flat.data_ptr() and adam.grad.data_ptr() == fm.flat_grad.data_ptr()
    assert torch.equal(adam.exp_avg, m) and torch.equal(adam.exp_avg_sq, v) and torch.equal(fm.flat.detach(), flat)
    assert adam.step_count == applied == st.adam.step_count == st.host_steps - st.skipped_steps
    for it in range(6, 11):
        st.step(S["cams"][it % 6], S["frames"][it % 6], S["gts"][it % 6])
    torch.cuda.synchronize()
    before = fm.state_dict()
    flat_before = fm.flat.detach().clone()
    st.step(S["cams"][5], S["frames"][5], S["gts"][5])
    torch.cuda.synchronize()
    st.check()
    assert st._graph is not None and st.overflows == 0 and st.flame_adam is adam
    assert st.host_steps == 12 and adam.step_count == st.adam.step_count == st.host_steps - st.skipped_steps
    _, v2, vo2 = _second_mesh(S, before, S["frames"][5])
    assert torch.equal(st.verts, v2) and torch.equal(st.verts_orig, vo2)
    assert float((fm.flat.detach() - flat_before).abs().max()) > 0 and float((flat_before - flat).abs().max()) > 0
    assert not torch.equal(adam.exp_avg, m)
