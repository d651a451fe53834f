"""GPU: `bake.BakeStep`, neural baking's step (fateavatar_amd/bake.py) on the head template: 676 points of the template's
26 x 26 UV raster (+ 64 template points where the binding is extended), a 24 x 40 texture, a 64 x 48 image.

Bit-for-bit checks run on a SINGLE-PIXEL scene (tests/test_gpu_camera_grad.py says why: the blend backward sums a
Gaussian's tiles with float atomics, so only a Gaussian that reaches one pixel has an order-free gradient): the prior
log-scales are about -9 and the opacity map about logit(0.005), so every splat's alpha >= 1 / 255 footprint has a radius below
half a pixel.  The convergence, overflow and export checks run on a VISIBLE scene (opacities about 0.5, the template's own
knn scale)."""
import math

import numpy as np
import pytest

from tests import bake_ref as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
TEX_H, TEX_W = 24, 40
IMG_H, IMG_W = 48, 64
ALL = ("color", "opacity", "scaling", "rotation", "offset")
SCALE_TERM = (0.1, 1.5)      # the reference's weight; a threshold the decoded scales (ratios up to e) actually cross


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch, gpu_device):
    """Without a device every test skips (gpu_device); every test starts from an empty binning-capacity guess."""
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


def _uniform(gen, *shape):
    import torch
    return torch.rand(*shape, generator=gen) * 2 - 1


def _setup(dev, single_pixel, template_points=64):
    """The baked avatar (its plan re-made for a 24 x 40 texture), the mesh, a 64 x 48 camera in front of the head."""
    import torch
    from fateavatar_amd import scenes, texture
    from fateavatar_amd.avatar import AvatarGaussians
    from fateavatar_amd.baked import BakedAvatar
    from fateavatar_amd.model import TorchCamera
    verts, faces, _ = scenes.head_geometry()
    pc = AvatarGaussians.from_template(dev, uv_resolution=26)
    assert pc.P == 676
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        pc._features_dc.copy_(_uniform(gen, pc.P, 1, 3).to(dev))
        pc._opacity.fill_(0.0)
        pc._rotation.copy_((_uniform(gen, pc.P, 4) + torch.tensor([2.0, 0, 0, 0])).to(dev))
        if single_pixel:
            pc._scaling.copy_((-9.0 + 0.1 * _uniform(gen, pc.P, 3)).to(dev))
        else:
            pc._scaling.add_((_uniform(gen, pc.P, 3) * 0.3).to(dev))
    baked = BakedAvatar(pc, tex_size=32, template_points=template_points, rng=np.random.default_rng(3))
    baked.plan = texture.TexturePlan(baked.plan.uv, TEX_H, TEX_W)
    canon = torch.from_numpy(verts).to(dev)
    centre = verts.mean(0).astype(np.float64)
    cam = TorchCamera(scenes.look_at_camera(centre + np.array([0.0, 0.0, 1.0]), centre, (0, 1, 0), 2 * math.atan(0.2 * IMG_W / IMG_H),
                                            2 * math.atan(0.2), IMG_H, IMG_W), dev)
    posed = canon + torch.tensor([0.004, -0.003, 0.002], device=dev)            # (any pose: a small rigid shift)
    bg = torch.ones(3, device=dev)
    gt = torch.rand(3, IMG_H, IMG_W, generator=torch.Generator().manual_seed(2)).to(dev)
    return dict(baked=baked, pc=pc, faces=torch.from_numpy(faces).to(dev), canon=canon, cam=cam, posed=posed, bg=bg, gt=gt, dev=dev)


def _texture(seed, single_pixel, dev):
    import torch
    t = _uniform(torch.Generator().manual_seed(seed), 1, 11, TEX_H, TEX_W)
    if single_pixel:
        t[:, 3:4] = math.log(0.005 / 0.995) + 0.05 * t[:, 3:4]                 # opacities 0.0048 .. 0.0053
    return t.to(dev)


def _make(S, **kw):
    from fateavatar_amd.bake import BakeStep
    from fateavatar_amd.loss import ScaleRatioTerm
    kw.setdefault("scale_term", ScaleRatioTerm(*SCALE_TERM))
    return BakeStep(S["baked"], S["faces"], S["canon"], S["cam"].clone(), S["bg"], **kw)


def _eager_composition(S, tex, bake=ALL, rot_weight=0.1, scale_term=SCALE_TERM):
    """The step's body as separate eager calls, in its order: decode, the frame, L1, the frame's backward, the terms on the
    decoded rows, decode backward.  -> (d_tex_out, loss, rot_loss, reg_loss, image)."""
    import torch
    from fateavatar_amd import texture
    from fateavatar_amd.bound import render_bound_batch
    from fateavatar_amd.loss import ScaleRatioTerm, l1_loss_and_grad, rot_term_and_grad, scale_ratio_term_and_grad
    baked = S["baked"]
    leaf = tex.clone().requires_grad_(True)
    _, values = texture.decode_attributes(leaf, baked.plan, baked.mean_scaling, baked.max_scaling)
    rows = {n: v.detach().requires_grad_(True) for n, v in values.items()}
    st = _make(S, use_graph=False)              # (its binding: the same MeshBinding the step renders through)
    out = render_bound_batch([S["cam"]], [baked._frame(rows, bake)], [S["posed"]], st.binding, S["bg"])[0]
    loss, g = l1_loss_and_grad(out["render"], S["gt"])
    out["render"].backward(g)
    d = {n: r.grad for n, r in rows.items()}
    for n in ("rotation", "scaling"):
        if d[n] is None:
            d[n] = torch.zeros_like(rows[n])
    rot_loss = rot_term_and_grad(values["rotation"].detach(), d["rotation"], weight=rot_weight)
    reg_loss = scale_ratio_term_and_grad(values["scaling"].detach(), d["scaling"], terms=ScaleRatioTerm(*scale_term))
    present = [n for n in R.NAMES if d[n] is not None]
    torch.autograd.backward([values[n] for n in present], [d[n] for n in present])
    torch.cuda.synchronize()
    return leaf.grad.clone(), loss.clone(), rot_loss.clone(), reg_loss.clone(), out["render"].detach().clone()


def test_one_step_is_the_eager_composition_and_the_replayed_graph_repeats_it(gpu_device):
    import torch
    S = _setup(gpu_device, single_pixel=True)
    tex = _texture(5, True, gpu_device)
    want = _eager_composition(S, tex)
    st_e, st_g = _make(S, use_graph=False), _make(S, use_graph=True)
    assert st_e.d_tex_out.shape == (1, 11, TEX_H, TEX_W) and st_e.adam is None and st_e.optim_texture is None
    runs = []
    for st, steps in ((st_e, 1), (st_g, 5)):                  # two eager steps, the capture, three replays
        for _ in range(steps):
            st.d_tex_out.fill_(float("nan"))
            loss = st.step(S["cam"], S["posed"], S["gt"], tex)
            torch.cuda.synchronize()
            runs.append((st.d_tex_out.clone(), loss.clone(), st.rot_loss.clone(), st.reg_loss.clone(), st.out["render"].clone()))
    assert st_e._graph is None and st_g._graph is not None and st_g.overflows == 0 and st_g.host_steps == 5
    st_g.check()
    assert int((st_e.out["radii"] > 0).sum()) > 300 and float(want[3][1]) > 50      # splats on screen, rows over the scale threshold
    assert float(want[0].abs().sum()) > 0 and float(want[2]) > 0
    for k, got in enumerate(runs):
        for a, b, what in zip(got, want, ("d_tex_out", "loss", "rot_loss", "reg_loss", "render")):
            assert bool(torch.isfinite(a).all()) and torch.equal(a.reshape(-1), b.reshape(-1)), (k, what)
    with pytest.raises(ValueError, match="required with it"):
        st_e.step(S["cam"], S["posed"], S["gt"])
    with pytest.raises(RuntimeError, match="owns no parameter"):
        st_e.state_dict()


def _parent_route(S, tex):
    """The route that exists without the step: `BakedAvatar.render(return_values=True)` on the sliced dictionary (colour
    activated outside, as the reference does for that route) + the torch rot term + `loss.scale_ratio_loss`, under autograd.
    -> (d_tex_out, L1 loss)."""
    import torch
    from fateavatar_amd.loss import scale_ratio_loss
    from fateavatar_amd.texture import SH_C0
    baked = S["baked"]
    leaf = tex.clone().requires_grad_(True)
    td = dict(R.slices(leaf))
    td["color"] = torch.tanh(td["color"]) * (0.5 / SH_C0)
    st = _make(S, use_graph=False)
    outs, values = baked.render([S["cam"]], [S["posed"]], st.binding, S["bg"], texture_dict=td, bake_attribute=ALL, return_values=True)
    l1 = torch.nn.functional.l1_loss(outs[0]["render"], S["gt"])
    total = l1 + 0.1 * R.rot_loss(values["rotation"]) + SCALE_TERM[0] * scale_ratio_loss(values["scaling"], SCALE_TERM[1])
    total.backward()
    torch.cuda.synchronize()
    return leaf.grad.clone(), l1.detach().clone()


def test_step_agrees_with_the_route_through_baked_render(gpu_device, monkeypatch):
    """rel-L2 of d_tex_out (and the relative error of the loss) against the route of `_parent_route`, allowed 4 x a floor
    measured here: that route with its rotation activation computed in float64 torch and rounded to float32 against itself
    with the activation in float32 — what ONE rounding of the rotation rows does to the result.  A scalar's floor counts as
    no less than one float32 rounding."""
    import torch
    from fateavatar_amd import texture
    S = _setup(gpu_device, single_pixel=True)
    tex = _texture(5, True, gpu_device)
    g32, l32 = _parent_route(S, tex)
    f32_act = texture.rotation_activation
    monkeypatch.setattr(texture, "rotation_activation", lambda t: f32_act(t.double()).float())
    g64, l64 = _parent_route(S, tex)
    monkeypatch.setattr(texture, "rotation_activation", f32_act)
    st = _make(S, use_graph=False)
    loss = st.step(S["cam"], S["posed"], S["gt"], tex)
    torch.cuda.synchronize()
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    floor_g, got_g = rel(g32, g64), rel(st.d_tex_out, g32)
    floor_l = max(abs(float(l32) - float(l64)) / float(l64), ULP)
    got_l = abs(float(loss) - float(l32)) / float(l32)
    print(f"step against the parent route: d_tex_out rel-L2 {got_g:.3e} (floor {floor_g:.3e}, also against the float64-activation "
          f"route {rel(st.d_tex_out, g64):.3e}); loss relative {got_l:.3e} (floor {floor_l:.3e})")
    for lo, hi, name in ((0, 3, "color"), (3, 4, "opacity"), (4, 7, "scaling"), (7, 10, "rotation"), (10, 11, "offset")):
        print(f"  slice {name}: rel-L2 {rel(st.d_tex_out[:, lo:hi], g32[:, lo:hi]):.3e} (floor {rel(g32[:, lo:hi], g64[:, lo:hi]):.3e})")
    assert got_g <= 4 * floor_g and got_l <= 4 * floor_l


def test_partial_bake_sends_the_terms_to_the_slices_the_frame_does_not_read(gpu_device):
    import torch
    from fateavatar_amd import texture
    from fateavatar_amd.loss import ScaleRatioTerm, rot_term_and_grad, scale_ratio_term_and_grad
    S = _setup(gpu_device, single_pixel=True, template_points=0)
    baked, dev = S["baked"], gpu_device
    assert baked.N == baked.P == 676
    tex = _texture(6, True, dev)
    bake = ("color", "opacity")
    st = _make(S, use_graph=False, bake_attribute=bake)
    st.step(S["cam"], S["posed"], S["gt"], tex)
    bare = _make(S, use_graph=False, bake_attribute=bake, rot_term=None, scale_term=None)
    bare.step(S["cam"], S["posed"], S["gt"], tex)
    torch.cuda.synchronize()
    assert bare.rot_loss is None and bare.reg_loss is None
    d = st.d_tex_out
    assert bool((d[:, 10:11] == 0).all())                                            # offset: read by nobody
    _, values = texture.decode_attributes(tex, baked.plan, baked.mean_scaling, baked.max_scaling)
    d_rot, d_scl = torch.zeros_like(values["rotation"]), torch.zeros_like(values["scaling"])
    rot_term_and_grad(values["rotation"], d_rot, weight=0.1)
    scale_ratio_term_and_grad(values["scaling"], d_scl, terms=ScaleRatioTerm(*SCALE_TERM))
    alone = torch.full_like(tex, float("nan"))
    texture.decode_backward_into(baked.plan, tex, baked.mean_scaling, baked.max_scaling, [None, None, d_scl, d_rot, None], alone)
    torch.cuda.synchronize()
    assert torch.equal(d[:, 4:10], alone[:, 4:10]) and float(d[:, 4:7].abs().sum()) > 0 and float(d[:, 7:10].abs().sum()) > 0
    assert bool((bare.d_tex_out[:, 4:11] == 0).all())                                # without the terms: nothing there
    assert torch.equal(d[:, 0:4], bare.d_tex_out[:, 0:4])                            # colour and opacity: the image term's
    assert float(d[:, 0:3].abs().sum()) > 0 and float(d[:, 3:4].abs().sum()) > 0
    # an extended binding has no prior rows for its template points
    with pytest.raises(RuntimeError, match="bake every attribute"):
        _make(_setup(dev, single_pixel=True), bake_attribute=bake)


def _target(S, seed):
    """The frame rendered from another texture."""
    import torch
    from fateavatar_amd.bake import BakeStep
    tex = _texture(seed, False, S["dev"])
    st = BakeStep(S["baked"], S["faces"], S["canon"], S["cam"].clone(), S["bg"], use_graph=False)
    st.step(S["cam"], S["posed"], S["gt"], tex)
    torch.cuda.synchronize()
    return st.out["render"].clone()


def test_feature_map_steps_learn_the_target_like_the_torch_composition(gpu_device, monkeypatch):
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.bake import BAKE_LR
    from fateavatar_amd.texture import SH_C0
    S = _setup(gpu_device, single_pixel=False)
    dev, baked = gpu_device, S["baked"]
    gt = _target(S, 21)
    st = _make(S, texture="feature_map", scale_term=None, generator=torch.Generator().manual_seed(7))
    assert st.optim_texture.shape == (1, 11, TEX_H, TEX_W) and float(st.optim_texture.min()) >= -1 and float(st.optim_texture.max()) <= 1
    again = _make(S, texture="feature_map", scale_term=None, generator=torch.Generator().manual_seed(7))
    assert torch.equal(again.optim_texture, st.optim_texture)
    p0 = st.optim_texture.clone()
    losses = []
    for k in range(30):
        losses.append(float(st.step(S["cam"], S["posed"], gt)))
        if k == 0:
            g1, p1 = st.d_tex_out.clone(), st.optim_texture.clone()
    assert st._graph is not None and st.overflows == 0 and st.adam.step_count == 30 and st.skipped_steps == 0
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    # the yardstick: the same loop through BakedAvatar.render + torch terms + torch.optim.Adam, eager
    leaf = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([leaf], lr=BAKE_LR)
    ref = []
    for k in range(30):
        td = dict(R.slices(leaf))
        td["color"] = torch.tanh(td["color"]) * (0.5 / SH_C0)
        outs, values = baked.render([S["cam"]], [S["posed"]], st.binding, S["bg"], texture_dict=td, bake_attribute=ALL, return_values=True)
        l1 = torch.nn.functional.l1_loss(outs[0]["render"], gt)
        opt.zero_grad(set_to_none=True)
        (l1 + 0.1 * R.rot_loss(values["rotation"])).backward()
        opt.step()
        ref.append(float(l1.detach()))
    r_first, r_last = sum(ref[:5]) / 5, sum(ref[-5:]) / 5
    print(f"30 feature-map steps: mean L1 of the first five {first:.5f} -> last five {last:.5f}; torch composition {r_first:.5f} -> {r_last:.5f}")
    assert r_last < r_first and last < first
    assert abs(losses[0] - ref[0]) <= 1e-4 * ref[0]                # (the same first frame: parity of the image, not of its bits)
    # step 1 is torch.optim.Adam's update from the step's own gradient: the exact updates agree to a few roundings of the
    # update (8 ulp of lr), and each result is then rounded once at the parameter's scale (one spacing, 2^-23 |p|)
    q = p0.clone().requires_grad_(True)
    q.grad = g1.clone()
    torch.optim.Adam([q], lr=BAKE_LR).step()
    err = (p1.double() - q.detach().double()).abs()
    tol = 2.0 ** -23 * torch.maximum(p0.abs(), p1.abs()).double() + 8 * ULP * BAKE_LR
    moved = g1 != 0
    print(f"first Adam step: worst error / tolerance {float((err / tol).max()):.3f}; texels moved {int(moved.sum())} of {moved.numel()}")
    assert bool((err <= tol).all()) and torch.equal(p1[~moved], p0[~moved]) and int(moved.sum()) > moved.numel() // 4
    # an overflowed frame: Adam skips the step on the device
    fresh = _make(S, texture="feature_map", scale_term=None, use_graph=False, generator=torch.Generator().manual_seed(8))
    fresh.step(S["cam"], S["posed"], gt)
    torch.cuda.synchronize()
    need = int(rasterizer.last_counts[0].num_instances)
    assert need > 500 and fresh.adam.step_count == 1 and float(fresh.overflow_word) == 0.0
    before, m0 = fresh.optim_texture.clone(), fresh.adam.exp_avg.clone()
    view = rasterizer._forward_view

    def tiny(*a, **kw):
        v = view(*a, **kw)
        v["cap"] = need // 2                                         # half the frame's instances
        return v
    monkeypatch.setattr(rasterizer, "_forward_view", tiny)
    with rasterizer.no_wait():
        fresh.step(S["cam"], S["posed"], gt)
    torch.cuda.synchronize()
    monkeypatch.setattr(rasterizer, "_forward_view", view)
    assert float(fresh.overflow_word) == 1.0 and fresh.adam.step_count == 1 and fresh.host_steps == 2 and fresh.skipped_steps == 1
    assert torch.equal(fresh.optim_texture, before) and torch.equal(fresh.adam.exp_avg, m0)
    assert rasterizer.check_async_overflow(0)                        # (the host sees it, and raises its capacity guess)
    fresh.step(S["cam"], S["posed"], gt)
    torch.cuda.synchronize()
    assert float(fresh.overflow_word) == 0.0 and fresh.adam.step_count == 2 and not torch.equal(fresh.optim_texture, before)


def test_checkpoint_resumes_with_the_same_bits(gpu_device):
    import torch
    S = _setup(gpu_device, single_pixel=True)
    gt = S["gt"]

    def make(seed):
        st = _make(S, texture="feature_map", generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            st.optim_texture[:, 3:4].mul_(0.05).add_(math.log(0.005 / 0.995))      # the single-pixel opacities
        return st
    a = make(11)
    for _ in range(3):
        a.step(S["cam"], S["posed"], gt)
    torch.cuda.synchronize()
    sd = a.state_dict()
    assert sd["global_step"] == 3 and list(sd["model"]) == ["decoder.optim_texture"]
    assert sd["model"]["decoder.optim_texture"].shape == (1, 11, TEX_H, TEX_W) and set(sd["optimizer"]) == {"exp_avg", "exp_avg_sq", "state"}
    b = make(12)
    assert not torch.equal(b.optim_texture, a.optim_texture)
    sd["model"]["_xyz"] = torch.zeros(3)                             # (a checkpoint of the reference also holds the avatar's entries)
    assert b.load_state_dict(sd) == ["_xyz"]
    assert torch.equal(b.optim_texture, a.optim_texture) and b.adam.step_count == 3 == b.host_steps
    for k in range(2):
        la, lb = a.step(S["cam"], S["posed"], gt), b.step(S["cam"], S["posed"], gt)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(a.d_tex_out, b.d_tex_out) and torch.equal(a.optim_texture, b.optim_texture), k
        assert torch.equal(a.rot_loss, b.rot_loss) and torch.equal(a.reg_loss, b.reg_loss), k
    assert a.adam.step_count == b.adam.step_count == 5 and a._graph is not None
    with pytest.raises(KeyError, match="decoder.optim_texture"):
        b.load_state_dict({"model": {}})


def test_export_renders_the_image_the_step_rendered(gpu_device):
    """`baked.export(step.texture_dict())` — colour activated outside, as the reference does on that route
    (train/baker.py:630) — is an `AvatarGaussians` whose plain frame is the step's image.  Not bit for bit: that route's colour
    goes through torch.tanh and its rotation through `rotation_activation` on the map, the step's through the kernel's own
    tanhf / sinf / cosf, so the rows differ by a few float32 roundings — colour by <= 4 ulp of 1.78, which reaches a pixel
    (sum of T alpha (C0 c + 0.5), sum of T alpha <= 1) as <= 4 ulp x 1.78 x 0.28 = 1.2e-7; the rotation rows by a few ulp of 1,
    which move a splat's conic entries, hence its alphas, by about as many ulp of theirs, at most some tens of Gaussians deep:
    1e-5 bounds the two together with an order of magnitude to spare, and a wrong slice or a missing activation shows at 1e-2."""
    import torch
    from fateavatar_amd.avatar import AvatarGaussians, _RawFrame
    from fateavatar_amd.bound import render_bound_batch
    from fateavatar_amd.texture import SH_C0
    S = _setup(gpu_device, single_pixel=False)
    gt = _target(S, 22)
    st = _make(S, texture="feature_map", use_graph=False, generator=torch.Generator().manual_seed(5))
    st.step(S["cam"], S["posed"], gt)                                # (one update: not the initial texture)
    torch.cuda.synchronize()
    td = st.texture_dict()
    assert list(td) == list(ALL) and [t.shape[1] for t in td.values()] == [3, 1, 3, 3, 1]
    assert td["color"].untyped_storage().data_ptr() == st.optim_texture.untyped_storage().data_ptr()      # views, not copies
    td = {n: t.clone() for n, t in td.items()}                       # the texture the next step renders from (and then updates)
    st.step(S["cam"], S["posed"], gt)
    torch.cuda.synchronize()
    image = st.out["render"]
    td["color"] = torch.tanh(td["color"]) * (0.5 / SH_C0)
    exported = S["baked"].export(td)
    assert isinstance(exported, AvatarGaussians) and exported.P == S["baked"].N
    with torch.no_grad():
        plain = render_bound_batch([S["cam"]], _RawFrame(exported, None), [S["posed"]], st.binding, S["bg"])[0]["render"]
    torch.cuda.synchronize()
    err = float((plain - image).abs().max())
    print(f"export against the step's image: max-abs {err:.3e}")
    assert float((image - image.mean()).abs().max()) > 0.05 and err <= 1e-5
