"""GPU: Gaussian attributes looked up in UV attribute maps (fateavatar_amd/texture.py, csrc/fr_texture.hip) and the baked
avatar rendered from them (fateavatar_amd/baked.py).

The oracle is torch itself on the CPU in float64 — F.grid_sample(activation(texture), 2 uv - 1, mode="bilinear",
padding_mode="border", align_corners=True), the reference's call (model/uv_decoder.py:179-202), and its autograd.

Tolerances.  Exact cases have none.  For the reference's layout the test measures the FLOOR on its own inputs, per layer
and with that layer's activation — torch's float32 CPU activation + grid_sample (+ autograd) against the same in float64 —
and holds the HIP outputs and texture gradients to 4 x that floor, in max-abs and in rel-L2, per layer (factor 4: a
different but legitimate fp32 order of two roundings; the mistakes this test exists for — align_corners, border, u / v
swapped, channel or layer order, an activation's derivative — show at >= 1e-2 on such textures).  The small shapes use the
same rule where the floor is a statistic of thousands of samples (N >= 1000); for N = 1 the floor is ONE rounding accident
(it can be 0), so there the bound is the larger of 4 x floor and an a-priori one: the sample position in texels carries
<= 4 ulp of (size - 1) of rounding per axis (2u - 1, + 1, / 2, * (size - 1)), which moves the interpolated value by at most
that times the largest texel-to-texel difference (<= 2 max|act(texture)|), plus 8 ulp of the value for the sum itself; the
gradient of a texel is weight x d_out x act', so the same position error times max|d_out| max|act'|."""

import numpy as np
import pytest

from fateavatar_amd import _lib, scenes

pytestmark = pytest.mark.gpu

C0 = 0.28209479177387814
MEAN_S, MAX_S = -5.0, -4.5           # a scaling prior's mean and mean + std (uv_decoder.py:298-301), log-scale units


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch, gpu_device):
    """Without a device every test skips (gpu_device); every test starts from an empty binning-capacity guess."""
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


# ------------------------------------------------------------------ the oracle
def _act_torch(kind, t):
    """The reference's activations (uv_decoder.py:133-156) in torch, any dtype."""
    import torch
    if kind == "color":
        return torch.tanh(t) * (0.5 / C0)
    if kind == "offset":
        return torch.tanh(t)
    if kind == "scaling":
        return MAX_S - torch.nn.functional.softplus(-(t + MEAN_S) + MAX_S)
    return t


def _act_hip(kind):
    from fateavatar_amd import texture
    return {"color": texture.COLOR_ACTIVATION, "offset": texture.OFFSET_ACTIVATION,
            "scaling": texture.scaling_activation(MEAN_S, MAX_S)}.get(kind)


def _oracle(textures, kinds, uv, d_outs, dtype):
    """([N,C] outputs, texture gradients) of the reference's look-up on the CPU in `dtype`."""
    import torch
    uv = uv.to(dtype)
    grid = (2 * uv - 1)[None, None]                                   # [1,1,N,2]
    outs, grads = [], []
    for t, kind, g in zip(textures, kinds, d_outs):
        x = t.detach().to(dtype).reshape((1,) + tuple(t.shape[-3:])).requires_grad_(True)
        o = torch.nn.functional.grid_sample(_act_torch(kind, x), grid, mode="bilinear", padding_mode="border", align_corners=True)
        o = o[0, :, 0, :].t()                                         # [N,C]
        o.backward(g.to(dtype))
        outs.append(o.detach())
        grads.append(x.grad.reshape(t.shape))
    return outs, grads


def _err(a, ref):
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    return float((a - ref).abs().max()), float((a - ref).norm() / max(float(ref.norm()), 1e-300))


def _hip(textures, kinds, uv, d_outs, H, W, as_dict=False):
    """texture_lookup + its backward on the device -> (outs, grads, plan), on the host."""
    import torch
    from fateavatar_amd import texture
    dev = torch.device("cuda:0")
    plan = texture.TexturePlan(uv.to(dev), H, W)
    tex = [t.to(dev).requires_grad_(True) for t in textures]
    acts = [_act_hip(k) for k in kinds]
    if as_dict:
        names = [f"layer{i}" for i in range(len(tex))]
        res = texture.texture_lookup(dict(zip(names, tex)), plan, dict(zip(names, acts)))
        assert list(res) == names
        outs = [res[n] for n in names]
    else:
        outs = texture.texture_lookup(tex, plan, acts)
    grads = torch.autograd.grad(outs, tex, [g.to(dev) for g in d_outs])
    torch.cuda.synchronize()
    return [o.detach().cpu() for o in outs], [g.cpu() for g in grads], plan


def _uniform(gen, *shape):
    import torch
    return torch.rand(*shape, generator=gen) * 2 - 1


def _check_against_floor(name, textures, kinds, uv, d_outs, H, W, small=False, as_dict=False):
    """HIP against the float64 oracle, held to 4 x the float32 oracle's own error (see the module docstring)."""
    import torch
    ref_o, ref_g = _oracle(textures, kinds, uv, d_outs, torch.float64)
    f32_o, f32_g = _oracle(textures, kinds, uv, d_outs, torch.float32)
    hip_o, hip_g, plan = _hip(textures, kinds, uv, d_outs, H, W, as_dict)
    ulp = 2.0 ** -24
    pos = 4 * ulp * ((W - 1) + (H - 1))
    for l, kind in enumerate(kinds):
        assert hip_o[l].shape == ref_o[l].shape == (uv.shape[0], textures[l].shape[-3]) and hip_g[l].shape == textures[l].shape
        for what, hip, f32, ref in (("forward", hip_o[l], f32_o[l], ref_o[l]), ("gradient", hip_g[l], f32_g[l], ref_g[l])):
            floor, got = _err(f32, ref), _err(hip, ref)
            bound = [4 * floor[0], 4 * floor[1]]
            if small:
                amax = float(_act_torch(kind, textures[l].double()).abs().max())
                if what == "forward":
                    apriori = pos * 2 * amax + 8 * ulp * amax
                else:
                    x = textures[l].double().requires_grad_(True)
                    _act_torch(kind, x).sum().backward()
                    gmax = float(d_outs[l].abs().max()) * float(x.grad.abs().max())
                    apriori = pos * gmax + 8 * ulp * gmax
                bound[0] = max(bound[0], apriori)
                bound[1] = max(bound[1], apriori * ref.numel() ** 0.5 / max(float(ref.double().norm()), 1e-300))
            print(f"{name} layer {l} ({kind or 'identity'}, C={textures[l].shape[-3]}) {what}: floor max-abs {floor[0]:.3e} rel-L2 {floor[1]:.3e} | "
                  f"HIP max-abs {got[0]:.3e} rel-L2 {got[1]:.3e} | bound {bound[0]:.3e} / {bound[1]:.3e}")
            assert np.isfinite(got[0]) and got[0] <= bound[0] and got[1] <= bound[1], (name, l, kind, what, floor, got, bound)
    return plan


# ------------------------------------------------------------------ 1. exact cases
def test_integer_coordinates_are_exact():
    """129 x 129, uv = (i / 128, j / 128): the sample position is an integer, so identity look-ups return the texels bit for
    bit, and with the points on distinct texels d_texture is d_out scattered, bit for bit (zeros elsewhere)."""
    import torch
    S = 129
    gen = torch.Generator().manual_seed(11)
    textures = [_uniform(gen, 3, S, S), _uniform(gen, 1, S, S), _uniform(gen, 4, S, S)]
    jj, ii = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    keep = torch.randperm(S * S, generator=gen)[:S * S // 2]                  # distinct texels, in a shuffled order
    ii, jj = ii.reshape(-1)[keep], jj.reshape(-1)[keep]
    uv = torch.stack([ii.float() / 128, jj.float() / 128], 1)                 # u is x (column i), v is y (row j)
    d_outs = [_uniform(gen, len(keep), t.shape[0]) for t in textures]
    outs, grads, _ = _hip(textures, [None] * 3, uv, d_outs, S, S)
    for t, o, g, d in zip(textures, outs, grads, d_outs):
        assert torch.equal(o, t[:, jj, ii].t())
        want = torch.zeros_like(t)
        want[:, jj, ii] = d.t()
        assert torch.equal(g, want)
    # channel / layer order and u-v orientation on a texture that encodes its own indices
    code = (torch.arange(4).view(4, 1, 1) * 1000000 + torch.arange(S).view(1, S, 1) * 1000 + torch.arange(S).view(1, 1, S)).float()
    outs, _, _ = _hip([code[:3], code[3:]], [None] * 2, uv, [torch.zeros(len(keep), 3), torch.zeros(len(keep), 1)], S, S)
    got = torch.cat(outs, 1)
    assert torch.equal(got, (torch.arange(4).view(1, 4) * 1000000 + jj.view(-1, 1) * 1000 + ii.view(-1, 1)).float())


def test_coordinates_outside_the_unit_square_return_the_edge_texel():
    import torch
    S = 129
    gen = torch.Generator().manual_seed(12)
    tex = _uniform(gen, 3, S, S)
    k = torch.arange(S)
    cases = {"left": (torch.full((S,), -0.5), k / 128.0, lambda: tex[:, k, 0]),
             "right": (torch.full((S,), 1.5), k / 128.0, lambda: tex[:, k, S - 1]),
             "top": (k / 128.0, torch.full((S,), -3.0), lambda: tex[:, 0, k]),
             "bottom": (k / 128.0, torch.full((S,), 1.0 + 2.0 ** -20), lambda: tex[:, S - 1, k]),
             "corner": (torch.full((S,), 7.0), torch.full((S,), -7.0), lambda: tex[:, 0, S - 1].view(3, 1).expand(3, S))}
    for name, (u, v, want) in cases.items():
        uv = torch.stack([u.float(), v.float()], 1)
        outs, grads, _ = _hip([tex], [None], uv, [torch.ones(S, 3)], S, S)
        assert torch.equal(outs[0], want().t()), name
        assert float(grads[0].sum()) == 3 * S, name                           # every weight lands on a texel, none is lost


# ------------------------------------------------------------------ 2. the reference's layout
_LAYOUT = {}


def _layout_case():
    """131 072 points: `uv_of_binding` of the template's UV raster with sampling seeds 0 and 1, concatenated; 512 x 512; the five
    reference layers (rotation as a 4-channel identity layer); textures and d_out uniform(-1, 1) from a seeded CPU generator."""
    import torch
    from fateavatar_amd import mesh_sampling, texture
    if not _LAYOUT:
        lay = scenes.head_uv()
        uvs = []
        for seed in (0, 1):
            fi, bc = mesh_sampling.uniform_sampling_barycoords(65536, lay[0], lay[1], rng=np.random.default_rng(seed))
            uvs.append(texture.uv_of_binding(fi, bc))
        uv = torch.cat(uvs)
        assert uv.shape == (131072, 2) and 0.0097 <= float(uv.min()) and float(uv.max()) <= 0.9942
        gen = torch.Generator().manual_seed(2024)
        kinds = ["color", None, "scaling", None, "offset"]
        textures = [_uniform(gen, c, 512, 512) for c in (3, 1, 3, 4, 1)]
        d_outs = [_uniform(gen, uv.shape[0], t.shape[0]) for t in textures]
        _LAYOUT.update(uv=uv, kinds=kinds, textures=textures, d_outs=d_outs)
    return _LAYOUT


def test_reference_layout_within_four_floors():
    c = _layout_case()
    plan = _check_against_floor("layout", c["textures"], c["kinds"], c["uv"], c["d_outs"], 512, 512)
    row_start, entries = plan.csr()
    longest = int((row_start[1:] - row_start[:-1]).max())
    print("layout: entries", int(entries.numel()), "texels touched", int(((row_start[1:] - row_start[:-1]) > 0).sum()), "longest row", longest)
    assert entries.numel() == 4 * 131072          # (no point of this layout sits on the last row / column)
    assert longest < 16


# ------------------------------------------------------------------ 3. other shapes
@pytest.mark.parametrize("N", [1, 100003])
@pytest.mark.parametrize("layers", [1, 8])
def test_small_textures_one_and_eight_layers(N, layers):
    """37 x 53 textures ([1,C,H,W] inputs for every other layer, dict in / dict out for eight), uv in [-0.1, 1.1]^2 (part of it
    clipped to the border), N = 1 and N = 100 003 (~200 entries per texel: long rows)."""
    import torch
    H, W = 37, 53
    gen = torch.Generator().manual_seed(100 * layers + (N % 97))
    chans = [3, 1, 3, 4, 1, 2, 4, 3][:layers] if layers > 1 else [3]
    kinds = ["color", None, "scaling", None, "offset", "offset", "color", "scaling"][:layers]
    textures = [_uniform(gen, c, H, W) if i % 2 == 0 else _uniform(gen, 1, c, H, W) for i, c in enumerate(chans)]
    uv = torch.rand(N, 2, generator=gen) * 1.2 - 0.1
    d_outs = [_uniform(gen, N, c) for c in chans]
    _check_against_floor(f"37x53 N={N} L={layers}", textures, kinds, uv, d_outs, H, W, small=N < 1000, as_dict=layers == 8)


# ------------------------------------------------------------------ 4. properties of the backward and the plan
def test_backward_writes_every_texel_repeats_its_bits_and_the_plan_matches_the_corners():
    import torch
    from fateavatar_amd import texture
    dev = torch.device("cuda:0")
    c = _layout_case()
    H = W = 512
    plan = texture.TexturePlan(c["uv"].to(dev), H, W)
    corners = plan.corners()
    assert not plan.has_csr
    row_start, entries = plan.csr()
    # the plan: corners past the border (-1) are EXCLUDED; row lengths = bincount of the indices fr_texture_corners returned
    flat = corners.reshape(-1).long()
    counts = torch.bincount(flat[flat >= 0], minlength=H * W)
    assert row_start.dtype == torch.int32 and entries.dtype == torch.int32 and row_start.numel() == H * W + 1
    assert int(row_start[0]) == 0 and torch.equal((row_start[1:] - row_start[:-1]).long(), counts)
    assert entries.numel() == int((flat >= 0).sum())
    texel_of_entry = torch.repeat_interleave(torch.arange(H * W, device=dev), counts)
    assert torch.equal(flat[entries.long()], texel_of_entry)                          # every entry sits in its texel's row
    same_row = texel_of_entry[1:] == texel_of_entry[:-1]
    assert bool((entries[1:] > entries[:-1])[same_row].all())                         # stable: (point, corner) order per row
    longest = int(counts.max())
    print("longest row of the layout case:", longest)
    assert longest < 16

    # the backward through the C ABI into NaN-filled buffers, twice
    tex = [t.to(dev) for t in c["textures"]]
    d_outs = [g.to(dev) for g in c["d_outs"]]
    acts = [_act_hip(k) or texture.IDENTITY for k in c["kinds"]]
    runs = []
    for _ in range(2):
        d_tex = [torch.full_like(t, float("nan")) for t in tex]
        rc = _lib.lib().fr_texture_lookup_backward(plan.N, plan.uv.data_ptr(), H, W, row_start.data_ptr(), entries.data_ptr(), len(tex),
                                                   texture._layers(tex, acts, d_outs=d_outs, d_textures=d_tex),
                                                   torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.FR_OK, _lib.last_error()
        torch.cuda.synchronize()
        runs.append(d_tex)
    untouched = (counts == 0).reshape(H, W)
    assert 1000 < int(untouched.sum()) < H * W // 2
    for a, b in zip(*runs):
        assert torch.isfinite(a).all()
        assert bool((a[:, untouched] == 0).all()) and not bool(torch.signbit(a[:, untouched]).any())   # exact +0.0
        assert torch.equal(a, b)
    # ... and the autograd route gives those bits
    leaves = [t.clone().requires_grad_(True) for t in tex]
    grads = torch.autograd.grad(texture.texture_lookup(leaves, plan, acts), leaves, d_outs)
    for a, g in zip(runs[0], grads):
        assert torch.equal(a, g)
    # a texture that needs no gradient gets none; the others are unchanged
    leaves = [t.clone().requires_grad_(i != 1) for i, t in enumerate(tex)]
    outs = texture.texture_lookup(leaves, plan, acts)
    torch.autograd.backward(outs, d_outs)
    assert leaves[1].grad is None
    for i in (0, 2, 3, 4):
        assert torch.equal(leaves[i].grad, runs[0][i])


def test_no_grad_builds_no_plan_and_the_first_backward_does():
    import torch
    from fateavatar_amd import texture
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    plan = texture.TexturePlan(torch.rand(1000, 2, generator=gen).to(dev), 16, 16)
    tex = _uniform(gen, 3, 16, 16).to(dev).requires_grad_(True)
    with torch.no_grad():
        out = texture.texture_lookup([tex], plan)[0]
    assert not out.requires_grad and not plan.has_csr
    out = texture.texture_lookup([tex], plan)[0]
    assert out.requires_grad and not plan.has_csr                    # built lazily, on the first backward
    out.sum().backward()
    assert plan.has_csr and tex.grad.shape == tex.shape
    with pytest.raises(RuntimeError, match="uv gets no gradient"):
        texture.TexturePlan(torch.rand(4, 2).to(dev).requires_grad_(True), 16, 16)
    with pytest.raises(RuntimeError, match=r"texture 0 must be on a HIP device \(there is no CPU path\)"):
        texture.texture_lookup([tex.detach().cpu()], plan)


# ------------------------------------------------------------------ 5. captured graph
def test_forward_and_backward_replayed_as_a_graph_match_eager():
    import torch
    from fateavatar_amd import texture
    dev = torch.device("cuda:0")
    c = _layout_case()
    plan = texture.TexturePlan(c["uv"].to(dev), 512, 512)
    plan.csr()                                                       # (the plan is built eagerly: it sorts and synchronises)
    acts = [_act_hip(k) for k in c["kinds"]]
    tex = [t.to(dev).requires_grad_(True) for t in c["textures"]]
    d_outs = [g.to(dev) for g in c["d_outs"]]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                    # warm the allocator on the capture stream
        torch.autograd.grad(texture.texture_lookup(tex, plan, acts), tex, d_outs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        outs = texture.texture_lookup(tex, plan, acts)
        grads = torch.autograd.grad(outs, tex, d_outs)
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(77)
    for rep in range(2):
        with torch.no_grad():
            for t, d in zip(tex, d_outs):                            # new contents in the captured buffers
                t.copy_(_uniform(gen, *t.shape).to(dev))
                d.copy_(_uniform(gen, *d.shape).to(dev))
            for o in list(outs) + list(grads):
                o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        leaves = [t.detach().clone().requires_grad_(True) for t in tex]
        e_outs = texture.texture_lookup(leaves, plan, acts)
        e_grads = torch.autograd.grad(e_outs, leaves, d_outs)
        torch.cuda.synchronize()
        for a, b in zip(list(outs) + list(grads), list(e_outs) + list(e_grads)):
            assert torch.isfinite(a).all() and torch.equal(a, b), rep


# ------------------------------------------------------------------ 6. / 7. the baked avatar
class _Holder:
    """What render_bound_batch() reads of a Gaussian holder."""
    max_sh_degree = 0
    fused_activations = True
    fused_densification_stats = None


def _baked_setup(dev, template_points=0, tex_size=128):
    import torch
    from fateavatar_amd import insta
    from fateavatar_amd.avatar import AvatarGaussians
    from fateavatar_amd.baked import BakedAvatar
    from fateavatar_amd.binding import face_scale
    from fateavatar_amd.model import TorchCamera
    transform, posed, faces = insta.synthetic_sequence(4, 128, 0)
    verts, _, _ = scenes.head_geometry()
    pc = AvatarGaussians.from_template(dev, uv_resolution=96)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        pc._features_dc.copy_(_uniform(gen, pc.P, 1, 3).to(dev))
        pc._opacity.fill_(0.0)
        pc._rotation.copy_((_uniform(gen, pc.P, 4) + torch.tensor([2.0, 0, 0, 0])).to(dev))   # (not unit: the prior normalises)
        pc._scaling.add_((_uniform(gen, pc.P, 3) * 0.3).to(dev))
    S = tex_size
    tex = {"color": _uniform(gen, 3, S, S), "opacity": _uniform(gen, 1, S, S), "scaling": _uniform(gen, 1, 3, S, S) * 0.5,
           "rotation": _uniform(gen, 3, S, S), "offset": _uniform(gen, 1, S, S)}
    tex = {n: t.to(dev) for n, t in tex.items()}
    avatar = BakedAvatar(pc, tex_size=S, template_points=template_points)
    faces_t = torch.from_numpy(faces).to(dev)
    binding = avatar.mesh_binding(faces_t, face_scale(torch.from_numpy(verts).to(dev), faces_t), 0.05, True)
    cams = [TorchCamera(cam, dev) for cam in insta.camera_arrays(transform)]
    return avatar, pc, binding, cams, torch.from_numpy(posed).to(dev), tex


ALL = ("color", "opacity", "scaling", "rotation", "offset")


@pytest.mark.parametrize("K,depth_alpha,bake", [(1, False, ("color", "opacity")), (3, False, ALL), (1, True, ALL),
                                                (3, True, ("color", "opacity", "offset"))])
def test_baked_render_is_lookup_then_render_bound_batch(K, depth_alpha, bake):
    """The image is `render_bound_batch` of the look-up's own outputs (detached leaves), bit for bit; with ONE rasterizer
    backward (the blend backward sums with float atomics and does not repeat its bits) the textures' gradients are the
    stand-alone look-up backward of the gradients retained on the looked-up tensors, bit for bit."""
    import torch
    from fateavatar_amd import texture
    from fateavatar_amd.bound import render_bound_batch
    dev = torch.device("cuda:0")
    avatar, pc, binding, cams, posed, tex = _baked_setup(dev)
    bg = torch.ones(3, device=dev)
    tex = {n: t.requires_grad_(True) for n, t in tex.items()}
    verts = [posed[k] for k in range(K)]
    outs, values = avatar.render(cams[:K], verts, binding, bg, texture_dict=tex, bake_attribute=bake, depth_alpha=depth_alpha,
                                 return_values=True)
    assert sorted(values) == sorted(set(bake) | {"opacity"}) and len(outs) == K
    for n, v in values.items():
        assert v.shape == (avatar.N, {"color": 3, "opacity": 1, "scaling": 3, "rotation": 4, "offset": 1}[n]) and v.requires_grad
        v.retain_grad()

    # the same frame from detached leaves, the attribute selection of uv_decoder.py:652-663 written out
    h = _Holder()
    leaf = {n: v.detach().clone().requires_grad_(True) for n, v in values.items()}
    pick = lambda n: leaf[n] if n in bake else avatar.prior[n]  # noqa: E731
    h.get_features, h._opacity = pick("color").reshape(avatar.N, 1, 3), leaf["opacity"]
    h._scaling, h._rotation, h._offset = pick("scaling"), pick("rotation"), pick("offset")
    ref = render_bound_batch(cams[:K], h, verts, binding, bg, depth_alpha=depth_alpha)
    torch.cuda.synchronize()
    for k in range(K):
        assert torch.equal(outs[k]["render"], ref[k]["render"]) and torch.equal(outs[k]["radii"], ref[k]["radii"]), k
        assert float((outs[k]["render"] - outs[k]["render"].mean()).abs().max()) > 0.05, k      # (something was drawn)
        assert ("depth" in outs[k]) == depth_alpha
        if depth_alpha:
            assert torch.equal(outs[k]["depth"], ref[k]["depth"]) and torch.equal(outs[k]["alpha"], ref[k]["alpha"]), k
    if "opacity" not in bake:      # the looked-up opacity is used regardless (uv_decoder.py:660)
        assert not torch.equal(values["opacity"], avatar.prior["opacity"])

    gen = torch.Generator().manual_seed(3)
    g_img = [(_uniform(gen, *outs[k]["render"].shape) / 4096).to(dev) for k in range(K)]
    torch.autograd.backward([o["render"] for o in outs], g_img)                                  # ONE rasterizer backward
    torch.cuda.synchronize()
    assert avatar.plan.has_csr
    retained = {n: v.grad for n, v in values.items()}
    for n, gr in retained.items():
        assert gr is not None and gr.shape == values[n].shape and torch.isfinite(gr).all() and float(gr.abs().sum()) > 0, n
    tex2 = {n: tex[n].detach().clone().requires_grad_(True) for n in values}
    vals2 = texture.gather_attributes_from_texture_dict(tex2, avatar.plan, avatar.mean_scaling, avatar.max_scaling)
    torch.autograd.backward([vals2[n] for n in values], [retained[n] for n in values])
    torch.cuda.synchronize()
    for n in tex:
        if n in values:
            assert torch.equal(values[n], vals2[n]), n
            assert tex[n].grad is not None and tex[n].grad.shape == tex[n].shape and torch.equal(tex[n].grad, tex2[n].grad), n
            assert float(tex[n].grad.abs().sum()) > 0, n
        else:
            assert tex[n].grad is None, n


def test_baked_render_without_grad_is_forward_only_and_builds_no_plan():
    import torch
    from fateavatar_amd import rasterizer
    dev = torch.device("cuda:0")
    avatar, pc, binding, cams, posed, tex = _baked_setup(dev)
    bg = torch.ones(3, device=dev)
    avatar.texture_dict = tex
    with torch.no_grad():
        fo = avatar.render(cams[:3], [posed[k] for k in range(3)], binding, bg, bake_attribute=ALL)
    torch.cuda.synchronize()
    assert rasterizer.last_forward_only[0] is True and not avatar.plan.has_csr
    leaves = {n: t.clone().requires_grad_(True) for n, t in tex.items()}
    full = avatar.render(cams[:3], [posed[k] for k in range(3)], binding, bg, texture_dict=leaves, bake_attribute=ALL)
    torch.cuda.synchronize()
    assert rasterizer.last_forward_only[0] is False and not avatar.plan.has_csr
    for a, b in zip(fo, full):
        assert not a["render"].requires_grad and b["render"].requires_grad and torch.equal(a["render"], b["render"])
    # argument errors of the glue
    with pytest.raises(RuntimeError, match="use mesh_binding"):
        avatar.render(cams[:1], [posed[0]], binding._replace(face_index=binding.face_index[:-1]), bg)
    with pytest.raises(RuntimeError, match="needs 'opacity'"):
        avatar.render(cams[:1], [posed[0]], binding, bg, texture_dict={"color": tex["color"]}, bake_attribute=("color",))
    with pytest.raises(RuntimeError, match="has no 'offset'"):
        avatar.render(cams[:1], [posed[0]], binding, bg, texture_dict={"opacity": tex["opacity"]}, bake_attribute=("offset",))


def test_export_renders_the_baked_image():
    """All five attributes baked, the binding extended by template points: `export()` is an `AvatarGaussians` with the
    looked-up values in its flat buffer whose `render_bound_batch` image is `BakedAvatar.render`'s, bit for bit."""
    import torch
    from fateavatar_amd.avatar import AvatarGaussians, _RawFrame
    from fateavatar_amd.bound import render_bound_batch
    dev = torch.device("cuda:0")
    avatar, pc, binding, cams, posed, tex = _baked_setup(dev, template_points=64 * 64)
    bg = torch.ones(3, device=dev)
    assert avatar.N > avatar.P == pc.P and binding.face_index.shape[0] == avatar.N
    assert torch.equal(avatar.face_index[:pc.P], pc.face_index) and torch.equal(avatar.bary_coords[:pc.P], pc.bary_coords)
    assert abs(avatar.mean_scaling - float(pc._scaling.mean())) < 1e-6
    assert abs(avatar.max_scaling - float(pc._scaling.mean() + pc._scaling.std())) < 1e-6
    assert torch.allclose(avatar.prior["rotation"].norm(dim=1), torch.ones(pc.P, device=dev), atol=1e-6)
    with pytest.raises(RuntimeError, match="bake every attribute"):
        avatar.render(cams[:1], [posed[0]], binding, bg, texture_dict=tex)      # (the priors have P rows, the binding N)
    verts = [posed[k] for k in range(3)]
    with torch.no_grad():
        baked = avatar.render(cams[:3], verts, binding, bg, texture_dict=tex, bake_attribute=ALL)
    exported = avatar.export(tex)
    assert isinstance(exported, AvatarGaussians) and exported.P == avatar.N
    values = avatar.gather(tex)
    for field, name, shape in (("_features_dc", "color", (1, 3)), ("_opacity", "opacity", (1,)), ("_offset", "offset", (1,)),
                               ("_rotation", "rotation", (4,)), ("_scaling", "scaling", (3,))):
        p = getattr(exported, field)
        assert p.shape == (avatar.N,) + shape and torch.equal(p.detach().reshape(avatar.N, -1), values[name])
        assert p.untyped_storage().data_ptr() == exported.flat.untyped_storage().data_ptr()
    assert torch.equal(exported.face_index, avatar.face_index) and torch.equal(exported.bary_coords, avatar.bary_coords)
    with torch.no_grad():
        plain = render_bound_batch(cams[:3], _RawFrame(exported, None), verts, binding, bg)
    torch.cuda.synchronize()
    for a, b in zip(baked, plain):
        assert torch.equal(a["render"], b["render"]) and torch.equal(a["radii"], b["radii"])
        assert float((a["render"] - a["render"].mean()).abs().max()) > 0.05


def test_gather_attributes_slices_the_decoder_output():
    """`gather_attributes` ([1,11,H,W], uv_decoder.py:85-107 with the slices of :225-245) = the dictionary route on the slices,
    colour activated here (tanh * 0.5 / C0)."""
    import torch
    from fateavatar_amd import texture
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(9)
    S, N = 64, 5000
    plan = texture.TexturePlan(torch.rand(N, 2, generator=gen).to(dev), S, S)
    nt = _uniform(gen, 1, 11, S, S).to(dev).requires_grad_(True)
    texture_dict, values = texture.gather_attributes(nt, plan, MEAN_S, MAX_S)
    assert list(values) == ["color", "opacity", "scaling", "rotation", "offset"]
    assert [tuple(texture_dict[n].shape) for n in values] == [(1, 3, S, S), (1, 1, S, S), (1, 3, S, S), (1, 3, S, S), (1, 1, S, S)]
    assert [tuple(values[n].shape) for n in values] == [(N, 3), (N, 1), (N, 3), (N, 4), (N, 1)]
    parts = {"color": nt[:, 0:3], "opacity": nt[:, 3:4], "scaling": nt[:, 4:7], "rotation": nt[:, 7:10], "offset": nt[:, 10:11]}
    by_dict = texture.gather_attributes_from_texture_dict({n: t.detach() for n, t in parts.items()}, plan, MEAN_S, MAX_S)
    for n in ("opacity", "scaling", "rotation", "offset"):
        assert torch.equal(values[n], by_dict[n]), n
    act = texture.texture_lookup([parts["color"].detach()], plan, [texture.COLOR_ACTIVATION])[0]
    assert torch.equal(values["color"], act) and not torch.equal(values["color"], by_dict["color"])
    sum(v.sum() for v in values.values()).backward()
    torch.cuda.synchronize()
    assert nt.grad.shape == nt.shape and torch.isfinite(nt.grad).all() and bool((nt.grad.abs().sum(dim=(0, 2, 3)) > 0).all())
