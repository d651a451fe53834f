"""GPU: forward-only frames (FR_FLAG_FORWARD_ONLY, include/fr_rasterizer.h) — the same images, radii, final transmittance and
contributor counts as the full forward of the same frame, bit for bit; none of the backward's hand-off written; a backward
handed such a frame's buffers refused; the handle left as the next frame expects it.  Checked through the C ABI and
through render / render_batch / render_bound_batch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from fateavatar_amd import _lib, scenes
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 200          # the handles of this module: 200 .. 211 (no other module uses them)
SENTINEL = 0xA5


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch, gpu_device):
    """Every test starts from an empty binning-capacity guess (see test_gpu_batch_parity); without a device, every test
    skips (gpu_device)."""
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


def _frame_bits(res, H, W):
    """(image, radii, final_T, n_contrib) of a `rasterize_gaussians` result tuple, on the host."""
    from fateavatar_amd import rasterizer
    _, color, radii, _, _, img = res
    fT, nc = rasterizer.image_aux(img, H, W)
    return [color.cpu().numpy(), radii.cpu().numpy(), fT.cpu().numpy(), nc.cpu().numpy()]


def _assert_bits(a, b, what):
    for name, x, y in zip(("image", "radii", "final_T", "n_contrib", "visible"), a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, name)


def _both(scs, kws, slots):
    """Each batch of scenes rendered full and forward-only (same slots, alternately) through rasterize_gaussians_batch, or
    rasterize_gaussians for one view; -> the two lists of per-view bits."""
    import torch
    from fateavatar_amd import rasterizer
    dev = torch.device("cuda:0")
    views = []
    for s, kw in zip(scs, kws):
        v = util._Frame()
        v._upload(s, dev, **kw)
        views.append(v)
    out = []
    for fo in (False, True, False):
        if len(views) == 1:
            with rasterizer.handle_slot(slots[0]):
                res = [rasterizer.rasterize_gaussians(*views[0]._forward_args(), _forward_only=fo)]
        else:
            res = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots, forward_only=fo)
        torch.cuda.synchronize()
        assert rasterizer.last_forward_only[0] is fo
        out.append([_frame_bits(r, v.H, v.W) for r, v in zip(res, views)])
    for k in range(len(views)):
        _assert_bits(out[0][k], out[2][k], ("full twice", k))   # (the frames are deterministic)
    return out[0], out[1]


def _check_same(scs, kws=None, slots=None, what=""):
    kws = kws or [{}] * len(scs)
    slots = slots or [SLOT + k for k in range(len(scs))]
    full, fo = _both(scs, kws, slots)
    for k, (a, b) in enumerate(zip(full, fo)):
        _assert_bits(a, b, (what, k))


# ------------------------------------------------------------------ bit identity through the ABI
@pytest.mark.parametrize("group", range(6))
def test_fuzz_scenes_bit_identical(group):
    """Mixed batches of 1 to 4 fuzz views (P, image shape, SH degree, M, scale / opacity regimes, backgrounds)."""
    stream = util.fuzz_stream(31000 + group, big=group >= 3)
    K = 1 + group % 4
    cases = [next(stream) for _ in range(K)]
    scs = [scenes.random_scene(P, H, W, **kw) for _, P, H, W, kw, _, _ in cases]
    _check_same(scs, what=f"fuzz{group}")


@pytest.mark.parametrize("group", range(6))
def test_known_answer_fixtures_bit_identical(group):
    """The 24 fixtures of tests/golden/known_answers.npz, four per batch (the batches of test_gpu_batch_parity)."""
    import torch
    from fateavatar_amd import rasterizer
    from tests import test_known_answers as ka
    from tests.test_gpu_batch_parity import KA_BATCHES
    dev = torch.device("cuda:0")
    fx = [ka._scene(n) for n in KA_BATCHES[group]]
    args = [ka.hip_forward_args(i, dev)[0] for i, _ in fx]
    bits = []
    for fo in (False, True):
        res = rasterizer.rasterize_gaussians_batch(args, slots=[SLOT + k for k in range(4)], forward_only=fo)
        torch.cuda.synchronize()
        bits.append([_frame_bits(r, int(i["H"]), int(i["W"])) for r, (i, _) in zip(res, fx)])
    for name, a, b in zip(KA_BATCHES[group], *bits):
        _assert_bits(a, b, name)


@pytest.mark.parametrize("opacity", [0.1, 0.5, 0.9])
def test_config2_bit_identical(opacity):
    """BASELINE config 2 (head template, 100 k Gaussians, 512^2, SH degree 3) alone and as a 4-view batch."""
    _check_same([scenes.head_scene(opacity=opacity)], what=f"config2-{opacity}")
    _check_same([scenes.head_scene(view=k, n_views=4, opacity=opacity) for k in range(4)], what=f"config2x4-{opacity}")


def test_config5_bit_identical():
    _check_same([scenes.head_scene(P=500_000, res=1024, sh_degree=3, scale=2.750e-4)], what="config5")


@pytest.mark.parametrize("P", [1400, 3000, 6000])
def test_long_tiles_and_the_big_sorter_bit_identical(P):
    """One 8x8 tile with P instances (22 to 94 blend units: the gather's long-tile path; above 2 048 the big sorter),
    alone, then first in a batch of three."""
    from tests.test_gpu_batch_parity import _long_scene, _short_scenes
    _check_same([_long_scene(P)], what=f"long{P}")
    _check_same([_long_scene(P)] + _short_scenes(), what=f"long{P}-batch")


_MODE_CODE = r"""
import sys; sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from fateavatar_amd import scenes
from tests import test_gpu_forward_only as t
scs = [scenes.head_scene(P=20000, res=256, sh_degree=3, seed=0, opacity=0.5),
       scenes.random_scene(4000, 64, 64, sh_degree=0, seed=5, opacity_lo=0.6, opacity_hi=0.99, scale_lo=0.02, scale_hi=0.08)]
for s in scs:
    t._check_same([s], what=sys.argv[2])
    t.check_hand_off_untouched([s], [t.SLOT])
if sys.argv[2] != 'gather':
    t._check_same(scs, what=sys.argv[2] + ' batch')
    t.check_hand_off_untouched(scs, [t.SLOT, t.SLOT + 1])
print('mode-ok')
"""


@pytest.mark.parametrize("mode", ["FR_CHAIN_SPINS=0", "FR_CHAIN_SPINS=3", "FR_BLEND_FWD=gather"])
def test_selectable_blend_paths_bit_identical(mode):
    """Every hand-off of the chained blend through its fallback (FR_CHAIN_SPINS=0 / 3), and the gather as a launch of its own
    (FR_BLEND_FWD=gather, one view): the same bits, and no hand-off written.  In a child process (the switches are read at
    handle creation) under a timeout."""
    env = dict(os.environ)
    k, v = mode.split("=")
    env[k] = v
    r = subprocess.run([sys.executable, "-c", _MODE_CODE, ROOT, "gather" if "gather" in mode else mode], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mode-ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


# ------------------------------------------------------------------ the hand-off is left alone
def _abi_forward(views, slots, fo, caps):
    """fr_forward (one view) / fr_forward_batch on scratch pre-filled with SENTINEL, with the binning capacities `caps`."""
    import torch
    from fateavatar_amd import rasterizer
    L = _lib.lib()
    caps = list(caps)
    for attempt in range(2):   # (a frame that overflows its capacity is repeated once with the capacity it reported)
        st = [rasterizer._forward_view(v._forward_args(), forward_only=fo) for v in views]
        for v, cap in zip(st, caps):
            v["cap"] = cap
            v["binning"] = torch.full((L.fr_binning_bytes(cap, v["W"], v["H"]),), SENTINEL, dtype=torch.uint8, device=v["geom"].device)
            v["geom"].fill_(SENTINEL)
            v["img"].fill_(SENTINEL)
        K = len(st)
        counts = (_lib.fr_counts * K)()
        stream = torch.cuda.current_stream().cuda_stream
        if K == 1:
            v = st[0]
            rc = L.fr_forward(_lib.handle(0, slots[0]), C.byref(v["prm"]), C.byref(v["inp"]), v["out_color"].data_ptr(),
                              v["radii"].data_ptr(), v["geom"].data_ptr(), v["img"].data_ptr(), v["binning"].data_ptr(), v["cap"],
                              counts, stream)
        else:
            handles, prm_p, inp_p, arr = rasterizer._batch_arrays(st, slots, 0)
            rc = L.fr_forward_batch(K, handles, prm_p, inp_p, arr("out_color"), arr("radii"), arr("geom"), arr("img"), arr("binning"),
                                    (C.c_uint64 * K)(*caps), counts, stream)
        torch.cuda.synchronize()
        if rc != _lib.FR_ERR_BINNING_CAPACITY:
            break
        caps = [max(cap, int(c.num_instances) + 1024) for cap, c in zip(caps, counts)]
    assert rc == _lib.FR_OK, (rc, _lib.last_error())
    return st, counts


def _hand_off(v, P, with_sh):
    """{name: bytes on the host} of every hand-off region of one view's scratch."""
    L = _lib.lib()
    out = {}
    gb, bb = v["geom"].data_ptr(), v["binning"].data_ptr()
    for field, n, name in ((6, P, "clamped"), (10, 4 * P, "opacity_act")) + (((9, 36 * P, "dcolor_ddir"),) if with_sh else ()):
        off = L.fr_debug_geometry_field(gb, P, field) - gb
        out[name] = v["geom"][off:off + n].cpu().numpy()
    for region, name in enumerate(("masks", "walks", "work list", "unit_state")):
        n = C.c_size_t()
        off = L.fr_debug_binning_region(bb, v["cap"], v["W"], v["H"], region, C.byref(n)) - bb
        out[name] = v["binning"][off:off + n.value].cpu().numpy()
    return out


def check_hand_off_untouched(scs, slots):
    """Pre-filled scratch: after a forward-only frame every hand-off region still holds the sentinel, after a full frame of
    the same scenes every region has been written to; image and radii bit-identical.  (A region the full frame writes must
    exist: the scenes have tiles of more than one blend unit.)"""
    import torch
    dev = torch.device("cuda:0")
    views = []
    for s in scs:
        v = util._Frame()
        v._upload(s, dev)
        views.append(v)
    full, counts = _abi_forward(views, slots, False, [4 * s.P + 65536 for s in scs])
    fo, counts_fo = _abi_forward(views, slots, True, [f["cap"] for f in full])
    for k, (s, a, b) in enumerate(zip(scs, full, fo)):
        assert counts[k].overflow == 0 and counts_fo[k].num_instances == counts[k].num_instances
        assert counts[k].max_tile_list > 64, (k, counts[k].max_tile_list)
        _assert_bits([a["out_color"].cpu().numpy(), a["radii"].cpu().numpy()], [b["out_color"].cpu().numpy(), b["radii"].cpu().numpy()],
                     ("abi", k))
        ha, hb = _hand_off(a, s.P, True), _hand_off(b, s.P, True)
        for name in ha:
            assert (hb[name] == SENTINEL).all(), (k, name, "written by a forward-only frame")
            assert not (ha[name] == SENTINEL).all(), (k, name, "not written by the full frame")


def test_hand_off_untouched_single_and_batched():
    scs = [scenes.head_scene(P=30000, res=256, sh_degree=3, seed=3, opacity=0.5),
           scenes.random_scene(5000, 96, 80, sh_degree=2, seed=8, opacity_lo=0.3, opacity_hi=0.95, scale_lo=0.02, scale_hi=0.06)]
    check_hand_off_untouched(scs[:1], [SLOT])
    check_hand_off_untouched(scs, [SLOT + 1, SLOT + 2])


# ------------------------------------------------------------------ the backward refuses forward-only buffers
def test_backward_refuses_forward_only_buffers():
    import torch
    from fateavatar_amd import rasterizer
    dev = torch.device("cuda:0")
    scs = [scenes.random_scene(3000, 64, 64, sh_degree=3, seed=k, opacity_lo=0.3, opacity_hi=0.9) for k in range(2)]
    views = []
    for s in scs:
        v = util._Frame()
        v._upload(s, dev)
        views.append(v)
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    for K in (1, 2):
        slots = [SLOT + 3 + k for k in range(K)]
        st, _ = _abi_forward(views[:K], slots, True, [4 * s.P + 65536 for s in scs[:K]])
        bw = []
        for v, f in zip(views[:K], st):
            g = torch.zeros((3, v.H, v.W), device=dev)
            b = rasterizer._backward_view(v._backward_args(g, (0, f["out_color"], f["radii"], f["geom"], f["binning"], f["img"])))
            for t in b["g"].values():
                if t is not None:
                    t.fill_(12345.0)
            bw.append(b)
        if K == 1:
            b = bw[0]
            rc = L.fr_backward(_lib.handle(0, slots[0]), C.byref(b["prm"]), C.byref(b["inp"]), b["radii"].data_ptr(),
                               b["geom"].data_ptr(), b["img"].data_ptr(), b["binning"].data_ptr(), b["dpix"].data_ptr(),
                               C.byref(b["grads"]), stream)
        else:
            handles, prm_p, inp_p, arr = rasterizer._batch_arrays(bw, slots, 0)
            grd_p = (C.POINTER(_lib.fr_grads) * K)(*[C.pointer(b["grads"]) for b in bw])
            rc = L.fr_backward_batch(K, handles, prm_p, inp_p, arr("radii"), arr("geom"), arr("img"), arr("binning"), arr("dpix"),
                                     grd_p, stream)
        assert rc == _lib.FR_ERR_INVALID_ARGUMENT and "forward-only" in _lib.last_error(), (K, rc, _lib.last_error())
        torch.cuda.synchronize()
        for b in bw:
            for name, t in b["g"].items():
                if t is not None:
                    assert (t == 12345.0).all(), (K, name)
    # ... and through the Python host: the buffer-returning forward with _forward_only=True, then its backward
    v = views[0]
    with rasterizer.handle_slot(SLOT + 3):
        res = rasterizer.rasterize_gaussians(*v._forward_args(), _forward_only=True)
        with pytest.raises(RuntimeError, match=r"\(code 1\).*forward-only"):
            rasterizer.rasterize_gaussians_backward(*v._backward_args(torch.zeros((3, v.H, v.W), device=dev), res))
        # a full frame on the same handle is differentiable again
        res = rasterizer.rasterize_gaussians(*v._forward_args())
        g = rasterizer.rasterize_gaussians_backward(*v._backward_args(torch.ones((3, v.H, v.W), device=dev), res))
        torch.cuda.synchronize()
        assert np.isfinite(g[0].cpu().numpy()).all() and float(g[0].abs().sum()) > 0


# ------------------------------------------------------------------ inference, then training, on one handle
def _grads_abi(v, slot, dpix, fo_first):
    import torch
    from fateavatar_amd import rasterizer
    with rasterizer.handle_slot(slot):
        if fo_first:
            rasterizer.rasterize_gaussians(*v._forward_args(), _forward_only=True)
        res = rasterizer.rasterize_gaussians(*v._forward_args())
        g = rasterizer.rasterize_gaussians_backward(*v._backward_args(dpix, res))
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in zip(util.GRAD_NAMES, g)}, _frame_bits(res, v.H, v.W)


def test_inference_then_training_on_one_handle():
    """A forward-only frame, then forward + backward on the same slot: the gradients of a fresh handle's frame (the
    batch-parity tolerance, float-atomic order), the same forward bits.  Through the ABI and through render()."""
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    from fateavatar_amd.render import render
    dev = torch.device("cuda:0")
    s = scenes.head_scene(P=30000, res=256, sh_degree=3, seed=5, opacity=0.5)
    v = util._Frame()
    v._upload(s, dev)
    dpix = torch.from_numpy((np.random.default_rng(3).uniform(-1, 1, (3, 256, 256)) / 65536).astype(np.float32)).to(dev)
    g_after, bits_after = _grads_abi(v, SLOT + 5, dpix, True)
    g_fresh, bits_fresh = _grads_abi(v, SLOT + 6, dpix, False)
    _assert_bits(bits_after, bits_fresh, "abi")
    for k in util.GRAD_NAMES:
        if g_fresh[k].size:
            assert np.isfinite(g_after[k]).all() and util.rel_l2(g_after[k], g_fresh[k]) < 1e-5, k

    cam, bg = TorchCamera(s.camera, dev), torch.from_numpy(s.bg).to(dev)
    w = dpix

    def train(slot, infer_first):
        pc = FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, s.sh_degree, dev, fused_activations=True)
        with rasterizer.handle_slot(slot):
            if infer_first:
                with torch.no_grad():
                    render(cam, pc, bg)
                torch.cuda.synchronize()
                assert rasterizer.last_forward_only[0] is True
            out = render(cam, pc, bg)
            assert rasterizer.last_forward_only[0] is False
            (out["render"] * w).sum().backward()
        torch.cuda.synchronize()
        return {n: pc.grad_of(n).cpu().numpy() for n in ("_xyz", "_opacity", "_scaling", "_rotation")}, \
            out["viewspace_points"].grad.cpu().numpy()

    (ga, sa), (gf, sf) = train(SLOT + 7, True), train(SLOT + 8, False)
    assert util.rel_l2(sa, sf) < 1e-5
    for n in ga:
        assert np.isfinite(ga[n]).all() and util.rel_l2(ga[n], gf[n]) < 1e-5, n


# ------------------------------------------------------------------ captured graphs
def test_forward_only_chains_replayed_as_graphs_match_eager():
    """Two 4-view forward-only launch chains of config-2 views, each captured on its own stream and replayed in flight
    together: every view's image and radii are the eager forward-only frame's (and the full frame's)."""
    import torch
    from fateavatar_amd import rasterizer
    dev = torch.device("cuda:0")
    scs = [scenes.head_scene(view=k, n_views=8, opacity=0.5) for k in range(8)]
    chains = []
    for c in range(2):
        slots = [SLOT + 4 * c + j for j in range(4)]
        views = []
        for s in scs[4 * c:4 * c + 4]:
            v = util._Frame()
            v._upload(s, dev)
            views.append(v)
        full = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots)
        eager = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots, forward_only=True)
        torch.cuda.synchronize()
        want = [_frame_bits(r, 512, 512) for r in eager]
        for k, r in enumerate(full):
            _assert_bits(_frame_bits(r, 512, 512), want[k], ("full vs forward-only", c, k))
        stream = torch.cuda.Stream(device=dev)
        with rasterizer.no_wait():
            stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(stream):
                rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots, forward_only=True)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
                fw = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots, forward_only=True)
        for r in fw:   # (garbage the replays must overwrite)
            r[1].fill_(-1.0)
            r[2].fill_(-7)
        # (the views stay referenced: the graph reads their tensors on every replay)
        chains.append(dict(graph=g, stream=stream, fw=fw, want=want, slots=slots, views=views))
    torch.cuda.synchronize()
    for _ in range(5):
        for ch in chains:
            with torch.cuda.stream(ch["stream"]):
                ch["graph"].replay()
    torch.cuda.synchronize()
    for c, ch in enumerate(chains):
        for k, (r, sl) in enumerate(zip(ch["fw"], ch["slots"])):
            with rasterizer.handle_slot(sl):
                assert not rasterizer.check_async_overflow(0), (c, k)
            _assert_bits(_frame_bits(r, 512, 512), ch["want"][k], ("graph", c, k))


# ------------------------------------------------------------------ automatic selection in render / render_batch / render_bound_batch
def _bound_setup(dev):
    import torch
    from fateavatar_amd import insta
    from fateavatar_amd.avatar import AvatarGaussians
    from fateavatar_amd.binding import face_scale
    from fateavatar_amd.bound import MeshBinding
    from fateavatar_amd.model import TorchCamera
    transform, posed, faces = insta.synthetic_sequence(4, 256, 0)
    verts, _, _ = scenes.head_geometry()
    pc = AvatarGaussians.from_template(dev, uv_resolution=128)
    g = torch.Generator(device="cpu").manual_seed(1)
    with torch.no_grad():
        pc._features_dc.copy_((torch.rand(pc.P, 1, 3, generator=g) * 2 - 1).to(dev))
        pc._opacity.fill_(float(np.log(0.5 / 0.5)))
    faces_t = torch.from_numpy(faces).to(dev)
    canon = face_scale(torch.from_numpy(verts).to(dev), faces_t)
    mb = MeshBinding(faces_t, pc.face_index, pc.bary_coords, canon, 0.05, True)
    cams = [TorchCamera(c, dev) for c in insta.camera_arrays(transform)]
    return pc, mb, cams, torch.from_numpy(posed).to(dev)


def test_render_entry_points_select_forward_only_and_keep_the_bits():
    """render() / render_batch() / render_bound_batch() under torch.no_grad() render forward-only frames (last_forward_only),
    with grad enabled full frames; set_forward_only(False) switches the choice off; images, radii and the bound values are
    the same bits either way."""
    import torch
    from fateavatar_amd import rasterizer
    from fateavatar_amd.avatar import _RawFrame
    from fateavatar_amd.bound import render_bound_batch
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    from fateavatar_amd.render import render, render_batch
    dev = torch.device("cuda:0")
    scs = [scenes.head_scene(P=20000, res=256, sh_degree=3, view=k, n_views=4, opacity=0.5) for k in range(4)]
    pc = FlatGaussians(scs[0].means3D, scs[0].shs, scs[0].opacities, scs[0].scales, scs[0].rotations, 3, dev, fused_activations=True)
    cams = [TorchCamera(s.camera, dev) for s in scs]
    bg = torch.from_numpy(scs[0].bg).to(dev)

    def bits(outs, extra=()):
        torch.cuda.synchronize()
        return [[o["render"].detach().cpu().numpy(), o["radii"].cpu().numpy(), o["visibility_filter"].cpu().numpy()]
                + [t.cpu().numpy() for t in (o.get("bound") or ())] for o in outs]

    entries = {
        "render": lambda: [render(cams[0], pc, bg)],
        "render_batch": lambda: render_batch(cams, pc, bg),
    }
    apc, mb, acams, posed = _bound_setup(dev)
    entries["render_bound_batch"] = lambda: render_bound_batch(acams, [_RawFrame(apc, None)] * 4, [posed[k] for k in range(4)], mb,
                                                               torch.ones(3, device=dev))
    for name, fn in entries.items():
        with torch.no_grad():
            fo = bits(fn())
        assert rasterizer.last_forward_only[0] is True, name
        with torch.no_grad(), rasterizer.set_forward_only(False):
            off = bits(fn())
        assert rasterizer.last_forward_only[0] is False, name
        with_grad = bits(fn())
        assert rasterizer.last_forward_only[0] is False, name
        for k, (a, b, c) in enumerate(zip(fo, off, with_grad)):
            for x, y, z in zip(a, b, c):
                assert np.array_equal(x, y) and np.array_equal(x, z), (name, k)
        assert float(np.abs(fo[0][0] - fo[0][0].mean()).max()) > 0.05, name   # (something was drawn)
