"""-m gpu: BATCHED frames (fr_forward_batch / fr_backward_batch, the path bench.py's `value`, render_batch and
render_bound_batch take) against the CPU oracle, view by view, with the single-frame tolerances of test_gpu_parity.py and
test_known_answers.py — and every view's forward against the same scene rendered alone, bit for bit
(include/fr_rasterizer.h: the results of a batch are those of K separate calls).

What a batch adds to a single frame: every launch runs on the LARGEST view's grid (each body stops at its own view's P,
tiles and units); the preprocess's dynamic LDS is the maximum over the views, each staging SH with its own M; the big-list
decision is shared (any view asking for the big sorter launches it for all, on view 0's side stream); the backward's grid
follows the maximum of the views' last counts, and each view decides for itself whether it stages dL_dsh; the overflow
retry regrows capacities per view, key buckets per handle.  Checked here: heterogeneous fuzz groups (image shapes, P, SH
degree and M, optional inputs side by side), the known-answer fixtures in mixed batches, long lists as a surprise and as
an expected case at either end of a batch, growth and stale buffers inside a batch, the benchmark's regime (4-view
batches of config 2, three chains in flight as captured graphs), per-view backward options, and the environment-selected
blend paths.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from fateavatar_amd import scenes
from tests import util
from tests.test_gpu_parity import _check_backward, _check_backward_capped, _check_forward

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALONE_SLOT = 100   # the handle the single-frame renders of the bit-equality checks use (no batch in this module uses it)
# (the fresh handles of this module are numbered from 101 on: other modules count on slots 11 and 12 not existing yet)


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch):
    """Every test starts from an empty binning-capacity guess (rasterizer._capacity_hint), restored afterwards: one large
    frame raises it to gigabytes, every view of every later batch would allocate that much, and the retry regrows it per
    view anyway."""
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


def _dpix(H, W, seed):
    return (np.random.default_rng(seed).uniform(-1, 1, (3, H, W)) / (H * W)).astype(np.float32)


def _alone(scs, kws, dev):
    """Each scene rendered alone (HipFrame) on ALONE_SLOT: (image, final T, n_contrib, radii, blend-record template) on the host."""
    from fateavatar_amd import rasterizer
    out = []
    with rasterizer.handle_slot(ALONE_SLOT):
        for s, kw in zip(scs, kws):
            h = util.HipFrame(s, dev, **kw)
            out.append(_forward_bits(h))
    return out


def _forward_bits(h):
    return (h.color.cpu().numpy(), h.final_T.cpu().numpy(), h.n_contrib.cpu().numpy(), h.radii.cpu().numpy(), h.geometry(8, 12))


def _same_bits(got, want, what):
    for name, x, y in zip(("image", "final_T", "n_contrib", "radii", "blend records"), got, want):
        vis = slice(None) if name != "blend records" else want[3] > 0     # (records of culled Gaussians are never read)
        assert np.array_equal(x[vis], y[vis]), (what, name)


def _assert_same_bits(b, alone, what):
    """Every view of the batch `b` gave exactly what its scene gives rendered alone."""
    for k, (v, a) in enumerate(zip(b, alone)):
        _same_bits(_forward_bits(v), a, (what, k))


def _check_views(b, scs, kws, dpixs, names, max_skip_frac=0.05):
    for v, s, kw, d, name in zip(b, scs, kws, dpixs, names):
        o = util.oracle_forward(s, **kw)
        _check_forward(o, v, name)
        _check_backward_capped(o, v, d, name, max_skip_frac=max_skip_frac)


# ------------------------------------------------------------------ a. heterogeneous fuzz groups
FUZZ_KINDS = {   # kind -> (seed, stream, random camera + optional inputs, groups)
    "small": (9701, False, False, 8),
    "big": (9702, True, False, 6),
    "inputs": (9703, False, True, 8),
}


def fuzz_groups(seed, big, n_groups):
    """Consecutive configurations of util.fuzz_stream(seed, big) in groups of K = 2, 3, 4, 2, 3, 4 ..."""
    stream = util.fuzz_stream(seed, big)
    for g in range(n_groups):
        yield [next(stream) for _ in range(2 + g % 3)]


def fuzz_group_views(seed, cases, camera_inputs):
    """The scenes, HipFrame keyword arguments, upstream gradients and names of one group (as tools/fuzz_parity.py)."""
    scs, kws, dpixs, names = [], [], [], []
    for it, P, H, W, kw, dpix, name in cases:
        s = scenes.random_scene(P, H, W, **kw)
        extra = {}
        if camera_inputs:
            s.camera = util.fuzz_camera(seed, it, H, W)
            extra = util.fuzz_inputs(seed, it, s)
            name += " camera" + ((" inputs=" + ",".join(sorted(extra))) if extra else "")
        scs.append(s), kws.append(extra), dpixs.append(dpix), names.append(name)
    return scs, kws, dpixs, names


@pytest.mark.parametrize("kind,group", [(k, g) for k, v in FUZZ_KINDS.items() for g in range(v[3])])
def test_fuzz_groups_batched(kind, group, gpu_device):
    """A group mixes P (1 .. 60 000), image shapes (8 .. 900 a side), SH degree 0 .. 3, M = (D + 1)^2 or 16, backgrounds,
    scale and opacity regimes — and ("inputs") colors_precomp / cov3D_precomp / scale_modifier views next to SH views under
    random cameras.  Every view: bit-equal to its scene alone, forward state and gradients against the oracle."""
    seed, big, ci, n = FUZZ_KINDS[kind]
    cases = list(fuzz_groups(seed, big, group + 1))[group]
    scs, kws, dpixs, names = fuzz_group_views(seed, cases, ci)
    names = [f"{kind}{group}[{k}] {nm}" for k, nm in enumerate(names)]
    alone = _alone(scs, kws, gpu_device)
    b = util.HipBatch(scs, gpu_device, per_view_kwargs=kws)
    _assert_same_bits(b, alone, names[0])
    _check_views(b, scs, kws, dpixs, names)


# ------------------------------------------------------------------ b. known answers through the batch
KA_BATCHES = [   # edge shapes, optional inputs and long lists side by side in one launch
    ("random_tiny_7x5", "big_lists", "random_inputs_colors", "single_centred"),
    ("random_big_600", "random_one_tile_16x16", "random_inputs_cov3d", "depth_tie"),
    ("random_past_a_tile_17x33", "random_inputs_both", "head_like_1500", "guard_band"),
    ("random_inputs_modifier_opaque", "alpha_clamp_forward_only", "random_camera_0", "head_like_opaque_700"),
    ("indefinite_precomp", "terminates", "random_camera_1", "random_camera_2"),
    ("alpha_clamp_gradient", "random_camera_3", "random_camera_4", "random_camera_5"),
]


@pytest.mark.parametrize("group", range(len(KA_BATCHES)))
def test_known_answers_through_the_batch(group, gpu_device):
    """The 24 fixtures of tests/golden/known_answers.npz in batches of four, each view held to its known answer with the
    tolerances of test_hip_matches_known_answers."""
    from fateavatar_amd import rasterizer
    from tests import test_known_answers as ka
    names = KA_BATCHES[group]
    fx = [ka._scene(n) for n in names]
    args = [ka.hip_forward_args(i, gpu_device) for i, _ in fx]
    slots = [0, 1, 2, 3]
    res = rasterizer.rasterize_gaussians_batch([a[0] for a in args], slots=slots)
    grads = rasterizer.rasterize_gaussians_backward_batch(
        [bwd(radii, geom, R, binning, img) for (_, bwd), (R, _c, radii, geom, binning, img) in zip(args, res)], slots=slots)
    import torch
    torch.cuda.synchronize()
    for name, (i, want), sl, (R, color, radii, geom, binning, img), g in zip(names, fx, slots, res, grads):
        fT, _ = rasterizer.image_aux(img, int(i["H"]), int(i["W"]))
        mtl = rasterizer.read_counts(gpu_device.index or 0, sl).max_tile_list
        ka.hip_compare(name, want, color, fT, radii, g if "dL_dmeans3D" in want else None, mtl)


# ------------------------------------------------------------------ c. long lists in a batch
def _long_scene(P):
    """test_long_tile_lists_take_the_multi_wave_and_fallback_sorts's fixture: P Gaussians on one 8x8 tile, depth ties."""
    rng = np.random.default_rng(3)
    s = scenes.random_scene(P, 32, 32, sh_degree=0, seed=9, spread=0.004, scale_lo=0.002, scale_hi=0.004,
                            opacity_lo=0.02, opacity_hi=0.05)
    s.means3D[:, 2] = 1.0 + rng.uniform(0, 0.5, s.P).astype(np.float32)
    s.means3D[::7, 2] = 1.25
    return s


def _short_scenes():
    return [scenes.random_scene(1500, 72, 56, sh_degree=1, seed=2, M=16, bg=(0.2, 0.5, 0.9)),
            scenes.random_scene(2000, 100, 130, sh_degree=3, seed=4, behind_fraction=0.2)]


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("P,lo,hi", [(1400, 1024, 2048), (3000, 2048, 4096), (6000, 4096, 1 << 30)])
def test_long_lists_in_a_batch(P, lo, hi, where, gpu_device):
    """Fresh slots: short lists only -> the long-list view as a surprise (no big sorter launched: k_tile_sort_batch's slow path
    for lists > 2048) -> the same batch again (the big sorter, launched for ALL views of the batch) -> short lists only.  The
    long-list view sits at index 0 or at index K - 1; per slot, max_tile_list proves the tier each fixture reaches."""
    from fateavatar_amd import rasterizer
    tier = [(1400, 1024, 2048), (3000, 2048, 4096), (6000, 4096, 1 << 30)].index((P, lo, hi))
    slots = [101 + 6 * tier + 3 * (where == "last") + j for j in range(3)]
    long_ = _long_scene(P)
    short = _short_scenes()
    short_only = short + [scenes.random_scene(1200, 40, 48, sh_degree=0, seed=7)]
    with_long = [long_] + short if where == "first" else short + [long_]
    i_long = 0 if where == "first" else 2
    dev = gpu_device
    oracles = {}

    def oracle(s):
        if id(s) not in oracles:
            oracles[id(s)] = util.oracle_forward(s)
        return oracles[id(s)]

    for step, batch in enumerate((short_only, with_long, with_long, short_only)):
        b = util.HipBatch(batch, dev, slots=slots)
        for k, (v, s) in enumerate(zip(b, batch)):
            name = f"long{P}-{where} step{step} view{k}"
            mtl = v.counts.max_tile_list
            if s is long_:
                assert lo < mtl <= hi, (name, mtl)
            else:
                assert mtl <= 1024, (name, mtl)
            _check_forward(oracle(s), v, name)
        if batch is with_long:
            from oracle import oracle as orc
            dpixs = [_dpix(s.camera.image_height, s.camera.image_width, 100 * step + k) for k, s in enumerate(batch)]
            hb = b.backward_all(dpixs)
            for k, s in enumerate(batch):
                ob = orc.backward(oracle(s), dpixs[k])
                # (the bounds of test_long_tile_lists_take_the_multi_wave_and_fallback_sorts for the long view)
                assert util.rel_l2(hb[k]["dL_dmeans2D"], ob.dL_dmeans2D) < 1e-4, (P, where, step, k)
                assert util.rel_l2(hb[k]["dL_dopacity"], ob.dL_dopacity) < 1e-4, (P, where, step, k)
        if step == 1:   # the long view of the surprise batch against the same view with the big sorter (step 2)
            first = _forward_bits(b[i_long])
        if step == 2:
            _same_bits(_forward_bits(b[i_long]), first, (P, where))


# ------------------------------------------------------------------ d. growth inside a batch
def _dense_scene():
    # ~2 M instances: past 4 P + 65 536 and past 8 x 64 keys per (tile, XCD) bucket
    return scenes.random_scene(6000, 128, 128, sh_degree=0, seed=5, opacity_lo=0.6, opacity_hi=0.99, scale_lo=0.02, scale_hi=0.08)


def _forward_batch_raw(b, caps):
    """fr_forward_batch straight through the ABI on the views' own tensors, with the binning capacities `caps`."""
    import torch
    from fateavatar_amd import _lib, rasterizer
    L = _lib.lib()
    K = len(b)
    prms = [rasterizer._params(v.means3D.shape[0], v.s.sh_degree, v.sh.shape[1] if v.sh.numel() else 0, v.W, v.H,
                               v.s.camera.tanfovx, v.s.camera.tanfovy, v.mod, False, False) for v in b]
    inps = [rasterizer._inputs(v.bg, v.means3D, v.sh, v.colors, v.op, v.scales, v.rots, v.cov, v.view, v.proj, v.campos) for v in b]
    bins = [torch.empty((L.fr_binning_bytes(c, v.W, v.H),), dtype=torch.uint8, device=b.dev) for v, c in zip(b, caps)]
    outs = [(torch.empty_like(v.color), torch.empty_like(v.radii), torch.empty_like(v.geom), torch.empty_like(v.img)) for v in b]
    arr = lambda ts: (C.c_void_p * K)(*[t.data_ptr() for t in ts])  # noqa: E731
    counts = (_lib.fr_counts * K)()
    rc = L.fr_forward_batch(K, (C.c_void_p * K)(*[_lib.handle(b.dev.index or 0, sl) for sl in b.slots]),
                            (C.POINTER(_lib.fr_params) * K)(*[C.pointer(p) for p in prms]),
                            (C.POINTER(_lib.fr_inputs) * K)(*[C.pointer(i) for i in inps]),
                            arr([o[0] for o in outs]), arr([o[1] for o in outs]), arr([o[2] for o in outs]), arr([o[3] for o in outs]),
                            arr(bins), (C.c_uint64 * K)(*caps), counts, torch.cuda.current_stream(b.dev).cuda_stream)
    torch.cuda.synchronize(b.dev)
    return rc, [(c.num_rendered, c.num_instances, c.max_tile_list, c.overflow) for c in counts]


def test_growth_inside_a_batch(gpu_device, monkeypatch):
    """A dense view overflows its initial binning capacity AND its initial key buckets while the batch's other views fit:
    the retry regrows that view only, and every view matches the oracle.  Then, through the ABI, one view at half its
    need: FR_ERR_BINNING_CAPACITY, the overflow flag of that view only, its true need reported.  Then the same slots for
    larger images (the tile grid grows: counters and buckets reallocated) and for smaller ones (stale, larger buffers)."""
    from fateavatar_amd import _lib, rasterizer
    dev = gpu_device
    slots = [120, 121, 122]
    rasterizer._capacity_hint.clear()
    L = _lib.lib()
    calls = []
    real = L.fr_forward_batch

    def spy(K, handles, prm, inp, *rest):
        rc = real(K, handles, prm, inp, *rest)
        counts = rest[-2]
        calls.append((rc, [int(counts[k].overflow) for k in range(K)]))
        return rc
    small = [scenes.random_scene(800, 40, 56, sh_degree=2, seed=21), scenes.random_scene(300, 24, 17, sh_degree=1, seed=22, M=16)]
    batch = [small[0], _dense_scene(), small[1]]
    with monkeypatch.context() as mp:   # (its own context: the module's capacity-guess patch stays in place)
        mp.setattr(L, "fr_forward_batch", spy)
        b = util.HipBatch(batch, dev, slots=slots)
    assert L.fr_forward_batch is real
    assert calls[0] == (_lib.FR_ERR_BINNING_CAPACITY, [0, 1, 0]), calls
    assert calls[-1][0] == _lib.FR_OK and len(calls) >= 2, calls
    need = [v.counts.num_instances for v in b]
    assert need[1] > 4 * batch[1].P + 65536 and b[1].counts.max_tile_list > 8 * 64, (need, b[1].counts.max_tile_list)
    names = [f"growth[{k}]" for k in range(3)]
    _check_views(b, batch, [{}] * 3, [_dpix(s.camera.image_height, s.camera.image_width, k) for k, s in enumerate(batch)], names)
    # ---- one view at half its need, the others at theirs: only that view overflows, and it reports what it needs
    for j in (1, 2):
        caps = [n + 1024 for n in need]
        caps[j] = max(1, need[j] // 2)
        rc, cnt = _forward_batch_raw(b, caps)
        assert rc == _lib.FR_ERR_BINNING_CAPACITY, (j, rc)
        assert [c[3] for c in cnt] == [int(k == j) for k in range(3)], (j, cnt)
        assert cnt[j][1] == need[j], (j, cnt, need)
    # ---- larger images on the same slots (tile grid grows), then smaller ones (stale, larger buffers)
    for tag, specs in (("larger", [(3000, 300, 420), (6000, 260, 130), (2500, 180, 700)]),
                       ("smaller", [(1000, 24, 40), (700, 33, 9), (1800, 64, 64)])):
        batch = [scenes.random_scene(P, H, W, sh_degree=k, seed=30 + k, opacity_lo=0.1, opacity_hi=0.9)
                 for k, (P, H, W) in enumerate(specs)]
        alone = _alone(batch, [{}] * 3, dev)
        b = util.HipBatch(batch, dev, slots=slots)
        _assert_same_bits(b, alone, tag)
        _check_views(b, batch, [{}] * 3, [_dpix(s.camera.image_height, s.camera.image_width, 7 + k) for k, s in enumerate(batch)],
                     [f"growth-{tag}[{k}]" for k in range(3)])


# ------------------------------------------------------------------ e. the benchmark's regime
def _config2_views(n, opacity=0.1):
    return [scenes.head_scene(view=k, n_views=n, opacity=opacity) for k in range(n)]


@pytest.mark.parametrize("opacity", [0.1, 0.9])
def test_config2_four_view_batch(opacity, gpu_device):
    """K = 4 views of BASELINE config 2 (head template, 100 k Gaussians, 512^2, SH degree 3) in one batch, at the initial
    opacity and at the one training reaches: every view bit-equal to its view alone and held to the single-frame bounds of
    test_config2_head_100k_512_forward_backward / test_config2_at_the_opacity_training_reaches."""
    scs = _config2_views(4, opacity)
    alone = _alone(scs, [{}] * 4, gpu_device)
    b = util.HipBatch(scs, gpu_device)
    _assert_same_bits(b, alone, f"config2x4-{opacity}")
    for k, (v, s) in enumerate(zip(b, scs)):
        name = f"config2x4-op{opacity}[{k}]"
        o = util.oracle_forward(s)
        _check_forward(o, v, name)
        assert v.counts.num_rendered == o.num_rendered
        # every view in the regime of the single-frame tests: the 4-wave medium sorter's tier, and at opacity 0.9 the early
        # termination share of test_config2_at_the_opacity_training_reaches
        assert 256 < v.counts.max_tile_list <= 1024, (name, v.counts.max_tile_list)
        terminated = float((o.final_T < 1e-3).mean())
        print(f"[opaque] {name}: {terminated:.1%} of the pixels end below T = 1e-3, max list {v.counts.max_tile_list}")
        if opacity >= 0.9:
            assert terminated > 0.15, (name, terminated)
        _check_backward(o, v, _dpix(512, 512, 11 + k), name, max_skip_frac=0.005 if opacity == 0.1 else 0.02)


class _GraphView:
    """View j of a captured launch chain, as the in-flight rounds left it: the forward outputs, the blend records and the
    gradients are copied to the host right after the rounds, before anything replays the chain again.  `backward(dpix)`
    returns those gradients when `dpix` is the upstream gradient the chain was captured with; any other dpix (the masked one
    of the no-exemption path) is written into the chain's static upstream gradient and the chain is replayed alone."""

    def __init__(self, chain, j, s, num_rendered):
        import torch
        from fateavatar_amd import rasterizer
        fw, self.chain, self.j, self.s = chain["fw"][j], chain, j, s
        self.num_rendered = num_rendered
        self.means3D, self.geom = chain["views"][j].means3D, fw[3]
        self.color, self.radii = fw[1].cpu(), fw[2].cpu()
        final_T, n_contrib = rasterizer.image_aux(fw[5], s.camera.image_height, s.camera.image_width)
        self.final_T, self.n_contrib = final_T.cpu(), n_contrib.cpu()
        self._rec = util._Frame.geometry(self, 8, 12)
        self.dpix_host = chain["dts"][j].cpu().numpy()
        self.grads = {k: a.cpu().numpy() for k, a in zip(util.GRAD_NAMES, chain["bw"][j])}
        torch.cuda.synchronize()

    def geometry(self, field, cols):
        assert field in (0, 1, 3, 8), field   # (the fields of the blend-record template: copied with the other outputs)
        return self._rec if field == 8 else util._Frame.geometry(self, field, cols)

    def backward(self, dpix):
        import torch
        if np.array_equal(dpix, self.dpix_host):
            return self.grads
        self.chain["dts"][self.j].copy_(torch.from_numpy(dpix))
        with torch.cuda.stream(self.chain["stream"]):
            self.chain["graph"].replay()
        torch.cuda.synchronize()
        return {k: a.cpu().numpy() for k, a in zip(util.GRAD_NAMES, self.chain["bw"][self.j])}


def test_bench_shape_three_chains_of_four_in_flight(gpu_device):
    """The shape bench.py times: 3 launch chains x 4-view batches of config 2 (12 views around the head, 12 handles), each
    chain on its own stream, captured as ONE graph (forward + backward) and replayed in flight with the others for 20
    rounds.  Every view's image, forward state and gradients are then held to the oracle with the single-frame bounds."""
    import torch
    from fateavatar_amd import rasterizer
    dev = gpu_device
    scs = _config2_views(12)
    chains = []
    for c in range(3):
        grp = scs[4 * c:4 * c + 4]
        slots = [124 + 4 * c + j for j in range(4)]   # (12 handles, as the bench's: none shared with another chain)
        b = util.HipBatch(grp, dev, slots=slots)    # eager first: the handles' buffers are sized outside the capture
        b.backward_all([None] * 4)
        dts = [torch.from_numpy(_dpix(512, 512, 11 + 4 * c + j)).to(dev) for j in range(4)]
        stream = torch.cuda.Stream(device=dev)
        ch = dict(views=b.views, stream=stream)

        def frame():
            fw = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in b.views], slots=slots)
            bw = rasterizer.rasterize_gaussians_backward_batch([v._backward_args(d, f) for v, f, d in zip(b.views, fw, dts)],
                                                               slots=slots)
            return fw, bw
        torch.cuda.synchronize()
        with rasterizer.no_wait():
            stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(stream):
                frame()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
                fw, bw = frame()
        ch.update(graph=g, fw=fw, bw=bw, dts=dts, slots=slots)
        chains.append(ch)
    torch.cuda.synchronize()
    for _ in range(20):   # in flight together, as bench.py's rounds
        for ch in chains:
            with torch.cuda.stream(ch["stream"]):
                ch["graph"].replay()
    torch.cuda.synchronize()
    for c, ch in enumerate(chains):
        for sl in ch["slots"]:
            with rasterizer.handle_slot(sl):
                assert not rasterizer.check_async_overflow(dev.index or 0), (c, sl)
    # every output of the in-flight rounds to the host BEFORE any check: a check that replays a chain (the no-exemption
    # path) must not overwrite what the other views are checked on
    views = []
    for c, ch in enumerate(chains):
        for j in range(4):
            counts = rasterizer.read_counts(dev.index or 0, ch["slots"][j])
            views.append(_GraphView(ch, j, scs[4 * c + j], int(counts.num_rendered)))
    for k, gv in enumerate(views):
        o = util.oracle_forward(scs[k])
        name = f"bench-chain{k // 4}[{k % 4}]"
        _check_forward(o, gv, name)
        _check_backward(o, gv, _dpix(512, 512, 11 + k), name, max_skip_frac=0.005)


# ------------------------------------------------------------------ f. per-view options in the backward
def test_backward_options_differ_per_view(gpu_device):
    """accumulates / outs / stats given per view of one fr_backward_batch: every accumulated array = old + gradient with
    culled rows untouched, the other arrays overwritten, the densification statistics of the one view that asks for them
    (test_backward_accumulates_into_the_arrays_it_is_told_to and test_fused_visibility_mask_and_densification_stats, per
    view of a batch)."""
    import torch
    dev = gpu_device
    scs = []
    for k in range(3):
        s = scenes.head_scene(P=3000, res=96, sh_degree=3, seed=12 + k, opacity=0.5, view=k, n_views=3)
        s.means3D[k::7] += 100.0          # out of the frustum: culled
        scs.append(s)
    b = util.HipBatch(scs, dev, slots=[0, 1, 2])
    names = util.GRAD_NAMES
    dpixs = [_dpix(96, 96, k) for k in range(3)]
    plain = b.backward_all(dpixs, as_numpy=False)
    added = [names, ("dL_dsh", "dL_dopacity"), ()]
    gen = torch.Generator().manual_seed(5)
    olds, outs = [], []
    for k in range(3):
        old = {n: torch.randn(plain[k][n].shape, generator=gen).to(dev) * float(plain[k][n].abs().max()) for n in names}
        olds.append(old)
        outs.append({n: old[n].clone() for n in names})
    P = [s.P for s in scs]
    acc, den = torch.rand((P[1], 1), device=dev), torch.zeros((P[1], 1), device=dev)
    acc0 = acc.clone()
    stats = [None, (acc, den), None]
    got = b.backward_all(dpixs, outs=outs, accumulates=added, stats=stats, as_numpy=False)
    for k in range(3):
        culled = b[k].radii == 0
        assert int(culled.sum()) >= 3000 // 7
        for n in names:
            assert got[k][n].data_ptr() == outs[k][n].data_ptr()
            want = olds[k][n] + plain[k][n] if n in added[k] else plain[k][n]
            tol = 2e-6 * max(float(plain[k][n].abs().max()), 1e-30)
            assert float((got[k][n] - want).abs().max()) <= tol, (k, n)
            if n in added[k]:
                assert torch.equal(got[k][n][culled], olds[k][n][culled]), (k, n)
            else:
                assert float(got[k][n][culled].abs().max()) == 0.0, (k, n)
    vis = (b[1].radii > 0).view(-1, 1)
    g2 = plain[1]["dL_dmeans2D"]
    want_acc = acc0 + torch.where(vis, torch.norm(g2[:, :2], dim=-1, keepdim=True), torch.zeros_like(acc0))
    assert float((acc - want_acc).abs().max()) <= 1e-6 * max(float(want_acc.abs().max()), 1e-30)
    assert torch.equal(den, vis.float())


def test_non_finite_view_leaves_the_other_views_alone(gpu_device):
    """A view with non-finite Gaussians (test_non_finite_gaussians_are_dropped_not_propagated's contract) next to clean
    views: it renders as its clean scene does, and the other views' outputs are bit for bit those of the same batch with
    the clean scene in its place (gradients: to atomic-summation order)."""
    dev = gpu_device
    s = scenes.random_scene(1500, 64, 80, sh_degree=1, seed=31)
    bad = np.zeros(s.P, bool)
    bad[[3, 400, 777, 1200, 55, 910]] = True
    clean = scenes.GaussianScene(s.means3D[~bad], s.scales[~bad], s.rotations[~bad], s.opacities[~bad], s.shs[~bad],
                                 s.sh_degree, s.bg, s.camera)
    s.opacities[3, 0] = np.nan
    s.scales[400, 1] = np.inf
    s.means3D[777, 0] = np.nan
    s.opacities[1200, 0] = -np.inf
    s.shs[55, 2, 1] = np.nan
    s.shs[910, 0, 0] = np.inf
    others = [scenes.random_scene(2500, 96, 72, sh_degree=3, seed=32), scenes.head_scene(P=20000, res=128, sh_degree=2, seed=1)]
    dpixs = [_dpix(96, 72, 1), _dpix(64, 80, 2), _dpix(128, 128, 3)]
    b1 = util.HipBatch([others[0], s, others[1]], dev)
    g1 = b1.backward_all(dpixs)
    b2 = util.HipBatch([others[0], clean, others[1]], dev)
    g2 = b2.backward_all(dpixs)
    assert (b1[1].radii.cpu().numpy()[bad] == 0).all()
    assert b1[1].num_rendered == b2[1].num_rendered, (b1[1].num_rendered, b2[1].num_rendered)
    assert np.isfinite(b1[1].color.cpu().numpy()).all()
    assert np.array_equal(b1[1].color.cpu().numpy(), b2[1].color.cpu().numpy())
    assert np.array_equal(b1[1].final_T.cpu().numpy(), b2[1].final_T.cpu().numpy())
    for k in ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_drotations"):
        assert np.isfinite(g1[1][k]).all() and np.abs(g1[1][k][bad]).max() == 0, k
        assert util.rel_l2(g1[1][k][~bad], g2[1][k]) < 1e-5, k
    for j in (0, 2):
        _same_bits(_forward_bits(b1[j]), _forward_bits(b2[j]), j)
        for k in util.GRAD_NAMES:
            assert np.isfinite(g1[j][k]).all() and util.rel_l2(g1[j][k], g2[j][k]) < 1e-5, (j, k)


# ------------------------------------------------------------------ g. environment-selected paths in a batch
_MODE_CODE = r"""
import sys; sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from fateavatar_amd import rasterizer, scenes
from tests import util
from tests.test_gpu_parity import _check_forward, _check_backward
dev = torch.device('cuda:0')
cols = np.random.default_rng(4).uniform(0, 1, (4000, 3)).astype(np.float32)
scs = [scenes.head_scene(P=20000, res=256, sh_degree=1, seed=0, opacity=0.5),
       scenes.random_scene(4000, 64, 64, sh_degree=0, seed=5, opacity_lo=0.6, opacity_hi=0.99, scale_lo=0.02, scale_hi=0.08),
       scenes.random_scene(4000, 90, 70, sh_degree=2, seed=6, opacity_lo=0.1, opacity_hi=0.9),
       scenes.random_scene(1500, 37, 51, sh_degree=3, seed=7, M=16, bg=(0.2, 0.4, 0.6))]
kws = [{}, {}, dict(colors_precomp=cols), dict(scale_modifier=0.7)]
if sys.argv[2] == 'gather':
    try:
        util.HipBatch(scs, dev, per_view_kwargs=kws)
        raise SystemExit('a batch was accepted under FR_BLEND_FWD=gather')
    except RuntimeError as e:
        assert '(code 4)' in str(e), str(e)
    scs, kws = scs[:1], kws[:1]
b = util.HipBatch(scs, dev, per_view_kwargs=kws)
for k, (v, s, kw) in enumerate(zip(b, scs, kws)):
    o = util.oracle_forward(s, **kw)
    _check_forward(o, v, f'mode[{k}]')
    H, W = s.camera.image_height, s.camera.image_width
    _check_backward(o, v, (np.random.default_rng(k).uniform(-1, 1, (3, H, W)) / (H * W)).astype(np.float32), f'mode[{k}]')
assert all(v.counts.max_tile_list > 64 for v in b[:2])
print('mode-ok')
"""


@pytest.mark.parametrize("mode", ["FR_BLEND_FWD=gather", "FR_CHAIN_SPINS=0", "FR_CHAIN_SPINS=3",
                                  "FR_DENSE_PAIRS_FWD=0,FR_DENSE_PAIRS_BWD=0", "FR_DENSE_PAIRS_FWD=9999,FR_DENSE_PAIRS_BWD=9999",
                                  "FR_HEAVY_PAIRS=0", "FR_HEAVY_PAIRS=99999"])
def test_selectable_blend_paths_in_a_batch(gpu_device, mode):
    """test_selectable_blend_paths_stay_correct for a 4-view heterogeneous batch (SH views of two degrees, a colors_precomp
    view, a scale_modifier view; long and short lists): every view against the oracle.  The gather as a launch of its own
    serves one view only: a batch must be refused (FR_ERR_UNSUPPORTED), one view must still be right.  In a subprocess (the
    switches are read at handle creation), one at a time, under a timeout."""
    env = dict(os.environ)
    for kv in mode.split(","):
        k, v = kv.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, "-c", _MODE_CODE, ROOT, "gather" if "gather" in mode else "batch"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mode-ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
