"""-m gpu: depth / alpha planes (FR_FLAG_DEPTH_ALPHA) on LONG tile lists, against the CPU oracle alone (tests/planes_ref.py).

The planes have kernel instances of their own at every stage — tile_sort_body<true>, unit_blend_chained_body<*, true>,
gather_tile<*, *, true> with its depth_state rows, unit_blend_bwd_sparse_body<true>, k_preprocess_bwd_planes — and
tests/test_gpu_depth_alpha.py reaches them on short lists, or on long ones only in a batch whose slots a plain frame has
armed.

The scenes: one 8x8 tile with 700 / 1 400 / 3 000 / 6 000 translucent entries (every sort tier, exact depth ties); an opaque
scene whose pixels terminate ~880 entries into lists of 3 000 / 6 000 (dozens of wholly dead trailing units); and, because
the pixels of both end within the first fourteen units of their lists, so that a wrong entry state of a later unit would
reach no gradient, the one-tile scene at opacities so low that its pixels blend to the very end of their lists, some 1 600
contributors each ("deep").

The launch forms: single and in a batch, the long list met as a SURPRISE (k_tile_sort_planes' own slow path) and with the big
sorter armed; forward-only; one plane gradient at a time; the gather as a launch of its own; every hand-off of the chain
through its fallback.

What makes a surprise, and how it is proven: the host launches the big sorter unless the handle's last counts show no list
above 2 048, and a frame whose (tile, XCD) key buckets overflow sorts nothing at all: it reports what it needs and is repeated
— by then its own counts have armed the big sorter.  A handle's buckets start at 64 keys and never shrink.  So every sequence
is long (grows the buckets) -> short (the counts say: no long list) -> long (the surprise) -> long (armed), and the surprise
and the armed frame each run under `one_attempt`, which asserts that the ABI's forward was entered once and returned FR_OK:
no overflow, no repeat, hence — with the short frame before it — no big sorter for the surprise.

Checks per planes frame (the reference: PlanesRef of the scene, nothing compiled from the code under test):
 (F1) the plain outputs pass `_check_forward` of tests/test_gpu_parity.py;
 (F2) alpha == 1 - final_T bit for bit, depth == alpha == 0 where n_contrib == 0, both planes finite;
 (F3) outside util.flip_pixels, |depth - ref| and |alpha - ref| <= 1e-5 + 1e-4 |ref| (the forward tolerance: the depth row is
      summed like a colour channel); the flip pixels are capped by `_check_backward`'s formula;
 (B)  gradients of <gC, C> + <gD, D> + <gA, A> (seeded upstreams / (H W), zero at the flip pixels): all eight arrays finite,
      rel-L2 <= max(1e-4, NOISE_K x the oracle's own float-order floor), rows of culled Gaussians exactly zero.

The handles of this module: 240 .. 276 (no other module uses them); every parametrised case has slots of its own, since a
sequence starts from a handle whose history it knows."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from fateavatar_amd import scenes
from tests import util
from tests.planes_ref import PlanesRef, compare_gradients
from tests.test_gpu_batch_parity import _long_scene, _short_scenes
from tests.test_gpu_parity import _check_forward

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 240
TIERS = {700: (256, 1024), 1400: (1024, 2048), 3000: (2048, 4096), 6000: (4096, 1 << 30)}   # max_tile_list in (lo, hi]
OUTPUTS = ("image", "final_T", "n_contrib", "depth", "alpha")


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch, gpu_device):
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


# ------------------------------------------------------------------ scenes
def translucent_scene(P):
    """The plain long-list tests' own fixture: P Gaussians on one 8x8 tile, opacity 0.02 .. 0.05, exact depth ties."""
    return _long_scene(P)


def opaque_scene(P):
    """Image-sized opaque splats: every Gaussian reaches every tile, every pixel terminates long before the end of its list."""
    s = scenes.random_scene(P, 32, 32, sh_degree=0, seed=9, spread=0.004, scale_lo=0.05, scale_hi=0.1, opacity_lo=0.6,
                            opacity_hi=0.95)
    rng = np.random.default_rng(3)
    s.means3D[:, 2] = 1.0 + rng.uniform(0, 0.5, s.P).astype(np.float32)
    s.means3D[::7, 2] = 1.25   # exact depth ties
    return s


DEEP_OPACITY = {3000: (0.006, 0.012), 6000: (0.005, 0.009)}


def deep_scene(P):
    """translucent_scene's geometry at opacities just above the alpha >= 1/255 test: the pixels under the splats blend every
    entry of the list, so every unit's entry state (unit_state, depth_state) carries gradient."""
    s = scenes.random_scene(P, 32, 32, sh_degree=0, seed=9, spread=0.004, scale_lo=0.002, scale_hi=0.004,
                            opacity_lo=DEEP_OPACITY[P][0], opacity_hi=DEEP_OPACITY[P][1])
    rng = np.random.default_rng(3)
    s.means3D[:, 2] = 1.0 + rng.uniform(0, 0.5, s.P).astype(np.float32)
    s.means3D[::7, 2] = 1.25   # exact depth ties
    return s


def short_scene():
    return scenes.random_scene(1200, 40, 48, sh_degree=0, seed=7)


@functools.lru_cache(maxsize=None)
def ref_of(kind, P=0):
    """The oracle's side of a scene, computed once per process and never modified.  kind: 'translucent' / 'opaque' / 'deep' (P),
    'short', 'batch-short' (P: the index into _short_scenes())."""
    if kind == "translucent":
        return PlanesRef(translucent_scene(P))
    if kind == "opaque":
        return PlanesRef(opaque_scene(P))
    if kind == "deep":
        return PlanesRef(deep_scene(P))
    if kind == "short":
        return PlanesRef(short_scene())
    return PlanesRef(_short_scenes()[P])


def assert_dead_tails(ref, what):
    """On the ORACLE, before anything runs on the GPU: at least four 8x8 blocks whose every pixel has terminated
    (final_T < 2e-4) and whose deepest contributor sits at least 128 entries before the end of the list — i.e. the kernel-side
    list of such a block ends in wholly dead units.  A change to random_scene cannot silently make the case a translucent one."""
    o = ref.o
    gx = (ref.W + 15) // 16
    blocks, deepest, shortest = 0, 0, 1 << 30
    for by in range(0, ref.H, 8):
        for bx in range(0, ref.W, 8):
            t = (by // 16) * gx + bx // 16
            n = int(o.ranges[t, 1]) - int(o.ranges[t, 0])
            fT, nc = o.final_T[by:by + 8, bx:bx + 8], o.n_contrib[by:by + 8, bx:bx + 8]
            if fT.shape == (8, 8) and np.all(fT < 2e-4) and int(nc.max()) + 128 <= n:
                blocks += 1
                deepest, shortest = max(deepest, int(nc.max())), min(shortest, n)
    print(f"[dead tails] {what}: {blocks} fully terminated 8x8 block(s), deepest contributor {deepest}, shortest list {shortest}; "
          f"num_rendered {o.num_rendered}, covered pixels {int((o.n_contrib > 0).sum())} of {ref.H * ref.W}")
    assert blocks >= 4, (what, blocks)


def long_ref(kind, P):
    """ref_of, with the opaque scenes' dead tails and the deep scenes' depth re-asserted on the oracle (and printed) in every
    test that uses one."""
    r = ref_of(kind, P)
    if kind == "opaque":
        assert_dead_tails(r, f"opaque{P}")
    if kind == "deep":   # (the list's last unit still contributes, to a pixel that has not terminated)
        deepest, n_px = int(r.o.n_contrib.max()), int((r.o.n_contrib > P - 64).sum())
        print(f"[deep] deep{P}: deepest contributor {deepest} of {P}, {n_px} pixel(s) reach the last unit, final_T there "
              f"{float(r.o.final_T[r.o.n_contrib > P - 64].min(initial=1)):.1e} .. {float(r.o.final_T[r.o.n_contrib > P - 64].max(initial=0)):.1e}")
        assert n_px >= 2 and deepest > P - 64, (kind, P, deepest, n_px)
    return r


# ------------------------------------------------------------------ frames
def _view(s, dev):
    v = util._Frame()
    v._upload(s, dev)
    return v


def _outputs(v, res):
    from fateavatar_amd import rasterizer
    fT, nc = rasterizer.image_aux(res[5], v.H, v.W)
    return dict(image=res[1].cpu().numpy(), final_T=fT.cpu().numpy(), n_contrib=nc.cpu().numpy(), depth=res[6].cpu().numpy(),
                alpha=res[7].cpu().numpy())


def same_bits(a, b, what):
    for k in OUTPUTS:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def check_planes_forward(ref, v, res, what, full=True):
    """(F1) (frames with a backward hand-off: `full`), (F2), (F3) -> (the frame's five outputs, its flip pixels)."""
    o = ref.o
    out = _outputs(v, res)
    if full:
        v._take_forward(res[:6])
        _check_forward(o, v, what)
    depth, alpha, fT, nc = out["depth"], out["alpha"], out["final_T"], out["n_contrib"]
    assert depth.shape == (v.H, v.W) and alpha.shape == (v.H, v.W), what
    # (F2)
    assert np.array_equal(alpha.view(np.uint32), (np.float32(1) - fT).view(np.uint32)), (what, "alpha != 1 - final_T")
    empty = nc == 0
    assert np.all(depth[empty] == 0) and np.all(alpha[empty] == 0), (what, "a plane is not 0 where nothing contributed")
    assert np.isfinite(depth).all() and np.isfinite(alpha).all(), what
    # (F3)
    bad = util.flip_pixels(o, out["image"], fT)
    cap = max(3, int(1e-4 * v.H * v.W), int(1e-7 * 256 * o.num_rendered))
    rd, ra = ref.depth.astype(np.float64), ref.alpha.astype(np.float64)
    ed = np.abs(depth - rd) - (1e-5 + 1e-4 * np.abs(rd))
    ea = np.abs(alpha - ra) - (1e-5 + 1e-4 * np.abs(ra))
    ok = ~bad
    print(f"[planes forward] {what}: {int(bad.sum())} flip pixel(s) (cap {cap}), {int(empty.sum())} empty pixel(s); outside them "
          f"max |depth - ref| {float(np.abs(depth - ref.depth)[ok].max(initial=0)):.2e}, "
          f"max |alpha - ref| {float(np.abs(alpha - ref.alpha)[ok].max(initial=0)):.2e}")
    if int(bad.sum()) > cap:   # (a finding to explain, not a cap to raise)
        ys, xs = np.nonzero(bad)
        print("[planes forward] margins of the flip pixels:", [(x, y, util.explain_pixel(o, x, y)) for x, y in zip(xs.tolist(), ys.tolist())][:32])
    assert int(bad.sum()) <= cap, (what, "flip pixels", int(bad.sum()), cap)
    assert np.all(ed[ok] <= 0), (what, "depth", float(ed[ok].max()), np.argwhere(ok & (ed > 0))[:8].tolist())
    assert np.all(ea[ok] <= 0), (what, "alpha", float(ea[ok].max()), np.argwhere(ok & (ea > 0))[:8].tolist())
    return out, bad


def upstreams(H, W, seed, bad, which="CDA"):
    """Seeded uniform upstreams / (H W), zero at the flip pixels; a plane not in `which` is None, the colour then zero."""
    r = np.random.default_rng(seed)
    gC = (r.uniform(-1, 1, (3, H, W)) / (H * W)).astype(np.float32)
    gD = (r.uniform(-1, 1, (H, W)) / (H * W)).astype(np.float32)
    gA = (r.uniform(-1, 1, (H, W)) / (H * W)).astype(np.float32)
    gC[:, bad], gD[bad], gA[bad] = 0.0, 0.0, 0.0
    if "C" not in which:
        gC[:] = 0.0
    return gC, gD if "D" in which else None, gA if "A" in which else None


_EXPECTED = {}   # (ref, seed, which, flip pixels) -> PlanesRef.gradients: two bit-identical frames share one reference


def expected(ref, seed, which, bad):
    key = (id(ref), seed, which, bad.tobytes())
    if key not in _EXPECTED:
        _EXPECTED[key] = ref.gradients(*upstreams(ref.H, ref.W, seed, bad, which))
    return _EXPECTED[key]


def _dev_t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def hip_backward(v, res, gC, gD, gA, planes=True):
    """The backward of a planes frame on the current handle slot -> {array: numpy}."""
    import torch
    from fateavatar_amd import rasterizer
    kw = dict(_planes=(res[8], _dev_t(gD, v.dev), _dev_t(gA, v.dev))) if planes else {}
    got = rasterizer.rasterize_gaussians_backward(*v._backward_args(_dev_t(gC, v.dev), res[:6]), **kw)
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in zip(util.GRAD_NAMES, got)}


def check_planes_backward(ref, v, res, bad, what, seed, which="CDA"):
    """(B) on the current handle slot -> the HIP gradients."""
    got = hip_backward(v, res, *upstreams(v.H, v.W, seed, bad, which))
    want, floor, bound = expected(ref, seed, which, bad)
    compare_gradients(got, want, floor, bound, ref.o.radii <= 0, f"{what} [{which}]")
    return got


@contextlib.contextmanager
def one_attempt(what):
    """Every forward launched inside goes through the ABI ONCE and returns FR_OK: the frame overflowed neither its binning
    capacity nor its key buckets and was not repeated (rasterizer._launch_forward repeats a frame that reports
    FR_ERR_BINNING_CAPACITY), so the attempt that was checked is the attempt whose sort path the sequence set up."""
    from fateavatar_amd import _lib
    L = _lib.lib()
    real = {n: getattr(L, n) for n in ("fr_forward", "fr_forward_batch")}
    calls = []

    def spy(name):
        def f(*args):
            rc = real[name](*args)
            calls.append((name, rc))
            return rc
        return f
    for n in real:
        setattr(L, n, spy(n))
    try:
        yield calls
    finally:
        for n, fn in real.items():
            setattr(L, n, fn)
    print(f"[attempts] {what}: {calls}")
    assert len(calls) == 1 and calls[0][1] == _lib.FR_OK, (what, "the frame overflowed and was repeated", calls)


def _forward(v, forward_only=False):
    import torch
    from fateavatar_amd import rasterizer
    res = rasterizer.rasterize_gaussians(*v._forward_args(), _depth_alpha=True, _forward_only=forward_only)
    torch.cuda.synchronize()
    return res, rasterizer.last_counts[v.dev.index or 0].max_tile_list


@functools.lru_cache(maxsize=None)
def block_contributors(kind, P):
    """On the ORACLE: the largest number of Gaussians that blend into some pixel of one 8x8 block (power <= 0 and alpha clear of
    the 1/255 test by 0.1 %, far outside fp32 rounding).  Each of them has to be in the kernel's list of that tile, whatever its
    footprint test leaves out: a lower bound of max_tile_list that owes nothing to the code under test."""
    r = ref_of(kind, P)
    o, f32, gx, best = r.o, np.float32, (r.W + 15) // 16, 0
    for by in range(0, r.H, 8):
        for bx in range(0, r.W, 8):
            tl = (by // 16) * gx + bx // 16
            ids = o.point_list[int(o.ranges[tl, 0]):int(o.ranges[tl, 1])].astype(np.int64)
            if ids.size == 0 or not (o.n_contrib[by:by + 8, bx:bx + 8] > 0).any():
                continue
            xy, co = o.means2D[ids], o.conic_opacity[ids]
            hit = np.zeros(ids.size, bool)
            for y in range(by, min(by + 8, r.H)):
                for x in range(bx, min(bx + 8, r.W)):
                    dx, dy = (xy[:, 0] - f32(x)).astype(f32), (xy[:, 1] - f32(y)).astype(f32)
                    power = (f32(-0.5) * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy).astype(f32)
                    hit |= (power <= 0) & (co[:, 3] * np.exp(np.minimum(power, f32(0))) >= f32(1.001 / 255.0))
            best = max(best, int(hit.sum()))
    return best


def _assert_tier(kind, P, mtl, what):
    if kind == "deep":
        # (the kernel's footprint test drops (tile, Gaussian) pairs whose alpha cannot reach 1/255 in the tile, so its list is
        # shorter than the oracle's 16x16 list: held between the oracle's contributors of one block and P; with more than
        # 1 024 entries the tile has more than 8 units and the 4-wave sorts; which tier beyond that is printed, not asserted)
        need = block_contributors(kind, P)
        print(f"[tier] {what}: max_tile_list {mtl}, the oracle blends {need} Gaussians into one 8x8 block (> 1024), P = {P}")
        assert 1024 < need <= mtl <= P, (what, need, mtl)
        return
    lo, hi = TIERS[P]
    print(f"[tier] {what}: max_tile_list {mtl} in ({lo}, {hi}]")
    assert lo < mtl <= hi, (what, mtl)


# ------------------------------------------------------------------ 1. single launch: surprise, then armed
def run_single(kind, P, slot, dev):
    """Fresh handle: the long planes frame (grows the key buckets), a short one (its counts say: no long list), the long frame
    as a surprise (for lists > 2 048 sorted by k_tile_sort_planes' own slow path: no big sorter was launched), the long frame
    again (big sorter armed), the short frame again.  (F1) - (F3) on every frame, (B) after the surprise and the armed frame,
    the three long frames' outputs bit-identical."""
    from fateavatar_amd import rasterizer
    ref, ref_s = long_ref(kind, P), ref_of("short")
    vl, vs = _view(ref.s, dev), _view(ref_s.s, dev)
    name = f"{kind}{P}"
    outs = []
    with rasterizer.handle_slot(slot):
        for step, launch in enumerate(("grow", "short", "surprise", "armed", "short")):
            what = f"{name} step{step} {launch}"
            if launch == "short":
                res, mtl = _forward(vs)
                assert mtl <= 1024, (what, mtl)
                check_planes_forward(ref_s, vs, res, what)
                continue
            with one_attempt(what) if launch != "grow" else contextlib.nullcontext():
                res, mtl = _forward(vl)
            _assert_tier(kind, P, mtl, what)
            out, bad = check_planes_forward(ref, vl, res, what)
            if kind != "opaque":
                assert (out["n_contrib"] == 0).any(), (what, "no empty pixel: (F2)'s zero test checks nothing")
            if launch != "grow":
                check_planes_backward(ref, vl, res, bad, what, seed=1000 + P)
            outs.append(out)
    same_bits(outs[0], outs[1], (name, "first frame against surprise"))
    same_bits(outs[1], outs[2], (name, "surprise against armed"))


SINGLE = [("translucent", 700), ("translucent", 1400), ("translucent", 3000), ("translucent", 6000), ("opaque", 3000), ("opaque", 6000),
          ("deep", 3000), ("deep", 6000)]


@pytest.mark.parametrize("kind,P", SINGLE)
def test_single_launch_surprise_then_armed(kind, P, gpu_device):
    run_single(kind, P, SLOT + SINGLE.index((kind, P)), gpu_device)


# ------------------------------------------------------------------ 2. one plane gradient at a time
ONE_PLANE = [("opaque", 3000), ("translucent", 1400), ("deep", 3000)]


@pytest.mark.parametrize("kind,P", ONE_PLANE)
def test_one_plane_gradient_at_a_time(kind, P, gpu_device):
    """unit_blend_bwd_sparse_body<true> loads depth_state only when dL_ddepth is non-null: (scratch, gD, None) and
    (scratch, None, gA), each with gC = 0, each against (B) with the other upstream zero; their sum plus the plain backward of
    gC agrees with the backward of all three inside the same bounds."""
    from fateavatar_amd import rasterizer
    ref = long_ref(kind, P)
    v = _view(ref.s, gpu_device)
    name, seed = f"one-plane {kind}{P}", 2000 + P
    with rasterizer.handle_slot(SLOT + len(SINGLE) + ONE_PLANE.index((kind, P))):
        res, mtl = _forward(v)
        _assert_tier(kind, P, mtl, name)
        _, bad = check_planes_forward(ref, v, res, name)
        g_d = check_planes_backward(ref, v, res, bad, name, seed, "D")
        g_a = check_planes_backward(ref, v, res, bad, name, seed, "A")
        g_all = check_planes_backward(ref, v, res, bad, name, seed, "CDA")
        gC = upstreams(v.H, v.W, seed, bad)[0]
        g_c = hip_backward(v, res, gC, None, None, planes=False)   # (the plain kernels on the planes frame's buffers)
    _, floor, bound = expected(ref, seed, "CDA", bad)
    for k in util.GRAD_NAMES:
        if g_all[k].size == 0:
            continue
        total = g_d[k].astype(np.float64) + g_a[k] + g_c[k]
        rl = util.rel_l2(total, g_all[k])
        print(f"[planes gradient] {name} {k}: depth-only + alpha-only + colour-only against all three: rel-L2 {rl:.2e} (bound {bound[k]:.1e})")
        assert rl <= bound[k], (name, k, rl, bound[k])
        assert np.any(g_d[k]) or k in ("dL_dcolors", "dL_dsh"), (name, k, "the depth gradient reaches nothing")


# ------------------------------------------------------------------ 3. batches: the long view first and last
def _batch_refs(kind, P, where):
    short = [ref_of("batch-short", 0), ref_of("batch-short", 1)]
    return [long_ref(kind, P)] + short if where == "first" else short + [long_ref(kind, P)]


def _forward_batch(views, slots, forward_only=False):
    import torch
    from fateavatar_amd import rasterizer
    res = rasterizer.rasterize_gaussians_batch([v._forward_args() for v in views], slots=slots, depth_alpha=True,
                                               forward_only=forward_only)
    torch.cuda.synchronize()
    return res, [rasterizer.read_counts(views[0].dev.index or 0, sl).max_tile_list for sl in slots]


def _short_only_batch(dev, slots, what):
    """A batch of short planes frames: afterwards every handle's counts say that no list is long, and the next launch does not
    start the big sorter."""
    refs = [ref_of("batch-short", 0), ref_of("batch-short", 1), ref_of("short")]
    views = [_view(r.s, dev) for r in refs]
    res, mtls = _forward_batch(views, slots)
    for k, (r, v) in enumerate(zip(refs, views)):
        assert mtls[k] <= 1024, (what, k, mtls[k])
        check_planes_forward(r, v, res[k], f"{what} short-only view{k}")


BATCHES = [("translucent", 6000, "first"), ("translucent", 6000, "last"), ("opaque", 3000, "first"), ("opaque", 3000, "last")]


def _check_batch_forward(kind, P, refs, views, res, mtls, i_long, what, full=True):
    """Tier per view and (F1) - (F3) per view -> per view (outputs, flip pixels)."""
    out = []
    for k, (r, v) in enumerate(zip(refs, views)):
        if k == i_long:
            _assert_tier(kind, P, mtls[k], f"{what} view{k}")
        else:
            assert mtls[k] <= 1024, (what, k, mtls[k])
        out.append(check_planes_forward(r, v, res[k], f"{what} view{k}", full=full))
    return out


@pytest.mark.parametrize("kind,P,where", BATCHES)
def test_batch_with_the_long_view_first_and_last(kind, P, where, gpu_device):
    """No plain batch renders on these slots.  The batch with the long view (grows its handle's buckets), short planes frames
    only, then the batch with the long view twice: the first launch meets the long list as a surprise
    (k_tile_sort_planes_batch's slow path), the second runs the big sorter for all views.  (F1) - (F3) per view after every
    launch, (B) per view after the surprise and the armed launch; the long view's outputs are bit-identical across all three."""
    from fateavatar_amd import rasterizer
    import torch
    dev = gpu_device
    slots = [SLOT + 11 + 3 * BATCHES.index((kind, P, where)) + j for j in range(3)]
    name = f"batch {kind}{P}-{where}"
    refs = _batch_refs(kind, P, where)
    i_long = 0 if where == "first" else 2
    views = [_view(r.s, dev) for r in refs]
    outs = []
    for launch in ("grow", "short", "surprise", "armed"):
        if launch == "short":
            _short_only_batch(dev, slots, name)
            continue
        what = f"{name} {launch}"
        with one_attempt(what) if launch != "grow" else contextlib.nullcontext():
            res, mtls = _forward_batch(views, slots)
        checked = _check_batch_forward(kind, P, refs, views, res, mtls, i_long, what)
        outs.append(checked[i_long][0])
        if launch == "grow":
            continue
        bads = [c[1] for c in checked]
        ups = [upstreams(v.H, v.W, 3000 + k, bad) for k, (v, bad) in enumerate(zip(views, bads))]
        got = rasterizer.rasterize_gaussians_backward_batch(
            [v._backward_args(_dev_t(u[0], dev), r[:6]) for v, u, r in zip(views, ups, res)], slots=slots,
            planes=[(r[8], _dev_t(u[1], dev), _dev_t(u[2], dev)) for u, r in zip(ups, res)])
        torch.cuda.synchronize()
        for k, (r, bad) in enumerate(zip(refs, bads)):
            want, floor, bound = expected(r, 3000 + k, "CDA", bad)
            compare_gradients({n: a.cpu().numpy() for n, a in zip(util.GRAD_NAMES, got[k])}, want, floor, bound, r.o.radii <= 0,
                              f"{what} view{k}")
    same_bits(outs[0], outs[1], (name, "first launch against surprise"))
    same_bits(outs[1], outs[2], (name, "surprise against armed"))


# ------------------------------------------------------------------ 4. forward-only planes
def run_forward_only_single(kind, P, slot, dev):
    """gather_tile<*, true, true>'s long branch (more than 8 units on a tile): the long planes frame in full (grows the key
    buckets; the bits to compare with), a short forward-only planes frame, the long one forward-only as a surprise, the long
    one forward-only again (armed): the five outputs of the forward-only frames are the full frame's bits, (F2) and (F3) hold
    on their own, and a backward on a forward-only frame's buffers is refused before anything is enqueued."""
    from fateavatar_amd import rasterizer
    ref, ref_s = long_ref(kind, P), ref_of("short")
    vl, vs = _view(ref.s, dev), _view(ref_s.s, dev)
    name = f"forward-only {kind}{P}"
    with rasterizer.handle_slot(slot):
        res, mtl = _forward(vl)
        _assert_tier(kind, P, mtl, f"{name} full")
        full, _ = check_planes_forward(ref, vl, res, f"{name} full")
        res, mtl = _forward(vs, forward_only=True)
        assert mtl <= 1024, (name, mtl)
        check_planes_forward(ref_s, vs, res, f"{name} short", full=False)
        with one_attempt(f"{name} surprise"):
            res, mtl = _forward(vl, forward_only=True)
        _assert_tier(kind, P, mtl, f"{name} surprise")
        fo1, bad = check_planes_forward(ref, vl, res, f"{name} surprise", full=False)
        gC, gD, gA = upstreams(vl.H, vl.W, 4000 + P, bad)
        with pytest.raises(RuntimeError, match=r"\(code 1\).*forward-only"):
            rasterizer.rasterize_gaussians_backward(*vl._backward_args(_dev_t(gC, dev), res[:6]),
                                                    _planes=(res[8], _dev_t(gD, dev), _dev_t(gA, dev)))
        with one_attempt(f"{name} armed"):
            res, mtl = _forward(vl, forward_only=True)
        _assert_tier(kind, P, mtl, f"{name} armed")
        fo2, _ = check_planes_forward(ref, vl, res, f"{name} armed", full=False)
    same_bits(fo1, full, (name, "forward-only (surprise) against full"))
    same_bits(fo2, full, (name, "forward-only (armed) against full"))


FORWARD_ONLY = [("opaque", 3000), ("translucent", 6000)]
FORWARD_ONLY_BATCHES = [(kind, P, where) for kind, P in FORWARD_ONLY for where in ("first", "last")]


@pytest.mark.parametrize("kind,P", FORWARD_ONLY)
def test_forward_only_planes_single(kind, P, gpu_device):
    run_forward_only_single(kind, P, SLOT + 23 + FORWARD_ONLY.index((kind, P)), gpu_device)


@pytest.mark.parametrize("kind,P,where", FORWARD_ONLY_BATCHES)
def test_forward_only_planes_in_a_batch(kind, P, where, gpu_device):
    """The batches of case 3 (long view first and last): in full (grows the buckets; the bits to compare with), short frames
    only, forward-only as a surprise, forward-only again (armed)."""
    from fateavatar_amd import rasterizer
    dev = gpu_device
    slots = [SLOT + 25 + 3 * FORWARD_ONLY_BATCHES.index((kind, P, where)) + j for j in range(3)]
    name = f"forward-only batch {kind}{P}-{where}"
    refs = _batch_refs(kind, P, where)
    i_long = 0 if where == "first" else 2
    views = [_view(r.s, dev) for r in refs]
    outs = {}
    for launch in ("full", "short", "surprise", "armed"):
        if launch == "short":
            _short_only_batch(dev, slots, name)
            continue
        fo = launch != "full"
        with one_attempt(f"{name} {launch}") if fo else contextlib.nullcontext():
            res, mtls = _forward_batch(views, slots, forward_only=fo)
        outs[launch] = _check_batch_forward(kind, P, refs, views, res, mtls, i_long, f"{name} {launch}", full=not fo)
        if launch == "surprise":
            ups = [upstreams(v.H, v.W, 5000 + k, o[1]) for k, (v, o) in enumerate(zip(views, outs[launch]))]
            with pytest.raises(RuntimeError, match=r"\(code 1\).*forward-only"):
                rasterizer.rasterize_gaussians_backward_batch(
                    [v._backward_args(_dev_t(u[0], dev), r[:6]) for v, u, r in zip(views, ups, res)], slots=slots,
                    planes=[(r[8], _dev_t(u[1], dev), _dev_t(u[2], dev)) for u, r in zip(ups, res)])
    for k in range(len(views)):
        same_bits(outs["surprise"][k][0], outs["full"][k][0], (name, k, "forward-only (surprise) against full"))
        same_bits(outs["armed"][k][0], outs["full"][k][0], (name, k, "forward-only (armed) against full"))


# ------------------------------------------------------------------ 5. the gather as its own launch; the chain through its fallback
_CHILD = r"""
import sys; sys.path.insert(0, sys.argv[1])
import torch
from tests import test_gpu_planes_long_lists as t
dev = torch.device("cuda:0")
for j, (kind, P) in enumerate((("opaque", 3000), ("translucent", 1400), ("deep", 3000))):
    t.run_single(kind, P, t.SLOT + 2 * j, dev)
    t.run_forward_only_single(kind, P, t.SLOT + 2 * j + 1, dev)
print("planes-long-ok")
"""


@pytest.mark.parametrize("env", [{"FR_BLEND_FWD": "gather"}, {"FR_CHAIN_SPINS": "0"},
                                 {"FR_DENSE_PAIRS_FWD": "0", "FR_DENSE_PAIRS_BWD": "0"}],
                         ids=["gather-launch", "chain-spins-0", "sparse-pairs"])
def test_blend_forms_in_a_child_process(env, gpu_device):
    """k_tile_gather_planes / k_tile_gather_fwd_only_planes as launches of their own (their `!__all(dead)` skip leaves the
    depth_state rows of wholly dead units unwritten: the backward must not use them), every hand-off of the chain computed from
    memory, and the sparse forms of both blend kernels: case 1 and the forward-only case for opaque 3 000, translucent 1 400 and
    deep 3 000 (every unit's depth_state carries gradient there), in a fresh child process each (the switches are read when a handle is created), under a timeout."""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env={**os.environ, **env}, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "planes-long-ok" in r.stdout, (env, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
