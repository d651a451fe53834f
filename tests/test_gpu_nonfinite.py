"""-m gpu: the non-finite-Gaussian contract ("Non-finite inputs") through every frame path.

A Gaussian whose position, scale, rotation, opacity or colour is NaN / +-inf is dropped like a culled one: radius 0, no
contribution, zero gradient rows, and every other Gaussian renders exactly as if it were absent.  tests/test_gpu_parity.py,
test_gpu_batch_parity.py and test_gpu_depth_alpha.py hold that for activated inputs on a plain frame; here it is held for
every field and input form, for dead colours on long tile lists, for the camera gradient, the visibility mask and the
densification statistics, for the four mesh bindings inside and in front of the frame, and for a captured step.

How every case is judged.  A scene S and a set B of its Gaussians made non-finite; the CLEAN scene is S without the rows of B
(for a bound frame: without those rows of the binding, the mesh unchanged).
  * The dirty HIP result against the project's high-precision reference OF THE CLEAN SCENE, with the bound the project holds
    that quantity to: the CPU oracle through `_check_forward` / `_check_backward` of tests/test_gpu_parity.py (plain frames);
    tests/camera_ref.py at 1e-4 of scale (camera gradients); the float64 restatements of the bindings under torch autograd at
    2e-4 rel-L2 (tests/test_gpu_phong.py:122) for bound frames.  Frames with RAW activations are held to what
    test_render_api_autograd_path holds them to: the oracle on the torch-activated values, image within 1e-5 + 1e-4 |ref| on
    99.99 % of the values, `radii > 0` equal, gradients chained through the activations (float64 autograd) within 1e-4 rel-L2.
  * The dirty HIP result against the clean HIP result: image, final_T, planes and radii[~B] bit for bit, num_rendered equal,
    gradient rows [~B] within 1e-5 rel-L2 (the blend backward's float atomics allow no tighter bound).
  * Rows [B] of every per-Gaussian gradient exactly zero, radii[B] == 0, every output finite.
Every comparison prints what it achieved next to its bound.

What these tests found when they were written (profiles/r24_nonfinite_contract.md): `num_rendered` counted dropped Gaussians
(4 041 against the clean scene's 4 021 for a NaN opacity or a NaN DC coefficient); the Phong vertex-gradient chain and the
stand-alone `fr_bind_backward*` kernels multiplied a dropped Gaussian's zero upstream rows by its own non-finite values
(540 of 1 200 values of d_verts not finite); and a dead-colour list that takes a tile past eight blend units changed the
summation order of the tile's image rows (one value off by one ulp).

The handles of this module: 300 .. 339 (no other module uses them)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from fateavatar_amd import scenes
from tests import util
from tests.test_gpu_parity import _check_backward, _check_forward

pytestmark = pytest.mark.gpu

SLOT = 300
H, W = 64, 80
ROW_BOUND = 1e-5          # dirty against clean HIP, gradient rows [~B]
BIND_BOUND = 2e-4         # binding gradients against float64 autograd (tests/test_gpu_phong.py:122)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(autouse=True)
def _own_capacity_guess(monkeypatch, gpu_device):
    from fateavatar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_capacity_hint", {})


def _mask(P, rows):
    m = np.zeros(P, bool)
    m[list(rows)] = True
    return m


def _rows(s, keep):
    return scenes.GaussianScene(s.means3D[keep], s.scales[keep], s.rotations[keep], s.opacities[keep], s.shs[keep], s.sh_degree,
                                s.bg, s.camera)


def _copy(s):
    return scenes.GaussianScene(s.means3D.copy(), s.scales.copy(), s.rotations.copy(), s.opacities.copy(), s.shs.copy(),
                                s.sh_degree, s.bg, s.camera)


def _dpix(h, w, seed=1):
    return (np.random.default_rng(seed).uniform(-1, 1, (3, h, w)) / (h * w)).astype(np.float32)


class Frame(util._Frame):
    """util.HipFrame on a handle slot of this module, with the forward's optional side outputs: raw activations, the visibility
    mask, forward-only, planes."""

    def __init__(self, s, dev, slot, raw=False, visible=False, forward_only=False, depth_alpha=False, **kw):
        import torch
        from fateavatar_amd import rasterizer
        self._upload(s, dev, **kw)
        self.raw, self.slot = raw, slot
        self.visible = torch.full((s.P,), 7, dtype=torch.uint8, device=dev) if visible else None
        with rasterizer.handle_slot(slot):
            res = rasterizer.rasterize_gaussians(*self._forward_args(), _raw=raw, _visible=self.visible, _forward_only=forward_only,
                                                 _depth_alpha=depth_alpha)
            self.counts = rasterizer.read_counts(dev.index or 0, slot)
        self.res = res
        self._take_forward(res[:6])
        self.depth, self.alpha = (res[6], res[7]) if depth_alpha else (None, None)

    def backward(self, dpix, **kw):
        import torch
        from fateavatar_amd import rasterizer
        g = torch.from_numpy(np.ascontiguousarray(dpix)).to(self.dev)
        with rasterizer.handle_slot(self.slot):
            out = rasterizer.rasterize_gaussians_backward(*self._backward_args(g), _raw=self.raw, **kw)
        torch.cuda.synchronize()
        self.extra = [o.cpu().numpy() for o in out[8:]]
        return {k: v.cpu().numpy() for k, v in zip(util.GRAD_NAMES, out)}


class Kept:
    """The rows `keep` of a frame, looking like a frame of the clean scene to `_check_forward` / `_check_backward`."""

    def __init__(self, h, keep):
        self._h, self._keep = h, keep
        self.num_rendered, self.color, self.final_T = h.num_rendered, h.color, h.final_T
        self.radii = h.radii[_t(keep, h.radii.device)]

    def geometry(self, field, cols, **kw):
        return self._h.geometry(field, cols, **kw)[self._keep]

    def backward(self, dpix):
        return {k: v[self._keep] for k, v in self._h.backward(dpix).items()}


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(h):
    out = dict(image=h.color.cpu().numpy(), final_T=h.final_T.cpu().numpy(), n_contrib=h.n_contrib.cpu().numpy())
    if getattr(h, "depth", None) is not None:
        out.update(depth=h.depth.cpu().numpy(), alpha=h.alpha.cpu().numpy())
    return out


def check_dropped_forward(what, h, hc, bad):
    """radii[B] == 0; image, final_T (and planes) and radii[~B] the clean frame's bits; num_rendered equal; all finite."""
    radii, radii_c = h.radii.cpu().numpy(), hc.radii.cpu().numpy()
    assert np.all(radii[bad] == 0), (what, "a non-finite Gaussian has a radius", radii[bad])
    assert np.array_equal(radii[~bad], radii_c), (what, "radii of the other Gaussians")
    got, want = _bits(h), _bits(hc)
    for k in want:
        assert np.isfinite(got[k]).all(), (what, k, "not finite", int((~np.isfinite(got[k])).sum()))
        same = np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8))
        print(f"[nonfinite forward] {what}: {k} differs from the clean frame in {int((got[k] != want[k]).sum())} value(s) (bound 0)")
        assert same, (what, k, "differs from the clean frame", float(np.abs(got[k].astype(np.float64) - want[k]).max()))
    print(f"[nonfinite forward] {what}: num_rendered {h.num_rendered}, clean {hc.num_rendered} (must be equal)")
    assert h.num_rendered == hc.num_rendered, (what, "num_rendered", h.num_rendered, hc.num_rendered)


def check_dropped_rows(what, g, gc, bad, names=None):
    """Every array of `g` (name -> numpy [P, ...]) finite, rows B exactly zero, rows ~B within ROW_BOUND of the clean run's."""
    for k in (names or g):
        a, c = g[k], gc[k]
        assert a.shape[0] == bad.shape[0] and a[~bad].shape == c.shape, (what, k, a.shape, c.shape)
        assert np.isfinite(a).all(), (what, k, "not finite", int((~np.isfinite(a)).sum()))
        if a.size == 0:
            continue
        assert np.all(a[bad] == 0), (what, k, "a dropped Gaussian has a gradient", float(np.abs(a[bad]).max()))
        rl = util.rel_l2(a[~bad], c)
        print(f"[nonfinite rows] {what} {k}: rows ~B against the clean frame rel-L2 {rl:.2e} (bound {ROW_BOUND:.0e})")
        assert rl <= ROW_BOUND, (what, k, rl)


# ------------------------------------------------------------------ 1. fields and input forms
def base_scene():
    return scenes.random_scene(1500, H, W, sh_degree=1, seed=31)     # test_non_finite_gaussians_are_dropped_not_propagated's


def _six_visible_rows():
    """Six Gaussians the ORACLE renders (radii > 0), spread over the scene's rows: dropping them changes the image (of that
    test's own six rows, three are outside the frustum to begin with)."""
    vis = np.nonzero(util.oracle_forward(base_scene()).radii > 0)[0]
    return tuple(int(i) for i in vis[np.linspace(0, vis.size - 1, 8).astype(int)[1:7]])


BAD_ROWS = _six_visible_rows()


@functools.lru_cache(maxsize=None)
def precomp_inputs():
    s = base_scene()
    cols = np.random.default_rng(5).uniform(0, 1, (s.P, 3)).astype(np.float32)
    return cols, util.oracle_forward(s).cov3D.copy()


def _kw(form, rows=slice(None)):
    cols, cov = precomp_inputs()
    return {"activated": {}, "cov3D_precomp": dict(cov3D_precomp=cov[rows].copy()),
            "colors_precomp": dict(colors_precomp=cols[rows].copy())}[form]


@functools.lru_cache(maxsize=None)
def clean_reference(form):
    """The clean scene of an input form with its oracle forward, computed once and never modified."""
    keep = ~_mask(1500, BAD_ROWS)
    s = _rows(base_scene(), keep)
    kw = _kw(form, keep)
    return SimpleNamespace(s=s, kw=kw, o=util.oracle_forward(s, **kw), dpix=_dpix(H, W))


_CLEAN_HIP = {}


def clean_hip(form, dev):
    """The clean scene of an input form through the HIP path, once: (frame, gradients)."""
    if form not in _CLEAN_HIP:
        r = clean_reference(form)
        hc = Frame(r.s, dev, SLOT + 1, **r.kw)
        _CLEAN_HIP[form] = (hc, hc.backward(r.dpix))
    return _CLEAN_HIP[form]


def judge_plain(what, h, bad, form, dev):
    r = clean_reference(form)
    hc, gc = clean_hip(form, dev)
    check_dropped_forward(what, h, hc, bad)
    check_dropped_rows(what, h.backward(r.dpix), gc, bad)
    v = Kept(h, ~bad)
    _check_forward(r.o, v, what)
    _check_backward(r.o, v, r.dpix, what)


def _poison(s, field, value):
    """`value` into `field` of every row of BAD_ROWS, the component changing from row to row."""
    for j, i in enumerate(BAD_ROWS):
        if field == "position":
            s.means3D[i, j % 3] = value
        elif field == "scale":
            s.scales[i, j % 3] = value
        elif field == "rotation":
            s.rotations[i, j % 4] = value
        elif field == "opacity":
            s.opacities[i, 0] = value
        elif field == "sh_dc":
            s.shs[i, 0, j % 3] = value
        else:
            s.shs[i, 1 + j % 3, (j + 1) % 3] = value


@pytest.mark.parametrize("value", [NAN, INF, -INF], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("field", ["position", "scale", "rotation", "opacity", "sh_dc", "sh_rest"])
def test_activated_inputs_every_field(gpu_device, field, value):
    """NaN, +inf and -inf in a position component, a scale, a rotation component, the opacity, a DC and a higher SH
    coefficient of six Gaussians of the 1 500."""
    s = base_scene()
    _poison(s, field, value)
    judge_plain(f"{field}={value}", Frame(s, gpu_device, SLOT), _mask(s.P, BAD_ROWS), "activated", gpu_device)


@pytest.mark.parametrize("form,value", [("cov3D_precomp", NAN), ("cov3D_precomp", INF), ("colors_precomp", NAN)],
                         ids=["cov3D-nan", "cov3D-inf", "colours-nan"])
def test_precomputed_covariances_and_colours(gpu_device, form, value):
    s = base_scene()
    kw = _kw(form)
    for j, i in enumerate(BAD_ROWS):
        kw[form][i, j % kw[form].shape[1]] = value
    judge_plain(f"{form}={value}", Frame(s, gpu_device, SLOT, **kw), _mask(s.P, BAD_ROWS), form, gpu_device)


# ---- raw activations
def _raw_scene(s):
    """`s` as RAW parameters (log scale, 1.7 x the quaternion, logit opacity), float32."""
    import torch
    op = torch.from_numpy(s.opacities)
    return scenes.GaussianScene(s.means3D.copy(), np.log(s.scales), (s.rotations * np.float32(1.7)).astype(np.float32),
                                torch.log(op / (1 - op)).numpy(), s.shs.copy(), s.sh_degree, s.bg, s.camera)


def _activate(raw, dtype):
    """torch's activations of the reference model (exp, normalize, sigmoid) on a raw scene: leaves and activated tensors."""
    import torch
    leaves = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (raw.scales, raw.rotations, raw.opacities)]
    return leaves, (torch.exp(leaves[0]), torch.nn.functional.normalize(leaves[1]), torch.sigmoid(leaves[2]))


class RawReference:
    """The oracle's side of a RAW scene: its forward on the float32 torch activations, and gradients chained through the
    activations by float64 autograd."""

    def __init__(self, raw):
        self.raw = raw
        _, (sc, rot, op) = _activate(raw, __import__("torch").float32)
        act = scenes.GaussianScene(raw.means3D, sc.detach().numpy(), rot.detach().numpy(), op.detach().numpy(), raw.shs, raw.sh_degree,
                                   raw.bg, raw.camera)
        self.o = util.oracle_forward(act)

    def gradients(self, dpix):
        import torch
        from oracle import oracle
        ob = oracle.backward(self.o, dpix)
        leaves, act = _activate(self.raw, torch.float64)
        torch.autograd.backward(list(act), [torch.from_numpy(g).double() for g in (ob.dL_dscales, ob.dL_drotations, ob.dL_dopacity)])
        return dict(dL_dmeans2D=ob.dL_dmeans2D, dL_dmeans3D=ob.dL_dmeans3D, dL_dsh=ob.dL_dsh, dL_dscales=leaves[0].grad.numpy(),
                    dL_drotations=leaves[1].grad.numpy(), dL_dopacity=leaves[2].grad.numpy())


def check_raw_against_oracle(what, h, keep, ref, dpix):
    """A raw frame's rows `keep` against RawReference (module docstring: test_render_api_autograd_path's bounds); dL/dpixel is
    zero at the pixels where the two blended different sets (util.flip_pixels), at most 1 % of them."""
    o = ref.o
    col, fT = h.color.cpu().numpy(), h.final_T.cpu().numpy()
    fc = util.frac_close(col, o.color, 1e-4, 1e-5)
    radii = h.radii.cpu().numpy()[keep]
    print(f"[nonfinite raw] {what}: image within tolerance on {fc:.6f} of the values (bound 0.9999), radii equal on "
          f"{np.mean(radii == o.radii):.6f}")
    assert np.isfinite(col).all() and fc >= 0.9999, (what, fc)
    assert np.array_equal(radii > 0, o.radii > 0), (what, "visibility")
    flips = util.flip_pixels(o, col, fT)
    assert int(flips.sum()) <= flips.size // 100, (what, int(flips.sum()))
    dpix = dpix.copy()
    dpix[:, flips] = 0
    want, got = ref.gradients(dpix), h.backward(dpix)
    for k, w in want.items():
        g = got[k][keep]
        assert np.isfinite(got[k]).all(), (what, k)
        rl = util.rel_l2(g, w)
        print(f"[nonfinite raw] {what} {k}: rel-L2 {rl:.2e} against the oracle chained through the activations (bound 1e-4)")
        assert rl <= 1e-4 and np.abs(w).max() > 0, (what, k, rl)
    return dpix


@functools.lru_cache(maxsize=None)
def raw_clean_reference():
    return RawReference(_rows(_raw_scene(base_scene()), ~_mask(1500, BAD_ROWS)))


@pytest.mark.parametrize("case", ["scale=100", "opacity=nan"])
def test_raw_activations_dropped(gpu_device, case):
    """Raw activations (FR_FLAG_RAW_ACTIVATIONS): a raw scale of 100, whose exp overflows to inf, and a NaN raw opacity."""
    raw = _raw_scene(base_scene())
    bad = _mask(raw.P, BAD_ROWS)
    for j, i in enumerate(BAD_ROWS):
        if case == "scale=100":
            raw.scales[i, j % 3] = 100.0
        else:
            raw.opacities[i, 0] = NAN
    ref = raw_clean_reference()
    h, hc = Frame(raw, gpu_device, SLOT + 2, raw=True), Frame(ref.raw, gpu_device, SLOT + 3, raw=True)
    check_dropped_forward(case, h, hc, bad)
    dpix = check_raw_against_oracle(case, h, ~bad, ref, _dpix(H, W))
    check_dropped_rows(case, h.backward(dpix), hc.backward(dpix), bad)


@pytest.mark.parametrize("case", ["opacity=+inf", "opacity=-inf", "quaternion=0"])
def test_raw_values_whose_activation_is_finite_are_not_dropped(gpu_device, case):
    """NOT dropped Gaussians (INTEGRATION.md says so): a raw opacity of +-inf activates to exactly 1 / 0, and an all-zero raw
    quaternion normalises to the zero quaternion (torch.nn.functional.normalize's clamp at 1e-12), i.e. to the identity
    rotation.  Such a Gaussian renders as the reference's arithmetic renders it: the frame is held to the oracle on the
    activated values with no row removed, every output is finite, and — raw opacity — the frame is, bit for bit, the frame
    with the finite raw opacity +-100, which activates to the same 1 / 0."""
    raw = _raw_scene(base_scene())
    twin = None
    if case.startswith("opacity"):
        v = INF if case.endswith("+inf") else -INF
        twin = _copy(raw)
        for i in BAD_ROWS:
            raw.opacities[i, 0], twin.opacities[i, 0] = v, np.sign(v) * 100.0
    else:
        for i in BAD_ROWS:
            raw.rotations[i] = 0.0
    everything = np.ones(raw.P, bool)
    h = Frame(raw, gpu_device, SLOT + 2, raw=True)
    assert np.all(h.radii.cpu().numpy()[list(BAD_ROWS)] > 0), (case, "rendered by the reference's arithmetic, hence not dropped")
    dpix = check_raw_against_oracle(case, h, everything, RawReference(raw), _dpix(H, W))
    if twin is not None:
        ht = Frame(twin, gpu_device, SLOT + 3, raw=True)
        nobody = np.zeros(raw.P, bool)
        check_dropped_forward(case + " against +-100", h, ht, nobody)
        check_dropped_rows(case + " against +-100", h.backward(dpix), ht.backward(dpix), nobody)


# ------------------------------------------------------------------ 2. dead colours on long lists
# A Gaussian whose geometry is finite and whose COLOUR is not has been binned by the time its colour is known: its instances
# stay in their tiles' lists with depth +inf and a record of opacity 0.  name -> (real Gaussians, dead ones, the sort tier
# (lo, hi] of the clean frame's longest list, that of the dirty frame's); every Gaussian of the fixture reaches the four
# centre tiles, so every wave of 64 Gaussians counts more than 256 instances: the second counting pass runs.
LONG = {
    "1-wave to 4-wave": (200, 600, (0, 256), (256, 1024)),
    "over 1024 and 2048": (900, 1500, (256, 1024), (2048, 4096)),
    "global fallback": (900, 3600, (256, 1024), (4096, 1 << 30)),
}


@functools.lru_cache(maxsize=None)
def long_case(name):
    from tests.test_gpu_batch_parity import _long_scene
    real, dead = LONG[name][:2]
    twin = _long_scene(real + dead)       # every Gaussian alive: what the dead ones' instances are counted like
    bad = _mask(twin.P, np.random.default_rng(17).permutation(twin.P)[:dead])
    dirty = _copy(twin)
    dirty.shs[bad, 0, 0] = NAN
    dirty.shs[np.nonzero(bad)[0][::3], 0, 1] = INF
    clean = _rows(twin, ~bad)
    return SimpleNamespace(dirty=dirty, twin=twin, clean=clean, bad=bad, o=util.oracle_forward(clean), dpix=_dpix(32, 32, 3))


def _tier(counts, lo_hi, what):
    print(f"[nonfinite long] {what}: longest tile list {counts.max_tile_list}, expected in ({lo_hi[0]}, {lo_hi[1]}]; "
          f"{counts.num_instances} instances")
    assert lo_hi[0] < counts.max_tile_list <= lo_hi[1], (what, counts.max_tile_list, lo_hi)


def judge_long(what, v, c, hc, gc):
    check_dropped_forward(what, v, hc, c.bad)
    check_dropped_rows(what, v.backward(c.dpix), gc, c.bad)
    k = Kept(v, ~c.bad)
    _check_forward(c.o, k, what)
    _check_backward(c.o, k, c.dpix, what)


@pytest.mark.parametrize("name", list(LONG))
def test_dead_colours_on_long_lists(gpu_device, name):
    """One 8x8-tile fixture with exact depth ties (test_long_tile_lists_take_the_multi_wave_and_fallback_sorts's): the real and
    the total list lengths fall into different sort tiers.  `fr_counts::num_instances` counts the dead instances, as
    INTEGRATION.md documents it: it is what the scene gives with those Gaussians alive."""
    c = long_case(name)
    hc = Frame(c.clean, gpu_device, SLOT + 5)
    ht = Frame(c.twin, gpu_device, SLOT + 6)
    h = Frame(c.dirty, gpu_device, SLOT + 4)
    _tier(hc.counts, LONG[name][2], name + " clean")
    _tier(h.counts, LONG[name][3], name + " dirty")
    print(f"[nonfinite long] {name}: num_instances {h.counts.num_instances}, with every Gaussian alive {ht.counts.num_instances}, "
          f"clean {hc.counts.num_instances}")
    assert h.counts.num_instances == ht.counts.num_instances > hc.counts.num_instances
    judge_long(name, h, c, hc, hc.backward(c.dpix))


def test_dead_colours_on_a_long_list_in_a_batch(gpu_device):
    """The first case as view 1 of a batch of two."""
    name = next(iter(LONG))
    c = long_case(name)
    hc = Frame(c.clean, gpu_device, SLOT + 5)
    b = util.HipBatch([base_scene(), c.dirty], gpu_device, slots=[SLOT + 7, SLOT + 8])
    _tier(b[1].counts, LONG[name][3], name + " dirty, view 1 of 2")
    judge_long(name + " view 1 of 2", b[1], c, hc, hc.backward(c.dpix))
    assert np.isfinite(b[0].color.cpu().numpy()).all()


@functools.lru_cache(maxsize=None)
def long_planes_reference():
    from tests.planes_ref import PlanesRef
    return PlanesRef(long_case(next(iter(LONG))).clean)


def test_dead_colours_on_a_long_list_forward_only_with_planes(gpu_device):
    """The first case forward-only (FR_FLAG_FORWARD_ONLY) with depth and alpha planes: image, final_T, depth and alpha are the
    clean frame's bits, and the planes pass tests/test_gpu_planes_long_lists.py's forward checks against the oracle's
    composite frame of the clean scene."""
    from tests.test_gpu_planes_long_lists import check_planes_forward
    name = next(iter(LONG))
    c = long_case(name)
    h = Frame(c.dirty, gpu_device, SLOT + 9, forward_only=True, depth_alpha=True)
    hc = Frame(c.clean, gpu_device, SLOT + 10, forward_only=True, depth_alpha=True)
    _tier(h.counts, LONG[name][3], name + " dirty, forward-only")
    check_dropped_forward(name + " forward-only planes", h, hc, c.bad)
    check_planes_forward(long_planes_reference(), h, h.res, name + " forward-only planes", full=False)


def test_dead_colours_that_need_a_larger_binning_capacity(gpu_device):
    """150 image-sized Gaussians with a NaN colour on 256 x 256 pixels: their 150 x 1 024 instances do not fit the capacity a
    frame of 500 Gaussians starts with (4 P + 65 536), the clean scene's do.  The frame reports the overflow, is repeated with
    the capacity it asked for and renders the clean image."""
    from fateavatar_amd import _lib
    res = 256
    s = scenes.random_scene(500, res, res, sh_degree=1, seed=41)
    bad = _mask(s.P, np.random.default_rng(2).permutation(s.P)[:150])
    clean = _rows(s, ~bad)
    s.scales[bad] = 0.6
    s.shs[bad, 0, 0] = NAN
    start = 4 * s.P + 65536                                # rasterizer._forward_view, with an empty capacity guess
    hc = Frame(clean, gpu_device, SLOT + 12)
    h = Frame(s, gpu_device, SLOT + 11)
    L = _lib.lib()
    print(f"[nonfinite capacity] instances: dirty {h.counts.num_instances}, clean {hc.counts.num_instances}; a frame starts with "
          f"{start}; binning buffer {h.binning.numel()} bytes, at the start {L.fr_binning_bytes(start, res, res)}")
    assert hc.counts.num_instances <= 4 * clean.P + 65536 < start < h.counts.num_instances
    assert h.counts.overflow == 0 and h.binning.numel() > L.fr_binning_bytes(start, res, res), "the frame was not repeated"
    assert hc.binning.numel() == L.fr_binning_bytes(4 * clean.P + 65536, res, res)
    check_dropped_forward("capacity", h, hc, bad)
    dpix = _dpix(res, res, 4)
    check_dropped_rows("capacity", h.backward(dpix), hc.backward(dpix), bad)
    o = util.oracle_forward(clean)
    _check_forward(o, Kept(h, ~bad), "capacity")
    _check_backward(o, Kept(h, ~bad), dpix, "capacity")


# ------------------------------------------------------------------ 3. camera gradient, 4. visibility and statistics
def mixed_dirty_scene():
    """Six fields at once: NaN opacity, inf scale, NaN position, NaN rotation, NaN higher SH coefficient, inf DC coefficient."""
    s, b = base_scene(), BAD_ROWS
    s.opacities[b[0], 0] = NAN
    s.scales[b[1], 1] = INF
    s.means3D[b[2], 0] = NAN
    s.rotations[b[3], 2] = NAN
    s.shs[b[4], 2, 1] = NAN
    s.shs[b[5], 0, 0] = INF
    return s


def _camera_case(h, dev):
    """dL/dpixel with the flip pixels zeroed, and the float64 camera reference of the CLEAN scene for it."""
    from tests import camera_ref as cr
    from tests.test_gpu_camera_grad import _mask_flips
    r = clean_reference("activated")
    dpix, _ = _mask_flips(r.o, h, cr.seeded_dpix(H, W), "nonfinite")
    return dpix, cr.camera_reference(r.s, r.o, dpix)


def test_camera_gradient_single_frame(gpu_device):
    """FR_FLAG_CAMERA_GRAD on the dirty scene: d_view, d_proj, d_campos finite and within 1e-4 of scale of tests/camera_ref.py
    on the clean scene (tests/test_gpu_camera_grad.py's `_check`)."""
    from tests.test_gpu_camera_grad import _check
    s = mixed_dirty_scene()
    bad = _mask(s.P, BAD_ROWS)
    h = Frame(s, gpu_device, SLOT + 13)
    dpix, ref = _camera_case(h, gpu_device)
    g = h.backward(dpix, _camera=True)
    _check(tuple(h.extra), ref, "nonfinite single")
    for k, a in g.items():
        assert np.isfinite(a).all() and (a.size == 0 or np.all(a[bad] == 0)), k


def test_camera_gradient_as_one_view_of_a_batch(gpu_device):
    import torch
    from fateavatar_amd import rasterizer
    from tests.test_gpu_camera_grad import _check
    s = mixed_dirty_scene()
    bad = _mask(s.P, BAD_ROWS)
    b = util.HipBatch([scenes.random_scene(900, 48, 40, sh_degree=1, seed=8), s], gpu_device, slots=[SLOT + 14, SLOT + 15])
    dpix, ref = _camera_case(b[1], gpu_device)
    gs = [_t(b[0].default_dpix, gpu_device), _t(dpix, gpu_device)]
    out = rasterizer.rasterize_gaussians_backward_batch([v._backward_args(g) for v, g in zip(b.views, gs)], slots=b.slots, camera=True)
    torch.cuda.synchronize()
    _check(tuple(t.cpu().numpy() for t in out[1][8:]), ref, "nonfinite view 1 of 2")
    for view in out:
        assert all(bool(torch.isfinite(t).all()) for t in view)
    for k, t in zip(util.GRAD_NAMES, out[1][:8]):
        assert t.numel() == 0 or float(t[_t(bad, gpu_device)].abs().max()) == 0.0, k


def test_visibility_mask_and_densification_statistics(gpu_device):
    """fr_aux::visible is 0 for the rows B and the clean frame's mask elsewhere.  The fused densification statistics (the
    backward's `_stats`) leave the rows B of both arrays untouched; elsewhere `denom` is the clean run's exactly, and
    `xyz_gradient_accum`, a norm of the dL_dmeans2D row, is the clean run's within that row's bound (ROW_BOUND)."""
    import torch
    s = mixed_dirty_scene()
    bad = _mask(s.P, BAD_ROWS)
    r = clean_reference("activated")
    h, hc = Frame(s, gpu_device, SLOT + 16, visible=True), Frame(r.s, gpu_device, SLOT + 17, visible=True)
    vis, vis_c = h.visible.cpu().numpy(), hc.visible.cpu().numpy()
    assert np.all(vis[bad] == 0) and np.array_equal(vis[~bad], vis_c) and np.array_equal(vis_c, (hc.radii > 0).cpu().numpy())
    assert 0 < int(vis_c.sum())
    stats = {}
    for name, f in (("dirty", h), ("clean", hc)):
        accum, denom = torch.zeros((f.s.P, 1), device=gpu_device), torch.zeros((f.s.P, 1), device=gpu_device)
        if name == "dirty":      # (sentinels in the rows B only: elsewhere a start at zero keeps the sums' own precision)
            accum[_t(bad, gpu_device)], denom[_t(bad, gpu_device)] = 5.0, 3.0
        f.backward(r.dpix, _stats=(accum, denom))
        stats[name] = (accum.cpu().numpy(), denom.cpu().numpy())
    (a, d), (ac, dc) = stats["dirty"], stats["clean"]
    assert np.all(a[bad] == 5.0) and np.all(d[bad] == 3.0), "the statistics of a dropped Gaussian were touched"
    assert np.array_equal(d[~bad], dc) and float(dc.max()) == 1.0
    rl = util.rel_l2(a[~bad], ac)
    print(f"[nonfinite stats] xyz_gradient_accum of the rows ~B against the clean run: rel-L2 {rl:.2e} (bound {ROW_BOUND:.0e})")
    assert np.isfinite(a).all() and rl <= ROW_BOUND and float(np.abs(ac).max()) > 0


# ------------------------------------------------------------------ 5. bound frames, all four modes
# The "turned" mesh of tests/test_gpu_phong.py::_meshes (V = 400, F = 700, N = 5 000 Gaussians) under a 64 x 80 camera.  The
# reference of a mode is its float64 restatement under torch autograd on the CLEAN binding, fed with the gradients of the bound
# values that the rasterizer's backward hands the stand-alone op on the clean scene (the rasterizer itself is held to the oracle
# by the plain-frame tests above): d_verts and the gradients of the mode's own parameter, rotation and scaling, each within
# BIND_BOUND, from the frame with the binding folded in and from the stand-alone op in front of render().
MODES = ("shell", "face_local", "phong", "deform")
OWN = {"shell": ("_offset", 1), "face_local": ("_xyz", 3), "phong": ("_uvd", 3), "deform": ("_deform", 10)}
SHELL_LEN = 0.05
PARAMS = ("own", "rotation", "scaling", "opacity", "features")


@functools.lru_cache(maxsize=None)
def bound_fixture():
    import math
    from tests import phong_ref as P
    cano, verts, faces, fi, bary = P.turned_mesh()
    P.assert_turned_mesh_is_well_posed(cano, verts, faces)
    N = fi.shape[0]
    rng = np.random.default_rng(23)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    own = dict(shell=f32(0.3 * rng.normal(size=(N, 1))), face_local=f32(0.1 * rng.normal(size=(N, 3))),
               phong=f32(0.05 * rng.normal(size=(N, 3))), deform=f32(0.3 * rng.normal(size=(N, 10))))
    par = dict(rotation=f32(rng.normal(size=(N, 4))), scaling=f32(math.log(0.15) + 0.3 * rng.normal(size=(N, 3))),
               opacity=f32(np.full((N, 1), math.log(0.6 / 0.4))), features=f32(rng.uniform(-1, 1, (N, 1, 3))))
    cam = scenes.look_at_camera((0.0, 0.0, -8.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 2 * math.atan(0.45), 2 * math.atan(0.45 * H / W), H, W)
    # six Gaussians close to the view axis (the camera looks along +z): in the image in every mode
    point = np.einsum("nij,ni->nj", verts[faces[fi]], bary)
    rows6 = np.argsort(point[:, 0] ** 2 + point[:, 1] ** 2)[:6]
    # a vertex of the first of them: every Gaussian on its faces
    vertex = int(faces[fi[rows6[0]], 0])
    on_vertex = (faces[fi] == vertex).any(axis=1)
    return SimpleNamespace(cano=cano, verts=verts, faces=faces, fi=fi, bary=bary, N=N, own=own, par=par, cam=cam,
                           bad={"rows": _mask(N, rows6), "vertex": on_vertex}, vertex=vertex, dpix=_dpix(H, W, 6),
                           bg=np.array([0.2, 0.5, 0.9], np.float32))


class Holder:
    """What render_batch() / render_bound_batch() read of a Gaussian holder for one frame."""
    fused_activations = True
    max_sh_degree = active_sh_degree = 0
    fused_densification_stats = None

    def __init__(self, mode, leaves, bound=None):
        self._opacity, self.get_features = leaves["opacity"], leaves["features"]
        if bound is None:     # raw parameters: the rasterizer evaluates the binding itself
            setattr(self, OWN[mode][0], leaves["own"])
            self._rotation, self._scaling = leaves["rotation"], leaves["scaling"]
        else:                 # the stand-alone op's outputs
            self.get_xyz, self._rotation, self._scaling = bound


def run_bound(mode, values, verts, keep, dev, fused):
    """One frame of the rows `keep` in `mode` — the binding folded into the frame (`fused`) or the stand-alone op in front of
    render_batch — and its backward under the fixture's dL/dpixel.  `values`: own / rotation / scaling [N, ...] as numpy.
    -> namespace(image, radii, d_verts, grads {PARAMS}, upstream: the gradients of the op's three outputs (stand-alone only))."""
    import torch
    from fateavatar_amd import binding as Bd
    from fateavatar_amd import bound as Bn
    from fateavatar_amd.model import TorchCamera
    from fateavatar_amd.render import render_batch
    fx = bound_fixture()
    t = lambda a: _t(a, dev)  # noqa: E731
    leaves = {k: t((values[k] if k in values else fx.par[k])[keep]).requires_grad_(True) for k in PARAMS}
    v = t(verts).requires_grad_(True)
    faces, fi, bary, cano = t(fx.faces), t(fx.fi[keep]), t(fx.bary[keep]), t(fx.cano)
    cam, bg = TorchCamera(fx.cam, dev), t(fx.bg)
    own, rot, scl = leaves["own"], leaves["rotation"], leaves["scaling"]
    b = None
    if fused:
        mb = {"shell": lambda: Bn.MeshBinding(faces, fi, bary, Bd.face_scale(cano, faces), SHELL_LEN, True),
              "face_local": lambda: Bn.FaceLocalBinding(faces, fi),
              "phong": lambda: Bn.PosedPhongBinding(faces, fi, bary, Bd.phong_canonical(cano, faces)),
              "deform": lambda: Bn.DeformBinding(faces, fi, bary)}[mode]()
        out = Bn.render_bound_batch([cam], [Holder(mode, leaves)], [v], mb, bg, slots=[SLOT + 20])[0]
    else:
        if mode == "shell":
            b = Bd.bind_gaussians(v, faces, fi, bary, Bd.face_scale(cano, faces), own, rot, scl, SHELL_LEN, True)
        elif mode == "face_local":
            b = Bd.bind_gaussians_face_local(v, faces, fi, own, rot, scl)
        elif mode == "phong":
            b = Bd.bind_gaussians_phong(v, faces, fi, bary, Bd.phong_frame(Bd.phong_canonical(cano, faces), v, differentiable=True),
                                        own, rot, scl)
        else:
            b = Bd.bind_gaussians_deform(v, faces, fi, bary, own, rot, scl)
        for x in b:
            x.retain_grad()
        out = render_batch([cam], [Holder(mode, leaves, b)], bg, slots=[SLOT + 21])[0]
    torch.autograd.backward([out["render"]], [t(fx.dpix)])
    torch.cuda.synchronize()
    n = lambda x: x.detach().cpu().numpy()  # noqa: E731
    return SimpleNamespace(image=n(out["render"]), radii=n(out["radii"]), d_verts=n(v.grad),
                           grads={k: n(leaves[k].grad) for k in PARAMS},
                           upstream=None if b is None else [n(x.grad) for x in b])


def reference_bind64(mode, values, verts, keep, upstream):
    """float64 autograd of the mode's restatement on the rows `keep`, under `upstream` (the gradients of its three outputs):
    -> (d_verts, {own, rotation, scaling})."""
    import torch
    from oracle import binding as B
    from tests import face_local_ref as FL
    from tests import flash_ref as FA
    from tests import phong_ref as P
    fx = bound_fixture()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()  # noqa: E731
    v = d(verts).requires_grad_(True)
    own, rot, scl = (d(values[k][keep]).requires_grad_(True) for k in ("own", "rotation", "scaling"))
    faces, fi, bary, cano = torch.from_numpy(fx.faces), torch.from_numpy(fx.fi[keep]), d(fx.bary[keep]), d(fx.cano)
    if mode == "shell":
        # oracle.binding.bind (model/fateavatar.py:225-258) with face_local_ref's matrix_to_quaternion: the same forward, and
        # pytorch3d's zero subgradient where oracle.binding's square root has a NaN one (face_local_ref's docstring)
        orien, fscale = B.face_orientation(v, faces)
        f = fi.long()
        ratio = (fscale / B.face_orientation(cano, faces)[1])[f]
        pos = (bary[..., None] * v[faces[f].long()]).sum(-2)
        out = (pos + B.face_normals(v, faces)[f] * SHELL_LEN * torch.tanh(own), B.quaternion_multiply(FL.matrix_to_quaternion(orien[f]), rot),
               scl + torch.log(ratio))
    elif mode == "face_local":
        out = FL.face_local_bind(v, faces, fi, own, rot, scl)
    elif mode == "phong":
        out = P.phong_bind(v, faces, fi, bary, P.mesh_frame(cano, faces, v), own, rot, scl)
    else:
        out = FA.deform_bind(v, faces, fi, bary, own, rot, scl)
    torch.autograd.backward(list(out), [d(u) for u in upstream])
    return v.grad.numpy(), dict(own=own.grad.numpy(), rotation=rot.grad.numpy(), scaling=scl.grad.numpy())


def clean_values(mode):
    fx = bound_fixture()
    return dict(own=fx.own[mode].copy(), rotation=fx.par["rotation"].copy(), scaling=fx.par["scaling"].copy())


_CLEAN_BOUND = {}


def clean_bound(mode, which, dev):
    """The clean binding of (mode, B) once: the folded frame, the stand-alone route and the float64 reference."""
    if (mode, which) not in _CLEAN_BOUND:
        fx = bound_fixture()
        keep = ~fx.bad[which]
        un = run_bound(mode, clean_values(mode), fx.verts, keep, dev, fused=False)
        fu = run_bound(mode, clean_values(mode), fx.verts, keep, dev, fused=True)
        assert int((fu.radii > 0).sum()) > 1000 and np.isfinite(un.upstream[0]).all()
        _CLEAN_BOUND[mode, which] = SimpleNamespace(fused=fu, unfused=un, ref=reference_bind64(mode, clean_values(mode), fx.verts, keep, un.upstream))
    return _CLEAN_BOUND[mode, which]


def _bind_rel(what, got, ref):
    assert np.isfinite(got).all(), (what, "not finite", int((~np.isfinite(got)).sum()))
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0, what
    rl = util.rel_l2(got, ref)
    print(f"[nonfinite bound] {what}: rel-L2 {rl:.2e} against float64 autograd on the clean binding (bound {BIND_BOUND:.0e})")
    assert rl <= BIND_BOUND, (what, rl)


def judge_bound(mode, which, values, verts, dev):
    fx = bound_fixture()
    bad = fx.bad[which]
    c = clean_bound(mode, which, dev)
    everything = np.ones(fx.N, bool)
    was_visible = int((run_bound(mode, clean_values(mode), fx.verts, bad, dev, fused=True).radii > 0).sum()) if which == "rows" else None
    for route, clean in (("folded", c.fused), ("stand-alone op", c.unfused)):
        what = f"{mode} {which} {route}"
        r = run_bound(mode, values, verts, everything, dev, fused=route == "folded")
        assert np.all(r.radii[bad] == 0) and np.array_equal(r.radii[~bad], clean.radii), what
        assert np.isfinite(r.image).all() and np.array_equal(r.image.view(np.uint8), clean.image.view(np.uint8)), (what, "image")
        check_dropped_rows(what, r.grads, clean.grads, bad)
        _bind_rel(what + " d_verts", r.d_verts, c.ref[0])
        for k, ref in c.ref[1].items():
            _bind_rel(f"{what} d_{k}", r.grads[k][~bad], ref)
    if was_visible is not None:
        print(f"[nonfinite bound] {mode}: {was_visible} of the {int(bad.sum())} Gaussians of B are rendered when finite")
        assert was_visible >= 4


def _poison_bound(mode, field, values, bad):
    three = (NAN, INF, -INF)
    for j, i in enumerate(np.nonzero(bad)[0]):
        if field == "rotation":
            values["rotation"][i, j % 4] = three[j % 3]
        elif field == "scaling":            # (-inf is a scale of exactly 0: finite)
            values["scaling"][i, j % 3] = (NAN, INF)[j % 2]
        elif mode == "shell":               # (tanh(+-inf) = +-1: finite)
            values["own"][i, 0] = NAN
        elif mode == "face_local":
            values["own"][i, j % 3] = three[j % 3]
        elif mode == "phong":               # (only the third column of uvd is read)
            values["own"][i, 2] = three[j % 3]
        else:                               # (tanh again: NaN only; a position, a rotation and a scale column in turn)
            values["own"][i, (0, 4, 8, 1, 3, 9)[j % 6]] = NAN


@pytest.mark.parametrize("field", ["own", "rotation", "scaling"])
@pytest.mark.parametrize("mode", MODES)
def test_bound_frames_drop_non_finite_gaussians(gpu_device, mode, field):
    """Six Gaussians with a non-finite value in their own position parameter (offset / local xyz / uvd / a deform row), their
    rotation or their scaling, in every mode, folded and stand-alone.  Phong: `PosedPhongBinding` through `render_bound_batch`,
    against the differentiable ops in front of render()."""
    fx = bound_fixture()
    values = clean_values(mode)
    _poison_bound(mode, field, values, fx.bad["rows"])
    judge_bound(mode, "rows", values, fx.verts, gpu_device)


@pytest.mark.parametrize("mode", ["shell", "face_local", "deform"])
def test_bound_frames_with_a_non_finite_vertex(gpu_device, mode):
    """One posed vertex NaN: every Gaussian on its faces is dropped and d_verts is finite — that of the binding without those
    Gaussians on the mesh with the vertex finite.  (The Phong mode is out of scope: its mesh pass is undefined there.)"""
    fx = bound_fixture()
    verts = fx.verts.copy()
    verts[fx.vertex, 1] = NAN
    print(f"[nonfinite bound] vertex {fx.vertex}: {int(fx.bad['vertex'].sum())} Gaussians on its faces")
    assert 6 <= int(fx.bad["vertex"].sum()) < fx.N // 10
    judge_bound(mode, "vertex", clean_values(mode), verts, gpu_device)


def test_phong_scatter_alone_with_non_finite_own_values(gpu_device):
    """`phong_scatter_frame_grads` (fr_bind_backward_phong_frame) with zero upstream rows for B and NaN / inf in B's uvd,
    rotation and scaling: d_verts, d_vert_normals, d_vert_quats and d_face_ratio are finite and within BIND_BOUND of float64
    autograd of `phong_bind` without B (the frame arrays as independent leaves, as test_scatter_matches_float64_autograd)."""
    import torch
    from fateavatar_amd.binding import phong_canonical, phong_frame, phong_scatter_frame_grads
    from tests import phong_ref as P
    dev = gpu_device
    fx = bound_fixture()
    bad = _mask(fx.N, np.random.default_rng(9).permutation(fx.N)[:40])
    keep = ~bad
    rng = np.random.default_rng(11)
    N, V, F = fx.N, fx.verts.shape[0], fx.faces.shape[0]
    uvd = (0.05 * rng.normal(size=(N, 3))).astype(np.float32)
    rot = rng.normal(size=(N, 4)).astype(np.float32)
    scl = rng.normal(size=(N, 3)).astype(np.float32)
    w = [rng.normal(size=s).astype(np.float32) for s in ((N, 3), (N, 4), (N, 3))]
    t = torch.from_numpy
    d = lambda a: t(np.ascontiguousarray(a)).double()  # noqa: E731
    v64 = d(fx.verts).requires_grad_(True)
    frame64 = [x.detach().requires_grad_(True) for x in P.mesh_frame(d(fx.cano), t(fx.faces), d(fx.verts))]
    out = P.phong_bind(v64, t(fx.faces), t(fx.fi[keep]), d(fx.bary[keep]), frame64, d(uvd[keep]), d(rot[keep]), d(scl[keep]))
    torch.autograd.backward(list(out), [d(a[keep]) for a in w])
    ref = [v64.grad, *[x.grad for x in frame64]]
    for j, i in enumerate(np.nonzero(bad)[0]):
        uvd[i, 2], rot[i, j % 4], scl[i, j % 3] = (NAN, INF, -INF)[j % 3], (INF, NAN, -INF)[j % 3], (-INF, INF, NAN)[j % 3]
        for a in w:
            a[i] = 0.0
    vd, fd = t(fx.verts).to(dev), t(fx.faces).to(dev)
    frame = phong_frame(phong_canonical(t(fx.cano).to(dev), fd), vd)
    outs = [torch.zeros(s, device=dev) for s in ((V, 3), (V, 3), (V, 4), (F,))]
    phong_scatter_frame_grads(vd, fd, t(fx.fi).to(dev), t(fx.bary).to(dev), frame, t(uvd).to(dev), t(rot).to(dev), t(scl).to(dev),
                              *[t(a).to(dev) for a in w], *outs)
    torch.cuda.synchronize()
    for name, g, r in zip(("d_verts", "d_vert_normals", "d_vert_quats", "d_face_ratio"), outs, ref):
        g = g.cpu().numpy()
        print(f"[nonfinite scatter] {name}: {int((~np.isfinite(g)).sum())} non-finite value(s) of {g.size}")
        _bind_rel(f"scatter alone {name}", g, r.numpy())


# ------------------------------------------------------------------ 6. one captured step
def test_captured_step_with_an_infinite_log_scale(gpu_device):
    """`SplattingStep(mesh_grad=True)` on the turned mesh, captured; after construction one Gaussian's log-scale is +inf.  Four
    steps (the third and the fourth are graph replays): `d_verts` is finite and within BIND_BOUND of the same step built
    without that Gaussian, and every other parameter stays finite.  Single-pixel Gaussians (tests/test_gpu_camera_grad.py's
    module docstring: log-scale -9, opacity 0.005), for which the frame's backward adds once per Gaussian and the two
    trajectories see the same gradients."""
    import torch
    from fateavatar_amd.binding import phong_canonical
    from fateavatar_amd.model import TorchCamera
    from fateavatar_amd.splatting import SplattingGaussians, SplattingStep
    dev = gpu_device
    fx = bound_fixture()
    t = lambda a: _t(a, dev)  # noqa: E731
    canonical = phong_canonical(t(fx.cano), t(fx.faces))
    cam, bg = TorchCamera(fx.cam, dev), torch.ones(3, device=dev)
    victim = int(np.nonzero(fx.bad["rows"])[0][0])
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(30 + k)).to(dev) for k in range(4)]
    rng = np.random.default_rng(3)
    uvd = (0.01 * rng.normal(size=(fx.N, 3))).astype(np.float32)
    dc = rng.uniform(-1, 1, (fx.N, 1, 3)).astype(np.float32)

    def run(keep, poison):
        pc = SplattingGaussians(t(fx.fi[keep]), t(fx.bary[keep]), -9.0, dev)
        with torch.no_grad():
            pc._uvd.copy_(t(uvd[keep]))
            pc._features_dc.copy_(t(dc[keep]))
            pc._opacity.fill_(float(np.log(0.0050 / 0.9950)))
        st = SplattingStep(pc, canonical, cam.clone(), bg, t(fx.verts), use_graph=True, mesh_grad=True)
        if poison:
            with torch.no_grad():
                pc._scaling[victim, 1] = INF
        grads = []
        for k in range(4):
            st.step(cam, t(fx.verts), gts[k])
            torch.cuda.synchronize()
            grads.append(st.d_verts.detach().cpu().numpy().copy())
        assert st._graph is not None, "the later steps are graph replays"
        return pc, grads

    everything = np.ones(fx.N, bool)
    without = everything.copy()
    without[victim] = False
    pc_c, g_c = run(without, False)
    pc_d, g_d = run(everything, True)
    for k in range(4):
        assert np.isfinite(g_d[k]).all(), (k, int((~np.isfinite(g_d[k])).sum()))
        assert np.abs(g_c[k]).max() > 0
        rl = util.rel_l2(g_d[k], g_c[k])
        print(f"[nonfinite step] step {k}: d_verts non-finite values 0, rel-L2 against the step without the Gaussian {rl:.2e} "
              f"(bound {BIND_BOUND:.0e})")
        assert rl <= BIND_BOUND, (k, rl)
    flat = pc_d.flat.detach().cpu().numpy()
    print(f"[nonfinite step] non-finite parameters after four steps: {int((~np.isfinite(flat)).sum())} (the one that was set)")
    assert int((~np.isfinite(flat)).sum()) == 1 and float(pc_d._scaling[victim, 1]) == INF
    for name, _ in pc_d.FIELDS:
        a, b = getattr(pc_d, name).detach().cpu().numpy(), getattr(pc_c, name).detach().cpu().numpy()
        if a.size:
            assert np.isfinite(a[without]).all() and util.rel_l2(a[without], b) <= 1e-3, name
