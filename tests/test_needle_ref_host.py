"""CPU: the float64 needle reference (tests/needle_ref.py) against the oracle alone.  These are the conditions under which the
GPU tests of tests/test_gpu_needles.py cannot hide a failure, and the reference has to meet them without the code under test:

  * the pixels it leaves out as UNDECIDED (an entry within the rounding band of a threshold) are at most 0.5 % of the covered
    pixels, so nearly every pixel is held to the bound;
  * every decided pixel of the oracle's colour and final_T — a plain fp32 evaluation of the loop — lies within the bound at the
    derivable worst case K = 8 (K_oracle, the smallest K at which it would, is printed: the kernel is held to 4 x that);
  * the bound can see a dropped pair: with one 8x8 tile of one needle left out of the float64 composite, the oracle's image
    falls outside it."""
import numpy as np
import pytest

from tests import needle_ref as nr


def test_needle_scenes_are_needles():
    """What the scenes are for: conditioning 1 / (1 - rho^2) in the 1e4s (A) and 1e5s (B), radii far beyond the image,
    centres off-image, opacities on the clamp and just above 1/255."""
    for name, cond_min, radius_min in (("A_seed1", 1e4, 500), ("A_seed2", 1e4, 500), ("B", 1e5, 2000)):
        r = nr.oracle_ref(name)
        o = r.o
        vis = o.radii > 0
        a, b, c = (o.conic_opacity[vis, k].astype(np.float64) for k in range(3))
        cond = a * c / (a * c - b * b)
        off = (o.means2D[vis, 0] < 0) | (o.means2D[vis, 0] > r.W - 1) | (o.means2D[vis, 1] < 0) | (o.means2D[vis, 1] > r.H - 1)
        print(f"[needles] {name}: {int(vis.sum())} visible, conditioning up to {cond.max():.2e}, radii up to {o.radii.max()}, "
              f"{int(off.sum())} centres off-image")
        assert cond.max() >= cond_min and o.radii.max() >= radius_min and off.any(), name
        assert (r.s.opacities == np.float32(0.99)).any() and (r.s.opacities == np.float32(0.0045)).any()
        assert r.s.camera.image_height == r.H and float(o.rgb[vis].min()) >= 0.0 and float(o.rgb[vis].max()) <= 1.0


def test_hand_built_needles_are_where_they_are_meant_to_be():
    """Scene C: the projected centres within 1e-5 pixel of the stated ones, the 45 degree conic symmetric to an ulp (a = c), the
    axis-aligned one diagonal, the seam cases strictly either side of y = 7.5."""
    c = {n: nr.oracle_ref("C_" + n).o for n in ("diag45_tile_corners", "diag45_shifted_2^-10", "axis_seam", "axis_seam_minus",
                                                "axis_seam_plus", "axis_one_tile_high", "offscreen_pointing_in")}
    want = {"diag45_tile_corners": (15.5, 15.5), "diag45_shifted_2^-10": (15.5 + 2.0 ** -10, 15.5), "axis_seam": (20.0, 7.5),
            "axis_seam_minus": (20.0, 7.5 - 1e-3), "axis_seam_plus": (20.0, 7.5 + 1e-3), "axis_one_tile_high": (12.0, 19.6),
            "offscreen_pointing_in": (-20.0, 30.0)}
    for n, o in c.items():
        assert o.radii[0] > 0 and np.abs(o.means2D[0].astype(np.float64) - np.array(want[n])).max() < 1e-5, (n, o.means2D[0])
    for n in ("diag45_tile_corners", "diag45_shifted_2^-10"):
        a, b, cc = (float(v) for v in c[n].conic_opacity[0, :3])
        assert abs(a - cc) <= 2.0 ** -22 * a and b < 0 and a * cc / (a * cc - b * b) > 1e3, (n, a, b, cc)
    assert c["diag45_shifted_2^-10"].means2D[0, 0] - c["diag45_tile_corners"].means2D[0, 0] == pytest.approx(2.0 ** -10, abs=2e-6)
    for n in ("axis_seam", "axis_seam_minus", "axis_seam_plus", "axis_one_tile_high"):
        a, b, cc = (float(v) for v in c[n].conic_opacity[0, :3])
        assert abs(b) < 1e-8 and a < 1e-3 < cc, (n, a, b, cc)
    assert c["axis_seam_minus"].means2D[0, 1] < 7.5 - 5e-4 and c["axis_seam_plus"].means2D[0, 1] > 7.5 + 5e-4
    assert abs(float(c["axis_seam"].means2D[0, 1]) - 7.5) < 1e-5


@pytest.mark.parametrize("name", nr.SCENE_NAMES)
def test_oracle_lies_within_the_float64_bound(name):
    r = nr.oracle_ref(name)
    c = r.comp8
    share = c.undecided_share()
    err = np.maximum(np.abs(r.o.color - c.color).max(0), np.abs(r.o.final_T - c.T))
    dec = ~c.undecided
    used = float((err / c.bound)[dec].max())
    print(f"[needle ref] {name}: covered {int(c.covered.sum())}, undecided {share:.3%} of them, oracle uses {used:.1%} of the K = 8 "
          f"bound, K_oracle {r.K_oracle:.3f}, kernel K {r.K_kernel:.3f} (undecided there: {c.at(r.K_kernel).undecided_share():.3%})")
    assert c.covered.any(), name
    assert share <= 0.005, (name, share)
    bad = dec & (err > c.bound)
    assert not bad.any(), (name, int(bad.sum()), used)
    assert r.K_oracle <= 8.0
    # n_contrib == 0 exactly where nothing is blended
    assert np.array_equal((r.o.n_contrib == 0)[dec], (c.n_blended == 0)[dec]), name


@pytest.mark.parametrize("name", ["A_seed1", "B"])
def test_the_bound_sees_one_dropped_tile(name):
    """A mutant of the REFERENCE: the needle that covers the most pixels loses the 8x8 tile in which it is blended at the fewest
    pixels (a rim tile: often a single pixel of alpha ~ 1/255).  The oracle, which blends it there, must then fail."""
    r = nr.oracle_ref(name)
    g, tx, ty = nr.rim_tile(r.comp8, r.W)
    m = nr.composite64(**r.state, bg=r.s.bg, H=r.H, W=r.W, K=8.0, drop=(g, tx, ty))
    err = np.maximum(np.abs(r.o.color - m.color).max(0), np.abs(r.o.final_T - m.T))
    bad = ~m.undecided & (err > m.bound)
    ys, xs = np.nonzero(bad)
    print(f"[needle ref] {name}: needle {g} without tile ({tx}, {ty}): {int(bad.sum())} pixel(s) outside the bound")
    assert bad.any(), name
    assert np.all((xs // 8 == tx) & (ys // 8 == ty)), "only the dropped tile may differ"


@pytest.mark.parametrize("name", ["A_seed2", "C_opacity_0.99"])
def test_backward64_is_the_oracles_backward(name):
    """A check of the MODEL (clamp pass-through, the (W / 2, H / 2) factor, which pixels blend what), not a bound anything else
    copies: the oracle's three conic-free gradients agree with backward64 to fp32 noise, amplified by the cancellation in
    `power` (measured 2e-5 .. 8e-4 on these scenes); a wrong model is off by O(1)."""
    r = nr.oracle_ref(name)
    for rim_only in (False, True):
        d, want, plain, seeded = r.gradient_reference(r.comp8.at(r.K_kernel), rim_only)
        print(f"[needle ref] {name} rim_only={rim_only}: oracle vs backward64 rel-L2 (means2D, opacity, colours) plain {plain}, "
              f"float order + contraction {seeded}")
        assert np.any(d != 0) and all(np.isfinite(w).all() and np.any(w != 0) for w in want)
        assert max(plain + seeded) < 1e-2, (name, plain, seeded)
