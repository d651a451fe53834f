"""Needle-shaped splats and a float64 reference of the blend loop whose tolerance follows the conditioning.  numpy / torch only:
nothing here runs the code under test.

A needle (long axis hundreds of pixels, width set by the 0.3 px^2 dilation) has a conic of conditioning 1 / (1 - rho^2) up to
1e5, and `power = -0.5 (a dx^2 + c dy^2) - b dx dy` then cancels terms of size m = (|a| dx^2 + |c| dy^2) / 2 + |b dx dy| ~ 1e4 ..
1e6 to a result of size 5: two correct fp32 evaluations differ by a few 1e-4 there, and the fixed 1e-4 / 1e-5 image tolerance of
the parity tests bounds nothing.  `composite64` evaluates the reference's loop (forward.cu:330-361) in float64 from the fp32
per-Gaussian state (centre, conic, opacity, depth, colour, radius: held bit-equal between oracle and kernel elsewhere) and
returns, per pixel,

  * a BOUND on what any fp32 evaluation may differ by: `power` is three products and two sums of terms bounded by m, at most 8
    roundings of 2^-24 m each whatever the order or the contractions (K = 8), so power is off by at most
    band = K 2^-24 m + 2e-6 (the 2e-6: exp and the product with the opacity), alpha by alpha x band, and a colour (in [0, 1]) or
    1 - T by at most 2 x sum(alpha T band) + 3e-6 over the blended entries;
  * whether the pixel is UNDECIDED: some entry that can still reach it sits within `band` of one of the loop's tests
    (power > 0, alpha < 1/255, the 0.99 clamp) or within 0.1 % of T (1 - alpha) < 1e-4.  Two correct implementations may take
    different decisions there; everywhere else they must take the float64 ones.

`backward64` is the same composite in torch float64 with those decisions fixed: the gradients that do not pass through the
conic (centre, opacity, colour), which are well-posed on needles."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from fateavatar_amd import scenes

U24 = 2.0 ** -24
C0 = 0.28209479177387814
BG = (0.1, 0.2, 0.3)


def _quat_mul(p, q):
    pr, px, py, pz = p.T
    qr, qx, qy, qz = q.T
    return np.stack([pr * qr - px * qx - py * qy - pz * qz, pr * qx + px * qr + py * qz - pz * qy,
                     pr * qy - px * qz + py * qr + pz * qx, pr * qz + px * qy - py * qx + pz * qr], 1)


def _scene(means, long_world, short, theta, tilt, op, rgb, H, W, tanfov=0.2):
    """A GaussianScene of needles: local x axis (the long scale) turned to (cos tilt cos theta, cos tilt sin theta, sin tilt)."""
    P = means.shape[0]
    z0 = np.zeros(P)
    qz = np.stack([np.cos(theta / 2), z0, z0, np.sin(theta / 2)], 1)
    qy = np.stack([np.cos(-tilt / 2), z0, np.sin(-tilt / 2), z0], 1)   # R_y(-tilt): x -> (cos tilt, 0, sin tilt)
    q = _quat_mul(qz, qy)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    sc = np.concatenate([np.asarray(long_world, np.float64)[:, None], short], 1)
    shs = ((np.asarray(rgb, np.float64) - 0.5) / C0)[:, None, :]
    fov = 2 * math.atan(tanfov)
    fovy = 2 * math.atan(tanfov * H / W) if H != W else fov
    cam = scenes.make_camera(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), fov, fovy, H, W)
    f = np.float32
    return scenes.GaussianScene(means.astype(f), sc.astype(f), q.astype(f), np.asarray(op, f).reshape(P, 1), shs.astype(f), 0,
                                np.asarray(BG, f), cam)


def needle_scene(P, H, W, seed, long_px_max):
    """P needles in front of the identity camera (tan(fov_x / 2) = 0.2): depth 0.8 .. 1.2, centres uniform over 1.15 x the
    frustum (some off-image), 1-sigma length log-uniform 4 .. long_px_max pixels, the two short scales log-uniform
    10^-4.5 .. 10^-2.7 (the 0.3 px^2 dilation then sets the width), long axis at a uniform angle in the image plane — a quarter
    of them within N(0, 1e-2) rad of a multiple of 45 degrees — tilted N(0, 0.15) rad out of it.  Opacity 0.02 .. 0.6; every 7th
    0.99 (clamped: the 3-sigma rectangle cuts inside its alpha >= 1/255 ellipse), every 11th 0.0045 (just above 1/255)."""
    rng = np.random.default_rng(seed)
    tanfov = 0.2
    focal = W / (2 * tanfov)
    z = rng.uniform(0.8, 1.2, P)
    cx = rng.uniform(-1.15, 1.15, P) * tanfov * z
    cy = rng.uniform(-1.15, 1.15, P) * (tanfov * H / W) * z
    long_px = np.exp(rng.uniform(math.log(4.0), math.log(long_px_max), P))
    short = 10.0 ** rng.uniform(-4.5, -2.7, (P, 2))
    theta = rng.uniform(0, 2 * math.pi, P)
    snapped = rng.random(P) < 0.25
    theta = np.where(snapped, rng.integers(0, 8, P) * (math.pi / 4) + rng.normal(0, 1e-2, P), theta)
    tilt = rng.normal(0, 0.15, P)
    op = rng.uniform(0.02, 0.6, P)
    op[::7] = 0.99
    op[::11] = 0.0045
    rgb = rng.uniform(0.05, 0.95, (P, 3))
    return _scene(np.stack([cx, cy, z], 1), long_px * z / focal, short, theta, tilt, op, rgb, H, W, tanfov)


def hand_needle(H, W, centre_px, theta, long_px, opacity, rgb=(0.9, 0.5, 0.2), z=1.0, short=1e-4):
    """One needle in the image plane with its centre at pixel coordinates `centre_px`, up to the fp32 rounding of the projection
    (a few 1e-6 pixel: not every fp32 pixel coordinate is the image of an fp32 mean)."""
    tanfov = 0.2
    focal = W / (2 * tanfov)
    px, py = centre_px
    means = np.array([[(px + 0.5 - W / 2) * z / focal, (py + 0.5 - H / 2) * z / focal, z]])
    return _scene(means, np.array([long_px * z / focal]), np.full((1, 2), short), np.array([theta]), np.array([0.0]),
                  [opacity], [rgb], H, W, tanfov)


def state_of_oracle(o):
    """composite64's per-Gaussian arguments from an oracle forward."""
    return dict(xy=o.means2D, conic_opacity=o.conic_opacity, depth=o.depths, radii=o.radii,
                rgb=o.rgb if o._inputs["colors_precomp"] is None else o._inputs["colors_precomp"])


def state_of_record(rec, radii):
    """The same from the kernel's blend-record template (`geometry(8, 12)`: centre, (-0.5 a, -b, -0.5 c), opacity, colour,
    depth in column 10; the scalings are exact) and its radii."""
    f = np.float32
    co = np.stack([rec[:, 2] * f(-2), -rec[:, 3], rec[:, 4] * f(-2), rec[:, 5]], 1).astype(f)
    return dict(xy=rec[:, 0:2].copy(), conic_opacity=co, depth=rec[:, 10].copy(), radii=np.asarray(radii), rgb=rec[:, 6:9].copy())


def _rect(px, py, r, H, W):
    """getRect (auxiliary.h:46-56) in fp32 -> the pixel ranges [x0, x1) x [y0, y1) of the 16x16 tiles it names."""
    f = np.float32
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r = f(int(r))
    x0 = min(gx, max(0, int((f(px) - r) / f(16))))
    y0 = min(gy, max(0, int((f(py) - r) / f(16))))
    x1 = min(gx, max(0, int((f(px) + r + f(15)) / f(16))))
    y1 = min(gy, max(0, int((f(py) + r + f(15)) / f(16))))
    return x0 * 16, min(x1 * 16, W), y0 * 16, min(y1 * 16, H)


@dataclass
class Composite:
    """`composite64`'s result.  bound = 2 (K s1 + s0) + 3e-6 and undecided = (k_und <= K) are kept in a form that can be
    evaluated again at another K (`at`): the decisions of the float64 walk do not depend on K."""
    K: float
    color: np.ndarray        # [3,H,W] float64
    T: np.ndarray            # [H,W]
    depth: np.ndarray        # [H,W]  sum of alpha T z
    n_blended: np.ndarray    # [H,W]  entries blended
    rim: np.ndarray          # [H,W]  some blended entry has alpha in [1/255, 3/255)
    s1: np.ndarray           # [H,W]  sum of alpha T 2^-24 m
    s0: np.ndarray           # [H,W]  sum of alpha T 2e-6
    k_und: np.ndarray        # [H,W]  smallest K at which the pixel is undecided (inf: never, 0: the T test)
    order: np.ndarray        # the blended Gaussians, front to back
    blend_idx: dict = field(repr=False, default_factory=dict)   # Gaussian -> flat indices of the pixels that blend it

    @property
    def bound(self):
        return 2.0 * (self.K * self.s1 + self.s0) + 3e-6

    @property
    def undecided(self):
        return self.k_und <= self.K

    @property
    def covered(self):
        return self.T < 1.0

    def at(self, K):
        import copy
        c = copy.copy(self)
        c.K = float(K)
        return c

    def undecided_share(self):
        return float((self.undecided & self.covered).sum()) / max(1, int(self.covered.sum()))

    def smallest_K(self, color, T):
        """The smallest K at which `color` / `T` lie within the bound on every pixel that is decided at K = 8."""
        err = np.maximum(np.abs(np.asarray(color, np.float64) - self.color).max(0), np.abs(np.asarray(T, np.float64) - self.T))
        need = (err - 3e-6) / 2.0 - self.s0
        dec = ~(self.k_und <= 8.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(need <= 0, 0.0, need / self.s1)     # (s1 = 0 with need > 0: nothing blended, yet off: inf)
        return float(k[dec].max()) if dec.any() else 0.0


def composite64(xy, conic_opacity, depth, radii, rgb, bg, H, W, K, drop=None):
    """The reference's blend loop in float64 from the fp32 per-Gaussian state.  Order: depth bits, then id (the reference's
    stable sort of (tile | depth) keys emitted in id order).  Each Gaussian is confined to the pixels of its reference
    rectangle.  Gates: power <= 0, alpha = min(0.99, o e^power) >= 1/255, stop at T (1 - alpha) < 1e-4.  dx, dy are the fp32
    differences every implementation forms first (centre - pixel), exact from there on.
    `drop` = (Gaussian, tx, ty): leave that Gaussian out of the 8x8 tile (tx, ty) — a mutant of the reference, to show what
    the bound can see."""
    f = np.float32
    xy, co = np.asarray(xy, f), np.asarray(conic_opacity, f)
    radii = np.asarray(radii)
    ids = np.nonzero(radii > 0)[0]
    dbits = np.asarray(depth, f).reshape(-1).view(np.uint32)
    ids = ids[np.lexsort((ids, dbits[ids]))]
    T = np.ones((H, W))
    C = np.zeros((3, H, W))
    D = np.zeros((H, W))
    s1, s0 = np.zeros((H, W)), np.zeros((H, W))
    done = np.zeros((H, W), bool)
    k_und = np.full((H, W), np.inf)
    nbl = np.zeros((H, W), np.int64)
    rim = np.zeros((H, W), bool)
    blend_idx, order = {}, []
    for g in ids.tolist():
        x0, x1, y0, y1 = _rect(xy[g, 0], xy[g, 1], radii[g], H, W)
        if x1 <= x0 or y1 <= y0:
            continue
        sl = (slice(y0, y1), slice(x0, x1))
        dx = (xy[g, 0] - np.arange(x0, x1, dtype=f)).astype(np.float64)[None, :]
        dy = (xy[g, 1] - np.arange(y0, y1, dtype=f)).astype(np.float64)[:, None]
        a, b, c, o = (float(v) for v in co[g])
        power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
        m = 0.5 * (abs(a) * dx * dx + abs(c) * dy * dy) + np.abs(b * dx * dy)
        raw = o * np.exp(np.minimum(power, 0.0))
        alpha = np.minimum(0.99, raw)
        live = ~done[sl]
        if drop is not None and drop[0] == g:
            ys, xs = np.arange(y0, y1)[:, None] // 8, np.arange(x0, x1)[None, :] // 8
            live = live & ~((xs == drop[1]) & (ys == drop[2]))
        cand = live & (power <= 0.0) & (alpha >= 1.0 / 255.0)
        tt = T[sl] * (1.0 - alpha)
        stop = cand & (tt < 1e-4)
        blend = cand & ~stop
        # the smallest K at which a test of this entry is within band = K 2^-24 m + 2e-6 of its threshold
        um = np.maximum(U24 * m, 1e-300)
        margin = np.minimum(np.abs(power), np.abs(math.log(255.0 * o) + power) if o > 0 else np.inf)
        margin = np.minimum(margin, np.abs(raw - 0.99) / 0.99)
        ku = np.maximum(0.0, (margin - 2e-6) / um)
        ku = np.where(cand & (np.abs(tt - 1e-4) <= 1e-3 * 1e-4), 0.0, ku)
        k_und[sl] = np.where(live, np.minimum(k_und[sl], ku), k_und[sl])
        if blend.any():
            w = np.where(blend, alpha * T[sl], 0.0)
            C[(slice(None),) + sl] += np.asarray(rgb[g], np.float64)[:, None, None] * w
            D[sl] += float(depth[g]) * w
            s1[sl] += w * U24 * m
            s0[sl] += w * 2e-6
            T[sl] = np.where(blend, tt, T[sl])
            nbl[sl] += blend
            rim[sl] |= blend & (alpha < 3.0 / 255.0)
            yy, xx = np.nonzero(blend)
            blend_idx[g] = (yy + y0) * W + (xx + x0)
            order.append(g)
        done[sl] |= stop
    color = C + T[None] * np.asarray(bg, np.float64)[:, None, None]
    return Composite(float(K), color, T, D, nbl, rim, s1, s0, k_und, np.asarray(order, np.int64), blend_idx)


def backward64(comp, xy, conic_opacity, rgb, bg, dL_dpix, H, W):
    """dL/d(centre), dL/d(opacity), dL/d(colour) of sum(dL_dpix x image) by torch float64 autograd of the same composite, the
    decisions fixed to `comp`'s (which pixels blend which Gaussian).  The conic is constant.  The 0.99 clamp passes the
    gradient through, as backward.cu:503-530 does (dL_dG = opacity x dL_dalpha whether or not alpha was clamped);
    dL_dmeans2D is the pixel-space gradient times (W / 2, H / 2) (backward.cu: ddelx_dx, ddely_dy).
    -> (dL_dmeans2D[:, :2], dL_dopacity [P,1], dL_dcolors [P,3]) as float64 numpy."""
    dd = torch.float64
    f = np.float32
    xy32, co = np.asarray(xy, f), np.asarray(conic_opacity, np.float64)
    X = torch.tensor(xy32.astype(np.float64), dtype=dd, requires_grad=True)
    O = torch.tensor(co[:, 3].copy(), dtype=dd, requires_grad=True)
    R = torch.tensor(np.asarray(rgb, np.float64), dtype=dd, requires_grad=True)
    Tt = torch.ones(H * W, dtype=dd)
    Cc = torch.zeros((3, H * W), dtype=dd)
    for g in comp.order.tolist():
        idx = comp.blend_idx[g]
        px, py = (idx % W).astype(f), (idx // W).astype(f)
        # the fp32 difference the loop forms, as a function of the centre: slope one, value fl32(centre - pixel)
        dx0, dy0 = (xy32[g, 0] - px).astype(np.float64), (xy32[g, 1] - py).astype(np.float64)
        dx = (X[g, 0] - X[g, 0].detach()) + torch.from_numpy(dx0)
        dy = (X[g, 1] - X[g, 1].detach()) + torch.from_numpy(dy0)
        a, b, c = co[g, 0], co[g, 1], co[g, 2]
        power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
        raw = O[g] * torch.exp(power)
        alpha = raw + (torch.clamp_max(raw, 0.99) - raw).detach()
        ti = torch.from_numpy(idx)
        Tin = Tt[ti]
        Cc = Cc.index_add(1, ti, R[g][:, None] * (alpha * Tin)[None, :])
        Tt = Tt.index_put((ti,), Tin * (1.0 - alpha))
    img = Cc + Tt[None, :] * torch.tensor(np.asarray(bg, np.float64), dtype=dd)[:, None]
    assert np.abs(img.detach().numpy().reshape(3, H, W) - comp.color).max() < 1e-12
    (img * torch.tensor(np.asarray(dL_dpix, np.float64).reshape(3, H * W), dtype=dd)).sum().backward()
    half = np.array([0.5 * W, 0.5 * H])
    return X.grad.numpy() * half[None, :], O.grad.numpy()[:, None], R.grad.numpy()


def upstream(comp, seed, rim_only):
    """dL/dpixel for the gradient checks: uniform noise / (H W) on every decided pixel — or on the decided RIM pixels only
    (some blended entry has alpha in [1/255, 3/255)), zero elsewhere: a dropped rim tile or mask bit is then a first-order
    error of the gradient, not 1e-4 of a needle's total."""
    H, W = comp.T.shape
    g = np.random.default_rng(seed).uniform(-1, 1, (3, H, W)) / (H * W)
    keep = ~comp.undecided & (comp.rim if rim_only else True)
    return (g * keep[None]).astype(np.float32)


# ------------------------------------------------------------------ the scenes of the needle tests
def scene_A(seed):
    return needle_scene(48, 128, 128, seed, 300)


def scene_B(seed=5):
    return needle_scene(160, 136, 200, seed, 1000)


def rim_tile(comp, W):
    """(Gaussian, tx, ty): the needle that is blended at the most pixels, and the 8x8 tile in which it is blended at the
    fewest (>= 1) — the tile whose loss changes the image least."""
    g = max(comp.blend_idx, key=lambda k: comp.blend_idx[k].size)
    idx = comp.blend_idx[g]
    tiles, n = np.unique(((idx // W) // 8) * 65536 + (idx % W) // 8, return_counts=True)
    t = int(tiles[np.argmin(n)])
    return g, t % 65536, t // 65536


C_H, C_W = 72, 40


def scenes_C():
    """name -> one needle on 72 x 40, at the places where the three footprint tests can go wrong."""
    q = math.pi / 4
    S = {}
    S["diag45_tile_corners"] = hand_needle(C_H, C_W, (15.5, 15.5), q, 40, 0.5)       # through (8k - 0.5, 8k - 0.5)
    S["diag45_shifted_2^-10"] = hand_needle(C_H, C_W, (15.5 + 2.0 ** -10, 15.5), q, 40, 0.5)
    for name, y in (("seam", 7.5), ("seam_minus", 7.5 - 1e-3), ("seam_plus", 7.5 + 1e-3)):
        S["axis_" + name] = hand_needle(C_H, C_W, (20.0, y), 0.0, 60, 0.5)
    S["axis_one_tile_high"] = hand_needle(C_H, C_W, (12.0, 19.6), 0.0, 60, 0.3)      # rows 16 .. 23: the rw > 1 && rh > 1 shortcut
    S["offscreen_pointing_in"] = hand_needle(C_H, C_W, (-20.0, 30.0), 0.3, 80, 0.5)
    S["opacity_0.99"] = hand_needle(C_H, C_W, (17.3, 33.1), 1.1, 50, 0.99)
    S["opacity_0.0045"] = hand_needle(C_H, C_W, (17.3, 33.1), 1.1, 50, 0.0045)
    return S


def all_scenes():
    """name -> scene: A (two seeds), B, and the cases of C."""
    S = {"A_seed1": scene_A(1), "A_seed2": scene_A(2), "B": scene_B()}
    S.update({"C_" + k: v for k, v in scenes_C().items()})
    return S


SCENE_NAMES = ("A_seed1", "A_seed2", "B") + tuple("C_" + k for k in (
    "diag45_tile_corners", "diag45_shifted_2^-10", "axis_seam", "axis_seam_minus", "axis_seam_plus", "axis_one_tile_high",
    "offscreen_pointing_in", "opacity_0.99", "opacity_0.0045"))
_CACHE = {}


class OracleRef:
    """What the needle tests need from the CPU side of one scene, computed once and left unchanged: the oracle's forward `o`,
    the float64 composite of its state at K = 8 (`comp8`), `K_oracle` (the smallest K at which the oracle's own image lies
    within the bound) and the K the kernel is held to, min(8, 4 K_oracle)."""

    def __init__(self, name):
        from tests import util
        self.name, self.s = name, all_scenes()[name]
        self.H, self.W = self.s.camera.image_height, self.s.camera.image_width
        self.o = util.oracle_forward(self.s)
        self.state = state_of_oracle(self.o)
        self.comp8 = composite64(**self.state, bg=self.s.bg, H=self.H, W=self.W, K=8.0)
        self.K_oracle = self.comp8.smallest_K(self.o.color, self.o.final_T)
        self.K_kernel = min(8.0, 4.0 * self.K_oracle)
        self._grad = {}

    def gradient_reference(self, comp, rim_only, seed=3):
        """(dL/dpixel, backward64's (means2D, opacity, colours), rel-L2 against them of the oracle's plain backward and of its
        backward in a seeded float order with contractions: the two measures of what an fp32 backward may be off by)."""
        from tests import util
        key = (rim_only, seed, comp.K)
        if key not in self._grad:
            d = upstream(comp, seed, rim_only)
            want = backward64(comp, self.state["xy"], self.state["conic_opacity"], self.state["rgb"], self.s.bg, d, self.H, self.W)
            runs = [oracle_backward(self.o, d), oracle_backward(self.o, d, 1, True)]
            rels = [[util.rel_l2(a, w) for a, w in zip((b.dL_dmeans2D[:, :2], b.dL_dopacity, b.dL_dcolors), want)] for b in runs]
            self._grad[key] = (d, want, rels[0], rels[1])
        return self._grad[key]


def oracle_backward(o, dpix, float_order=0, contract=False):
    """The oracle's backward: plain (double sums), or with float sums in a seeded order and / or nvcc-style contractions — on
    ONE thread then, so that the order, and with it every bound derived from the result, is the same in every run."""
    from oracle import oracle
    if not float_order and not contract:
        return oracle.backward(o, dpix)
    n = oracle.num_threads()
    oracle.set_num_threads(1)
    oracle.set_bwd_float_order(float_order)
    oracle.set_bwd_contract(contract)
    try:
        return oracle.backward(o, dpix)
    finally:
        oracle.set_bwd_float_order(0)
        oracle.set_bwd_contract(False)
        oracle.set_num_threads(n)


def pooled(rows):
    """Root of the sum of squares, per array, of per-case relative errors: every case of a scene weighs the same."""
    return [math.sqrt(sum(float(r[i]) ** 2 for r in rows)) for i in range(len(rows[0]))]


def oracle_ref(name) -> OracleRef:
    if name not in _CACHE:
        _CACHE[name] = OracleRef(name)
    return _CACHE[name]
