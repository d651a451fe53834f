"""The float64 reference of the camera-pose gradients (FR_FLAG_CAMERA_GRAD): the differentiable torch restatement of the
forward that tests/test_oracle_autograd.py holds the oracle's backward to, stated again here with the CAMERA as a variable.

`V` (world_view_transform), `F` (full_proj_transform) and `cam` (camera_center) are leaves expanded to ONE COPY PER
GAUSSIAN ([P,4,4], [P,4,4], [P,3]).  One backward then gives, per entry of the three, both the camera gradient (the sum of
the copies' gradients over P) and its SCALE: the sum of the absolute per-Gaussian contributions, which is what a float32 sum
of those contributions can be held to (|error| <= 1e-4 scale is the project's gradient parity).

As in the original, the discrete decisions are the oracle's (sorted per-tile lists, n_contrib, the alpha and power tests of
the float32 run) and the reference's stop-gradient on guard-band-clamped view-space x / y (backward.cu:168-176, 262-264) is
part of the function: parity means reproducing it.  It also renders the depth plane sum z alpha T of FR_FLAG_DEPTH_ALPHA.
Central finite differences are no check of any of this: the alpha-threshold and `power <= 0` masks flip under a 1e-6
perturbation."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

from fateavatar_amd import scenes
from tests import util

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]
DD = torch.float64

# the issue's scenes: guard-band-clamped Gaussians (49 of 214 visible at seed 3) / every Gaussian visible, none clamped
SCENE_KW = dict(M=16, scale_lo=0.01, scale_hi=0.06, opacity_lo=0.2, opacity_hi=0.9, bg=(0.2, 0.5, 0.9), tanfov=0.25)


def scene(seed=3, deg=3, spread=0.45, P=260):
    return scenes.random_scene(P, 48, 40, sh_degree=deg, seed=seed, spread=spread, **SCENE_KW)


def seeded_dpix(H, W):
    """The seeded dL/dpixel of tests/test_oracle_autograd.py."""
    return np.random.default_rng(1).uniform(-1, 1, (3, H, W)).astype(np.float32)


def seeded_ddepth(H, W):
    return np.random.default_rng(2).uniform(-1, 1, (H, W)).astype(np.float32)


def sh_rgb(deg, sh, d):
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    r = C0 * sh[:, 0]
    if deg > 0:
        r = r - C1 * y * sh[:, 1] + C1 * z * sh[:, 2] - C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = r + C2[0] * xy * sh[:, 4] + C2[1] * yz * sh[:, 5] + C2[2] * (2 * zz - xx - yy) * sh[:, 6] + \
            C2[3] * xz * sh[:, 7] + C2[4] * (xx - yy) * sh[:, 8]
    if deg > 2:
        r = r + C3[0] * y * (3 * xx - yy) * sh[:, 9] + C3[1] * xy * z * sh[:, 10] + C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + \
            C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12] + C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + \
            C3[5] * z * (xx - yy) * sh[:, 14] + C3[6] * x * (xx - 3 * yy) * sh[:, 15]
    return torch.clamp_min(r + 0.5, 0.0)


def torch_render(s, f, Pr, V, F, cam, cov3D=None, Vw=None):
    """float64 differentiable forward.  Pr: dict of leaf tensors (means3D, scales, rotations, opacities, shs); V, F [P,4,4] and
    cam [P,3]: the camera, one copy per Gaussian (row-vector convention: p' = [x y z 1] @ V); cov3D [P,6]: the covariance
    given instead of scales and rotations; Vw: a second copy of V for its OTHER use, the rotation inside the 2D covariance's
    T = J W (V itself then only makes the view-space mean).  Returns (image [3,H,W], depth [H,W])."""
    c = s.camera
    H, W = c.image_height, c.image_width
    m = Pr["means3D"]
    hom = torch.cat([m, torch.ones_like(m[:, :1])], 1)
    pv = torch.einsum("pi,pij->pj", hom, V)
    ph = torch.einsum("pi,pij->pj", hom, F)
    pw = 1.0 / (ph[:, 3] + 1e-7)
    ndc = ph[:, :2] * pw[:, None]
    pix = torch.stack([((ndc[:, 0] + 1) * W - 1) * 0.5, ((ndc[:, 1] + 1) * H - 1) * 0.5], 1)
    if cov3D is None:
        q = Pr["rotations"]
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
        M = R @ torch.diag_embed(Pr["scales"])
        Sig = M @ M.transpose(1, 2)
    else:
        c0, c1, c2, c3, c4, c5 = (cov3D[:, k] for k in range(6))
        Sig = torch.stack([c0, c1, c2, c1, c3, c4, c2, c4, c5], 1).view(-1, 3, 3)
    # EWA with the reference's stop-gradient on clamped t.x / t.y
    tx, ty, tz = pv[:, 0], pv[:, 1], pv[:, 2]
    limx, limy = 1.3 * c.tanfovx, 1.3 * c.tanfovy
    cx = torch.where((tx / tz).abs() > limx, (torch.clamp(tx / tz, -limx, limx) * tz).detach(), tx)
    cy = torch.where((ty / tz).abs() > limy, (torch.clamp(ty / tz, -limy, limy) * tz).detach(), ty)
    fx, fy = W / (2 * c.tanfovx), H / (2 * c.tanfovy)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * cx / (tz * tz), zero, fy / tz, -fy * cy / (tz * tz)], 1).view(-1, 2, 3)
    Wm = (V if Vw is None else Vw)[:, :3, :3].transpose(1, 2)  # view rotation acting on column vectors
    T = J @ Wm
    cov = T @ Sig @ T.transpose(1, 2)
    a, b, cc = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * cc - b * b
    conic = torch.stack([cc / det, -b / det, a / det], 1)
    d = m - cam
    d = d / d.norm(dim=1, keepdim=True)
    rgb = sh_rgb(s.sh_degree, Pr["shs"], d)
    op = Pr["opacities"][:, 0]

    img = torch.zeros((3, H, W), dtype=DD)
    depth = torch.zeros((H, W), dtype=DD)
    bg = torch.tensor(s.bg, dtype=DD)
    gx = (W + 15) // 16
    ncon = torch.tensor(f.n_contrib.astype(np.int64))
    for tile in range(f.ranges.shape[0]):
        r0, r1 = int(f.ranges[tile, 0]), int(f.ranges[tile, 1])
        tx0, ty0 = (tile % gx) * 16, (tile // gx) * 16
        ys, xs = torch.meshgrid(torch.arange(ty0, min(ty0 + 16, H)), torch.arange(tx0, min(tx0 + 16, W)), indexing="ij")
        Tt = torch.ones(ys.shape, dtype=DD)
        Cc = torch.zeros((3,) + ys.shape, dtype=DD)
        Dz = torch.zeros(ys.shape, dtype=DD)
        last = ncon[ys, xs]
        for k in range(r0, r1):
            g = int(f.point_list[k])
            dx, dy = pix[g, 0] - xs, pix[g, 1] - ys
            power = -0.5 * (conic[g, 0] * dx * dx + conic[g, 2] * dy * dy) - conic[g, 1] * dx * dy
            alpha = torch.clamp_max(op[g] * torch.exp(power), 0.99)
            use = ((k - r0) < last) & (power <= 0) & (alpha >= 1.0 / 255.0)
            w = torch.where(use, alpha * Tt, torch.zeros_like(Tt))
            Cc = Cc + rgb[g][:, None, None] * w
            Dz = Dz + tz[g] * w
            Tt = torch.where(use, Tt * (1 - alpha), Tt)
        img[:, ys, xs] = Cc + Tt * bg[:, None, None]
        depth[ys, xs] = Dz
    return img, depth


def camera_reference(s, f, dpix, ddepth=None, cov3D=None):
    """The float64 camera gradients of loss = sum(image * dpix) (+ sum(depth * ddepth)) for the scene `s` with the oracle
    forward `f`.  Returns a namespace: per-Gaussian gradients pV [P,4,4], pF [P,4,4], pcam [P,3] (their sums dV, dF, dcam are
    the camera gradients, the sums of their absolute values sV, sF, scam the scales), dmeans [P,3] = dL/dmeans3D, and the
    rendered image / depth.  sV_paths: the scale of the view matrix with a Gaussian's two paths — through the view-space mean and
    through W — taken in absolute value SEPARATELY: for a Gaussian inside the guard band the two cancel analytically in
    view[2][0] and view[2][1] (sV has nothing of it there), while float32 forms them as separate products and resolves their
    sum no better than eps times their size."""
    c = s.camera
    Pn = s.P
    Pr = {k: torch.tensor(v, dtype=DD, requires_grad=(k == "means3D")) for k, v in
          dict(means3D=s.means3D, scales=s.scales, rotations=s.rotations, opacities=s.opacities, shs=s.shs).items()}
    ex = lambda a: torch.tensor(np.asarray(a), dtype=DD).expand((Pn,) + np.shape(a)).clone().requires_grad_(True)  # noqa: E731
    V, F, cam, Vw = ex(c.world_view_transform), ex(c.full_proj_transform), ex(c.camera_center), ex(c.world_view_transform)
    img, depth = torch_render(s, f, Pr, V, F, cam, None if cov3D is None else torch.tensor(cov3D, dtype=DD), Vw=Vw)
    loss = (img * torch.tensor(dpix, dtype=DD)).sum()
    if ddepth is not None:
        loss = loss + (depth * torch.tensor(ddepth, dtype=DD)).sum()
    loss.backward()
    n = lambda t: t.detach().numpy()  # noqa: E731
    pV, pF, pcam = n(V.grad) + n(Vw.grad), n(F.grad), n(cam.grad)
    return SimpleNamespace(sV_paths=(np.abs(n(V.grad)) + np.abs(n(Vw.grad))).sum(0), pV=pV, pF=pF, pcam=pcam, dV=pV.sum(0), dF=pF.sum(0), dcam=pcam.sum(0), sV=np.abs(pV).sum(0),
                           sF=np.abs(pF).sum(0), scam=np.abs(pcam).sum(0), dmeans=n(Pr["means3D"].grad), image=n(img),
                           depth=n(depth))


def rigid_identity(view, proj, dmeans_sum, dcam, dV, dF):
    """Both sides of the rigid-motion identity: moving every Gaussian and the camera position by the same vector is the same as
    changing the translation rows of the two matrices, so with Pm = V^-1 F
        sum_i dL/dmeans3D_i + dL/dcampos = V[:3,:3] . (dV + dF Pm^T)[3,:3].
    Takes absolute values as well (scales): -> (lhs [3], rhs [3])."""
    V, F = np.asarray(view, np.float64), np.asarray(proj, np.float64)
    Pm = np.linalg.inv(V) @ F
    return (np.asarray(dmeans_sum, np.float64) + np.asarray(dcam, np.float64),
            V[:3, :3] @ (np.asarray(dV, np.float64) + np.asarray(dF, np.float64) @ Pm.T)[3, :3])


def identity_scale(view, proj, ref):
    """The abs-sum scale of the identity's residual lhs - rhs: every per-Gaussian term of either side, in absolute value."""
    V, F = np.asarray(view, np.float64), np.asarray(proj, np.float64)
    Pm = np.linalg.inv(V) @ F
    return np.abs(ref.dmeans).sum(0) + ref.scam + np.abs(V[:3, :3]) @ (ref.sV + ref.sF @ np.abs(Pm).T)[3, :3]


@functools.lru_cache(maxsize=None)
def case(name):
    """The scenes the camera tests share, each with its oracle forward and its float64 reference, computed once:
    "deg3" (seed 3, spread 0.45: clamped Gaussians), "deg1" (seed 4, SH degree 1), "near" (spread 0.12: all visible, none
    clamped).  -> (scene, oracle forward, dL/dpixel, reference)."""
    s = {"deg3": lambda: scene(3, 3), "deg1": lambda: scene(4, 1), "near": lambda: scene(3, 3, spread=0.12)}[name]()
    f = util.oracle_forward(s)
    dpix = seeded_dpix(s.camera.image_height, s.camera.image_width)
    return s, f, dpix, camera_reference(s, f, dpix)
