"""MonoGaussianAvatar's per-point arithmetic restated in plain torch (any dtype, any device): the yardstick of
fateavatar_amd/mono.py's fused calls.  Written from the arithmetic of include/fr_rasterizer.h (fr_point_lbs, fr_nearest_vertex,
fr_lbs_terms), with torch.inverse and einsums where the kernels have closed forms; differentiable by autograd.
Pinned to the reference's own Python by tests/test_reference_runs_host.py: `deform_points` (with its seven gradients, the frame's
pose state included) to recorded runs of `FLAME.forward_pts` over flame/lbs.py's `inverse_pts` / `forward_pts`
(tests/golden/reference_skinning.npz), `lbs_terms` times `fateavatar_amd.mono.reference_lbs_weights` to
`MonoGaussianAvatarLoss.accumulate_gradients` with and without a `var_expression` (tests/golden/reference_mono_terms*.npz).
`nearest_vertex` stays builder-pinned (pytorch3d's knn_points is absent)."""
from __future__ import annotations

import math

import torch


def deform_points(points, shapedirs, posedirs, weights, canonical, frame):
    """points [N,3], shapedirs [N,3,E], posedirs [N,36,3], weights [N,J]; a pose state is (betas [E], pose_feature [36],
    transforms [J,4,4] or [J,16]).  -> xyz [N,3].
        T_c = sum_j w_j A^c_j      z = T_c^-1 (p, 1)
        x   = z[:3] - S beta_c - P^T phi_c + S beta + P^T phi
        xyz = (sum_j w_j A_j (x, 1))[:3]                (no division by the homogeneous coordinate)"""
    beta_c, phi_c, A_c = canonical
    beta, phi, A = frame
    J = weights.shape[1]
    A_c, A = A_c.reshape(J, 4, 4), A.reshape(J, 4, 4)
    one = torch.ones_like(points[:, :1])
    T_c = torch.einsum("nj,jab->nab", weights, A_c)
    z = torch.einsum("nab,nb->na", torch.inverse(T_c), torch.cat([points, one], 1))
    x = z[:, :3] - torch.einsum("nkl,l->nk", shapedirs, beta_c) - torch.einsum("nik,i->nk", posedirs, phi_c) \
        + torch.einsum("nkl,l->nk", shapedirs, beta) + torch.einsum("nik,i->nk", posedirs, phi)
    T = torch.einsum("nj,jab->nab", weights, A)
    return torch.einsum("nab,nb->na", T, torch.cat([x, one], 1))[:, :3]


def deform_points_backward(points, shapedirs, posedirs, weights, canonical, frame, g):
    """The WRITTEN backward (the sketch of the design): (d_points, d_shapedirs, d_posedirs, d_weights) for dL/dxyz = g."""
    beta_c, phi_c, A_c = canonical
    beta, phi, A = frame
    J = weights.shape[1]
    A_c, A = A_c.reshape(J, 4, 4), A.reshape(J, 4, 4)
    one = torch.ones_like(points[:, :1])
    T_c = torch.einsum("nj,jab->nab", weights, A_c)
    Ti = torch.inverse(T_c)
    z = torch.einsum("nab,nb->na", Ti, torch.cat([points, one], 1))
    x = z[:, :3] + torch.einsum("nkl,l->nk", shapedirs, beta - beta_c) + torch.einsum("nik,i->nk", posedirs, phi - phi_c)
    T = torch.einsum("nj,jab->nab", weights, A)
    d_x = torch.einsum("nab,na->nb", T[:, :3, :3], g)                              # T3^T g
    d_S = d_x[:, :, None] * (beta - beta_c)[None, None, :]
    d_P = (phi - phi_c)[None, :, None] * d_x[:, None, :]
    u = torch.einsum("nab,na->nb", Ti, torch.cat([d_x, torch.zeros_like(one)], 1))  # T_c^-T (d_x, 0)
    y = torch.einsum("jab,nb->nja", A, torch.cat([x, one], 1))[:, :, :3]            # A_j (x, 1)
    d_w = torch.einsum("na,nja->nj", g, y) - torch.einsum("na,jab,nb->nj", u, A_c, z)
    return u[:, :3], d_S, d_P, d_w


def nearest_vertex(points, verts, chunk: int = 1024):
    """(index int64 [N], dist2 [N]): the vertex with the smallest (dx*dx + dy*dy) + dz*dz, d = point - vertex, evaluated in the
    tensors' dtype in exactly this order; ties go to the lowest index."""
    idx, d2 = [], []
    for s in range(0, points.shape[0], chunk):
        p = points[s:s + chunk]
        dx, dy, dz = (p[:, None, k] - verts[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        best = d.min(dim=1).values
        first = (d == best[:, None]).to(torch.int8).argmax(dim=1)      # the first (lowest) index that attains the minimum
        idx.append(first), d2.append(best)
    return torch.cat(idx), torch.cat(d2)


def lbs_terms(index, weights, posedirs, shapedirs, gt_weights, gt_posedirs, gt_shapedirs):
    """The three plain mean squared errors (weights, posedirs, shapedirs) against the tables' rows `index`: a 3-vector."""
    i = index.long()
    return torch.stack([((weights - gt_weights[i]) ** 2).mean(), ((posedirs - gt_posedirs[i]) ** 2).mean(),
                        ((shapedirs - gt_shapedirs[i]) ** 2).mean()])


def rodrigues(r):
    """Axis-angle [J,3] -> rotation matrices [J,3,3]."""
    th = r.norm(dim=1).clamp_min(1e-12)
    k = r / th[:, None]
    K = torch.zeros((r.shape[0], 3, 3), dtype=r.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    I = torch.eye(3, dtype=r.dtype)[None]
    return I + torch.sin(th)[:, None, None] * K + (1 - torch.cos(th))[:, None, None] * (K @ K)


def rigid_bones(J, angle_scale, gen, dtype=torch.float64):
    """[J,4,4] rigid transforms: axis-angle angle_scale * N(0,1), translation 0.1 * N(0,1); bone 0 the identity."""
    R = rodrigues(angle_scale * torch.randn((J, 3), generator=gen, dtype=torch.float64))
    A = torch.zeros((J, 4, 4), dtype=torch.float64)
    A[:, :3, :3], A[:, :3, 3], A[:, 3, 3] = R, 0.1 * torch.randn((J, 3), generator=gen, dtype=torch.float64), 1.0
    A[0] = torch.eye(4, dtype=torch.float64)
    return A.to(dtype)


def recipe(N, E, J, seed=0):
    """The test inputs, float64 on the CPU: points 0.3 N(0,1), bases 0.01 N(0,1), weights softmax(2 N(0,1)) with the first rows
    one-hot, one block scaled so that its sums lie in [0.5, 2] and (J > 1) rows without bone 0; rigid bones from axis-angle 0.2 N(0,1)
    (canonical) and 0.6 N(0,1) (frame), bone 0 the identity.  -> (points, shapedirs, posedirs, weights, canonical, frame, g).
    J = 1 (bone 0 alone, the identity): no row can go without bone 0, and the points are 0.05 N(0,1) — there xyz = p + w o with
    o the blendshape offset (about 0.03), and d xyz / d w = o is what two terms of the size of p leave: with points of 0.3 a
    row of that gradient misses float64 by 4e-6 in float32 plain torch already, which measures the inputs and no kernel."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)  # noqa: E731
    points, S, P = (0.3 if J > 1 else 0.05) * rn(N, 3), 0.01 * rn(N, 3, E), 0.01 * rn(N, 36, 3)
    w = torch.softmax(2 * rn(N, J), dim=1)
    n1 = min(J, N)                                   # one-hot rows, one per bone
    w[:n1] = torch.eye(J, dtype=torch.float64)[:n1]
    a, b = min(N, 8), min(N, 24)                     # a block whose sums lie in [0.5, 2]
    if b > a:
        w[a:b] *= torch.exp(math.log(2.0) * (2 * torch.rand((b - a, 1), generator=gen, dtype=torch.float64) - 1)) \
            .clamp(0.5, 2.0)
    c, d = min(N, 24), min(N, 40)                    # rows without bone 0 (J = 1: there is no other bone to carry the row)
    if d > c and J > 1:
        w[c:d, 0] = 0.0
        w[c:d] /= w[c:d].sum(1, keepdim=True)
    canonical = (rn(E), rn(36) * 0.3, rigid_bones(J, 0.2, gen))
    frame = (rn(E), rn(36) * 0.3, rigid_bones(J, 0.6, gen))
    return points, S, P, w, canonical, frame, rn(N, 3)


def deform_points_closed_form(points, shapedirs, posedirs, weights, canonical, frame, g):
    """The kernels' arithmetic (fateavatar_amd/csrc/fr_point_lbs.hip) transcribed: with T_c = [[R, t], [0, s]], s = sum_j w_j,
        z3 = R^-1 (p - t / s), z4 = 1 / s;  u3 = R^-T d_x, u4 = -(t . u3) / s;  d_w_j = g . (R_j x + t_j) - (u3 . (R^c_j z3 + t^c_j z4) + u4 z4)
    with a cofactor inverse of the 3x3 block.  -> (xyz, d_points, d_shapedirs, d_posedirs, d_weights)."""
    beta_c, phi_c, A_c = canonical
    beta, phi, A = frame
    J = weights.shape[1]
    A_c, A = A_c.reshape(J, 4, 4), A.reshape(J, 4, 4)
    Tc = torch.einsum("nj,jab->nab", weights, A_c[:, :3, :])
    T = torch.einsum("nj,jab->nab", weights, A[:, :3, :])
    s = weights.sum(1, keepdim=True)
    R, t = Tc[:, :, :3], Tc[:, :, 3]
    cof = torch.stack([torch.linalg.cross(R[:, 1], R[:, 2]), torch.linalg.cross(R[:, 2], R[:, 0]),
                       torch.linalg.cross(R[:, 0], R[:, 1])], dim=2)          # columns of adj(R) ...
    Ri = cof / (R[:, 0] * cof[:, :, 0]).sum(1)[:, None, None]                 # ... over det R
    z3 = torch.einsum("nab,nb->na", Ri, points - t / s)
    z4 = 1.0 / s
    x = z3 + torch.einsum("nkl,l->nk", shapedirs, beta - beta_c) + torch.einsum("nik,i->nk", posedirs, phi - phi_c)
    xyz = torch.einsum("nab,nb->na", T[:, :, :3], x) + T[:, :, 3]
    d_x = torch.einsum("nab,na->nb", T[:, :, :3], g)
    d_S = d_x[:, :, None] * (beta - beta_c)[None, None, :]
    d_P = (phi - phi_c)[None, :, None] * d_x[:, None, :]
    u3 = torch.einsum("nab,na->nb", Ri, d_x)
    u4 = -(t * u3).sum(1, keepdim=True) / s
    y = torch.einsum("jab,nb->nja", A[:, :3, :3], x) + A[None, :, :3, 3]
    v = torch.einsum("jab,nb->nja", A_c[:, :3, :3], z3) + A_c[None, :, :3, 3] * z4[:, :, None]
    d_w = torch.einsum("na,nja->nj", g, y) - (torch.einsum("na,nja->nj", u3, v) + u4 * z4)
    return xyz, u3, d_S, d_P, d_w
