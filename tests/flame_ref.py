"""The torch restatement of FLAME's linear blend skinning with FateAvatar's deltas, for a batch of one (flame/lbs.py:24-101 as
flame/FLAME.py:131-204 calls it): the reference of every comparison in tests/test_flame_host.py and tests/test_gpu_flame.py, and
the stock-PyTorch route of tools/train_synthetic.py --torch-flame.  It runs in whatever dtype and on whatever device its inputs
have (float64 for the ground truth, float32 on the CPU for the measured error bound), and it is differentiable."""
import torch

JOINTS, POSE_FEATURES = 5, 36


def _angle_and_generator(r: torch.Tensor):
    angle = (r + 1e-8).norm(dim=1, keepdim=True)
    d = r / angle
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    o = torch.zeros_like(x)
    return angle, torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=1).view(-1, 3, 3)


def rotation_offset(r: torch.Tensor) -> torch.Tensor:
    """R - I for r [J,3] WITHOUT the detour through I: sin K + 2 sin^2(angle / 2) K K, the same angle and direction as
    `rodrigues`.  In floating point 1 - cos(angle) loses every digit once cos rounds to 1 (float32: below 2.4e-4 rad) and
    (I + x) - I rounds x to the spacing of 1; this form keeps full relative precision at any angle."""
    angle, K = _angle_and_generator(r)
    return torch.sin(angle)[:, :, None] * K + (2 * torch.sin(angle / 2) ** 2)[:, :, None] * (K @ K)


def rodrigues(r: torch.Tensor, stable_rotation: bool = False) -> torch.Tensor:
    """batch_rodrigues (flame/lbs.py:238-269) for r [J,3]: angle = |r + 1e-8|, direction = r / angle, R = I + sin K + (1 - cos) K K;
    `stable_rotation`: I + rotation_offset(r), the same matrix in exact arithmetic."""
    eye = torch.eye(3, dtype=r.dtype, device=r.device)
    if stable_rotation:
        return eye + rotation_offset(r)
    angle, K = _angle_and_generator(r)
    return eye + torch.sin(angle)[:, :, None] * K + (1 - torch.cos(angle))[:, :, None] * (K @ K)


def rigid_chain(R: torch.Tensor, joints: torch.Tensor, parents) -> torch.Tensor:
    """batch_rigid_transform (flame/lbs.py:285-342): A [J,4,4] — the chain of (R_j, joint_j - joint_parent), then every
    transform's translation minus its rotation applied to the joint's rest position."""
    G = []
    for j in range(R.shape[0]):
        rel = joints[j] if j == 0 else joints[j] - joints[int(parents[j])]
        T = torch.cat([torch.cat([R[j], rel[:, None]], dim=1),
                       torch.tensor([[0, 0, 0, 1]], dtype=R.dtype, device=R.device)], dim=0)
        G.append(T if j == 0 else G[int(parents[j])] @ T)
    G = torch.stack(G)
    shift = torch.zeros_like(G)
    shift[:, :3, 3] = (G[:, :3, :3] @ joints[:, :, None])[:, :, 0]
    return G - shift


def lbs(expression, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, n_shape,
        delta_shapedirs=None, delta_posedirs=None, delta_vertex=None, stable_rotation=False):
    """`(verts [V,3], pose_feature [36], A [5,4,4])` of FLAME.forward_with_delta_blendshape (None deltas: FLAME.forward).
    `stable_rotation` (default off: the reference's own form): R and the pose feature from `rotation_offset`."""
    S = shapedirs if delta_shapedirs is None else shapedirs + delta_shapedirs
    P = posedirs if delta_posedirs is None else posedirs + delta_posedirs
    vt = v_template if delta_vertex is None else v_template + delta_vertex
    betas = torch.cat([torch.zeros(n_shape, dtype=expression.dtype, device=expression.device), expression])
    v_shaped = vt + S @ betas
    joints = J_regressor @ v_shaped
    if stable_rotation:
        D = rotation_offset(pose.view(-1, 3))
        R, phi = torch.eye(3, dtype=D.dtype, device=D.device) + D, D[1:].reshape(-1)
    else:
        R = rodrigues(pose.view(-1, 3))
        phi = (R[1:] - torch.eye(3, dtype=R.dtype, device=R.device)).reshape(-1)
    v_posed = v_shaped + (phi @ P).view(-1, 3)
    A = rigid_chain(R, joints, parents)
    T = (lbs_weights @ A.view(A.shape[0], 16)).view(-1, 4, 4)
    verts = (T[:, :3, :3] @ v_posed[:, :, None])[:, :, 0] + T[:, :3, 3]
    return verts, phi, A


def random_model(V, n_shape, n_exp, seed, dtype=torch.float32):
    """A seeded FLAME-shaped model with parents (-1, 0, 1, 1, 1) and its inputs — random tables of FLAME's magnitudes (a head of
    0.2 m, directions of millimetres, rows of the regressor and of the skinning weights that sum to 1), non-zero deltas, an
    expression of unit scale and rotations of a few tenths of a radian.  A dict of CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)  # noqa: E731
    L = n_shape + n_exp
    Jr = torch.rand(JOINTS, V, generator=g, dtype=torch.float64)
    W = torch.rand(V, JOINTS, generator=g, dtype=torch.float64) + 0.05
    m = dict(v_template=0.1 * rn(V, 3), shapedirs=0.004 * rn(V, 3, L), posedirs=0.002 * rn(POSE_FEATURES, 3 * V),
             J_regressor=Jr / Jr.sum(1, keepdim=True), lbs_weights=W / W.sum(1, keepdim=True),
             delta_shapedirs=0.001 * rn(V, 3, L), delta_posedirs=0.0005 * rn(POSE_FEATURES, 3 * V), delta_vertex=0.002 * rn(V, 3),
             expression=rn(n_exp), pose=0.3 * rn(3 * JOINTS), g=rn(V, 3))
    m = {k: v.to(dtype) for k, v in m.items()}
    m["parents"] = torch.tensor([-1, 0, 1, 1, 1])
    m["n_shape"], m["n_exp"] = n_shape, n_exp
    return m


def run(m, dtype, with_deltas=True, stable_rotation=False):
    """Forward and backward of `lbs` on the model dict `m` in `dtype` for dLoss/dverts = m['g']: a dict with `verts`,
    `pose_feature`, `A` and the gradients `d_delta_shapedirs`, `d_delta_posedirs`, `d_delta_vertex`, `d_expression`, `d_pose`."""
    c = lambda k: m[k].detach().to(dtype)  # noqa: E731
    leaf = lambda k: c(k).clone().requires_grad_(True)  # noqa: E731
    e, p = leaf("expression"), leaf("pose")
    dS, dP, dV = (leaf(k) if with_deltas else None for k in ("delta_shapedirs", "delta_posedirs", "delta_vertex"))
    verts, phi, A = lbs(e, p, c("v_template"), c("shapedirs"), c("posedirs"), c("J_regressor"), m["parents"], c("lbs_weights"),
                        m["n_shape"], dS, dP, dV, stable_rotation=stable_rotation)
    verts.backward(c("g"))
    out = dict(verts=verts.detach(), pose_feature=phi.detach(), A=A.detach(), d_expression=e.grad, d_pose=p.grad)
    if with_deltas:
        out.update(d_delta_shapedirs=dS.grad, d_delta_posedirs=dP.grad, d_delta_vertex=dV.grad)
    return out
