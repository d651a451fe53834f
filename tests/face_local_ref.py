"""TEST HELPER — GaussianAvatars' face-local binding restated in stock PyTorch (any dtype, any device): the reference of
every face-local test.

reference: model/baseline/gaussianavatars.py:144-171 —
    xyz      = (R_f . local_xyz) * s_f + c_f
    rotation = quaternion_multiply(F.normalize(matrix_to_quaternion(R_f)), rotation)
    scaling  = scaling + log(s_f)
with R, s = compute_face_orientation(verts, faces, return_scale=True) and c the mean of the face's three vertices.  The
building blocks are oracle/binding.py's, pinned bit-exactly to the reference's mesh_compute by tests/golden/golden_binding.npz.

One of them is restated here for its BACKWARD: oracle.binding.matrix_to_quaternion takes pytorch3d's `_sqrt_positive_part` as
where(x > 0, sqrt(clamp(x, 0)), 0), whose autograd is NaN wherever x <= 0 (0 * inf) — and the posed head template has
faces turned by exactly half a turn about an axis, x == 0.  pytorch3d itself (0.7.7, rotation_conversions.py) assigns the
square roots through the positive mask, which gives those entries a zero gradient; `matrix_to_quaternion` below does the
same.  Its forward is oracle.binding's, bit for bit (tests/test_face_local_host.py holds it to that)."""
import torch

from oracle import binding as B


def _sqrt_positive_part(x):
    """pytorch3d 0.7.7: sqrt(max(0, x)) with a zero subgradient where x <= 0."""
    ret = torch.zeros_like(x)
    positive = x > 0
    ret[positive] = torch.sqrt(x[positive])
    return ret


def matrix_to_quaternion(m):
    """oracle.binding.matrix_to_quaternion with pytorch3d's own `_sqrt_positive_part`."""
    m00, m01, m02 = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    m10, m11, m12 = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    m20, m21, m22 = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                             1.0 - m00 - m11 + m22], dim=-1))
    by_rijk = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    cand = by_rijk / (2.0 * torch.clamp(q_abs[..., None], min=0.1))
    sel = q_abs.argmax(dim=-1)
    out = torch.gather(cand, -2, sel[..., None, None].expand(*sel.shape, 1, 4)).squeeze(-2)
    return B.standardize_quaternion(out)


def face_local_bind(verts, faces, binding, local_xyz, rotation, scaling):
    """verts [V,3]; faces [F,3]; binding [N] (face of every Gaussian); local_xyz [N,3]; rotation [N,4]; scaling [N,3].
    Returns (xyz [N,3], rotation [N,4], scaling [N,3])."""
    orien, fscale = B.face_orientation(verts, faces)                                   # :149
    centre = verts[faces.long()].mean(dim=-2)                                          # :144-146
    fi = binding.long()
    quat = torch.nn.functional.normalize(matrix_to_quaternion(orien)[fi])              # :154-155
    out_scaling = scaling + torch.log(fscale[fi])                                      # :169
    out_rotation = B.quaternion_multiply(quat, rotation)                               # :170
    xyz = torch.bmm(orien[fi], local_xyz[..., None]).squeeze(-1) * fscale[fi] + centre[fi]   # :171
    return xyz, out_rotation, out_scaling


def quaternion_candidates(verts, faces):
    """Which of matrix_to_quaternion's four candidates every face selects: [F] int64."""
    m, _ = B.face_orientation(verts, faces)
    x = torch.stack([1.0 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], 1.0 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2],
                     1.0 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], 1.0 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], dim=-1)
    return x.argmax(dim=-1)
