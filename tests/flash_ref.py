"""FlashAvatar's per-frame arithmetic restated in plain torch, any dtype, any device: what the MLP-deformed binding
(FR_BIND_DEFORM) and the Huber launch are tested against.

reference: model/baseline/flashavatar.py:242-276 (`forward`), :380-390 (`quatProduct_batch`), train/loss.py:217-221, :231-239
(`get_huber_loss`, the mouth term).  Written from the arithmetic, not from the reference's program text;
tests/test_flash_host.py pins it by hand cases, by gradcheck and by the written backward formulas, and
tests/test_reference_runs_host.py pins `huber_loss` and `quat_product` to recorded runs of the reference's own
`FlashAvatarLoss.accumulate_gradients` and `FlashAvatar.quatProduct_batch` (tests/golden/reference_image_terms.npz cases
`huber_plain` / `huber_mouth`, tests/golden/reference_mlp*.npz case `quat`; the module imports with stand-ins for pytorch3d).
`deform_bind` stays builder-pinned: `forward` runs the CUDA rasterizer."""
import torch

ALPHA, MASK_WEIGHT = 0.1, 40.0


def quat_product(q1, q2):
    """The Hamilton product q1 (x) q2 of [N,4] quaternions (r, x, y, z), sign kept:
    r = r1 r2 - v1 . v2,  v = r1 v2 + r2 v1 + v1 x v2."""
    r1, v1, r2, v2 = q1[:, :1], q1[:, 1:], q2[:, :1], q2[:, 1:]
    r = r1 * r2 - (v1 * v2).sum(dim=1, keepdim=True)
    v = r1 * v2 + r2 * v1 + torch.linalg.cross(v1, v2, dim=1)
    return torch.cat([r, v], dim=1)


def deform_bind(verts, faces, face_index, bary, deform, rotation, scaling):
    """(xyz [N,3], rotation [N,4], scaling [N,3]) of one frame: t = tanh(deform) of the MLP's ten RAW outputs,
    xyz = barycentric point + t[0:3];  rotation = rotation (x) (exp(t[3]), t[4:7]);  scaling = scaling * exp(t[7:10])."""
    t = torch.tanh(deform)
    tri = verts[faces.long()[face_index.long()]]                        # [N,3,3]
    xyz = (tri * bary.unsqueeze(-1)).sum(dim=1) + t[:, 0:3]
    delta = torch.cat([torch.exp(t[:, 3:4]), t[:, 4:7]], dim=1)
    return xyz, quat_product(rotation, delta), scaling * torch.exp(t[:, 7:10])


def huber(x, alpha=ALPHA):
    """h(x) = 0.5 x^2 if |x| < alpha else alpha (|x| - 0.5 alpha), elementwise."""
    ax = x.abs()
    return torch.where(ax < alpha, 0.5 * x * x, alpha * (ax - 0.5 * alpha))


def huber_loss(img, gt, mask=None, alpha=ALPHA, mask_weight=MASK_WEIGHT):
    """(huber + mask_weight * mouth, huber, mouth) of [C,H,W] images; `mask` [1,H,W] or [H,W] with values in [0,1], broadcast
    over the channels; without one, mouth is 0."""
    d = img - gt
    h = huber(d, alpha).mean()
    m = huber(mask.reshape(1, *d.shape[-2:]) * d, alpha).mean() if mask is not None else torch.zeros((), dtype=d.dtype, device=d.device)
    return h + mask_weight * m, h, m
