"""Torch restatements (any dtype, CPU) of what csrc/fr_bake.hip computes, for tests/test_bake_host.py and the GPU tests.

decode: `UVDecoder._gather_attribute` (model/uv_decoder.py:85-107) on the slices of :225-245 — the activations of :133-174
(`rotation_activation` is fateavatar_amd.texture's restatement of :158-174, pinned by tests/test_texture_host.py) and
F.grid_sample(.., "bilinear", "border", align_corners=True) (:179-202).
rot term: train/loss.py:612-617 on pytorch3d 0.7.7's quaternion_to_axis_angle (transforms/rotation_conversions.py), by its
formula: pytorch3d is not installed where this project is developed."""
import torch

from fateavatar_amd.texture import SH_C0, TEXTURE_CHANNELS, rotation_activation

NAMES = tuple(n for n, _ in TEXTURE_CHANNELS)
WIDTHS = {"color": 3, "opacity": 1, "scaling": 3, "rotation": 4, "offset": 1}


def slices(tex_out):
    """{name: [1,C,H,W]} of a [1,11,H,W] decoder output."""
    out, off = {}, 0
    for name, c in TEXTURE_CHANNELS:
        out[name] = tex_out[:, off:off + c]
        off += c
    return out


def activate(name, t, mean_scaling, max_scaling):
    if name == "color":
        return torch.tanh(t) * (0.5 / SH_C0)
    if name == "offset":
        return torch.tanh(t)
    if name == "scaling":
        return max_scaling - torch.nn.functional.softplus(-(t + mean_scaling) + max_scaling)
    if name == "rotation":
        return rotation_activation(t)
    return t


def decode(tex_out, uv, mean_scaling, max_scaling):
    """{name: [N,C]} in `tex_out`'s dtype: activate every slice, then grid_sample it at 2 uv - 1."""
    grid = (2 * uv.to(tex_out.dtype) - 1)[None, None]                          # [1,1,N,2]
    out = {}
    for name, t in slices(tex_out).items():
        o = torch.nn.functional.grid_sample(activate(name, t, mean_scaling, max_scaling), grid, mode="bilinear",
                                            padding_mode="border", align_corners=True)
        out[name] = o[0, :, 0, :].t()
    return out


def decode_with_grad(tex_out, uv, mean_scaling, max_scaling, d_values, dtype):
    """({name: [N,C]}, d_tex_out [1,11,H,W]) in `dtype`: `decode` and its autograd for the upstream gradients `d_values`."""
    x = tex_out.detach().to(dtype).requires_grad_(True)
    vals = decode(x, uv, mean_scaling, max_scaling)
    torch.autograd.backward([vals[n] for n in NAMES], [d_values[n].to(dtype) for n in NAMES])
    return {n: v.detach() for n, v in vals.items()}, x.grad


def quaternion_to_axis_angle(q):
    """pytorch3d 0.7.7, on rows whose element 0 is taken for the real part.  A row that is zero everywhere has atan2(0, 0):
    its real part is replaced by the constant 1 in front of atan2 (the same half angle, 0, and no 0 / 0 in autograd), so
    that row gets gradient 0 like every other row whose vector part is 0 (autograd's rule for the norm)."""
    v, w = q[..., 1:], q[..., :1]
    n = torch.linalg.vector_norm(v, dim=-1, keepdim=True)
    w = torch.where((n == 0) & (w == 0), torch.ones_like(w), w)
    half = torch.atan2(n, w)
    ang = 2 * half
    small = ang.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(ang), ang)
    s = torch.where(small, 0.5 - (ang * ang) / 48, torch.sin(half) / safe)
    return v / s


def rot_loss(rotation):
    """train/loss.py:612-617: mean(raw[:,0]^2) + mean(raw[:,2]^2), raw = quaternion_to_axis_angle(rotation)."""
    raw = quaternion_to_axis_angle(rotation)
    return torch.mean(raw[..., 0] ** 2) + torch.mean(raw[..., 2] ** 2)


def rot_loss_and_grad(rotation, dtype):
    r = rotation.detach().to(dtype).requires_grad_(True)
    loss = rot_loss(r)
    loss.backward()
    return loss.detach(), r.grad
