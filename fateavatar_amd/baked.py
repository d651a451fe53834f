"""The BAKED FateAvatar: Gaussians whose attributes are not parameters but are looked up from UV attribute maps every frame.

reference: model/uv_decoder.py — `UVDecoder._parsing_avatar_model` (:286-340: the prior attributes of a trained avatar, its
binding extended by the 65 536 template points of `_register_template_mesh` :43-83, the UV coordinates of all of them),
`UVDecoder.forward` (:387-542, the neural-baking training step: textures -> look-up -> bind -> render),
`render_from_texture_dict` (:564-690, what avatar_edit_baked.py and the GUI call per frame on an edited texture
dictionary) and `_export_avatar_model` (:342-385, baked textures back into a plain avatar).

What is native here: the look-up of all attribute maps is one HIP kernel per direction (`texture.texture_lookup`) and its
[N,C] outputs are what `render_bound_batch` takes as RAW parameters, so a baked frame is: rotation activation (torch, on the
texture) -> one look-up launch -> the rasterizer's launch chain with the binding inside its per-Gaussian kernels.  One look-up
serves all K views of a batch.  The baking trainer's step is `bake.BakeStep`, on this class; the U-Net / decoder that produces
the textures in training and the texture editor stay stock PyTorch.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .avatar import AvatarGaussians
from .bound import MeshBinding, render_bound_batch
from .texture import (TEXTURE_CHANNELS, TexturePlan, gather_attributes_from_texture_dict, uv_of_binding)

ATTRIBUTES = tuple(name for name, _ in TEXTURE_CHANNELS)   # colour, opacity, scaling, rotation, offset
TEMPLATE_POINTS = 256 * 256                                 # uv_decoder.py:52-56


class _BakedFrame:
    """What render_bound_batch() reads of a Gaussian holder, for one frame's looked-up (or prior) raw attributes."""
    max_sh_degree = 0            # uv_decoder.py:443, 617
    fused_activations = True
    fused_densification_stats = None

    def __init__(self, color, opacity, scaling, rotation, offset):
        self.get_features = color            # [N,1,3]: cat(features_dc, features_rest) with an empty rest (M = 1)
        self._opacity, self._scaling, self._rotation, self._offset = opacity, scaling, rotation, offset


class BakedAvatar:
    """`UVDecoder` without its network: the prior attributes of an `AvatarGaussians`, the (optionally extended) binding,
    the look-up plan of its UV coordinates and a texture dictionary."""

    def __init__(self, pc: AvatarGaussians, tex_size: int = 512, template_points: int = 0, texture_dict: Optional[dict] = None,
                 rng: Optional[np.random.Generator] = None):
        """`_parsing_avatar_model` (uv_decoder.py:286-340).  `template_points` > 0 appends that many points of the template's
        UV raster to the binding "for more dense distribution" (:303-308; the reference appends 65 536 = `TEMPLATE_POINTS`,
        sampled as `_register_template_mesh` does).  The PRIOR attributes keep the avatar's own P rows (:290-298), as in the
        reference: with an extended binding only the looked-up attributes have a row for every point, so every attribute
        has to be baked then.  `texture_dict`: {'color', 'opacity', 'scaling', 'rotation', 'offset'} -> [C,H,W] or
        [1,C,H,W] device tensors (rotation with 3 channels), kept as the default of `render` / `export`."""
        from . import mesh_sampling, scenes
        dev = pc.flat.device
        with torch.no_grad():
            self.prior = {"color": pc._features_dc.detach().clone(), "opacity": pc._opacity.detach().clone(),
                          "offset": pc._offset.detach().clone(),
                          "rotation": torch.nn.functional.normalize(pc._rotation.detach()),     # :295-296
                          "scaling": pc._scaling.detach().clone()}
            self.mean_scaling = float(self.prior["scaling"].mean().item())                      # :298-301
            self.std_scaling = float(self.prior["scaling"].std().item())
            self.max_scaling = self.mean_scaling + self.std_scaling
        self.P = pc.P
        face_index, bary = pc.face_index, pc.bary_coords
        if template_points:
            uv = scenes.head_uv()
            if uv is None:
                raise RuntimeError("the head template's UV layout is not in fateavatar_amd/data/head_template_geom.npz")
            fi, bc = mesh_sampling.uniform_sampling_barycoords(int(template_points), uv[0], uv[1], rng=rng)
            face_index = torch.cat([face_index, torch.from_numpy(fi).to(dev, torch.int32)]).contiguous()
            bary = torch.cat([bary, torch.from_numpy(bc).to(dev, torch.float32)]).contiguous()
        self.face_index, self.bary_coords = face_index, bary
        self.N = int(face_index.shape[0])
        self.tex_size = int(tex_size)
        self.plan = TexturePlan(uv_of_binding(face_index, bary), self.tex_size, self.tex_size)   # :310-325
        self.texture_dict = texture_dict

    def mesh_binding(self, faces, face_scale_canonical, shell_len: float, resize_scale: bool = True) -> MeshBinding:
        """The `MeshBinding` of this avatar's (extended) point set on a mesh topology."""
        return MeshBinding(faces, self.face_index, self.bary_coords, face_scale_canonical, float(shell_len), bool(resize_scale))

    def gather(self, texture_dict: Optional[dict] = None) -> dict:
        """{name: [N,C]} looked up from the dictionary (`_gather_attribute_from_texture_dict`, uv_decoder.py:109-131)."""
        texture_dict = self.texture_dict if texture_dict is None else texture_dict
        if texture_dict is None:
            raise RuntimeError("BakedAvatar: no texture dictionary")
        return gather_attributes_from_texture_dict(texture_dict, self.plan, self.mean_scaling, self.max_scaling)

    def _frame(self, values: dict, bake_attribute) -> _BakedFrame:
        """The attribute selection of uv_decoder.py:652-663: looked-up where baked, the prior elsewhere — and the looked-up
        opacity regardless of `bake_attribute` (:660)."""
        unknown = [a for a in bake_attribute if a not in ATTRIBUTES]
        if unknown:
            raise RuntimeError(f"BakedAvatar: unknown attributes {unknown}; known: {ATTRIBUTES}")
        chosen = {}
        for name in ("color", "scaling", "rotation", "offset"):
            if name in bake_attribute:
                if name not in values:
                    raise RuntimeError(f"BakedAvatar: '{name}' is to be baked but the texture dictionary has no '{name}'")
                chosen[name] = values[name]
            else:
                if self.N != self.P:
                    raise RuntimeError(f"BakedAvatar: the binding was extended to {self.N} points but the prior '{name}' has "
                                       f"{self.P} rows: bake every attribute")
                chosen[name] = self.prior[name]
        if "opacity" not in values:
            raise RuntimeError("BakedAvatar: the texture dictionary needs 'opacity' (the looked-up opacity is always used)")
        return _BakedFrame(chosen["color"].reshape(self.N, 1, 3), values["opacity"], chosen["scaling"], chosen["rotation"],
                           chosen["offset"])

    def render(self, cameras, posed_verts, binding: MeshBinding, bg, texture_dict: Optional[dict] = None,
               bake_attribute=("color", "opacity"), depth_alpha: bool = False, return_values: bool = False, slots=None):
        """`render_from_texture_dict` (uv_decoder.py:564-690) — and, with grad enabled, the look-up / bind / render part of
        `UVDecoder.forward` (:387-542): K views (cameras, posed vertex sets) of this avatar with its attributes looked up
        from `texture_dict` (default: the one given at construction).  `binding`: `mesh_binding(...)`.  Returns the list of
        render() dicts of `render_bound_batch`; with `return_values` also the dictionary of looked-up [N,C] tensors, the
        nodes of the autograd graph the frame was rendered from (for regularisers on the decoded values, :530-534).
        Gradients reach the textures through one gather launch; under torch.no_grad() the frame is forward-only."""
        if binding.face_index.shape[0] != self.N:
            raise RuntimeError(f"BakedAvatar.render: the binding has {binding.face_index.shape[0]} points, this avatar {self.N} "
                               "(use mesh_binding())")
        texture_dict = self.texture_dict if texture_dict is None else texture_dict
        if texture_dict is None:
            raise RuntimeError("BakedAvatar: no texture dictionary")
        needed = {"opacity", *bake_attribute}
        values = self.gather({n: t for n, t in texture_dict.items() if n in needed})
        outs = render_bound_batch(list(cameras), self._frame(values, tuple(bake_attribute)), posed_verts, binding, bg, slots=slots,
                                  depth_alpha=depth_alpha)
        return (outs, values) if return_values else outs

    @torch.no_grad()
    def export(self, texture_dict: Optional[dict] = None) -> AvatarGaussians:
        """`_export_avatar_model` (uv_decoder.py:342-385): a plain `AvatarGaussians` on the extended binding whose five
        parameters are the looked-up values of ALL five textures."""
        values = self.gather(texture_dict)
        missing = [a for a in ATTRIBUTES if a not in values]
        if missing:
            raise RuntimeError(f"BakedAvatar.export: the texture dictionary lacks {missing}")
        pc = AvatarGaussians(self.face_index.cpu().numpy(), self.bary_coords.cpu().numpy(), 0.0, self.plan.device)
        for field, name in (("_features_dc", "color"), ("_opacity", "opacity"), ("_offset", "offset"), ("_rotation", "rotation"),
                            ("_scaling", "scaling")):
            p = getattr(pc, field)
            p.copy_(values[name].reshape(p.shape))
        return pc
