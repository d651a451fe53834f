"""What neural baking's kernels cost: the two decode launches (`texture.decode_attributes`: fr_bake_decode,
fr_bake_decode_backward) and the rot term (`loss.rot_term_and_grad`: fr_rot_term), csrc/fr_bake.hip.

    python tools/bake_cost.py [--iters 200] [--rounds 5] [--out profiles/r32_bake_kernels.json]

At the reference's layout — 131 072 points (`uv_of_binding` of the template's UV raster, sampling seeds 0 and 1), a
[1,11,512,512] decoder output, float32 —: the time per call of
    decode_forward / decode_backward   the fused launches on preallocated buffers (the backward: ONE walk per texel),
    gather_forward / gather_backward   `gather_attributes` — `rotation_activation` in torch on the map, then
                                       fr_texture_lookup; its autograd backward: fr_texture_lookup_backward (one walk per layer),
                                       the slice gradients added up, and the activation's dozen autograd kernels,
    rot_fused / rot_torch              the rot term with its gradient against the three torch lines of train/loss.py:612-617 on
                                       tests/bake_ref.py's quaternion_to_axis_angle with their backward (needs the checkout's
                                       tests/ next to tools/),
measured as tools/pixel_loss_cost.py measures the sibling terms — back-to-back calls on one stream between two device events,
the variants alternated round by round, and the fused variants also as twenty calls captured into one graph (a replay's time
/ 20: what a captured step pays) — with that file's helpers.  A run without a GPU fails."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
os.environ.setdefault("FR_TUNE_RUNTIME", "1")

from pixel_loss_cost import GRAPH_CALLS, _alternate, _graphed, _median, _row  # noqa: E402

MEAN_S, MAX_S = -5.0, -4.5


def measure(iters, rounds):
    import torch
    from fateavatar_amd import _lib, mesh_sampling, scenes, texture
    from fateavatar_amd.loss import rot_term_and_grad, rot_term_workspace
    from tests import bake_ref
    dev = torch.device("cuda:0")
    lay = scenes.head_uv()
    uvs = []
    for seed in (0, 1):
        fi, bc = mesh_sampling.uniform_sampling_barycoords(65536, lay[0], lay[1], rng=np.random.default_rng(seed))
        uvs.append(texture.uv_of_binding(fi, bc))
    uv = torch.cat(uvs).to(dev)
    N, S = uv.shape[0], 512
    plan = texture.TexturePlan(uv, S, S)
    row_start, entries = plan.csr()
    gen = torch.Generator().manual_seed(2024)
    tex = (torch.rand(1, 11, S, S, generator=gen) * 2 - 1).to(dev)
    widths = dict(bake_ref.WIDTHS)
    vals = {n: torch.empty(N, w, device=dev) for n, w in widths.items()}
    d_vals = {n: (torch.rand(N, w, generator=gen) * 2 - 1).to(dev) for n, w in widths.items()}
    d_tex = torch.empty_like(tex)
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    L = _lib.lib()

    def decode_forward():
        _lib.check(L.fr_bake_decode(N, uv.data_ptr(), S, S, tex.data_ptr(), MEAN_S, MAX_S, *[vals[n].data_ptr() for n in bake_ref.NAMES],
                                    stream()), "fr_bake_decode")

    def decode_backward():
        _lib.check(L.fr_bake_decode_backward(N, uv.data_ptr(), S, S, row_start.data_ptr(), entries.data_ptr(), tex.data_ptr(), MEAN_S,
                                             MAX_S, *[d_vals[n].data_ptr() for n in bake_ref.NAMES], d_tex.data_ptr(), stream()),
                   "fr_bake_decode_backward")

    leaf = tex.clone().requires_grad_(True)
    kept = {}

    def gather_forward():
        kept["v"] = texture.gather_attributes(leaf, plan, MEAN_S, MAX_S)[1]

    def gather_backward():      # (on the graph the last gather_forward left: retained, so the block times the backward alone)
        leaf.grad = None
        torch.autograd.backward([kept["v"][n] for n in bake_ref.NAMES], [d_vals[n] for n in bake_ref.NAMES], retain_graph=True)

    decode_forward()
    rot = vals["rotation"]
    d_rot, l1, ws = torch.zeros(N, 4, device=dev), torch.zeros(1, device=dev), rot_term_workspace(dev)

    def rot_torch():
        r = rot.detach().requires_grad_()
        loss = bake_ref.rot_loss(r)
        (g,) = torch.autograd.grad(0.1 * loss, r)
        return loss, g

    run = {"decode_forward": decode_forward, "gather_forward": gather_forward, "decode_backward": decode_backward,
           "gather_backward": gather_backward, "rot_fused": lambda: rot_term_and_grad(rot, d_rot, out=l1, weight=0.1, workspace=ws),
           "rot_torch": rot_torch}
    gather_forward()
    n_it = {k: iters if k in ("decode_forward", "decode_backward", "rot_fused") else max(10, iters // 10) for k in run}
    us = _alternate(run, n_it, rounds)
    fused = ("decode_forward", "decode_backward", "rot_fused")
    replay = {k: _graphed(run[k]) for k in fused}
    us_dev = {k: [t / GRAPH_CALLS for t in v] for k, v in _alternate(replay, {k: iters for k in replay}, rounds).items()}
    torch.cuda.synchronize()
    med = {k: _median(v) for k, v in us.items()}
    longest = int((row_start[1:] - row_start[:-1]).max())
    return dict(points=N, texture=[11, S, S], entries=int(entries.numel()), longest_list=longest, calls_per_round=n_it,
                us_per_call=_row(us), us_per_call_in_a_graph=_row(us_dev),
                gather_over_decode_forward=round(med["gather_forward"] / med["decode_forward"], 2),
                gather_over_decode_backward=round(med["gather_backward"] / med["decode_backward"], 2),
                rot_torch_over_fused=round(med["rot_torch"] / med["rot_fused"], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bake_cost: needs a GPU (nothing here is measured without one)")
    doc = dict(what="neural baking's kernels: time per call of fr_bake_decode / fr_bake_decode_backward against gather_attributes forward / "
                    "backward, and of fr_rot_term against its float32 torch restatement with backward (device events around "
                    "back-to-back calls, alternated round by round)",
               device=torch.cuda.get_device_name(0), bake_kernels=measure(a.iters, a.rounds))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
