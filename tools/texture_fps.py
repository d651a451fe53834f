"""The UV-texture look-up of a baked avatar against what a user has without it: the reference's own sequence in torch.

Workload ("the layout case"): the reference's UV layout — `uv_of_binding` of the template's UV raster, sampling seeds 0 and 1
concatenated, 131 072 points — on 512 x 512 textures, the five attribute maps of model/uv_decoder.py:225-245 (colour 3,
opacity 1, scaling 3, rotation 3 -> 4, offset 1 channel).
  (a) torch     the five activations (uv_decoder.py:133-174), five F.grid_sample(..., "bilinear", "border", align_corners=True)
                and the permute to [N,C] (:179-202); backward = their autograd (scatter with float atomics);
  (b) hip       `texture.gather_attributes`-style: rotation activation in torch, then ONE `texture_lookup` launch with the other
                activations inside; backward = one gather launch over the plan (+ torch's rotation-activation backward).
Four cells — forward alone and forward + backward, eager and replayed as a captured graph — with (a) and (b) ALTERNATED round
by round in one process; the figure of a cell is the median over the rounds of the mean time per call (rounds x calls >= 200).
  (c) frames    `BakedAvatar.render` under torch.no_grad() (all five attributes baked, one 512^2 view per call) against the
                torch look-up of (a) feeding `render_bound_batch`: frames/s.
`--trace-loop N`: only run N eager forward + backward calls of (b) and of (a) — the body of a
`rocprofv3 --kernel-trace --stats` run for the two kernels' durations.

    python tools/texture_fps.py [--calls 25] [--rounds 12] [--out profiles/r09_texture_lookup.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fateavatar_amd import mesh_sampling, rasterizer, scenes, texture  # noqa: E402

MEAN_S, MAX_S = -5.0, -4.5
NAMES = ("color", "opacity", "scaling", "rotation", "offset")
CHANNELS = dict(texture.TEXTURE_CHANNELS)


def layout_uv():
    lay = scenes.head_uv()
    uvs = []
    for seed in (0, 1):
        fi, bc = mesh_sampling.uniform_sampling_barycoords(65536, lay[0], lay[1], rng=np.random.default_rng(seed))
        uvs.append(texture.uv_of_binding(fi, bc))
    return torch.cat(uvs)


def torch_lookup(tex: dict, uv: torch.Tensor) -> dict:
    """(a): uv_decoder.py:85-107 in stock torch."""
    grid = (2 * uv - 1)[None, None]
    act = {"color": torch.tanh(tex["color"]) * (0.5 / texture.SH_C0), "opacity": tex["opacity"],
           "scaling": MAX_S - torch.nn.functional.softplus(-(tex["scaling"] + MEAN_S) + MAX_S),
           "rotation": texture.rotation_activation(tex["rotation"]), "offset": torch.tanh(tex["offset"])}
    out = {}
    for n in NAMES:
        o = torch.nn.functional.grid_sample(act[n], grid, mode="bilinear", padding_mode="border", align_corners=True)
        out[n] = o.permute(0, 2, 3, 1).squeeze(1)[0]            # [N,C], as the reference hands it on
    return out


def hip_lookup(tex: dict, plan: texture.TexturePlan) -> dict:
    """(b)."""
    t = dict(tex, rotation=texture.rotation_activation(tex["rotation"]))
    acts = {"color": texture.COLOR_ACTIVATION, "scaling": texture.scaling_activation(MEAN_S, MAX_S), "offset": texture.OFFSET_ACTIVATION}
    return texture.texture_lookup(t, plan, acts)


def make_cells(dev, uv):
    gen = torch.Generator().manual_seed(2024)
    plan = texture.TexturePlan(uv.to(dev), 512, 512)
    plan.csr()
    uv_d = plan.uv
    tex = {n: (torch.rand(1, CHANNELS[n], 512, 512, generator=gen) * 2 - 1).to(dev).requires_grad_(True) for n in NAMES}
    d_out = {n: (torch.rand(uv.shape[0], 4 if n == "rotation" else CHANNELS[n], generator=gen) * 2 - 1).to(dev) for n in NAMES}
    leaves, gouts = [tex[n] for n in NAMES], [d_out[n] for n in NAMES]

    def fwd(look):
        with torch.no_grad():
            return look()

    def fwd_bwd(look):
        out = look()
        return torch.autograd.grad([out[n] for n in NAMES], leaves, gouts)

    looks = {"torch": lambda: torch_lookup(tex, uv_d), "hip": lambda: hip_lookup(tex, plan)}
    cells = {}
    for side, look in looks.items():
        cells[("forward", side)] = lambda look=look: fwd(look)
        cells[("forward_backward", side)] = lambda look=look: fwd_bwd(look)
    return cells, looks, tex, plan


def graph_of(fn, dev):
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        keep = fn()
    torch.cuda.synchronize()

    def replay():
        with torch.cuda.stream(stream):
            g.replay()
    return g, replay, keep


def timed(fn, calls):
    """Mean seconds per call over `calls` calls that end in a device synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def alternate(pair: dict, calls, rounds, warmup=5):
    """{side: median over rounds of the mean time per call}, the sides alternated (and their order swapped) round by round."""
    for fn in pair.values():
        for _ in range(warmup):
            fn()
    t = {k: [] for k in pair}
    for r in range(rounds):
        for k in (list(pair) if r % 2 == 0 else list(pair)[::-1]):
            t[k].append(timed(pair[k], calls))
    return {k: statistics.median(v) for k, v in t.items()}, t


def baked_frames(dev, calls, rounds):
    """(c): no-grad frames of a baked avatar (65 536 + 65 536 template points, everything baked), 512^2, one view per call."""
    from fateavatar_amd import insta
    from fateavatar_amd.avatar import AvatarGaussians
    from fateavatar_amd.baked import ATTRIBUTES, BakedAvatar, _BakedFrame
    from fateavatar_amd.binding import face_scale
    from fateavatar_amd.bound import render_bound_batch
    from fateavatar_amd.model import TorchCamera
    transform, posed, faces = insta.synthetic_sequence(8, 512, 0)
    verts, _, _ = scenes.head_geometry()
    pc = AvatarGaussians.from_template(dev, uv_resolution=256)
    avatar = BakedAvatar(pc, tex_size=512, template_points=65536, rng=np.random.default_rng(1))
    gen = torch.Generator().manual_seed(7)
    tex = {n: (torch.rand(1, CHANNELS[n], 512, 512, generator=gen) * 2 - 1).to(dev) for n in NAMES}
    tex["scaling"] = tex["scaling"] * 0.3
    faces_t = torch.from_numpy(faces).to(dev)
    mb = avatar.mesh_binding(faces_t, face_scale(torch.from_numpy(verts).to(dev), faces_t), 0.05, True)
    cams = [TorchCamera(c, dev) for c in insta.camera_arrays(transform)]
    posed = torch.from_numpy(posed).to(dev)
    bg = torch.ones(3, device=dev)
    uv = avatar.plan.uv
    state = {"i": 0}

    def look_torch():     # `_gather_attribute_from_texture_dict` (uv_decoder.py:109-131) in stock torch
        grid = (2 * uv - 1)[None, None]
        act = {"color": tex["color"], "opacity": tex["opacity"],
               "scaling": avatar.max_scaling - torch.nn.functional.softplus(-(tex["scaling"] + avatar.mean_scaling) + avatar.max_scaling),
               "rotation": texture.rotation_activation(tex["rotation"]), "offset": torch.tanh(tex["offset"])}
        return {n: torch.nn.functional.grid_sample(act[n], grid, mode="bilinear", padding_mode="border", align_corners=True)
                .permute(0, 2, 3, 1).squeeze(1)[0].contiguous() for n in NAMES}

    def frame_hip():
        i = state["i"] = (state["i"] + 1) % len(cams)
        return avatar.render([cams[i]], [posed[i]], mb, bg, texture_dict=tex, bake_attribute=ATTRIBUTES)[0]["render"]

    def frame_torch():
        i = state["i"] = (state["i"] + 1) % len(cams)
        v = look_torch()
        h = _BakedFrame(v["color"].reshape(avatar.N, 1, 3), v["opacity"], v["scaling"], v["rotation"], v["offset"])
        return render_bound_batch([cams[i]], h, [posed[i]], mb, bg)[0]["render"]

    with torch.no_grad():
        med, rounds_t = alternate({"torch": frame_torch, "hip": frame_hip}, calls, rounds)
        assert rasterizer.last_forward_only[0] is True
        state["i"] = 0
        a = frame_hip()
        state["i"] = 0
        b = frame_torch()
        diff = float((a - b).abs().max())
    return {"points": avatar.N, "image": 512, "frames_per_s": {k: round(1.0 / v, 1) for k, v in med.items()},
            "ratio_hip_over_torch": round(med["torch"] / med["hip"], 4), "max_abs_image_difference": diff,
            "rounds_ms": {k: [round(1e3 * x, 4) for x in v] for k, v in rounds_t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=25, help="calls per timed round")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--trace-loop", type=int, default=0, help="only run this many eager forward + backward calls of each side")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.trace_loop or args.calls * args.rounds >= 200, "median of at least 200 replays"
    dev = torch.device("cuda:0")
    uv = layout_uv()
    cells, looks, tex, plan = make_cells(dev, uv)
    if args.trace_loop:
        for side in ("hip", "torch"):
            for _ in range(args.trace_loop):
                cells[("forward_backward", side)]()
            torch.cuda.synchronize()
        return
    row_start, entries = plan.csr()
    rows = (row_start[1:] - row_start[:-1])
    sum_c = sum(4 if n == "rotation" else CHANNELS[n] for n in NAMES)
    out = dict(tool="tools/texture_fps.py", device=torch.cuda.get_device_name(0), calls_per_round=args.calls, rounds=args.rounds,
               layout=dict(points=int(uv.shape[0]), texture=512, sum_channels=sum_c, entries=int(entries.numel()),
                           texels_touched=int((rows > 0).sum()), longest_row=int(rows.max()), mean_row=round(float(rows[rows > 0].float().mean()), 3)),
               algorithmic_bytes=dict(forward=8 * uv.shape[0] + 4 * uv.shape[0] * sum_c,
                                      backward_written=4 * sum_c * 512 * 512,
                                      backward_csr=4 * (512 * 512 + 1) + 4 * int(entries.numel()),
                                      backward_d_out=4 * uv.shape[0] * sum_c, backward_raw_texels=4 * 7 * 512 * 512),
               cells={})
    # the two sides compute the same thing
    with torch.no_grad():
        a, b = looks["torch"](), looks["hip"]()
        out["max_abs_difference_forward"] = {n: float((a[n] - b[n]).abs().max()) for n in NAMES}
    ga, gb = cells[("forward_backward", "torch")](), cells[("forward_backward", "hip")]()
    out["max_abs_difference_gradient"] = {n: float((x - y).abs().max()) for n, x, y in zip(NAMES, ga, gb)}
    slower = []
    for what in ("forward", "forward_backward"):
        eager = {side: cells[(what, side)] for side in ("torch", "hip")}
        graphs = {side: graph_of(fn, dev) for side, fn in eager.items()}
        for mode, pair in (("eager", eager), ("graph", {side: g[1] for side, g in graphs.items()})):
            med, rounds_t = alternate(pair, args.calls, args.rounds)
            cell = {"ms_per_call": {k: round(1e3 * v, 5) for k, v in med.items()}, "ratio_torch_over_hip": round(med["torch"] / med["hip"], 4),
                    "rounds_ms": {k: [round(1e3 * x, 5) for x in v] for k, v in rounds_t.items()}}
            out["cells"][f"{what}/{mode}"] = cell
            if med["hip"] > med["torch"]:
                slower.append(f"{what}/{mode}")
            print(what, mode, cell["ms_per_call"], "torch/hip", cell["ratio_torch_over_hip"], flush=True)
        del graphs
    out["hip_slower_in"] = slower
    out["baked_frames"] = baked_frames(dev, args.calls, args.rounds)
    print("baked frames/s", out["baked_frames"]["frames_per_s"], flush=True)
    doc = json.dumps(out, indent=1)
    print(doc)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
