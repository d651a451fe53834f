"""No-grad rendering speed, forward-only frames (FR_FLAG_FORWARD_ONLY) against full frames — the counterpart of the
reference's `fps_performance_test` / `fps_unit` (train/trainer.py:541-573), the frames/s figure avatar papers report.

Two workloads:
  config2   BASELINE config 2: the head template, 100 k Gaussians, 512^2, SH degree 3 — `render()` / `render_batch()`;
  reenact   reenactment: `AvatarGaussians.from_template` (the reference's UV initialisation, 65 536 Gaussians) rendered
            straight from a sequence of posed vertices (`render_bound_batch`), 512^2.
Three modes each:
  one       one frame per call, under torch.no_grad();
  batch4    four views per launch chain;
  graph4    a four-view launch chain captured into a graph and replayed.
Every (workload, mode) runs both variants — forward-only (the automatic choice under no_grad) and full
(`rasterizer.set_forward_only(False)`) — alternated round by round in one process, each round timed over `--frames`
frames after a warm-up.  Per-stage times (fr_profile_read, per launch chain) come from a separate profiled pass of the eager
modes.  Prints one JSON document (and writes it to --out).

    python tools/render_fps.py [--frames 400] [--rounds 5] [--out profiles/r07_render_fps.json]
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

from fateavatar_amd import _lib, rasterizer, scenes  # noqa: E402


def config2(dev):
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    from fateavatar_amd.render import render, render_batch
    s = scenes.head_scene()
    pc = FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, s.sh_degree, dev, fused_activations=True)
    cams = [TorchCamera(scenes.head_scene(P=16, view=k, n_views=4).camera, dev) for k in range(4)]
    bg = torch.from_numpy(s.bg).to(dev)
    return dict(one=lambda i: render(cams[i % 4], pc, bg)["render"],
                batch4=lambda i: render_batch(cams, pc, bg)[-1]["render"])


def reenact(dev, n_frames=32):
    from fateavatar_amd import insta
    from fateavatar_amd.avatar import AvatarGaussians, _RawFrame
    from fateavatar_amd.binding import face_scale
    from fateavatar_amd.bound import MeshBinding, render_bound_batch
    from fateavatar_amd.model import TorchCamera
    transform, posed, faces = insta.synthetic_sequence(n_frames, 512, 0)
    verts, _, _ = scenes.head_geometry()
    pc = AvatarGaussians.from_template(dev, uv_resolution=256)
    g = torch.Generator(device="cpu").manual_seed(1)
    with torch.no_grad():   # a trained-looking avatar: coloured, half opaque
        pc._features_dc.copy_((torch.rand(pc.P, 1, 3, generator=g) * 2 - 1).to(dev))
        pc._opacity.fill_(0.0)
    faces_t = torch.from_numpy(faces).to(dev)
    mb = MeshBinding(faces_t, pc.face_index, pc.bary_coords, face_scale(torch.from_numpy(verts).to(dev), faces_t), 0.05, True)
    cams = [TorchCamera(c, dev) for c in insta.camera_arrays(transform)]
    posed = torch.from_numpy(posed).to(dev)
    frame = _RawFrame(pc, None)
    bg = torch.ones(3, device=dev)
    n = len(cams)
    return dict(one=lambda i: render_bound_batch([cams[i % n]], [frame], [posed[i % n]], mb, bg)[0]["render"],
                batch4=lambda i: render_bound_batch([cams[(4 * i + k) % n] for k in range(4)], [frame] * 4,
                                                    [posed[(4 * i + k) % n] for k in range(4)], mb, bg)[-1]["render"])


def timed(fn, calls, views_per_call, warmup=10):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    torch.cuda.synchronize()
    return calls * views_per_call / (time.perf_counter() - t0)


def stages(fn, calls, dev_index=0):
    """Mean ms per call of every stage (the first view's handle: slot 0), from fr_profile_read."""
    torch.cuda.synchronize()
    _lib.profile_enable(dev_index, True)
    for i in range(calls):
        fn(i)
    torch.cuda.synchronize()
    st = _lib.profile_read(dev_index)
    _lib.profile_enable(dev_index, False)
    return {k: round(ms / calls, 5) for k, (ms, n) in st.items() if n}


def graph_of(fn, dev):
    """fn(0) captured (four views, no host wait) on a stream of its own; eager frames of it first size the handles."""
    stream = torch.cuda.Stream(device=dev)
    with rasterizer.no_wait():
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            for _ in range(3):
                fn(0)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
            fn(0)
    torch.cuda.synchronize()

    def replay(_i):
        with torch.cuda.stream(stream):
            g.replay()
    return g, replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400, help="frames per timed round (rounded to whole calls)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    variants = {"forward_only": True, "full": False}
    out = dict(tool="tools/render_fps.py", device=torch.cuda.get_device_name(0), frames_per_round=args.frames,
               rounds=args.rounds, workloads={})
    for wname, make in (("config2", config2), ("reenact", reenact)):
        fns = make(dev)
        res = {}
        with torch.no_grad():
            # the graph mode: one capture per variant, made before anything is timed
            graphs = {}
            for vname, auto in variants.items():
                with rasterizer.set_forward_only(auto):
                    graphs[vname] = graph_of(fns["batch4"], dev)
            for mode in ("one", "batch4", "graph4"):
                per = 1 if mode == "one" else 4
                calls = max(1, args.frames // per)
                fps = {v: [] for v in variants}
                for r in range(args.rounds):   # alternated: full and forward-only share every drift of the box
                    for vname, auto in (list(variants.items()) if r % 2 == 0 else list(variants.items())[::-1]):
                        with rasterizer.set_forward_only(auto):
                            fn = graphs[vname][1] if mode == "graph4" else fns[mode]
                            fps[vname].append(timed(fn, calls, per))
                            if mode != "graph4":
                                assert rasterizer.last_forward_only[0] is auto, (wname, mode, vname)
                m = {}
                for vname, auto in variants.items():
                    m[vname] = dict(frames_per_s=round(statistics.median(fps[vname]), 1),
                                    rounds=[round(x, 1) for x in fps[vname]])
                    if mode != "graph4":
                        with rasterizer.set_forward_only(auto):
                            m[vname]["stage_ms_per_chain"] = stages(fns[mode], min(calls, 100))
                m["speedup"] = round(m["forward_only"]["frames_per_s"] / m["full"]["frames_per_s"], 4)
                res[mode] = m
                print(wname, mode, {v: m[v]["frames_per_s"] for v in variants}, "speedup", m["speedup"], flush=True)
            # the images the two variants leave are the same bits
            imgs = {}
            for vname, auto in variants.items():
                with rasterizer.set_forward_only(auto):
                    imgs[vname] = fns["batch4"](0).cpu().numpy()
            res["images_bit_identical"] = bool(np.array_equal(imgs["forward_only"], imgs["full"]))
            del graphs
        out["workloads"][wname] = res
        torch.cuda.synchronize()
    doc = json.dumps(out, indent=1)
    print(doc)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
