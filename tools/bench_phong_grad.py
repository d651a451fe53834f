#!/usr/bin/env python
"""Time the two calls of the Phong-surface binding's vertex gradient alone, on the head template (V = 5 023, F = 10 006):
fr_bind_backward_phong_frame (one launch, N Gaussians) and fr_phong_frame_backward (two launches, per mesh).

    python tools/bench_phong_grad.py [--N 10000 100000 --repeats 3 --calls 200 --warmup 20] [--json PATH]

A repeat is, for every N in turn, device events around `--calls` back-to-back launches of the scatter and then of the mesh pass's
backward (the C entry points, no autograd around them); the repeats alternate the sizes.  Prints one JSON line with the mean of
the repeats' per-call times.  Per-KERNEL durations come from running this under `rocprofv3 --kernel-trace --stats`: every size
launches exactly (warmup + repeats x calls) k_bind_phong_frame_bwd, told apart by their grids, and the two kernels of the mesh
pass's backward do not depend on N."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fateavatar_amd import insta  # noqa: E402
from fateavatar_amd.binding import (PhongGradBuffers, phong_canonical, phong_frame, phong_frame_backward,  # noqa: E402
                                    phong_scatter_frame_grads)
from fateavatar_amd.splatting import sample_bary_on_triangles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_phong_grad: needs the GPU (there is no CPU path and no CPU timing)")
    dev = torch.device("cuda", 0)
    _, posed, faces = insta.synthetic_sequence(4, 64, 0)
    posed_t, faces_t = torch.from_numpy(posed).to(dev), torch.from_numpy(faces).to(dev).to(torch.int32).contiguous()
    c = phong_canonical(posed_t[0], faces_t)
    verts = posed_t[2].contiguous()
    V, F = int(verts.shape[0]), int(faces_t.shape[0])
    frame = phong_frame(c, verts)
    buf = PhongGradBuffers(V, F, dev, zeroed=True)
    cases = {}
    for N in a.N:
        g = torch.Generator().manual_seed(N)
        fi, bary = sample_bary_on_triangles(F, N, g)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
        cases[N] = (verts, faces_t, fi.to(dev, torch.int32), bary.to(dev), frame, 0.01 * r(N, 3), r(N, 4), r(N, 3), r(N, 3), r(N, 4),
                    r(N, 3), buf.d_verts, buf.d_vert_normals, buf.d_vert_quats, buf.d_face_ratio)

    def scatter(N):
        phong_scatter_frame_grads(*cases[N])

    def mesh_backward(_N):
        phong_frame_backward(c, verts, buf.d_vert_normals, buf.d_vert_quats, buf.d_face_ratio, buf.d_verts, buf.workspace)

    def timed(fn, N, calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn(N)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / calls * 1e3      # us per call

    for N in a.N:
        buf.zero_()
        timed(scatter, N, a.warmup)
        timed(mesh_backward, N, a.warmup)
    times = {N: {"scatter": [], "mesh_backward": []} for N in a.N}
    for _ in range(a.repeats):
        for N in a.N:
            buf.zero_()      # (the sums stay finite over the calls of one window)
            times[N]["scatter"].append(timed(scatter, N, a.calls))
            times[N]["mesh_backward"].append(timed(mesh_backward, N, a.calls))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf.d_verts).all())
    out = {"metric": "vertex gradient of the Phong-surface binding: us per call, device events around back-to-back calls "
                     "(launch gaps included; kernel durations: rocprofv3)",
           "V": V, "F": F, "calls_per_repeat": a.calls, "repeats": a.repeats,
           "sizes": {str(N): {k: {"mean_us": round(statistics.mean(v), 3), "repeats_us": [round(x, 3) for x in v]}
                              for k, v in times[N].items()} for N in a.N},
           "atomics_per_gaussian": 31, "scatter_grid": {str(N): int(np.ceil(N / 256)) for N in a.N},
           "mesh_backward_grid": int(np.ceil(V / 32)), "workspace_bytes": 28 * V}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
