#!/usr/bin/env python
"""Time fr_point_lbs_backward_pose (the gradients of MonoGaussianAvatar's point deformation to the frame's pose state) alone, against
the float32 plain-torch restatement's backward to the frame state on the same device and against its own byte model.

    python tools/bench_mono_pose.py [--N 100000 --E 50 --J 6 --rounds 5] [--json PATH]

A round is device events around `--calls` launches of the fused kernel (the C entry point, no autograd around it), then around
`--torch-calls` backward passes of tests/mono_ref.py (torch.autograd.grad on a graph that is kept, so the forward is not in the
time); the two alternate.  Bytes the launch must read: N x (3 E + 108 + J + 3 + 3) floats (S, P, w, p, g; the 1.2 KB of pose
states and the per-workgroup partials, 512 x 272 floats written and read once, are not counted).  Prints one JSON line.  Needs the
checkout's tests/ next to tools/ (the restatement and the recipe live there)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fateavatar_amd import _lib, mono  # noqa: E402
from tests import mono_ref  # noqa: E402

HBM_ACHIEVABLE = 6.29e12     # bytes/s a streaming read reaches on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--E", type=int, default=50)
    ap.add_argument("--J", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--torch-calls", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mono_pose: needs the GPU (there is no CPU path and no CPU timing)")
    dev = torch.device("cuda", 0)
    N, E, J = a.N, a.E, a.J
    p, S, P, w, c, f, g = mono_ref.recipe(N, E, J)
    x = [t.float().to(dev).contiguous() for t in (p, S, P, w)]
    c, f, g = [t.float().to(dev).contiguous() for t in c], [t.float().to(dev).contiguous() for t in f], g.float().to(dev).contiguous()
    d = mono._describe(*x, c, f)
    ws = mono.pose_workspace(dev)
    outs = [torch.empty_like(t) for t in f]

    def fused():
        _lib.launch("fr_point_lbs_backward_pose", dev, C.byref(d), g.data_ptr(), *[t.data_ptr() for t in outs], ws.data_ptr())

    frame = [t.clone().requires_grad_(True) for t in f]
    xyz = mono_ref.deform_points(*x, tuple(c), tuple(frame))

    def torch_backward():
        return torch.autograd.grad(xyz, frame, g, retain_graph=True)

    def timed(fn, calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / calls

    for _ in range(3):
        fused()
        want = torch_backward()
    torch.cuda.synchronize()
    rel = [float((a_ - b_).norm() / b_.norm()) for a_, b_ in zip(outs, want)]
    t_fused, t_torch = [], []
    for _ in range(a.rounds):
        t_fused.append(timed(fused, a.calls))
        t_torch.append(timed(torch_backward, a.torch_calls))
    assert int(ws.count_nonzero()) == 0
    bytes_read = N * (3 * E + 108 + J + 3 + 3) * 4
    ms = statistics.median(t_fused)
    out = {"metric": "fr_point_lbs_backward_pose alone: ms per launch (device events around back-to-back launches)",
           "N": N, "E": E, "J": J, "calls_per_round": a.calls, "fused_ms_rounds": [round(t, 5) for t in t_fused],
           "torch_backward_ms_rounds": [round(t, 4) for t in t_torch], "fused_ms": round(ms, 5),
           "torch_backward_ms": round(statistics.median(t_torch), 4), "torch_over_fused": round(statistics.median(t_torch) / ms, 1),
           "bytes_read_model": bytes_read, "bytes_per_s": round(bytes_read / (ms * 1e-3), 0),
           "share_of_achievable_hbm_6.29TBps": round(bytes_read / (ms * 1e-3) / HBM_ACHIEVABLE, 3),
           "rel_l2_vs_torch_float32": [float(f"{r:.3e}") for r in rel]}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
