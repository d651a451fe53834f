"""What the depth and alpha planes (FR_FLAG_DEPTH_ALPHA, `render(..., depth_alpha=True)`) cost at BASELINE config 2 (the head
template, 100 k Gaussians, 512^2, SH degree 3): frames/s with and without them, alternated round by round in one process,
for no-grad frames (forward-only) and for render + backward (an image term, and with planes an alpha and a depth term).

    python tools/depth_alpha_cost.py [--frames 300] [--rounds 5] [--out profiles/r08_depth_alpha.json]

The per-kernel table comes from a kernel trace of a fixed workload (120 render + backward frames, then 120 no-grad frames),
one process per variant:

    rocprofv3 --kernel-trace --stats -d DIR_PLAIN -o run -- python tools/depth_alpha_cost.py --workload plain
    rocprofv3 --kernel-trace --stats -d DIR_PLANES -o run -- python tools/depth_alpha_cost.py --workload planes
    python tools/depth_alpha_cost.py --table DIR_PLAIN/run_results.db DIR_PLANES/run_results.db --out FILE

(--table adds the table to FILE's JSON document if it exists.)
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _setup():
    import torch
    from fateavatar_amd import scenes
    from fateavatar_amd.model import FlatGaussians, TorchCamera
    dev = torch.device("cuda:0")
    s = scenes.head_scene()
    pc = FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, s.sh_degree, dev, fused_activations=True)
    cam, bg = TorchCamera(s.camera, dev), torch.from_numpy(s.bg).to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    w = (torch.randn(3, 512, 512, generator=g) / 512 ** 2).to(dev)
    wd = (torch.randn(1, 512, 512, generator=g) / 512 ** 2).to(dev)
    return pc, cam, bg, w, wd


def _frames(env, planes, n, grad):
    import torch
    from fateavatar_amd.render import render
    pc, cam, bg, w, wd = env
    if not grad:
        with torch.no_grad():
            for _ in range(n):
                render(cam, pc, bg, depth_alpha=planes)
        return
    for _ in range(n):
        out = render(cam, pc, bg, depth_alpha=planes)
        loss = (out["render"] * w).sum()
        if planes:
            loss = loss + (out["alpha"] * wd).sum() + (out["depth"] * wd).sum()
        loss.backward()


def measure(frames, rounds):
    import torch
    env = _setup()
    res = {}
    for name, grad in (("nograd", False), ("render_backward", True)):
        for planes in (False, True):
            _frames(env, planes, 20, grad)
        torch.cuda.synchronize()
        for r in range(rounds):
            for planes in ((False, True) if r % 2 == 0 else (True, False)):
                torch.cuda.synchronize()
                t = time.perf_counter()
                _frames(env, planes, frames, grad)
                torch.cuda.synchronize()
                res.setdefault(f"{name}_{'planes' if planes else 'plain'}", []).append(frames / (time.perf_counter() - t))
    out = {"what": "frames/s at config 2 through render(), plain against depth_alpha=True, alternated round by round",
           "frames_per_round": frames}
    for k, v in res.items():
        out[k] = dict(median=round(sorted(v)[len(v) // 2], 1), rounds=[round(x, 1) for x in v])
    for name in ("nograd", "render_backward"):
        out[f"{name}_planes_cost_pct"] = round(100.0 * (out[f"{name}_plain"]["median"] / out[f"{name}_planes"]["median"] - 1.0), 2)
    return out


def kernel_table(db_plain, db_planes):
    """Per kernel: launches and mean µs in the two traces (rocprofv3's SQLite output), and the rasterizer's own kernel time
    per frame of each kind."""
    import sqlite3

    def load(path):
        db = sqlite3.connect(path)
        d = collections.defaultdict(list)
        for name, s, e in db.execute("select name, start, end from kernels"):
            m = re.search(r"fr::(\w+)", name)
            d[m.group(1) if m else name[:48]].append((e - s) / 1000.0)
        return d
    a, b = load(db_plain), load(db_planes)
    rows = []
    for k in sorted(set(a) | set(b), key=lambda k: -(sum(a.get(k, [])) + sum(b.get(k, [])))):
        ta, tb = a.get(k, []), b.get(k, [])
        rows.append(dict(kernel=k, plain_launches=len(ta), plain_us=round(sum(ta) / len(ta), 2) if ta else None,
                         planes_launches=len(tb), planes_us=round(sum(tb) / len(tb), 2) if tb else None))
    return rows


def frame_sums(rows):
    """The rasterizer's kernels per render + backward frame and per no-grad frame (the fixed workload of --workload)."""
    us = {r["kernel"]: (r["plain_us"], r["planes_us"]) for r in rows}

    def pick(names, col):
        return round(sum(us[n][col] for n in names if n in us and us[n][col] is not None), 2)
    fwd = ["k_preprocess_fwd", "k_tile_totals", "k_tile_sort", "k_tile_sort_planes"]
    out = {}
    for col, tag in ((0, "plain"), (1, "planes")):
        blend = "k_unit_blend_chained_planes" if col else "k_unit_blend_chained"
        blend_fo = "k_unit_blend_chained_fwd_only_planes" if col else "k_unit_blend_chained_fwd_only"
        bwd = ["k_unit_blend_bwd_sparse_planes", "k_preprocess_bwd_planes"] if col else ["k_unit_blend_bwd_sparse", "k_preprocess_bwd"]
        out[f"render_backward_us_{tag}"] = pick(fwd + [blend] + bwd, col)
        out[f"nograd_us_{tag}"] = pick(["k_preprocess_fwd_only", "k_tile_totals", "k_tile_sort", "k_tile_sort_planes", blend_fo], col)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--workload", choices=("plain", "planes"), default=None, help="the fixed workload for a kernel trace")
    ap.add_argument("--table", nargs=2, metavar=("DB_PLAIN", "DB_PLANES"), default=None)
    a = ap.parse_args()
    if a.workload:
        import torch
        env = _setup()
        _frames(env, a.workload == "planes", 120, True)
        _frames(env, a.workload == "planes", 120, False)
        torch.cuda.synchronize()
        return
    if a.table:
        doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        rows = kernel_table(*a.table)
        doc["kernel_trace"] = dict(what="rocprofv3 --kernel-trace: 120 render + backward and 120 no-grad frames per variant; "
                                   "mean µs per launch", kernels=rows, per_frame=frame_sums(rows))
    else:
        doc = measure(a.frames, a.rounds)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
