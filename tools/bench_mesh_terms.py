#!/usr/bin/env python
"""The mesh-terms launch alone against two stock-PyTorch versions of the same loss and gradient, on the head template
(V = 5023), timed with device events.

    python tools/bench_mesh_terms.py [--launches 200 --repeats 3]

  * fused      — `loss.mesh_terms_and_grad` (fr_mesh_terms: both losses and the gradient, one launch), `--launches` of them
                 back-to-back in ONE captured graph
  * dense      — the reference's formulation (train/loss.py:112-121): L.to_dense() [V,V], two mm forward, autograd backward;
                 captured in a graph the same way, and eager
  * sparse     — the same expression with torch.sparse.mm on the COO Laplacian, eager (sparse kernels do not capture)
Prints one JSON line: microseconds per evaluation (loss + gradient), the median and the range over the repeats; the variants
are alternated within every repeat."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fateavatar_amd import scenes  # noqa: E402
from fateavatar_amd.binding import mesh_laplacian  # noqa: E402
from fateavatar_amd.loss import REFERENCE_MESH_TERMS, mesh_terms_and_grad, mesh_terms_workspace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    verts, faces, _ = scenes.head_geometry()
    vo = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(dev)
    V = int(vo.shape[0])
    g = torch.Generator().manual_seed(0)
    v = (vo + (0.003 * torch.randn(V, 3, generator=g)).to(dev)).contiguous()
    lap = mesh_laplacian(torch.from_numpy(np.asarray(faces)).to(dev), V)
    dense = lap.to_dense()
    sparse = dense.to_sparse().coalesce()
    w = float(REFERENCE_MESH_TERMS.laplacian_weight)
    d_verts, out, ws = torch.zeros_like(v), torch.zeros(2, device=dev), mesh_terms_workspace(dev)
    leaf = v.clone().requires_grad_(True)

    def fused():
        mesh_terms_and_grad(v, vo, lap, REFERENCE_MESH_TERMS, d_verts=d_verts, out=out, workspace=ws)

    def torch_version(mm, L):
        def run():
            leaf.grad = None
            basis = mm(L, vo).detach()
            (w * ((mm(L, leaf) - basis) ** 2).sum(dim=-1, keepdim=True).mean()).backward()
        return run

    def captured(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(a.launches):
                fn()
        torch.cuda.synchronize()
        return graph.replay

    def timed(fn, evaluations):
        fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / evaluations

    def loop(fn):
        def run():
            for _ in range(a.launches):
                fn()
        return run

    dense_fn, sparse_fn = torch_version(torch.mm, dense), torch_version(torch.sparse.mm, sparse)
    variants = {"fused_graph": (captured(fused), a.launches), "dense_graph": (captured(dense_fn), a.launches),
                "fused_eager": (loop(fused), a.launches), "dense_eager": (loop(dense_fn), a.launches),
                "sparse_eager": (loop(sparse_fn), a.launches)}
    mm_only = captured(lambda: torch.mm(dense, vo))     # ONE dense product: what the "16 us per product" estimate is about
    variants["dense_one_product_graph"] = (mm_only, a.launches)
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, (fn, n) in variants.items():
            times[k].append(timed(fn, n))
    # the three agree on what they compute
    fused()
    d_verts.zero_()
    fused()
    dense_fn()
    torch.cuda.synchronize()
    agree = float((d_verts - leaf.grad).norm() / leaf.grad.norm())
    print(json.dumps({"metric": "mesh terms: microseconds per loss + gradient evaluation, head template", "V": V, "nnz": int(lap.col.numel()),
                      "launches_per_timing": a.launches, "repeats": a.repeats,
                      "us": {k: {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
                             for k, t in times.items()},
                      "fused_vs_dense_gradient_rel_l2": agree}))


if __name__ == "__main__":
    main()
