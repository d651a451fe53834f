"""(GPU) The fused deformation MLP's forward and backward alone: HIP events over --calls eager calls of each at FlashAvatar's
shape (51 embedded columns + 59 condition columns -> 256 x 6 -> 10), per size one JSON line with the time per call and the
achieved FLOP rate against the MI355X's f32 peak (157.3 TF, exact-f32 MFMA = the vector rate) and the 122 TF of an untuned
LDS-tiled f32-MFMA GEMM at 4096^3 (MI355X_MICROARCH, "Matrix cores").

    python tools/mlp_kernel_time.py [--P 16384 100000] [--calls 200] [--layers 6]

The FLOP counts are the products the algorithm needs (2 per multiply-add), from the shapes:
    forward   2 N (De 256 + (L - 1) 256^2 + 256 D_out)            (the condition half is 256 Dc per FRAME: not counted)
    backward  the same again for dW, plus 2 N ((L - 1) 256^2 + 256 D_out) for dH (layer 0 has no input gradient)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_TF, GUIDE_TF = 157.3, 122.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="+", default=[16_384, 100_000])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--layers", type=int, default=6)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device (there is no CPU path)")
    from fateavatar_amd.mlp import DeformMLP, embed_points
    dev = torch.device("cuda", 0)
    De, Dc, W, D_out, L = 51, 59, 256, 10, a.layers
    for N in a.P:
        g = torch.Generator().manual_seed(0)
        mlp = DeformMLP(embed_points(torch.rand(N, 3, generator=g) * 0.4 - 0.2).to(dev).contiguous(), Dc, layers=L, out_dim=D_out)
        cond = (0.3 * torch.randn(Dc, generator=g)).to(dev)
        d_out = torch.randn(N, D_out, generator=g).to(dev)
        out, d_cond = torch.empty(N, D_out, device=dev), torch.empty(Dc, device=dev)
        fwd = lambda: mlp.forward_into(cond, out)                      # noqa: E731
        bwd = lambda: mlp.backward_from(d_out, cond, d_cond)           # noqa: E731
        flop_f = 2.0 * N * (De * W + (L - 1) * W * W + W * D_out)
        flop_b = flop_f + 2.0 * N * ((L - 1) * W * W + W * D_out)
        res = {"N": N, "layers": L, "calls": a.calls, "workspace_MB": None}
        for name, fn, flop in (("forward", fwd, flop_f), ("backward", bwd, flop_b)):
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.calls
            tf = flop / (ms * 1e-3) / 1e12
            res[name] = {"ms_per_call": round(ms, 4), "GFLOP": round(flop / 1e9, 3), "TF_per_s": round(tf, 2),
                         "share_of_157TF_peak": round(tf / PEAK_TF, 3), "against_122TF_untuned_gemm": round(tf / GUIDE_TF, 3)}
        res["workspace_MB"] = round(mlp._workspace.numel() / 1e6, 1)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
