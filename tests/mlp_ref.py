"""The torch restatement of FlashAvatar's point embedding and deformation MLP (model/baseline/flashavatar.py:396-464, fed as in
:238-240): the reference of every comparison in tests/test_mlp_host.py and tests/test_gpu_mlp.py.  It runs in whatever dtype its
inputs have (float64 for the ground truth, float32 on the CPU for the measured error bound).  `embed` and `run` are pinned to
recorded runs of the reference's own `Embedder(8)` and `MLP(110, 10, 256, 2)` by tests/test_reference_runs_host.py
(tests/golden/reference_mlp*.npz, cases `embed` and `mlp`)."""
import torch


def embed(points: torch.Tensor, n_freqs: int = 8) -> torch.Tensor:
    """Embedder (:396-430): the list of functions [identity, sin(. f0), cos(. f0), sin(. f1), ...] with f = 2^linspace(0, n-1, n),
    each applied to the [N,3] points, concatenated along the columns."""
    blocks = [points]
    freqs = torch.pow(2.0, torch.linspace(0.0, n_freqs - 1, steps=n_freqs))     # float32, as the reference's
    for k in range(n_freqs):
        scaled = points * freqs[k]
        blocks.append(scaled.sin())
        blocks.append(scaled.cos())
    return torch.cat(blocks, dim=1)


class RefMLP(torch.nn.Module):
    """`MLP` (:434-464) with the reference's attribute names, so that its state_dict has the reference's keys."""

    def __init__(self, input_dim, output_dim, hidden_dim=256, hidden_layers=8):
        super().__init__()
        self.fcs = torch.nn.ModuleList([torch.nn.Linear(input_dim, hidden_dim)] +
                                       [torch.nn.Linear(hidden_dim, hidden_dim) for _ in range(hidden_layers - 1)])
        self.output_linear = torch.nn.Linear(hidden_dim, output_dim)

    def forward(self, h):
        for fc in self.fcs:
            h = torch.nn.functional.relu(fc(h))
        return self.output_linear(h)


def run(weights, biases, E, cond, d_out):
    """Forward and backward of the network on [E | cond repeated] in the dtype of `weights`: a dict with the raw outputs `out`,
    the pre-activations `z` of the hidden layers, and the gradients `d_weights` / `d_bias` (lists, output layer last) and `d_cond`
    for dLoss/d(out) = `d_out`."""
    dt = weights[0].dtype
    W = [w.detach().to(dt).clone().requires_grad_(True) for w in weights]
    B = [b.detach().to(dt).clone().requires_grad_(True) for b in biases]
    c = cond.detach().to(dt).clone().requires_grad_(True)
    h = torch.cat([E.to(dt), c.expand(E.shape[0], c.shape[0])], dim=1)
    zs = []
    for w, b in zip(W[:-1], B[:-1]):
        z = torch.nn.functional.linear(h, w, b)
        zs.append(z.detach())
        h = torch.relu(z)
    out = torch.nn.functional.linear(h, W[-1], B[-1])
    out.backward(d_out.to(dt))
    zero = torch.zeros_like
    return dict(out=out.detach(), z=zs, d_weights=[w.grad if w.grad is not None else zero(w) for w in W],
                d_bias=[b.grad if b.grad is not None else zero(b) for b in B], d_cond=c.grad if c.grad is not None else zero(c))
