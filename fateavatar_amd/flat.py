"""The flat parameter holder every Gaussian model here derives from.

All parameters of a model live in ONE flat fp32 buffer and their gradients in one flat buffer, one [P, width] run per field:
the fused Adam is one kernel over the buffer (optim.py), the data-parallel exchange is a single all-reduce (dp.py), and the
HIP kernels write gradients straight into their field's run (rasterizer.GradOut).  A subclass describes itself — `FIELDS`,
`SHAPES`, `ROW_BUFFERS` — and builds its initial values; the buffers, the gradient bookkeeping and the row surgery are here.
"""
from __future__ import annotations

import torch

from .rasterizer import GradOut


class FlatParams(torch.nn.Module):
    FIELDS = ()        # ((parameter name, floats per row), ...) in flat-buffer order = the order of the optimizer groups
    SHAPES = {}        # parameter name -> shape of one row
    ROW_BUFFERS = ()   # ((attribute, dtype, resize() keyword), ...): per-row tensors that are no parameters but follow the rows

    @property
    def P(self) -> int:
        return self._rows

    def widths(self):
        """Floats per row of each field, in flat-buffer order."""
        return [w for _, w in self.FIELDS]

    def shapes(self):
        """Shape of one row of each field, in flat-buffer order."""
        return [self.SHAPES[name] for name, _ in self.FIELDS]

    def _wants_slot(self, name: str) -> bool:
        """Whether the parameter reaches a HIP kernel raw (the rasterizer or a binding op), which then writes its gradient
        straight into the flat gradient buffer (rasterizer.py `_fr_grad_out`): no accumulation kernel, no zero-fill."""
        return True

    def _bind(self, raw):
        """(Re)build the flat value / gradient buffers from one raw tensor per field ([P, ...] each) and make every
        parameter, and its gradient slot, a view into them."""
        P, dev = int(raw[0].shape[0]), raw[0].device
        flat = torch.empty(P * sum(self.widths()), dtype=torch.float32, device=dev)
        off = 0
        for w, r in zip(self.widths(), raw):
            flat[off:off + P * w].copy_(r.detach().reshape(-1))
            off += P * w
        self._attach(flat, P)

    def _attach(self, flat, P):
        n = flat.numel()
        self._rows, self.flat = P, flat
        # the gradient buffer, and behind it (same allocation, so that ONE all-reduce carries both) the step's OVERFLOW WORD:
        # the rasterizer's backward sets it to 1 when its frame overflowed the binning capacity inside a replayed graph (all
        # its gradients are zero then), and the fused Adam skips a step whose word — summed over lanes and ranks — is not 0
        self._grad_store = torch.zeros(n + 4, dtype=torch.float32, device=flat.device)
        self.flat_grad = self._grad_store[:n]
        self.overflow_word = self._grad_store[n:n + 1]
        self._grad_views = {}
        off = 0
        for (name, _), w, shp in zip(self.FIELDS, self.widths(), self.shapes()):
            p = torch.nn.Parameter(flat[off:off + P * w].view((P,) + tuple(shp)))
            self._grad_views[name] = gv = self.flat_grad[off:off + P * w].view(p.shape)
            if self._wants_slot(name):
                p._fr_grad_out = GradOut(gv)
            setattr(self, name, p)
            off += P * w

    def lane(self):
        """A second set of leaves over the SAME parameter storage (and the same row buffers) with a gradient buffer of its
        own: what another view of a batch, rendered in flight together with this one, back-propagates into."""
        o = type(self).__new__(type(self))
        torch.nn.Module.__init__(o)
        o.__dict__.update({k: v for k, v in self.__dict__.items() if k not in o.__dict__})   # all but the Module's own state
        o._attach(self.flat, self.P)
        return o

    def begin_step(self):
        """Drop the previous gradients (set_to_none, like the reference's zero_grad(set_to_none=True),
        train/iteration.py:49): the next backward ASSIGNS instead of accumulating."""
        for name, _ in self.FIELDS:
            getattr(self, name).grad = None

    def grad_view(self, name: str) -> torch.Tensor:
        """The run of the flat gradient buffer that belongs to the field `name`, as [P, width]."""
        return self._grad_views[name].flatten(1)

    def collect_grads(self) -> torch.Tensor:
        """After backward: make `flat_grad` hold every parameter's gradient.  What a kernel wrote into its slot is there
        already; a field without a gradient is zeroed; a gradient autograd made itself (the activated parameters of an
        unfused model, the halves of a concatenated SH block — these come back as non-contiguous slices) is copied in."""
        for name, view in self._grad_views.items():
            if view.numel() == 0:
                continue
            g = getattr(self, name).grad
            if g is None:
                view.zero_()
            elif g.data_ptr() != view.data_ptr() or not g.is_contiguous():
                view.copy_(g)
        return self.flat_grad

    def exchange_buffer(self) -> torch.Tensor:
        """`collect_grads()` + the overflow word behind it: what a data-parallel step all-reduces (SUM)."""
        self.collect_grads()
        return self._grad_store

    @torch.no_grad()
    def resize(self, keep_mask=None, new_rows=None, order=None, **new_buffers) -> torch.Tensor:
        """Prune, re-order and / or append rows (reference: _prune_low_opacity_points / _uv_densify,
        model/fateavatar.py:610-711): the rows where `keep_mask` is False are dropped — or the rows are taken in the sequence
        `order` (row indices: a permutation re-stores the set in another order) —, then `new_rows` — one raw tensor
        [n_new, ...] per field, in FIELDS order — are appended, with their row buffers under the keywords ROW_BUFFERS names.
        The row buffers follow the rows.  The flat buffers are rebuilt and every parameter is a new nn.Parameter (as in the
        reference); returns the row map (int64 [P_new]: the old row of every new row, -1 for appended ones) that optimizer
        state has to follow (FusedAdam.remap_rows)."""
        dev = self.flat.device
        keys = {key for _, _, key in self.ROW_BUFFERS}
        if not set(new_buffers) <= keys:
            raise TypeError(f"resize: unexpected keywords {sorted(set(new_buffers) - keys)}")
        if order is not None:
            if keep_mask is not None:
                raise ValueError("resize: keep_mask or order, not both")
            old_index = order.to(dev, torch.int64).reshape(-1)
        else:
            keep = torch.ones(self.P, dtype=torch.bool, device=dev) if keep_mask is None else keep_mask.to(dev).bool().reshape(-1)
            if keep.numel() != self.P:
                raise ValueError("keep_mask must have one entry per Gaussian")
            old_index = torch.nonzero(keep).reshape(-1)
        raw = [getattr(self, name).detach()[old_index] for name, _ in self.FIELDS]
        bufs = [getattr(self, attr)[old_index] for attr, _, _ in self.ROW_BUFFERS]
        n_new = 0
        if new_rows is not None:
            n_new = int(new_rows[0].shape[0])
            raw = [torch.cat([r, a.to(dev, torch.float32).reshape((n_new,) + tuple(r.shape[1:]))]) for r, a in zip(raw, new_rows)]
            for i, (_, dtype, key) in enumerate(self.ROW_BUFFERS):
                add = new_buffers.get(key)
                if add is None or int(add.shape[0]) != n_new:
                    raise ValueError(f"{key} must hold one entry per appended row")
                bufs[i] = torch.cat([bufs[i], add.to(dev, dtype).reshape((n_new,) + tuple(bufs[i].shape[1:]))])
        for (attr, _, _), b in zip(self.ROW_BUFFERS, bufs):
            setattr(self, attr, b.contiguous())
        self._bind(raw)
        return torch.cat([old_index, torch.full((n_new,), -1, dtype=torch.int64, device=dev)])
