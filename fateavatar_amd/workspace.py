"""The scratch of the fused "loss + gradient in one launch" kernels, kept per stream.

Every such kernel elects its last workgroup through counters in a workspace and sums per-workgroup partials left there
(sum_over_workgroups, csrc/fr_common.hpp); the workspace is zeroed once and the kernel leaves it zeroed.  Two launches that
overlap on the device — the lanes of AvatarBatchStep run on their own streams, each from its own captured graph — must not
share one (the loss scalars would mix; include/fr_rasterizer.h says the same of every entry point that takes one).  So by
default an op keeps one workspace per (device, current stream), and a caller may pass its own."""
from __future__ import annotations

import torch


class StreamWorkspace:
    """The workspaces of ONE op: `maker` is the name of its public `*_workspace()` function, `nbytes(*need)` the library's
    size query, `on` whose device a workspace must be on ("image's"), `first` / `maker_args` the op's wording of the one
    message that differs."""

    def __init__(self, maker: str, nbytes, on: str, first: str = "first call", maker_args: str = "device"):
        self.maker, self.nbytes, self.on, self.first, self.maker_args = maker, nbytes, on, first, maker_args
        self.kept = {}   # (device index, stream handle) -> zeroed scratch

    def fresh(self, dev, *need) -> torch.Tensor:
        """A zeroed workspace on `dev` that the caller owns (`need`: the size query's arguments, if it has any)."""
        if not isinstance(dev, (torch.device, str, int)):
            raise RuntimeError(f"{self.maker}: a device, not {type(dev).__name__}")
        dev = torch.device("cuda", dev) if isinstance(dev, int) else torch.device(dev)
        if dev.type != "cuda":
            raise RuntimeError(f"{self.maker}: a HIP device, not {dev} (there is no CPU path)")
        return torch.zeros((self.nbytes(*need),), dtype=torch.uint8, device=dev)

    def resolve(self, dev: torch.device, workspace, who: str, need=None) -> torch.Tensor:
        """The caller's `workspace`, checked, or the one kept for (`dev`, current stream): made on the first call, which must
        not be captured, and made anew when it is smaller than `need` asks for (one buffer per stream, grown to the largest)."""
        nbytes = self.nbytes(*(need or ()))
        if workspace is not None:
            if not (workspace.is_cuda and workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous()
                    and workspace.numel() >= nbytes):
                raise RuntimeError(f"{who}: workspace must come from {self.maker}() on the {self.on} device")
            return workspace
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        ws = self.kept.get(key)
        if ws is None or ws.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():    # (torch.zeros inside a capture would become part of the graph)
                raise RuntimeError(f"{who}: {self.first} on this stream happens inside a graph capture; call it once eagerly on the "
                                   f"stream first, or pass workspace={self.maker}({self.maker_args})")
            ws = self.kept[key] = self.fresh(dev, *(need or ()))
        return ws
