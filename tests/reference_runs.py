"""TEST HELPER — the recorded runs of the reference's own Python (tests/golden/reference_*.npz, written by
tests/golden/make_reference_runs.py, whose docstring has the layout): one dictionary of all files, and a view of one case.
Reads tests/golden/ only."""
import functools
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -24            # one float32 rounding, relative


@functools.lru_cache(maxsize=None)
def everything():
    """{key: numpy array} of every reference_*.npz (the keys are unique across the files), and the files' notes."""
    arrays, notes = {}, []
    paths = sorted(glob.glob(os.path.join(GOLDEN, "reference_*.npz")))
    assert paths, "tests/golden/reference_*.npz are missing"
    for path in paths:
        with np.load(path) as z:
            for k in z.files:
                if k == "notes":
                    notes.append(str(z[k]))
                    continue
                assert k not in arrays, (k, path)
                arrays[k] = z[k]
    return arrays, "\n".join(notes)


class Case:
    """One recorded case: `inp(name)` an input (float32 / integer tensor, a copy), `out(name)` the reference's float64 result,
    `e32(name)` the reference's own float32 error on it, `param(name)` a field of the reference's Params, `scalar(name)` any
    other recorded number (a margin, a yardstick)."""

    def __init__(self, name, inputs_of=None):
        self.name, self.inputs_of = name, inputs_of or name
        self.arrays = everything()[0]
        assert any(k.startswith(name + "_") for k in self.arrays), name

    def has(self, name):
        return f"{self.name}_in_{name}" in self.arrays or f"{self.inputs_of}_in_{name}" in self.arrays

    def inp(self, name):
        own = f"{self.name}_in_{name}"
        a = self.arrays[own if own in self.arrays else f"{self.inputs_of}_in_{name}"]
        assert a.dtype in (np.float32, np.int32, np.int64), (name, a.dtype)
        return torch.from_numpy(a.copy())

    def out(self, name):
        a = self.arrays[f"{self.name}_{name}"]
        return torch.from_numpy(np.asarray(a, dtype=np.float64).copy())

    def e32(self, name):
        return float(self.arrays[f"{self.name}_{name}_e32"])

    def param(self, name):
        return float(self.arrays[f"{self.name}_param_{name}"])

    def scalar(self, name):
        return float(self.arrays[f"{self.name}_{name}"])

    def outputs(self):
        head = self.name + "_"
        return [k[len(head):-4] for k in self.arrays if k.startswith(head) and k.endswith("_e32")]


def rel(got, want):
    """rel-L2 of `got` against the float64 `want` (a scalar: the relative difference); a zero truth takes the plain norm."""
    got, want = torch.as_tensor(got).detach().cpu().double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    n = float(want.norm())
    return float((got - want).norm()) / n if n > 0 else float((got - want).norm())


def float32_allowance(case, name, factor=4.0):
    """`factor` x the recorded e32 of an output.  A loss word is ONE float: its e32 is a draw between nothing and a few
    roundings, not a scale (tests/test_gpu_splatting_loss.py), so for a scalar e32 counts as no less than one float32 rounding."""
    e = case.e32(name)
    return factor * (max(e, EPS) if case.out(name).numel() == 1 else e)
