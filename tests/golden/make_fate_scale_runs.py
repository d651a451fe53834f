"""Generate tests/golden/reference_fate_scale.npz: runs of the reference's OWN `FateAvatarLoss.accumulate_gradients` for its
scale term (train/loss.py:144-151), recorded as plain data in the layout of tests/golden/make_reference_runs.py (its docstring
has it; tests/reference_runs.py loads this file with the rest).

Runs ONLY in the build container (needs /root/reference); no test imports this file.  Run as

    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_fate_scale_runs.py            (writes the fixture)
    PYTHONDONTWRITEBYTECODE=1 python -B tests/golden/make_fate_scale_runs.py --check    (compares a fresh run with the committed one)

The method is called unmodified, on the CPU, in float32 and in float64, by the committed generator's means (imported from it:
its appended stand-in modules for lpips / pytorch3d / torchvision, `bare` = `__new__` + `nn.Module.__init__` with only `params`,
`l1_loss` and `l2_loss`, `leaf`, `both`, `record`).  vgg_weight = lpips_weight = laplacian_weight = 0; rgb_weight, scale_weight
and scale_threshold are config/fateavatar.yaml's.  None of the reference's text is in this file.

Recorded per case: `scale_loss` (out['scale_loss'], unweighted) and `d_scaling`, the gradient of out['loss'] — rgb_weight x L1 of
two constant images, which does not depend on the scales, + scale_weight x scale_loss — with respect to a `_scaling` leaf, with
model_outputs['scale'] = exp(_scaling).  Margins (conditions on the inputs, asserted here on the float64 of the float32 inputs):
every row's |ratio / threshold - 1| >= 1e-2, and in every row over the threshold the two largest and the two smallest activated
components differ by >= 1e-3 relative (no tie calls).  The seed is re-drawn until the inputs meet them."""
import importlib.util
import math
import os
import sys

import numpy as np
import torch
import yaml

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_reference_runs", os.path.join(OUT, "make_reference_runs.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)          # (the reference on sys.path, the stand-ins appended, train.loss imported as base.ref_loss)

from tests import fate_scale_ref  # noqa: E402

FILE = "reference_fate_scale.npz"
P_ROWS, SEED = 257, 311
GATE_MARGIN, TIE_MARGIN = 1e-2, 1e-3


def configured():
    with open(os.path.join(base.REF, "config", "fateavatar.yaml")) as f:
        loss = yaml.safe_load(f)["loss"]
    w = loss["weight"]
    thr = loss["scale_threshold"] if "scale_threshold" in loss else w["scale_threshold"]
    return base.ref_loss.FateAvatarLoss.Params(rgb_weight=w["rgb_loss"], scale_weight=w["scale_loss"], scale_threshold=thr,
                                               vgg_weight=0.0, lpips_weight=0.0, laplacian_weight=0.0)


def case(out, name, s, params, expect_zero):
    gate, tie = fate_scale_ref.margins(s, params.scale_threshold)
    assert gate >= GATE_MARGIN and tie >= TIE_MARGIN, (name, gate, tie)
    out[f"{name}_margin_ratio"] = np.float64(gate)
    if math.isfinite(tie):
        out[f"{name}_margin_tie"] = np.float64(tie)
    img, gt = torch.full((1, 3, 2, 2), 0.25), torch.full((1, 3, 2, 2), 0.5)

    def run(dt):
        L = base.bare(base.ref_loss.FateAvatarLoss, params=params, l1_loss=torch.nn.L1Loss(reduction="mean"),
                      l2_loss=torch.nn.MSELoss(reduction="mean"))
        raw = base.leaf(s, dt)
        o = L.accumulate_gradients({"rgb_image": img.to(dt), "scale": torch.exp(raw)}, {"rgb": gt.to(dt)})
        assert sorted(o) == ["loss", "rgb_loss", "scale_loss"], sorted(o)
        (g,) = torch.autograd.grad(o["loss"], raw)
        return dict(scale_loss=o["scale_loss"].detach(), d_scaling=g)

    r32, r64 = base.both(run)
    zero = float(r64["scale_loss"]) == 0 and int(r64["d_scaling"].count_nonzero()) == 0
    assert zero == expect_zero, name
    base.record(out, name, dict(scaling=s), r32, r64,
                dict(rgb_weight=params.rgb_weight, scale_weight=params.scale_weight, scale_threshold=params.scale_threshold))


def main(check):
    params = configured()
    assert params.scale_weight > 0 and params.scale_threshold > 1
    out = {}
    for attempt in range(100):          # re-draw until the inputs alone meet the margins
        gen = torch.Generator().manual_seed(SEED + 1009 * attempt)
        mixed = fate_scale_ref.draw_scaling(P_ROWS, gen, params.scale_threshold, over=0.5)
        none = fate_scale_ref.draw_scaling(P_ROWS, gen, params.scale_threshold, over=0.0)
        ok = all(g >= GATE_MARGIN and t >= TIE_MARGIN for g, t in (fate_scale_ref.margins(x, params.scale_threshold) for x in (mixed, none)))
        if ok:
            break
    else:
        raise AssertionError("no seed keeps the rows clear of the threshold and of ties")
    scale = torch.exp(mixed.double())
    n_over = int((scale.max(1).values / scale.min(1).values > params.scale_threshold).sum())
    assert 0.35 * P_ROWS <= n_over <= 0.65 * P_ROWS, n_over
    case(out, "fatescale_mixed", mixed, params, expect_zero=False)
    case(out, "fatescale_none", none, params, expect_zero=True)
    # model/fateavatar.py:176: one starting log-scale on all three axes of every row
    case(out, "fatescale_init", torch.full((P_ROWS, 3), float(np.float32(math.log(3e-3)))), params, expect_zero=True)
    notes = (f"fatescale_*: FateAvatarLoss.accumulate_gradients with config/fateavatar.yaml's rgb / scale weights and scale_threshold, "
             f"every other weight 0, on two constant 2x2 images (the L1 term does not depend on the scales); seed attempt {attempt + 1}; "
             f"fatescale_mixed has {n_over} of {P_ROWS} rows over the threshold; d_scaling is the gradient of out['loss'] (scale_weight "
             "applied); fatescale_none and fatescale_init are exactly zero (their e32 is the plain norm of the float32 run)")
    path = os.path.join(OUT, FILE)
    if check:
        with np.load(path) as have:
            assert sorted(have.files) == sorted(list(out) + ["notes"]), FILE
            same = all(np.array_equal(have[k], out[k]) for k in out)
        print(f"{FILE}: {'identical arrays' if same else 'DIFFERS'}")
        assert same, FILE
        return
    np.savez_compressed(path, notes=np.array(notes), **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size <= 100_000, (path, size)


if __name__ == "__main__":
    main(check="--check" in sys.argv[1:])
