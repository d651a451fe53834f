"""Fuzz campaign: random scene configurations, HIP vs oracle (forward state, image, gradients).  GPU box.
    python tools/fuzz_parity.py N SEED [big|huge]   (FR_FUZZ_ONLY=k: only iteration k; FR_FUZZ_CAMERA=1: random look-at cameras; FR_FUZZ_INPUTS=1: colors_precomp / cov3D_precomp / scale_modifier drawn per case; huge: 60 k - 400 k Gaussians, 512 - 1400 pixels a side)
FR_FUZZ_BATCH=K: iterations K g .. K g + K - 1 are rendered as ONE batch (tests/util.HipBatch: fr_forward_batch /
fr_backward_batch, every view's gradient through the batched backward) and every view is held to the same checks; iteration
numbers are the stream's, so FR_FUZZ_ONLY=k runs the group that holds k and reports case k.
The configurations come from tests/util.fuzz_stream; a failing iteration k is replayed with tools/diag/fuzz_replay.py /
fuzz_bisect.py and pinned in tests/test_gpu_configs.py (test_fuzz_regression_*)."""
import itertools
import os
import sys
import traceback

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fateavatar_amd import rasterizer, scenes  # noqa: E402
from tests import util  # noqa: E402
from tests.test_gpu_parity import _check_backward_capped, _check_forward  # noqa: E402

dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1234
big = ("huge" if sys.argv[3] == "huge" else True) if len(sys.argv) > 3 else False
bad = 0
kinds = {}
batch = int(os.environ.get("FR_FUZZ_BATCH", "0"))


def views_of(case):
    it, P, H, W, kw, dpix, name = case
    s = scenes.random_scene(P, H, W, **kw)
    if os.environ.get("FR_FUZZ_CAMERA"):   # a random look-at camera instead of the identity view (util.fuzz_camera)
        s.camera = util.fuzz_camera(seed, it, H, W)
    extra = util.fuzz_inputs(seed, it, s) if os.environ.get("FR_FUZZ_INPUTS") else {}   # the API's optional inputs, drawn per case
    name += (" inputs=" + ",".join(sorted(extra))) if extra else ""
    return s, extra, name


def check(it, s, extra, h, dpix, name):
    global bad
    try:
        o = util.oracle_forward(s, **extra)
        _check_forward(o, h, name)
        # (as tests/test_gpu_configs.py: at most 5 % of the rows exempt by threshold flips, else the flips are masked out of
        # dL/dpixel and no row is exempt; aggregate bound 1e-4 for every scene)
        _check_backward_capped(o, h, dpix, name, max_skip_frac=0.05)
        print("ok  ", name, "inst", h.counts.num_instances, "maxlist", h.counts.max_tile_list, flush=True)
    except Exception as e:
        bad += 1
        kind = "skipped-row bound" if "exempt too many rows" in repr(e) else "PARITY"
        kinds[kind] = kinds.get(kind, 0) + 1
        print("FAIL", kind, name, repr(e)[:300], flush=True)
        traceback.print_exc(limit=2)


only = int(os.environ["FR_FUZZ_ONLY"]) if os.environ.get("FR_FUZZ_ONLY") else None
cases = itertools.islice(util.fuzz_stream(seed, big), n)
if batch:
    # groups of `batch` consecutive iterations, every group one fr_forward_batch / fr_backward_batch
    while True:
        group = list(itertools.islice(cases, batch))
        if not group:
            break
        if only is not None and only not in [c[0] for c in group]:
            continue
        if os.environ.get("FR_FUZZ_PRINT_KW"):
            for it, P, H, W, kw, _dpix, _name in group:
                print("kw", it, dict(P=P, H=H, W=W, **kw), flush=True)
        # (a capacity guess of one big group, times K views, for every later group: start each group from none instead)
        rasterizer._capacity_hint.clear()
        try:
            vs = [views_of(c) for c in group]
            b = util.HipBatch([v[0] for v in vs], dev, per_view_kwargs=[v[1] for v in vs])
        except Exception as e:
            if "(code 3)" in str(e):   # FR_ERR_HIP: the device is in an unknown state, nothing more is launched on it
                raise
            bad += len(group)
            kinds["BATCH"] = kinds.get("BATCH", 0) + len(group)
            print("FAIL", "BATCH", [c[0] for c in group], repr(e)[:300], flush=True)
            continue
        for c, (s, extra, name), h in zip(group, vs, b):
            if only is None or c[0] == only:
                check(c[0], s, extra, h, c[5], f"{name} [batch of {len(group)}, view {c[0] - group[0][0]}]")
else:
    for it, P, H, W, kw, dpix, name in cases:
        if only is not None and it != only:
            continue
        if os.environ.get("FR_FUZZ_PRINT_KW"):
            print("kw", it, dict(P=P, H=H, W=W, **kw), flush=True)
        try:
            s, extra, name = views_of((it, P, H, W, kw, dpix, name))
            h = util.HipFrame(s, dev, **extra)
        except Exception as e:
            if "(code 3)" in str(e):
                raise
            bad += 1
            kinds["PARITY"] = kinds.get("PARITY", 0) + 1
            print("FAIL", "PARITY", name, repr(e)[:300], flush=True)
            continue
        check(it, s, extra, h, dpix, name)
print("failures:", bad, kinds)
