"""bench.py --dump-outputs: the timed path's last step written out as float32 .npy files, the same from run to run.
On the CPU through FR_BENCH_STUB=1 (the control flow and the files), on the GPU against the CPU oracle (the arrays are
what the timed frames computed, whichever way they were replayed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=300):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_stub_dump_is_float32_and_repeats(tmp_path):
    runs = []
    for k, steps in enumerate((3, 3, 5)):
        d = str(tmp_path / f"run{k}")
        j = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", d], {"FR_BENCH_STUB": "1"})
        assert j["steps"] == steps and j["ms_per_step"] > 0
        assert j["dumped_outputs"] == {"dir": d, "view": 0, "fraction_kept": 1.0}
        runs.append(_load(d))
    assert list(runs[0]) == ["flat_grad"] and runs[0]["flat_grad"].dtype == np.float32
    # same arguments, same files; the stub's gradient carries the index of the frame, so it is the LAST step's
    assert np.array_equal(runs[0]["flat_grad"], runs[1]["flat_grad"])
    assert not np.array_equal(runs[0]["flat_grad"], runs[2]["flat_grad"])


def test_dump_refuses_what_it_does_not_cover():
    env = dict(os.environ, FR_BENCH_STUB="1")
    for args in (["--gpus", "2", "--dump-outputs", "x"], ["--steps", "0"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "error" in r.stderr, (args, r.stderr[-500:])


def test_write_outputs_keeps_a_fixed_sample_under_the_limit(tmp_path):
    """(in a child process: importing bench.py sets ROCm runtime switches for the process)"""
    code = (
        "import os, sys, numpy as np\n"
        "sys.path.insert(0, sys.argv[1])\n"
        "import bench\n"
        "a = {'big': np.arange(3_000_000, dtype=np.float64).reshape(1000, 1000, 3), 'small': np.arange(10, dtype=np.int32)}\n"
        "for d in ('a', 'b'):\n"
        "    print(bench.write_outputs(os.path.join(sys.argv[2], d), a, limit=4_000_000))\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    frac = float(r.stdout.split()[0])
    assert 0.3 < frac < 0.34
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 4_000_000
    for k in ("big", "small"):
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k])
    big = a["big"]
    assert big.ndim == 1 and big.size == int(3_000_000 * frac) and (np.diff(big) > 0).all()   # sorted positions, no repeats
    assert big.max() < 3_000_000 and a["small"].size == int(10 * frac)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [["--in-flight", "1", "--chains", "off"], ["--in-flight", "0", "--chains", "2x1"],
                                  ["--in-flight", "1", "--no-graph"]], ids=["view_graph", "launch_chain", "eager"])
def test_dump_matches_the_oracle(gpu_device, tmp_path, mode):
    import torch

    from fateavatar_amd import scenes
    from fateavatar_amd.model import FlatGaussians
    from oracle import oracle

    P, res = 5000, 128
    d = str(tmp_path / "out")
    j = _bench(["--gpus", "1", "--steps", "4", "--warmup", "2", "--P", str(P), "--res", str(res), "--rounds", "1",
                "--cpu-seconds", "0", "--no-dp-reference", "--no-opaque", "--no-coherent", "--no-runtime-defaults",
                "--no-config5", "--dump-outputs", d] + mode, timeout=600)
    assert j["steps"] == 4 and j["ms_per_step"] > 0 and j["dumped_outputs"]["fraction_kept"] == 1.0
    if "--chains" in mode and mode[mode.index("--chains") + 1] == "2x1":
        assert j["config"]["launch_chains_in_flight"] == {"chains": 1, "views_per_chain": 2}
    got = _load(d)
    assert sorted(got) == sorted(["render", "radii", "dL_dmeans2D", "grad_xyz", "grad_features", "grad_opacity",
                                  "grad_scaling", "grad_rotation"])
    assert all(a.dtype == np.float32 for a in got.values())

    # bench.py's view 0: the frontal camera of head_scene, its fixed upstream gradient
    s = scenes.head_scene(P=P, res=res, sh_degree=3, seed=0)
    pc = FlatGaussians(s.means3D, s.shs, s.opacities, s.scales, s.rotations, s.sh_degree, torch.device("cpu"))
    g = ((torch.rand((3, res, res), generator=torch.Generator().manual_seed(1)) < 0.5).float() * 2 - 1) / (3 * res * res)
    c = s.camera
    f = oracle.forward(bg=s.bg, viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, campos=c.camera_center,
                       tanfovx=c.tanfovx, tanfovy=c.tanfovy, H=res, W=res, sh_degree=s.sh_degree,
                       means3D=pc.get_xyz.detach().numpy(), opacities=pc.get_opacity.detach().numpy(),
                       scales=pc.get_scaling.detach().numpy(), rotations=pc.get_rotation.detach().numpy(),
                       shs=pc.get_features.detach().numpy())
    b = oracle.backward(f, g.numpy())
    assert got["render"].shape == f.color.shape
    assert np.mean(np.abs(got["render"] - f.color) <= 1e-5 + 1e-4 * np.abs(f.color)) >= 0.9999
    assert np.array_equal(got["radii"], f.radii.astype(np.float32)) and (f.radii > 0).sum() > 100
    # the raw parameters' gradients: the oracle's (activated) ones through sigmoid / exp / normalize.  The scene's
    # Gaussians are isotropic, so turning one changes nothing: its rotation gradient is 0 (the floor of the bound)
    op, sc = pc.get_opacity.detach().numpy().astype(np.float64), pc.get_scaling.detach().numpy().astype(np.float64)
    q = pc._rotation.detach().numpy().astype(np.float64)
    qn = np.linalg.norm(q, axis=1, keepdims=True)
    dq = b.dL_drotations.astype(np.float64)
    d_rot = (dq - q / qn * (q / qn * dq).sum(1, keepdims=True)) / qn
    floor = 1e-3 * np.linalg.norm(b.dL_dmeans3D)
    for name, ref in (("dL_dmeans2D", b.dL_dmeans2D), ("grad_xyz", b.dL_dmeans3D), ("grad_features", b.dL_dsh),
                      ("grad_opacity", b.dL_dopacity * op * (1 - op)), ("grad_scaling", b.dL_dscales * sc),
                      ("grad_rotation", d_rot)):
        assert got[name].shape == ref.shape and np.isfinite(got[name]).all(), name
        err = np.linalg.norm(got[name] - ref) / max(np.linalg.norm(ref), floor)
        assert err < 1e-4, (name, err)
