"""bench.py without --full: the same timed frames as a full run, and nothing measured beside them."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what only --full measures (null in a plain run's line)
FULL_ONLY = ("roofline", "roofline_config5", "cpu_baseline", "stage_us", "stage_frac", "stage_frac_required",
             "one_frame_at_a_time", "runtime_defaults", "scaling_reference", "dp_reference_at_1", "opaque",
             "coherent_layout", "batched_views", "frame_roofline")


def _bench(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(lines[0])


def test_stub_plain_line_has_every_field():
    j = _bench(["--steps", "3", "--warmup", "1"], {"FR_BENCH_STUB": "1"})
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step") + FULL_ONLY:
        assert k in j
    assert all(j[k] is None for k in FULL_ONLY)


@pytest.mark.gpu
def test_plain_run_times_the_frames_of_a_full_run_and_nothing_else(gpu_device):
    common = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--P", "5000", "--res", "128", "--rounds", "1",
              "--in-flight", "0", "--chains", "2x1"]
    plain = _bench(common)
    full = _bench(common + ["--full", "--cpu-seconds", "0", "--no-dp-reference", "--no-opaque", "--no-coherent",
                            "--no-runtime-defaults", "--no-config5"])
    for j in (plain, full):
        assert j["steps"] == 4 and j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "frames/s"
        assert j["config"]["launch_chains_in_flight"] == {"chains": 1, "views_per_chain": 2}
    # view 0's counts: read from its last timed frame (plain) or from an eager frame after the profiled ones (full)
    for k in ("num_rendered", "tile_instances_8x8", "max_tile_list"):
        assert plain["config"][k] == full["config"][k] > 0, k
    assert all(plain[k] is None for k in FULL_ONLY)
    assert full["stage_us"] and full["roofline"] and full["roofline"]["launches"] > 0 and full["batched_views"]
