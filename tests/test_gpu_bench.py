"""bench.py as the measurement runs call it: a plain run does the timed workload and prints its result line, nothing more; --steps
sets the number of timed steps; --dump-outputs writes what the last timed step returned, the same rewards from run to run; --full
keeps everything else the benchmark measures (here: the dominant-kernel roofline probe and the legs file)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2"] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert lines and lines[-1].startswith("{") and len(lines[-1]) <= 4096
    return lines, json.loads(lines[-1])


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    lines, res = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["higher_is_better"] is True
    assert res["unit"] == "reward-pairs/sec" and res["dtype"] == "f16" and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(2 * 1e3 / res["ms_per_step"], rel=1e-3)        # B = 2 rows per timed step
    # nothing beyond the headline: no golden sweep, no legs, no CPU baseline, no dominant-kernel probe, no legs file
    assert not any(l.startswith("#leg") for l in lines)
    assert "parity_check" not in res and "cpu_baseline" not in res and "legs" not in res and res["legs_file"] is None
    assert res["roofline"]["kernel_ms"] is None and res["roofline"]["whole_pass_frac"] > 0
    got = np.load(tmp_path / "a" / "rewards.npy")
    assert got.dtype == np.float32 and got.shape == (2, 1) and np.isfinite(got).all()
    assert sorted(os.listdir(tmp_path / "a")) == ["rewards.npy"]
    # same arguments but the step counts -> same inputs, same rewards
    _, res1 = _bench("--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "b"))
    assert res1["steps"] == 1 and res1["warmup"] == 0
    assert np.array_equal(np.load(tmp_path / "b" / "rewards.npy"), got)


def test_full_run_keeps_the_roofline_probe_and_the_legs_file():
    lines, res = _bench("--steps", "1", "--warmup", "1", "--full", "--quick")
    assert any(l.startswith("#leg roofline ") for l in lines)
    rf = res["roofline"]
    assert rf["kernel_ms"] > 0 and rf["vendor_plain_gemm_ms"] > 0 and rf["kernel"].startswith("gemm_bt8_kernel")
    assert res["legs_file"] and os.path.exists(os.path.join(ROOT, res["legs_file"]))

