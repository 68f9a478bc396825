"""bench.py on a real GPU: a plain run times exactly --steps steps and carries the headline only; --full adds the other measurements;
--dump-outputs writes what the last timed step returned, the same numbers in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rays", "1024", "--warmup", "1"] + list(flags)
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only_and_its_dumped_outputs_reproduce(tmp_path):
    runs = [_run("--steps", "3", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for j in runs:
        assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["dtype"] == "bf16"
        assert j["unit"] == "rays/s" and j["higher_is_better"] is True
        assert abs(j["value"] - 1024 * 1e3 / j["ms_per_step"]) <= 1e-3 * j["value"]
        assert j["kernels"] == {} and j["roofline"] is None and j["balanced"] is None and j["cpu_baseline"] is None
        assert j["config"]["eager_ms_per_step"] is None and j["config"]["runner_loop_ms_per_step"] is None
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert {"loss.npy", "rgb.npy", "depth.npy", "params.npy", "grad.npy"} <= set(names)
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64e6 + 256 * len(names)       # (+ the .npy headers)
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
    assert abs(float(np.load(tmp_path / "a" / "loss.npy")) - runs[0]["config"]["loss"]) <= 1e-6
    assert np.load(tmp_path / "a" / "rgb.npy").shape == (1024, 3)


def test_full_run_adds_the_other_measurements():
    j = _run("--steps", "3", "--full", "--no-cpu-baseline")
    assert j["steps"] == 3 and j["ms_per_step"] > 0
    assert j["config"]["eager_ms_per_step"] > 0 and j["config"]["runner_loop_ms_per_step"] > 0
    assert {"expert_fwd", "expert_bwd", "expert_wgrad"} <= set(j["kernels"]) and j["roofline"]["bound"] in ("hbm", "mfma")
    assert j["balanced"]["value"] > 0 and j["config"]["balanced_value"] == j["balanced"]["value"]
