"""bench.py's plain run: the contract's keys and nothing of what --full adds, and --dump-outputs writes the last timed
step's results - the same values as the line's `result`, the same files from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--rows", "3000", "--dim", "64", "--dump-outputs", str(out_dir)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_result(tmp_path):
    first, second = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in first, key
    assert first["steps"] == 3 and first["unit"] == "embeddings/s" and first["higher_is_better"] is True
    assert first["value"] == pytest.approx(2 * 3000 / (first["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("roofline", "variants", "result_check", "process_cold", "cpu_baseline", "warm", "first_call", "filter"):
        assert key not in first, key
    names = sorted(first["result"])
    for run in ("a", "b"):
        assert sorted(os.listdir(tmp_path / run)) == [f"{name}.npy" for name in names], run
    for name in names:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and float(a) == first["result"][name], name
        assert np.array_equal(a, b), name                 # same arguments -> same inputs -> same outputs
    assert first["result"] == second["result"]
