"""bench.py's plain run: the headline line alone (the extra measurements wait for --full), exactly --steps timed steps, and
--dump-outputs writing what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench(*args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_options_are_listed():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    batch, steps = 1 << 16, 3
    line = _bench("--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(batch), "--dump-outputs", str(tmp_path))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(batch * 1e3 / line["ms_per_step"], rel=1e-6)
    assert "other_configs" not in line and "cpu_baseline" not in line and line["no_settle_run"] is None
    out, loss, params = (np.load(tmp_path / f"{n}.npy") for n in ("output", "loss", "params"))
    assert out.dtype == np.float32 and out.shape == (batch, 3) and np.isfinite(out).all()
    assert loss.dtype == np.float64 and loss.shape == (1,) and loss[0] == pytest.approx(line["config"]["loss_first_last"][1])
    assert params.dtype == np.float32 and params.size > 0 and np.isfinite(params).all()
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20
