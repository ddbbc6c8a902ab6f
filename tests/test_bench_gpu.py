"""A plain `bench.py` run end to end on a small workload: one JSON line without the --full measurements, and the outputs of
its last timed step under --dump-outputs, the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--trunk", "resnet-50", "--size", "128", "--batch", "2", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_bench_dumps_the_last_step(tmp_path):
    out = _run(tmp_path / "a")
    assert out["metric"] == "train images/sec" and out["unit"] == "images/sec" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0 and abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) < 0.01 * out["value"]
    assert out["roofline"] is None and out["cpu_baseline"] is None          # --full only
    assert sorted(os.listdir(tmp_path / "a")) == ["loss.npy", "state_sample.npy"]
    loss, state = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "state_sample.npy")
    assert loss.dtype == np.float32 and abs(float(loss) - out["config"]["final_loss"]) < 1e-4
    assert state.dtype == np.float32 and state.ndim == 1 and state.size > 0 and np.isfinite(state).all()

    _run(tmp_path / "b")                # same arguments: same inputs and perturbation draws, same outputs
    for name in ("loss.npy", "state_sample.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)), name
