"""bench.py's command line and its --dump-outputs writer, without a GPU (the end-to-end run is tests/test_bench_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_by_default_full_on_request():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--steps", "3", "--full", "--dump-outputs", "out", "--dump-convs", "c.json"])
    assert a.full and a.dump_outputs == "out" and a.dump_convs == "c.json"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--dump-convs", "c.json"], ["--dump-launches", "l.json"]])
def test_rejected_command_lines(argv):
    import bench
    with pytest.raises(SystemExit) as e:
        bench.parse(argv)
    assert e.value.code == 2


def test_output_arrays_are_a_fixed_float32_sample(tmp_path):
    import bench
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(64, 128, 3), torch.nn.BatchNorm2d(128))     # 73 728 weights > DUMP_SAMPLE
    loss = torch.tensor(2.5, dtype=torch.float64)
    a, b = bench.output_arrays(m, loss), bench.output_arrays(m, loss)
    assert set(a) == {"loss", "state_sample"}
    assert a["loss"].dtype == np.float32 and a["loss"].shape == () and a["loss"] == 2.5
    # conv weight sampled, conv bias + BN weight / bias / running mean / running var whole, num_batches_tracked skipped
    assert a["state_sample"].dtype == np.float32 and a["state_sample"].shape == (bench.DUMP_SAMPLE + 5 * 128,)
    assert np.array_equal(a["state_sample"], b["state_sample"])
    w = m[0].weight.detach().reshape(-1)
    assert np.isin(a["state_sample"][:bench.DUMP_SAMPLE], w.numpy()).all()
    assert np.array_equal(a["state_sample"][bench.DUMP_SAMPLE:bench.DUMP_SAMPLE + 128], m[0].bias.detach().numpy())

    bench.write_outputs(str(tmp_path / "out"), a)
    assert sorted(os.listdir(tmp_path / "out")) == ["loss.npy", "state_sample.npy"]
    assert np.array_equal(np.load(tmp_path / "out" / "state_sample.npy"), a["state_sample"])
    with pytest.raises(SystemExit):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT // 4 + 1, np.float32)})
    assert not os.path.exists(tmp_path / "big")
