"""bench.py's command line: a plain run measures and reports the headline only,
``--full`` adds the measurements that take runs of their own, and
``--dump-outputs DIR`` writes the last timed step's outputs -- the same from run
to run, because the timed steps start from the state the warm-up left whatever
the time-sized soak did."""
import json
import os

import numpy as np
import pytest

import bench

TINY = ["--gpus", "1", "--config", "c2", "--dim", "192", "--batch", "96", "--steps", "3", "--warmup", "2"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("step_spread", "roofline", "roofline_encoder_gemm", "cpu_baseline")


def test_options_default_to_a_plain_run():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_save_outputs_writes_float32_npy(tmp_path):
    d = str(tmp_path / "new" / "dir")
    bench.save_outputs(d, {"a": np.arange(6, dtype=np.float64).reshape(2, 3), "b": np.float32(2.5)})
    assert sorted(os.listdir(d)) == ["a.npy", "b.npy"]
    a = np.load(os.path.join(d, "a.npy"))
    assert a.dtype == np.float32 and a.shape == (2, 3) and a[1, 2] == 5.0
    assert np.load(os.path.join(d, "b.npy")).dtype == np.float32


def _run(capsys, extra):
    bench.run(bench.parse_args(TINY + extra))
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_reports_headline_and_dumps_reproducible_outputs(capsys, tmp_path):
    dirs = [str(tmp_path / n) for n in ("a", "b")]
    # different soak lengths: the timed steps must not see them
    res = [_run(capsys, ["--soak-s", s, "--dump-outputs", d]) for s, d in zip(("0", "0.05"), dirs)]
    for r in res:
        assert all(k in r for k in HEADLINE) and not any(k in r for k in FULL_ONLY)
        assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["dtype"] == "bf16"
        assert r["value"] == pytest.approx(96 * 1e3 / r["ms_per_step"], rel=1e-3)
    assert res[1]["soak_steps"] > 0 == res[0]["soak_steps"]
    assert res[0]["final_loss"] == res[1]["final_loss"]
    names = sorted(os.listdir(dirs[0]))
    assert names == ["adam_exp_avg.npy", "adam_exp_avg_sq.npy", "bn_running.npy", "loss.npy", "params.npy"]
    total = 0
    for n in names:
        a, b = (np.load(os.path.join(d, n)) for d in dirs)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0, n
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(os.path.join(dirs[0], "loss.npy"))[0]) == res[0]["final_loss"]


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements(capsys):
    r = _run(capsys, ["--soak-s", "0", "--full", "--cpu-budget", "0.2"])
    assert all(k in r for k in HEADLINE + FULL_ONLY)
    assert r["step_spread"]["steps"] == 3 and r["roofline"]["launches_timed"] == 3
