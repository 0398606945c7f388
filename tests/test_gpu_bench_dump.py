"""bench.py's plain run and `--dump-outputs` on the device, in-process on a c2 problem cut to
1024 rows per worker (8 workers x 1024 x 1024 fp32, nwait = n: every kernel deterministic):

  * a plain run carries the headline keys and none of the `--full` measurements;
  * two runs with the same arguments write the same x / recvbuf / repochs, bit for bit;
  * `--steps` sets the number of timed epochs: the dump of a run one step shorter is the
    iterate before the last update, and x_5 = x_4 - eta * sum_i recvbuf_i of the longer run;
  * x after 5 epochs against the fp64 numpy descent on the oracle's inputs (oracle/lsq.py).
"""
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, WARMUP, STEPS, SEED = 8 * 1024, 2, 3, 1234


@pytest.fixture(scope="module")
def bench_mod(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import bench
    return bench


def _run(bench, monkeypatch, capsys, out, steps, extra=()):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(WARMUP),
                                      "--seed", str(SEED), "--dump-outputs", str(out)] + list(extra))
    args = bench.parse()
    cfg = dict(bench.CONFIGS["c2"], config="c2", rows=ROWS)
    capsys.readouterr()
    bench.run_single(args, cfg)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {k: np.load(out / (k + ".npy")) for k in ("x", "recvbuf", "repochs")}


@pytest.fixture(scope="module")
def reference():
    """fp64 descent on the oracle's copy of the inputs: x after WARMUP + STEPS full-gradient
    epochs from x = 0 (nwait = n: every worker fresh, weight n / n = 1)."""
    import bench
    import lsq
    cols = bench.CONFIGS["c2"]["cols"]
    A = lsq.gen_matrix(SEED, 0, ROWS, cols, "f32").astype(np.float64)
    b = lsq.gen_vector(SEED, 0, ROWS, "f32").astype(np.float64)
    eta = bench.step_size(ROWS, cols)
    x = np.zeros(cols)
    for _ in range(WARMUP + STEPS):
        x = x - eta * (A.T @ (A @ x - b))
    return x


def test_plain_run_dumps_reproducible_outputs(bench_mod, monkeypatch, capsys, tmp_path, reference):
    bench = bench_mod
    n, cols = bench.CONFIGS["c2"]["workers"], bench.CONFIGS["c2"]["cols"]
    line, a = _run(bench, monkeypatch, capsys, tmp_path / "a", STEPS)
    # the headline keys, and nothing that takes a run of its own
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == STEPS and line["ms_per_step"] > 0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert "python_loop_it_per_s" not in line and line["cpu_baseline"] is None
    assert "measured_read_peak" not in line["roofline"]
    assert a["x"].dtype == np.float32 and a["x"].shape == (cols,)
    assert a["recvbuf"].dtype == np.float32 and a["recvbuf"].shape == (n * cols,)
    assert a["repochs"].dtype == np.float64 and a["repochs"].tolist() == [WARMUP + STEPS] * n
    # same arguments, same outputs
    _, b = _run(bench, monkeypatch, capsys, tmp_path / "b", STEPS)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    # one timed step fewer: the iterate the last epoch's gradients (recvbuf of `a`) were taken
    # at; the device update is fp32: x - eta * (sum of n gradients), a few roundings each
    _, c = _run(bench, monkeypatch, capsys, tmp_path / "c", STEPS - 1)
    assert c["repochs"].tolist() == [WARMUP + STEPS - 1] * n
    eta = bench.step_size(ROWS, cols)
    g = a["recvbuf"].astype(np.float64).reshape(n, cols)
    want = c["x"].astype(np.float64) - eta * g.sum(axis=0)
    slack = (n + 3) * 2.0 ** -24 * (np.abs(c["x"]).astype(np.float64) + eta * np.abs(g).sum(axis=0))
    assert np.all(np.abs(a["x"] - want) <= slack), float(np.max(np.abs(a["x"] - want) - slack))
    # against fp64: each epoch's gradient is within the kernel's 1e-5 (BASELINE north_star) and
    # the step 0.9 / L does not amplify an earlier epoch's error, so 1e-5 per epoch
    import lsq
    err = lsq.rel_err(a["x"], reference)
    print("x rel err vs fp64 after %d epochs: %.3g" % (WARMUP + STEPS, err))
    assert err <= 1e-5 * (WARMUP + STEPS), err


def test_full_run_keeps_its_measurements(bench_mod, monkeypatch, capsys, tmp_path):
    """--full: the Python-driven loop and the measured read ceiling are back in the line (the
    CPU baseline, a 12 s sample of the full problem, is left out here)."""
    line, d = _run(bench_mod, monkeypatch, capsys, tmp_path / "f", STEPS, ["--full", "--no-cpu-baseline"])
    assert line["python_loop_it_per_s"] > 0 and "python loop beside it" in line["loop"]
    r = line["roofline"]
    assert r["measured_read_peak"] > 0 and r["frac_of_measured_read_peak"] is not None
    assert line["cpu_baseline"] is None
    assert np.all(np.isfinite(d["x"])) and np.all(np.isfinite(d["recvbuf"]))
