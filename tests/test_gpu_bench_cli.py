"""bench.py's command line on one GPU: a plain run times exactly --steps steps and prints the headline only; --dump-outputs
writes the last timed step's outputs, and two runs with the same arguments compute on identical inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_steps_and_dumps_outputs(tmp_path):
    dumps = [tmp_path / "a", tmp_path / "b"]
    runs = [_bench("--steps", "7", "--warmup", "1", "--windows", "3", "--rays-per-gpu", "128", "--dump-outputs", str(d))
            for d in dumps]
    d = runs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 7 and d["windows"] == 3 and d["window_steps"] == [3, 2, 2]
    assert sorted(d["window_ms"])[1] == pytest.approx(d["ms_per_step"])
    assert d["value"] == pytest.approx(128 * d["config"]["samples_per_ray"] / (d["ms_per_step"] * 1e-3), rel=1e-6)
    # the secondary measurements belong to --full
    for k in ("power", "forward_only", "roofline", "roofline_composite", "fp32_exact", "cpu_baseline", "psnr_vs_ref"):
        assert k not in d, k

    names = sorted(os.listdir(dumps[0]))
    assert names == sorted(os.listdir(dumps[1]))
    assert "loss.npy" in names and "out_color.npy" in names
    assert any(n.startswith("param_udf.") for n in names) and any(n.startswith("grad_udf.") for n in names)
    total = 0
    for n in names:
        a, b = np.load(dumps[0] / n), np.load(dumps[1] / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape, n
        assert np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(dumps[0] / "out_color.npy").shape == (128, 3)
    # identical inputs: the same rays and weights, so the same render up to the step's own run-to-run spread
    for n in ("loss.npy", "out_color.npy", "out_z_vals.npy", "out_weights.npy", "param_udf.lin0.bias.npy"):
        np.testing.assert_allclose(np.load(dumps[0] / n), np.load(dumps[1] / n), rtol=1e-4, atol=1e-5, err_msg=n)
