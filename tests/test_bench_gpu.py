"""bench.py's plain run: the headline line alone, `--steps` honoured, and `--dump-outputs` writing the last timed step's
log-likelihood, the value the library gives for the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(nhp, tmp_path):
    N, M, steps = 64, 20_000, 7
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                          "--nodes", str(N), "--events", str(M), "--dump-outputs", str(dump)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == steps and line["warmup"] == 2 and line["status"] == "ok"
    assert line["ms_per_step"] > 0.0 and line["value"] > 0.0
    assert "cpu_baseline" not in line and "other_workloads" not in line and "configs" not in line    # --full only
    ll = np.load(dump / "loglik.npy")
    assert ll.dtype == np.float64 and ll.shape == (1,)
    assert ll[0] == line["loglik"][0]
    times, nodes, T = nhp.synthetic.s_metric_data(N, M, kbar=8.0)
    proc = nhp.synthetic.s_metric_process(N, M, T, "exponential", 1.0)
    want = nhp.loglikelihood(proc, (times, nodes, T), recursive=False)
    assert abs(ll[0] - want) <= 1e-10 * abs(want), (ll[0], want)
