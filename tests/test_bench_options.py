"""bench.py's plain run (the headline line only) and --dump-outputs: the arrays written are the last timed step's outputs, the oracle's
on the same seeded inputs.  The argument checks run without a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _bench(extra, env_extra=None, timeout=600):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + extra, capture_output=True, text=True, timeout=timeout, env=env)


def test_bad_arguments_are_refused_before_any_work(tmp_path):
    r = _bench(["--steps", "0"], timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stdout + r.stderr
    r = _bench(["--gpus", "2", "--dump-outputs", str(tmp_path / "out")], env_extra={"WORLD_SIZE": "2"}, timeout=300)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "out"
    r = _bench(["--gpus", "1", "--workload", "c2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    N, dim, M = 4096, 4, 4096
    assert d["metric"] == "GP fit+predict pts/sec (K+Cholesky, N=%d d=%d)" % (N, dim)
    assert d["unit"] == "pts/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] == pytest.approx((N + M) / (d["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("cpu_baseline", "parity_vs_oracle", "python_api", "propagate", "likelihood_f1", "c2",
              "kernel_classes_from_untimed_profiling_step"):
        assert k not in d, k                  # measured with --full only
    assert "mfma_probe_tflops" not in d["roofline"] and d["roofline"]["achieved"] > 0

    mean, var = np.load(out / "mean.npy"), np.load(out / "var.npy")
    assert mean.dtype == np.float64 and var.dtype == np.float64 and mean.shape == (M,) and var.shape == (M,)
    import bench
    from oracle import oracle as orc
    x, t, xs, theta = bench.recipe(N, dim, M)
    om, ov = orc.OracleGP(x, t, theta).estimate_many(xs)
    v = float(np.exp(theta[0]))
    np.testing.assert_allclose(mean + t.mean(), om, rtol=1e-6, atol=1e-9 * v)     # gpx_predict's mean is that of the centred targets
    np.testing.assert_allclose(var, ov, rtol=1e-6, atol=1e-9 * v)
