#!/usr/bin/env python3
"""Generate tests/golden/periodic.npz by importing the genuine reference's PeriodicCovariance (skgpuppy/Covariance.py:361-433).

Runs only where the reference tree is available (GPX_REFERENCE, as tools/gen_golden.py, whose import shims it reuses).  Nothing of the
reference travels: explicit input AND output arrays are written.  Per case (N, d) of tests/_periodic_ld.GOLDEN_CASES, keys c<N>_<d>_*:
x, t (centred), theta, K = cov_matrix(x), dK [2 + 3 d, 40, 40] = every _d_cov_matrix_d_theta_ij on the first 40 rows, beta = Kinv t,
nll, grad = _d_nll_d_theta, xs [64, d] (query 3 equals training row 5), mean / var = estimate_many(xs), theta0 = get_theta(x, t).

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_periodic_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))        # (the tests' model modules import the repository's oracle package)

import gen_golden  # noqa: E402
import _periodic_ld as pl  # noqa: E402


def main():
    gen_golden._install_shims()
    sys.path.insert(0, gen_golden.REF)
    sys.dont_write_bytecode = True
    from skgpuppy.Covariance import PeriodicCovariance
    from skgpuppy.GaussianProcess import GaussianProcess
    out = {}
    for N, d in pl.GOLDEN_CASES:
        x, t, theta = pl.make_case(N, d)
        cov = PeriodicCovariance()
        xs = pl.make_queries(x, 64, pl.seed_of(N, d) + 1)
        gp = GaussianProcess(x, t, cov, theta.copy())
        mean, var = gp.estimate_many(xs)
        sub = x[:40]
        key = "c%d_%d_" % (N, d)
        out[key + "x"], out[key + "t"], out[key + "theta"], out[key + "xs"] = x, t, theta, xs
        out[key + "K"] = cov.cov_matrix(x, theta)
        out[key + "dK"] = np.array([cov._d_cov_matrix_d_theta_ij(sub, sub, theta, j) for j in range(len(theta))])
        out[key + "beta"] = np.asarray(gp._get_beta())
        out[key + "nll"] = np.float64(cov._negativeloglikelihood(x, t, theta))
        out[key + "grad"] = np.asarray(cov._d_nll_d_theta(x, t, theta), dtype=float)
        out[key + "mean"], out[key + "var"] = np.asarray(mean), np.asarray(var)
        out[key + "theta0"] = cov.get_theta(x, t)
        print(key, "nll", out[key + "nll"], "cond", np.linalg.cond(out[key + "K"]))
    path = os.path.join(gen_golden.OUT, "periodic.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
