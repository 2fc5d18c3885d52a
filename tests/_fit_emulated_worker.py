"""Child process of tests/test_fit_emulated.py: fits under the knobs of its environment (GPX_FIT_EMU, GPX_FIT_EMU_GROUP, GPX_EMU_MIN_K and
the schedule switches are read once per process), one JSON line on stdout.

  fit N d OUT   two gpx_fit of the recipe problem in this process: jitter, hash of L's bytes (and of the second fit's), backward error
                of the factor against the device Gram; L, alpha and estimate_many of 777 queries saved to OUT (.npz)
  dup N d AT    the recipe problem with vt = 0 and 150 numerically identical rows from row AT on (the recipe of the multi-device test):
                a non-positive pivot there.  Reports the jitter the fit ended with and whether alpha is finite.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402,F401  (its HIP runtime first, as in the rest of the suite)
import skgpuppy_amd as sk  # noqa: E402

import _accuracy as acc  # noqa: E402


def main():
    mode, N, d = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    x, t, xs, theta = acc.recipe(N, d, 777)
    out = {"mode": mode, "N": N, "d": d}
    if mode == "fit":
        K = sk.GaussianCovariance().cov_matrix(x, theta)
        gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
        out["jitter"] = gp._dev().jitter()
        L = gp._dev().chol()
        beta = gp._get_beta()
        mean, var = gp.estimate_many(xs)
        gp._dev().close()
        gp2 = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
        out["hash"], out["hash2"] = acc.digest(L), acc.digest(gp2._dev().chol())
        gp2._dev().close()
        out["offdiag"], out["diag"] = acc.chol_backward_error(L, K)
        np.savez(sys.argv[4], L=L, beta=beta, mean=mean, var=var)
    elif mode == "dup":
        at = int(sys.argv[4])
        rng = np.random.RandomState(N + at)
        x[at:at + 150] = x[at] + 1e-9 * rng.randn(150, d)
        theta[1] = -np.inf
        with np.errstate(divide="ignore"):
            gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
            out["jitter"] = gp._dev().jitter()
            out["finite"] = bool(np.isfinite(gp._get_beta()).all())
            out["hash"] = acc.digest(gp._dev().chol())
        gp._dev().close()
    else:
        raise SystemExit("unknown mode %r" % mode)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
