"""Child process of tests/test_backward_error.py: one factorisation under the schedule knobs of its environment (they are read once per
process), its backward error computed here, one JSON line on stdout.

  fit N d [HASH]   gpx_fit of the recipe problem: hash of L's bytes and chol_backward_error of the device factor against the device Gram
                   (skipped when the hash equals HASH, the default schedule's: the same bytes have the same backward error)
  spd_inverse N d  gpx_spd_inverse of the device Gram: inverse_residual, exact symmetry, log det
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import skgpuppy_amd as sk  # noqa: E402
from skgpuppy_amd import _gpx  # noqa: E402

import _accuracy as acc  # noqa: E402


def main():
    mode, N, d = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    x, t, _xs, theta = acc.recipe(N, d)
    K = sk.GaussianCovariance().cov_matrix(x, theta)
    out = {"mode": mode, "N": N, "d": d}
    if mode == "fit":
        gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
        out["jitter"] = gp._dev().jitter()
        L = gp._dev().chol()
        gp._dev().close()
        out["hash"] = acc.digest(L)
        if len(sys.argv) < 5 or sys.argv[4] != out["hash"]:
            out["offdiag"], out["diag"] = acc.chol_backward_error(L, K)
    elif mode == "spd_inverse":
        X = np.empty((N, N))
        ld = ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_spd_inverse(_gpx.ptr(K), N, _gpx.ptr(X), ctypes.byref(ld)), "gpx_spd_inverse")
        out["residual"] = acc.inverse_residual(K, X)
        out["symmetric"] = bool(np.array_equal(X, X.T))
        out["logdet"] = ld.value
    else:
        raise SystemExit("unknown mode %r" % mode)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
