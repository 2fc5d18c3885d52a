#!/usr/bin/env python3
"""Generate tests/golden/linear.npz by importing the genuine reference's first-order propagator
(skgpuppy/UncertaintyPropagation.py:213-242: UncertaintyPropagationLinear).

Runs only where the reference tree is available (GPX_REFERENCE, as tools/gen_golden.py, whose import shims it reuses).  Nothing of the
reference travels: explicit output arrays are written.  The models and inputs are the existing fixtures (x, t_raw, theta, u*, Sigma* of
tests/golden/<name>.npz); this file holds, per model and (u_i, Sigma_j) pair,

  ga_<name>     [nu, nS, 2]  the reference's propagate_GA(u_i, Sigma_j) = (mu(u) + meant, sum_k g_k^2 Sigma_kk + vt), g by central
                             differences of gp(x)[0] with step 1e-5
  delta_<name>  [nu, nS, 2]  |analytic model - reference| per entry: the same two numbers with g in closed form (tests/_predict_grad_model.py
                             in long double, on the reference's own beta).  It is the reference's finite-difference error, measured here on
                             the CPU; the GPU test allows the device 4 delta_ref of the golden values.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_linear_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))

import gen_golden  # noqa: E402
import _predict_grad_model as pg  # noqa: E402

MODELS = ("kat1_grid", "n203_d3", "n256_d8")


def analytic(x, theta, beta, meant, u, Sigma):
    """(mu(u) + meant, sum_k g_k^2 Sigma_kk + vt) in long double; the Gaussian kernel's rows carry no +vt on equality"""
    r = pg.mean_grad(x, theta, beta, u[None, :], 0)
    g = r["dmean"][0][0]
    _v, vt, _w = pg.params(theta, x.shape[1])
    return np.array([r["mean"][0][0] + pg.LD(meant), (g * g * np.diagonal(Sigma).astype(pg.LD)).sum() + vt])


def main():
    gen_golden._install_shims()
    sys.path.insert(0, gen_golden.REF)
    sys.dont_write_bytecode = True
    import skgpuppy.UncertaintyPropagation as UPmod
    from skgpuppy.Covariance import GaussianCovariance
    from skgpuppy.GaussianProcess import GaussianProcess
    out = {}
    for name in MODELS:
        with np.load(os.path.join(gen_golden.OUT, name + ".npz")) as z:
            g = {k: z[k] for k in z.files}
        x, t, theta = g["x"], g["t_raw"], g["theta"]
        gp = GaussianProcess(x, t, GaussianCovariance(), theta.copy())
        up = UPmod.UncertaintyPropagationLinear(gp)
        nu, nS = int(g["nu"]), int(g["nS"])
        ga, delta = np.empty((nu, nS, 2)), np.empty((nu, nS, 2))
        beta = np.asarray(gp._get_beta(), dtype=float)
        for i in range(nu):
            for j in range(nS):
                u, S = np.asarray(g["u%d" % i], dtype=float), np.asarray(g["Sigma%d" % j], dtype=float)
                ga[i, j] = up.propagate_GA(u, S)
                delta[i, j] = np.abs(analytic(np.asarray(x, dtype=float), theta, beta, gp._get_mean_t(), u, S) - ga[i, j].astype(pg.LD)).astype(float)
        out["ga_" + name], out["delta_" + name] = ga, delta
        print(name, "ga[0,0]", ga[0, 0], "largest delta_ref", delta.max(0))
    path = os.path.join(gen_golden.OUT, "linear.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
