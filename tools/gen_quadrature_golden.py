#!/usr/bin/env python3
"""Generate tests/golden/quadrature.npz by importing the genuine reference's numerical propagators
(skgpuppy/UncertaintyPropagation.py:90-162: UncertaintyPropagationNumericalHG, UncertaintyPropagationMC).

Runs only where the reference tree is available (GPX_REFERENCE, as tools/gen_golden.py, whose import shims it reuses).  Nothing of the
reference travels: explicit input AND output arrays are written.  The models themselves are the existing fixtures (x, t_raw, theta of
tests/golden/<name>.npz) and tests/_periodic_ld.make_case; this file holds, per model,

  (1) hg_<name>_*   UncertaintyPropagationNumericalHG: order, u [3, d] (u1 is a training row), Sigma [2, d, d] (Sigma1 has off-diagonal
      entries -- which the reference's rule ignores), mean [3, 2] = propagate_mean, ga [3, 2, 2] = propagate_GA, y [3, 2, 9] =
      m + k sqrt(var), k = -4 .. 4, dens [3, 2, 9] = propagate_many(y).  The reference fixes order 4; at d = 8 that is 65536 gp(x) calls
      per expectation, so n256_d8 is recorded at ORDER 2 (256 nodes): the class's own code runs, its module-level integrate_hermgauss_nd
      is handed the order.
  (2) mc_<name>_*   UncertaintyPropagationMC(n = 200).propagate_GA after numpy.random.seed(seed): samples [3, 200, d] = the three sample
      sets the reference drew (numpy.random.multivariate_normal wrapped), exp [3] = its three expectations (mean, E var, E mean^2),
      ga [2] = what it returned.
  (3) hgper_*       the reference's PeriodicCovariance model of _periodic_ld.make_case(203, 3) under HG, as (1) with one u pair.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/gen_quadrature_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))

import gen_golden  # noqa: E402
import _periodic_ld as pl  # noqa: E402

HG_MODELS = {"n203_d3": 4, "grid_int": 4, "n256_d8": 2}       # name -> order
MC_MODELS = {"n203_d3": 11, "grid_int": 12}                   # name -> seed
PERIODIC_CASE = (203, 3)


def inputs(x, seed):
    """u [3, d]: inside the data's box, u1 a training row; Sigma [2, d, d]: a diagonal one and a full SPD one"""
    d = x.shape[1]
    rng = np.random.RandomState(seed)
    lo, hi = x.min(0), x.max(0)
    u = lo + (hi - lo) * rng.uniform(0.3, 0.7, (3, d))
    u[1] = x[len(x) // 3]
    s = (hi - lo) * rng.uniform(0.01, 0.04, d)
    R = rng.uniform(-0.4, 0.4, (d, d))
    C = np.eye(d) + 0.5 * (R + R.T) / d
    full = (s[:, None] * s[None, :]) * (C.dot(C.T))
    return u, np.array([np.diag(s * s), full])


def hg_group(out, key, gp, HG, UPmod, order, u, Sigma):
    orig = UPmod.integrate_hermgauss_nd
    UPmod.integrate_hermgauss_nd = lambda f, m, S, _o: orig(f, m, S, order)
    try:
        up = HG(gp)
        nu, nS = len(u), len(Sigma)
        mean, ga = np.empty((nu, nS)), np.empty((nu, nS, 2))
        y, dens = np.empty((nu, nS, 9)), np.empty((nu, nS, 9))
        for i in range(nu):
            for j in range(nS):
                mean[i, j] = up.propagate_mean(u[i], Sigma[j])
                ga[i, j] = up.propagate_GA(u[i], Sigma[j])
                y[i, j] = ga[i, j, 0] + np.arange(-4, 5) * np.sqrt(ga[i, j, 1])
                dens[i, j] = up.propagate_many(y[i, j], u[i], Sigma[j])
    finally:
        UPmod.integrate_hermgauss_nd = orig
    out[key + "order"], out[key + "u"], out[key + "Sigma"] = np.int64(order), u, Sigma
    out[key + "mean"], out[key + "ga"], out[key + "y"], out[key + "dens"] = mean, ga, y, dens
    print(key, "order", order, "ga[0,0]", ga[0, 0], "ga[1,1]", ga[1, 1], "dens peak", dens.max())


def mc_group(out, key, gp, MC, UPmod, seed, u, Sigma, n=200):
    drawn, exps = [], []
    orig_mvn, orig_exp = np.random.multivariate_normal, UPmod.expected_value_monte_carlo

    def mvn(mean, cov, size=None):
        s = orig_mvn(mean, cov, size)
        drawn.append(np.array(s))
        return s

    def expval(func, mu, S, n_=1000):
        e = orig_exp(func, mu, S, n_)
        exps.append(float(e))
        return e

    np.random.multivariate_normal, UPmod.expected_value_monte_carlo = mvn, expval
    try:
        np.random.seed(seed)
        ga = MC(gp, n).propagate_GA(u, Sigma)
    finally:
        np.random.multivariate_normal, UPmod.expected_value_monte_carlo = orig_mvn, orig_exp
    assert len(drawn) == 3 and len(exps) == 3
    out[key + "seed"], out[key + "u"], out[key + "Sigma"] = np.int64(seed), u, Sigma
    out[key + "samples"], out[key + "exp"], out[key + "ga"] = np.array(drawn), np.array(exps), np.array(ga, dtype=float)
    print(key, "ga", ga, "exp", exps)


def main():
    gen_golden._install_shims()
    sys.path.insert(0, gen_golden.REF)
    sys.dont_write_bytecode = True
    import skgpuppy.UncertaintyPropagation as UPmod
    from skgpuppy.Covariance import GaussianCovariance, PeriodicCovariance
    from skgpuppy.GaussianProcess import GaussianProcess
    HG, MC = UPmod.UncertaintyPropagationNumericalHG, UPmod.UncertaintyPropagationMC
    out = {}
    gps = {}
    for k, name in enumerate(sorted(set(HG_MODELS) | set(MC_MODELS))):
        with np.load(os.path.join(gen_golden.OUT, name + ".npz")) as g:
            x, t, theta = g["x"], g["t_raw"], g["theta"]
        gps[name] = (GaussianProcess(x, t, GaussianCovariance(), theta.copy()), x, 500 + k)
    for name, order in HG_MODELS.items():
        gp, x, seed = gps[name]
        u, Sigma = inputs(np.asarray(x, dtype=float), seed)
        hg_group(out, "hg_%s_" % name, gp, HG, UPmod, order, u, Sigma)
    for name, seed in MC_MODELS.items():
        gp, x, iseed = gps[name]
        u, Sigma = inputs(np.asarray(x, dtype=float), iseed)
        mc_group(out, "mc_%s_" % name, gp, MC, UPmod, seed, u[0], Sigma[1])
    N, d = PERIODIC_CASE
    x, t, theta = pl.make_case(N, d)
    gp = GaussianProcess(x, t, PeriodicCovariance(), theta.copy())
    u, Sigma = inputs(x, 700)
    hg_group(out, "hgper_", gp, HG, UPmod, 4, u[:2], Sigma)
    path = os.path.join(gen_golden.OUT, "quadrature.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
