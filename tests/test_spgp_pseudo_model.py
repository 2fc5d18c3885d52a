"""The algebra behind GaussianProcess.pseudo_gp(), on the host: the SPGP predictor is a dense GP predictor over the pseudo-inputs with
alpha = beta and K^-1 = P (tests/_spgp_pseudo.py), so Girard's exact moments on (xbar, beta, P) are the moments of the SPGP predictive
distribution itself; and the long-double models that tests/test_spgp_pseudo.py holds the device to accept (xbar, P, beta) as they are.  No GPU.

Bounds.  Predictor identity: the project's own SPGP bars against the oracle (tests/test_gpu_parity.py, test_spgp_vs_oracle_ragged_and_large_m):
2e-5 on the mean, 2e-6 v on the variance -- both sides are float64 evaluations through explicit inverses of K_M + 1e-5 I.  Exact moments against
the 24-node Gauss-Hermite mixture moments of that predictor: 1e-9 absolute (the rule is exact for polynomials of degree 47 per axis; at
Sigma_kk <= 0.3, w = 0.04 the integrand's Hermite coefficients fall far below that).  Oracle against the long-double models: the rule of
tests/_dense_ld.py, rho_ref from the float64 evaluation of the same model."""
import numpy as np
import pytest

from oracle import oracle as orc

import _dense_ld as dl
import _predict_grad_model as pg
import _spgp_pseudo as sp


_CACHE = {}


def model(name):
    if name not in _CACHE:
        x, t, th, th_gc, xb = sp.make_model(name)
        beta, P = sp.beta_P(x, t, th_gc, xb)
        _CACHE[name] = (x, t, th, th_gc, xb, beta, P)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_pseudo_predictor_is_the_spgp_predictor(name):
    x, t, th, th_gc, xb, beta, P = model(name)
    N, d, m = sp.MODELS[name]
    xs = np.random.RandomState(5).uniform(0, 10, (50, d))
    mu, var = sp.predictor(xs, th_gc, xb, beta, P, np.mean(t))
    omu, ovar = orc.OracleSPGP(x, t, th, m).estimate_many(xs)
    dm, dv = np.abs(mu - omu).max(), np.abs(var - ovar).max()
    print("model %s: worst mean difference %.3e, worst variance difference %.3e, max|P| %.4g, min eig P %.4g" %
          (name, dm, dv, np.abs(P).max(), np.linalg.eigvalsh(P).min()))
    assert dm <= 2e-5 and dv <= 2e-6 * np.exp(th_gc[0])
    assert np.array_equal(P, P.T)


@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_moments_are_the_mixture_moments_of_the_predictor(name):
    x, t, th, th_gc, xb, beta, P = model(name)
    d = sp.MODELS[name][1]
    meant = np.mean(t)
    shim = sp.Shim(th_gc, xb, beta, P, meant)
    for i, u in enumerate(sp.inputs(name, 2)):
        # a diagonal Sigma: the reference's Exact normalisers and Delta^-1 read Sigma's diagonal alone (det(I + Winv * Sigma) is an
        # elementwise product, UncertaintyPropagation.py:247-257), so only then are its moments those of the mixture
        S = np.diag(np.diag(sp.full_sigma(d, 300 + i)))
        em, ev = orc.exact_propagate(shim, u, S)
        qm, qv = sp.gauss_hermite_moments(lambda X: sp.predictor(X, th_gc, xb, beta, P, meant), u, S)
        print("model %s input %d: mean difference %.3e, variance difference %.3e" % (name, i, abs(em - qm), abs(ev - qv)))
        assert abs(em - qm) <= 1e-9 and abs(ev - qv) <= 1e-9


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_long_double_models_accept_the_pseudo_basis(name):
    """_dense_ld.exact_builtin / approx_partials and _predict_grad_model on (xbar, theta, P, beta), quirk off, state what the oracle's
    functions compute on the shim, and what the predictor is"""
    x, t, th, th_gc, xb, beta, P = model(name)
    d = sp.MODELS[name][1]
    meant = np.mean(t)
    shim = sp.Shim(th_gc, xb, beta, P, meant)
    u, S = sp.inputs(name, 1)[0], sp.full_sigma(d, 77)
    args = (xb, th_gc, P, beta, u, S)
    # Exact
    want, ref = dl.exact_builtin(*args, defect="quirk"), dl.exact_builtin(*args, dt=np.float64, defect="quirk")
    rho = dl.rho_of({k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in ("mean", "var")})
    em, ev = orc.exact_propagate(shim, u, S)
    dl.assert_within({"mean": dl.distances(em - meant, *want["mean"]), "var": dl.distances(ev, *want["var"])}, rho, "exact " + name)
    # Approx
    want, ref = dl.approx_partials(*args, defect="quirk"), dl.approx_partials(*args, dt=np.float64, defect="quirk")
    rho = dl.rho_of({k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in ("mean", "sigma2", "rest")})
    am, as2, arest = orc.approx_parts(shim, u, S)
    dl.assert_within({"mean": dl.distances(am, *want["mean"]), "sigma2": dl.distances(as2, *want["sigma2"]),
                      "rest": dl.distances(arest, *want["rest"])}, rho, "approx " + name)
    # the predictor's value rows: mean and variance of _predict_grad_model are the predictor's
    U = sp.inputs(name, 5)
    mg, vg = pg.mean_grad(xb, th_gc, beta, U, 0), pg.var_grad(xb, th_gc, P, U, 0)
    mg64, vg64 = pg.mean_grad(xb, th_gc, beta, U, 0, dt=np.float64), pg.var_grad(xb, th_gc, P, U, 0, dt=np.float64)
    rho = dl.rho_of({"mean": dl.distances(mg64["mean"][0], *mg["mean"]), "var": dl.distances(vg64["var"][0], *vg["var"])})
    mu, var = sp.predictor(U, th_gc, xb, beta, P, 0.0)
    dl.assert_within({"mean": dl.distances(mu, *mg["mean"]), "var": dl.distances(var, *vg["var"])}, rho, "predictor " + name)
    # and its gradients are the derivatives of those: central differences of the long-double values, step 2^-10 (exact on the grid),
    # Truncation h^2 / 6 |f'''|: with g(s) = exp(-s^2 / 2), max |g'| = 0.61, |g''| = 1, |g'''| = 1.38, a term c_i has |c'''| <= 1.38 w^(3/2) c
    # and a product c_i c_j at most (2 * 1.38 + 6 * 0.61) w^(3/2) = 6.4 w^(3/2) times its size: 8e-9 of the scale at w = 0.04 -- bar 1e-7
    h = 2.0 ** -10
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        mp, mm = pg.mean_grad(xb, th_gc, beta, U + e, 0), pg.mean_grad(xb, th_gc, beta, U - e, 0)
        vp, vm = pg.var_grad(xb, th_gc, P, U + e, 0), pg.var_grad(xb, th_gc, P, U - e, 0)
        fd_m, fd_v = (mp["mean"][0] - mm["mean"][0]) / (2 * h), (vp["var"][0] - vm["var"][0]) / (2 * h)
        assert np.all(np.abs(fd_m - mg["dmean"][0][:, k]) <= 1e-7 * mg["mean"][1])
        assert np.all(np.abs(fd_v - vg["dvar"][0][:, k]) <= 1e-7 * vg["var"][1])
