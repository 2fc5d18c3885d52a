"""Leave-one-out cross-validation on the device (scikit-gpuppy_amd/csrc/loo.hip; gpx_loo, gpx_loo_grad; GaussianProcess.loo / loo_nlp,
objective="loo"): predictions, the fused gradient kernel, finite differences across refits, handle history, refusals, the objective.

The gradient restated on the host: with P = K^-1, c_i = 1/2 (1 / P_ii + alpha_i^2 / P_ii^2), g = P (alpha / diag P) and
W = P diag(c) P - 1/2 (g alpha^T + alpha g^T):  S_0 = sum W Kf,  S_k = sum W Kf w_k (x_ik - x_jk)^2,  T = tr W;  grad = [S_0, vt T, -S_k / 2].
A sum's scale is the sum of its absolute terms, the inner sum taken apart: |W_kl| -> sum_i |P_ki| c_i |P_il| + 1/2 (|g_k| |alpha_l| + |alpha_k| |g_l|)."""
import inspect

import numpy as np
import pytest

from conftest import load_golden, torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from skgpuppy_amd.Covariance import _MaternModel, _MatrixModel
from skgpuppy_amd.GaussianProcess import _DeviceModel

import _accuracy as acc
import _dense_ld as dl

pytestmark = pytest.mark.gpu


def model_grad(x, theta, Kinv, alpha, dt=dl.LD, blas=False):
    """(gradient [2 + d], scales [2 + d]) in dt; blas: the N^3 products in float64 BLAS (their error, N u, is far below the rule's floor)"""
    xl, d = np.asarray(x, dtype=np.float64).astype(dt), np.shape(x)[1]
    v, vt, w = dl.params(theta, d, dt)
    P, al = np.asarray(Kinv).astype(dt), np.asarray(alpha).astype(dt)
    dg = np.diagonal(P)
    c, g = (1 / dg + al * al / (dg * dg)) / 2, P.dot(al / dg)
    Pm, cm = (np.asarray(Kinv, dtype=np.float64), c.astype(np.float64)) if blas else (P, c)
    W = (Pm * cm).dot(Pm.T).astype(dt) - (np.outer(g, al) + np.outer(al, g)) / 2
    A = (np.abs(Pm) * cm).dot(np.abs(Pm).T).astype(dt) + (np.outer(np.abs(g), np.abs(al)) + np.outer(np.abs(al), np.abs(g))) / 2
    D = [w[k] * (xl[:, k][:, None] - xl[:, k][None, :]) ** 2 for k in range(d)]
    Kf = v * np.exp(-sum(D) / 2)
    S = [(W * Kf).sum(), vt * np.trace(W)] + [-(W * Kf * D[k]).sum() / 2 for k in range(d)]
    B = [(A * Kf).sum(), vt * np.trace(A)] + [(A * Kf * D[k]).sum() / 2 for k in range(d)]
    return np.array(S, dt), np.array(B, dt)


def by_deletion(K, t):
    """(mean [N], variance [N]) of every point from a NumPy Cholesky of K without its row and column"""
    mean, var = np.empty(len(t)), np.empty(len(t))
    for i in range(len(t)):
        keep = np.arange(len(t)) != i
        z = np.linalg.solve(np.linalg.cholesky(K[np.ix_(keep, keep)]), np.stack([K[keep, i], t[keep]], 1))
        mean[i], var[i] = z[:, 0].dot(z[:, 1]), K[i, i] - z[:, 0].dot(z[:, 0])
    return mean, var


def loo_distance(got, want, t):
    """the larger of max |mean - mean'| / max |t| and max |var - var'| / var'"""
    return max(float(np.abs(got[0] - want[0]).max() / np.abs(t).max()), float((np.abs(got[1] - want[1]) / want[1]).max()))


def loo(model):
    mean, var, nlp = np.empty(model.n), np.empty(model.n), np.empty(1)
    _gpx.check(_gpx.lib.gpx_loo(model.handle, _gpx.ptr(mean), _gpx.ptr(var), _gpx.ptr(nlp)), "gpx_loo")
    return mean, var, nlp[0]


def grad(name, model, d):
    g = np.empty(d + 2)
    _gpx.check(getattr(_gpx.lib, name)(model.handle, _gpx.ptr(g)), name)
    return g


def check_predictions(model, K, tc, what):
    """gpx_loo against deletion, within _accuracy.bound() of what LAPACK's inverse of the same K gives for the same identity"""
    want, Pl = by_deletion(K, tc), acc.lapack_inverse(K)
    lapack = loo_distance((tc - Pl.dot(tc) / np.diagonal(Pl), 1.0 / np.diagonal(Pl)), want, tc)
    mean, var, nlp = loo(model)
    dist = loo_distance((mean, var), want, tc)
    print("%s: LAPACK %.3e  device %.3e  bound %.3e" % (what, lapack, dist, acc.bound(lapack)))
    assert dist <= acc.bound(lapack)
    # L is the Gaussian log density of the device's own predictions (t - mean re-forms alpha_i / P_ii to u |t| / |t - mean|: 1e-10 is ample)
    assert nlp == pytest.approx(0.5 * len(tc) * np.log(2 * np.pi) + 0.5 * np.sum(np.log(var) + (tc - mean) ** 2 / var), rel=1e-10)


@pytest.mark.parametrize("N,d", [(37, 1), (129, 3)])
def test_predictions_are_refits(N, d):
    x, t, _xs, theta = acc.recipe(N, d)
    model = _DeviceModel(_gpx.f64(x), _gpx.f64(t - t.mean()), _gpx.f64(theta))
    check_predictions(model, sk.GaussianCovariance().cov_matrix(x, theta), t - t.mean(), "N=%d d=%d" % (N, d))
    gp, (mean, var, nlp) = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta), loo(model)
    assert np.array_equal(gp.loo()[0], mean + t.mean()) and np.array_equal(gp.loo()[1], var) and gp.loo_nlp() == nlp


@pytest.mark.parametrize("N,d,dup", [(100, 1, False), (129, 8, True), (300, 17, False), (1100, 3, False)])
def test_fused_gradient_against_long_double(N, d, dup):
    """gpx_loo_grad within 32 max(rho_ref, 1000 u) of the long-double sums on the device's own K^-1 and alpha, on the scale of its absolute
    terms (inner sum included).  (100, 1): one diagonal tile with padding; (129, 8): the first off-diagonal tile, one live row in the second
    tile row, a duplicated training row; (300, 17): three tile rows, two blocks of coordinates; (1100, 3): nine tile rows, past lower_tile's
    group of eight -- there the model's N^3 products run in float64 BLAS: their error, N u of the scale, is far below the floor of 1000 u."""
    x, t, theta = dl.make_case(N, d, dl.seed_of(N, d))
    x[N - 1] = x[3] if dup else x[N - 1]
    model = _DeviceModel(_gpx.f64(x), _gpx.f64(t), _gpx.f64(theta))
    args = (x, theta, model.kinv(), model.alpha())
    want, scale = model_grad(*args, blas=N > 512)
    rho = dl.rho_of({"grad": dl.distances(model_grad(*args, dt=np.float64)[0], want, scale)})
    dist = {"grad": dl.distances(grad("gpx_loo_grad", model, d), want, scale)}
    print("N=%d d=%d: rho_ref %.3e  device %.3e  bound %.3e" % (N, d, rho, dist["grad"].max(), dl.bound(rho)))
    dl.assert_within(dist, rho, what="gpx_loo_grad N=%d d=%d" % (N, d))


def test_gradient_matches_finite_differences():
    """the case, step and tolerance of tests/test_gpu_parity.py::test_gradient_matches_finite_differences, across refits"""
    g = load_golden("n203_d3")
    cov, t, th, eps = sk.GaussianCovariance(), g["t_centered"], g["theta"].copy(), 1e-5
    got = cov._d_loo_nlp_d_theta(g["x"], t, th)
    for j, e in enumerate(eps * np.eye(len(th))):
        num = (cov._loo_nlp(g["x"], t, th + e) - cov._loo_nlp(g["x"], t, th - e)) / (2 * eps)
        assert got[j] == pytest.approx(num, rel=1e-4, abs=1e-4)


def test_history_changes_no_bit():
    x, t, xs, theta = acc.recipe(300, 3, 5)
    model = _DeviceModel(_gpx.f64(x), _gpx.f64(t - t.mean()), _gpx.f64(theta))
    n0, g0 = grad("gpx_nll_grad", model, 3), grad("gpx_loo_grad", model, 3)
    assert np.array_equal(grad("gpx_loo_grad", model, 3), g0) and np.array_equal(grad("gpx_nll_grad", model, 3), n0)
    model.predict(_gpx.f64(xs))
    assert np.array_equal(grad("gpx_loo_grad", model, 3), g0)


def test_refusals():
    x, t, _xs, theta = acc.recipe(37, 1)
    tc, out, Kg = t - t.mean(), np.empty(3), sk.GaussianCovariance().cov_matrix(x, theta)
    pseudo = sk.GaussianProcess(x, t, sk.SPGPCovariance(5), np.concatenate([theta, x[:5].ravel()])).pseudo_gp()._dev()
    assert _gpx.lib.gpx_loo(pseudo.handle, None, None, _gpx.ptr(out)) == _gpx.lib.gpx_loo_grad(pseudo.handle, _gpx.ptr(out)) == _gpx.GPX_ERR_STATE
    for what, model, K in (("gpx_fit_matrix", _MatrixModel(Kg, tc), Kg),
                           ("gpx_matern_fit", _MaternModel(x, tc, theta, 5), sk.MaternCovariance(2.5).cov_matrix(x, theta))):
        check_predictions(model, K, tc, what)
        assert _gpx.lib.gpx_loo_grad(model.handle, _gpx.ptr(out)) == _gpx.GPX_ERR_STATE


def test_objective():
    from scipy.optimize import fmin_l_bfgs_b
    np.random.seed(11)
    x, cov = np.linspace(0, 10, 60)[:, None], sk.GaussianCovariance()
    gp = sk.GaussianProcess(x, sk.GaussianProcess.get_realisation(x, cov, np.log(np.array([2.0, 0.01, 0.5]))), cov, objective="loo")
    assert gp.loo_nlp() <= cov._loo_nlp(x, gp.t, cov.get_theta(x, gp.t))
    assert np.abs(cov._d_loo_nlp_d_theta(x, gp.t, gp.theta_min)).max() < inspect.signature(fmin_l_bfgs_b).parameters["pgtol"].default
    with pytest.raises(NotImplementedError, match="Gaussian"):
        sk.GaussianProcess(x, gp.t, sk.MaternCovariance(2.5), objective="loo")
