"""MaternCovariance on the device (csrc/matern.hip; the gpx_matern_* entry points and the Python classes on top) against the long-double
model of tests/_matern_ld.py, NumPy's Cholesky of the model's K, and -- for the propagation of nu = 5/2 -- the generic route on the same
kernel restated on the base class (PyMatern: host scalars, 3 N Python calls per input).

Bounds (none fitted to a device result; tests/_matern_ld.py states the rules):
  Gram and derivative entries: 8 * max(rho_K, 4) = 32 units of u K (1 + s), rho_K the float64 restatement's own worst error (2.7);
  gradient: every one of the d + 2 sums on the scale of its absolute terms, 32 * max(rho_ref, 1000 u), from the device's own K^-1 and alpha;
  fit / solve / predict: SURVEY 8a -- rtol 1e-6 / atol 1e-9 v for predictions, 1e-9 relative for nll and log det;
  propagation against the generic route: the two-device-paths bounds of tests/test_propagate_many.py (mean 2e-9, variance 2 * 1e-8 v) and
  tests/test_inverse_many.py (dvh rtol 2e-6 / atol 2e-8 v, sigma2 4e-8).
GPX_MATERN_RECORD=<file> appends the measured worst ratios."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import _matern_ld as ml
import _quadrature_model as qm

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from skgpuppy_amd.Covariance import _MaternModel, _MatrixModel, _PeriodicModel
from skgpuppy_amd.InverseUncertaintyPropagation import InverseUncertaintyPropagationApprox as IUP

pytestmark = pytest.mark.gpu
V, VT = 2.0, 0.01
NU2 = ml.NU2_ALL


def _record(line):
    print(line)
    path = os.environ.get("GPX_MATERN_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _cov(nu2):
    return sk.MaternCovariance(nu2 / 2.0)


def _gram(xi, n1, xj, n2, d, theta, nu2, deriv=-1):
    K = np.empty((n1, n2))
    st = _gpx.lib.gpx_matern_gram(_gpx.ptr(xi), n1, _gpx.ptr(xj), n2, d, _gpx.ptr(_gpx.f64(theta)), nu2, deriv, _gpx.ptr(K))
    _gpx.check(st, "gpx_matern_gram")
    return K


@functools.lru_cache(maxsize=None)
def rho_K():
    """the float64 restatement's worst error over (130, 257) x D_ALL x both nu (tests/test_matern_model.py holds it under GRAM_FLOOR)"""
    worst = 0.0
    for nu2 in NU2:
        for d in ml.D_ALL:
            xi, xj, theta = ml.make_gram_case(130, 257, d)
            worst = max(worst, float(ml.gram_units(ml.kernel_parts(xi, xj, theta, nu2, np.float64)["K"], ml.kernel_parts(xi, xj, theta, nu2)).max()))
    _record("rho_K (float64 restatement) = %.3e -> bound %.3e units of u K (1 + s)" % (worst, ml.gram_bound(worst)))
    return worst


# ------------------------------------------------------------------------------------------------
# Gram
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("d", ml.D_ALL)
@pytest.mark.parametrize("n1,n2", ml.GRAM_SHAPES)
def test_gram_against_the_model(n1, n2, d, nu2):
    xi, xj, theta = ml.make_gram_case(n1, n2, d)
    ld = ml.kernel_parts(xi, xj, theta, nu2)
    K = _gram(xi, n1, xj, n2, d, theta, nu2)
    units = ml.gram_units(K, ld)
    lim = ml.gram_bound(rho_K())
    _record("gram (%d, %d) d=%d nu2=%d: worst %.3f units = %.4f of the bound %.2f" % (n1, n2, d, nu2, units.max(), units.max() / lim, lim))
    assert np.all(units <= lim), (units.max(), lim)
    # rows of xi that equal a row of xj carry exactly v + vt: sqrt(0) = 0, exp(0) = 1, no 0 * inf
    eq = ld["eq"]
    assert eq.sum() >= (n1 > 3)
    v, vt, _w = ml.params(theta, d, np.float64)
    assert np.all(K[eq] == v + vt)
    np.testing.assert_array_equal(_cov(nu2).cov_matrix_ij(xi, xj, theta), K)


@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("d", ml.D_ALL)
def test_gram_bit_equalities(d, nu2):
    x, _t, theta = ml.make_case(257, d)
    x[200] = x[17]                                                       # a duplicate training row
    K = _gram(x, 257, x, 257, d, theta, nu2)
    np.testing.assert_array_equal(K, K.T)                                # K_ij == K_ji: the fit never computes the upper half
    v, vt, _w = ml.params(theta, d, np.float64)
    assert K[200, 17] == v + vt and K[17, 200] == v + vt and np.all(np.diag(K) == v + vt)
    xj = ml.make_case(130, d, seed=5)[0]
    full = _gram(x, 257, xj, 130, d, theta, nu2)
    for a, b in ((0, 1), (63, 130), (129, 257)):                         # rows a:b of a call equal a call on rows a:b
        np.testing.assert_array_equal(_gram(np.ascontiguousarray(x[a:b]), b - a, xj, 130, d, theta, nu2), full[a:b])


@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("d", ml.D_ALL)
def test_every_derivative_against_the_model(d, nu2):
    n1, n2 = (130, 257) if d <= 3 else (64, 129)
    xi, xj, theta = ml.make_gram_case(n1, n2, d)
    ld = ml.kernel_parts(xi, xj, theta, nu2, keep=True)
    lim = ml.gram_bound(rho_K())
    cov = _cov(nu2)
    worst = 0.0
    for j in range(2 + d):
        dK = cov._d_cov_matrix_d_theta_ij(xi, xj, theta, j)
        units = ml.deriv_units(dK, ld, theta, j)
        worst = max(worst, float(units.max()))
        assert np.all(units <= lim), (j, units.max(), lim)
    _record("deriv (%d, %d) d=%d nu2=%d: worst %.3f units = %.4f of the bound" % (n1, n2, d, nu2, worst, worst / lim))
    dvt = cov._d_cov_matrix_d_theta_ij(xi, xj, theta, 1)
    assert np.all(dvt[~ld["eq"]] == 0) and np.all(dvt[ld["eq"]] == np.exp(theta[1]))


# ------------------------------------------------------------------------------------------------
# fit, solve, predict
# ------------------------------------------------------------------------------------------------
def _numpy_reference(x, t, theta, nu2, xs, dt=ml.LD):
    """(K^-1, alpha, mean, var, nll, logdet, L) from NumPy's Cholesky of the MODEL's K (long double, rounded to float64; the large cases
    pass dt = np.float64: the restatement, within 4 u of the model entry by entry, without gigabytes of long doubles)"""
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    K = ml.kernel_parts(x, x, theta, nu2, dt)["K"].astype(np.float64)
    kv = ml.kernel_parts(xs, x, theta, nu2, dt)["K"].astype(np.float64)
    c = cho_factor(K, lower=True)
    alpha = cho_solve(c, t)
    z = solve_triangular(c[0], kv.T, lower=True)
    v, vt, _w = ml.params(theta, x.shape[1], np.float64)
    return (cho_solve(c, np.eye(len(x))), alpha, kv.dot(alpha), (v + vt) - (z * z).sum(0), ml.nll(K, t), 2 * np.log(np.diag(c[0])).sum(), np.tril(c[0]))      # (cho_factor leaves the other triangle as it was)


@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("N,d", ml.FIT_CASES)
def test_fit_solve_predict(N, d, nu2):
    x, t, theta = ml.make_case(N, d)
    xs = ml.make_queries(x, 64, ml.seed_of(N, d) + 1)
    cov = _cov(nu2)
    gp = sk.GaussianProcess(x, t, cov, theta.copy())
    assert gp._route() == "matern"
    mean, var = gp.estimate_many(xs)
    Kinv, alpha, rm, rv, rnll, rlogdet, L = _numpy_reference(x, gp.t, theta, nu2, xs)
    kscale = np.abs(Kinv).max()
    np.testing.assert_allclose(gp.Kinv, Kinv, rtol=1e-6, atol=1e-7 * kscale)
    np.testing.assert_allclose(gp._get_beta(), alpha, rtol=1e-6, atol=1e-8 * np.abs(alpha).max())
    np.testing.assert_allclose(mean, rm + gp.meant, rtol=1e-6, atol=1e-9 * V)
    np.testing.assert_allclose(var, rv, rtol=1e-6, atol=1e-9 * V)
    # gpx_solve: L^-1 B and K^-1 B for two right-hand sides
    B = np.random.RandomState(N + d).randn(2, N)
    kb, lb = np.empty_like(B), np.empty_like(B)
    _gpx.check(_gpx.lib.gpx_solve(gp._dev().handle, _gpx.ptr(B), 2, _gpx.ptr(lb), _gpx.ptr(kb)), "gpx_solve")
    ref_kb, ref_lb = Kinv.dot(B.T).T, np.linalg.solve(L, B.T).T
    np.testing.assert_allclose(kb, ref_kb, rtol=1e-6, atol=1e-8 * np.abs(ref_kb).max())
    np.testing.assert_allclose(lb, ref_lb, rtol=1e-6, atol=1e-8 * np.abs(ref_lb).max())
    for q in (0, 3):                                                    # (query 3 equals a training row)
        m0, v0 = gp.estimate(xs[q])
        np.testing.assert_allclose([m0, v0], [mean[q], var[q]], rtol=1e-6, atol=1e-9 * V)
    nll = cov._negativeloglikelihood(x, gp.t, theta)
    np.testing.assert_allclose(nll, rnll, rtol=1e-9)
    np.testing.assert_allclose(cov._log_det_cov_matrix(x, theta), rlogdet, rtol=1e-9)
    np.testing.assert_allclose(cov.inv_cov_matrix(x, theta), Kinv, rtol=1e-6, atol=1e-7 * kscale)
    assert gp._dev().jitter() == 0.0


def _chol_of(handle, n):
    out = np.empty((n, n))
    _gpx.check(_gpx.lib.gpx_chol(handle, _gpx.ptr(out)), "gpx_chol")
    return out


@pytest.mark.parametrize("nu2", NU2)
def test_fit_matrix_of_the_device_gram_is_the_fit(nu2):
    """gpx_fit_matrix on gpx_matern_gram's matrix gives gpx_matern_fit's factor bit for bit.  N = 1153 pads to 1280, the smallest shape
    whose assembly is split: the first outer panel's 1024 columns, then the rest off the origin of the buffer."""
    N, d = 1153, 3
    x, t, theta = ml.make_case(N, d)
    K = _gram(x, N, x, N, d, theta, nu2)
    model = _MaternModel(x, t, theta, nu2)
    L1 = _chol_of(model.handle, N)
    assert model.jitter() == 0.0
    model.close()
    m = _MatrixModel(K, None)
    L2 = _chol_of(m.handle, N)
    assert m.jitter() == 0.0
    m.close()
    assert np.array_equal(L1, L2), np.abs(L1 - L2).max()


@pytest.mark.parametrize("nu2", NU2)
def test_few_and_many_queries_and_the_place_in_the_batch(nu2):
    """N = 2100 (three slabs: the few-vector solver serves up to 32 queries): 32 and 33 queries against the same NumPy reference; the same
    query at two places among 300 and in a call of 33 gives the same bits (the many-row solver computes a row whatever its neighbours)"""
    N, d = 2100, 3
    x, t, theta = ml.make_case(N, d)
    xs = ml.make_queries(x, 300, 41)
    xs[250] = xs[7]
    model = _MaternModel(x, t, theta, nu2)
    _Kinv, _alpha, rm, rv, _nll, _ld, _L = _numpy_reference(x, t, theta, nu2, xs, np.float64)
    for m in (32, 33, 300):
        mean, var = model.predict(np.ascontiguousarray(xs[:m]))
        np.testing.assert_allclose(mean, rm[:m], rtol=1e-6, atol=1e-9 * V, err_msg="m=%d" % m)
        np.testing.assert_allclose(var, rv[:m], rtol=1e-6, atol=1e-9 * V, err_msg="m=%d" % m)
    m300, v300 = model.predict(xs)
    assert m300[250] == m300[7] and v300[250] == v300[7]
    m33, v33 = model.predict(np.ascontiguousarray(xs[:33]))
    assert m33[7] == m300[7] and v33[7] == v300[7]
    model.close()


@pytest.mark.parametrize("nu2", NU2)
def test_predict_from_five_slabs_on(nu2):
    """N = 5200 (six slabs of 1024 columns): the left-looking solve with emulated updates needs a bound on every solved row -- sqrt(v + vt)
    here, the equality term included.  Against NumPy's Cholesky of the model's K on SURVEY 8a's bounds; 300 queries, one a training row."""
    N, d, m = 5200, 2, 300
    x, t, theta = ml.make_case(N, d)
    xs = ml.make_queries(x, m, 31)
    model = _MaternModel(x, t, theta, nu2)
    mean, var = model.predict(xs)
    assert model.jitter() == 0.0
    model.close()
    _Kinv, _alpha, rm, rv, _nll, _ld, _L = _numpy_reference(x, t, theta, nu2, xs, np.float64)
    np.testing.assert_allclose(mean, rm, rtol=1e-6, atol=1e-9 * V)
    np.testing.assert_allclose(var, rv, rtol=1e-6, atol=1e-9 * V)


# ------------------------------------------------------------------------------------------------
# gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu2", NU2)
@pytest.mark.parametrize("d", ml.D_ALL)
@pytest.mark.parametrize("N", ml.GRAD_N)
def test_gradient_against_the_model(N, d, nu2):
    x, t, theta = ml.make_case(N, d)
    model = _MaternModel(x, t, theta, nu2)
    g1, g2 = model.nll_grad(), model.nll_grad()
    np.testing.assert_array_equal(g1, g2)                                # fixed-order reduction
    Kinv, alpha = model.kinv(), model.alpha()
    model.close()
    want, scale = ml.grad(x, theta, nu2, Kinv, alpha)
    ref, _ = ml.grad(x, theta, nu2, Kinv, alpha, np.float64)
    rho = float(ml.distances(ref, want, scale).max())
    dist = ml.distances(g1, want, scale)
    _record("grad N=%d d=%d nu2=%d: rho_ref %.3e bound %.3e device worst %.3e = %.5f of the bound" % (N, d, nu2, rho, ml.bound(rho), dist.max(), dist.max() / ml.bound(rho)))
    ml.assert_within({"grad": dist}, rho, "gpx_matern_nll_grad N=%d d=%d nu2=%d" % (N, d, nu2))


@pytest.mark.parametrize("nu2", NU2)
def test_jitter_retry(nu2):
    """duplicated training rows without noise: K is exactly singular, the fit retries with +1e-5 I as gpx_fit_matrix does on the same K"""
    x = np.repeat((0.05 * np.arange(128.0))[:, None], 2, 0)
    theta = np.array([np.log(2.0), -np.inf, np.log(0.05)])
    t = np.sin(x[:, 0])
    t = t - t.mean()
    Knp = ml.kernel_parts(x, x, theta, nu2, np.float64)["K"]
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(Knp)
    pm, mm = _MaternModel(x, t, theta, nu2), _MatrixModel(Knp, t)
    assert pm.jitter() == 1e-5 and mm.jitter() == 1e-5
    xs = np.linspace(0.0, 6.4, 50)[:, None]
    kv = ml.kernel_parts(xs, x, theta, nu2, np.float64)["K"]
    m1, v1 = pm.predict(xs)
    m2, v2 = mm.predict_kv(kv, np.full(50, V))
    np.testing.assert_allclose(m1, m2, rtol=1e-6, atol=1e-6)             # (cond (K + 1e-5 I) ~ 1e6: the two factor different roundings of K)
    np.testing.assert_allclose(v1, v2, rtol=1e-6, atol=1e-7 * V)
    pm.close()
    mm.close()


@pytest.mark.parametrize("nu2", NU2)
def test_ml_fit(nu2):
    """GaussianProcess(x, t, MaternCovariance(nu)) without theta: L-BFGS-B on the fused NLL / gradient, judged by the NumPy restatement
    (the judge of tests/test_periodic.py::test_ml_fit); the NLL at the returned theta is not above the start's"""
    rng = np.random.RandomState(11)
    x = np.sort(rng.uniform(0, 10, 60))[:, None]
    t = np.sin(2 * np.pi * x[:, 0] / 2.5) + 0.1 * rng.randn(60)
    cov = _cov(nu2)
    gp = sk.GaussianProcess(x, t, cov)

    def judge(theta):
        K = ml.kernel_parts(x, x, theta, nu2, np.float64)["K"]
        Kinv = np.linalg.inv(K)
        g, _ = ml.grad(x, theta, nu2, Kinv, Kinv.dot(gp.t), np.float64)
        return ml.nll(K, gp.t), g

    nll0, _g0 = judge(cov.get_theta(x, gp.t))
    nll1, g1 = judge(gp.theta_min)
    assert nll1 <= nll0, (nll0, nll1)
    assert np.abs(g1).max() < 5e-2 * max(1.0, abs(nll1)), (g1, nll1)


# ------------------------------------------------------------------------------------------------
# propagation, nu = 5/2: the fused route against the generic route on the same kernel
# ------------------------------------------------------------------------------------------------
class PyMatern(sk.Covariance):
    """MaternCovariance(2.5) restated on the base class: the generic route (gpx_fit_matrix on the operator's own matrix, C / J / H from N
    host calls each).  cov_matrix_ij is the float64 restatement of tests/_matern_ld.py instead of N^2 Python calls."""
    nu, _nu2 = 2.5, 5
    __call__ = sk.MaternCovariance.__call__
    _radial = sk.MaternCovariance._radial
    _kf_g = sk.MaternCovariance._kf_g
    get_Jacobian = sk.MaternCovariance.get_Jacobian
    get_Hessian = sk.MaternCovariance.get_Hessian
    get_theta = sk.MaternCovariance.get_theta

    def cov_matrix_ij(self, xi, xj, theta):
        return ml.kernel_parts(np.atleast_2d(xi), np.atleast_2d(xj), theta, self._nu2, np.float64)["K"]


class PyMatern32(PyMatern):
    """nu = 3/2 on the base class: no Jacobian / Hessian"""
    nu, _nu2 = 1.5, 3
    get_Jacobian = sk.Covariance.get_Jacobian
    get_Hessian = sk.Covariance.get_Hessian


PROP_CASES = ((127, 3), (1500, 8), (640, 1), (640, 8), (640, 9), (640, 64))
_PROP = {}


def _prop_gps(N, d):
    """(fused gp, generic gp, x) of the ragged recipe of tests/test_propagate_many.py with the length scales kept alive at large d"""
    if (N, d) not in _PROP:
        rng = np.random.RandomState(100 + N + d)
        x = rng.uniform(0, 10, (N, d))
        t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
        theta = np.log(np.array([2.0, 0.01] + [0.04 * min(1.0, 3.0 / d)] * d))
        gp = sk.GaussianProcess(x, t, sk.MaternCovariance(2.5), theta.copy())
        py = sk.GaussianProcess(x, t, PyMatern(), theta.copy())
        assert gp._route() == "matern" and py._route() == "generic"
        _PROP[(N, d)] = (gp, py, x)
    return _PROP[(N, d)]


def _inputs(x, B, d, seed):
    """tests/_propagate_many_worker.py's inputs: every 37th one a copy of a training row, a full SPD Sigma for each"""
    rng = np.random.RandomState(seed)
    U = rng.uniform(0, 10, (B, d))
    U[::37] = x[rng.randint(0, len(x), len(U[::37]))]
    A = rng.uniform(-0.1, 0.1, (B, d, d))
    S = np.einsum("bij,bkj->bik", A, A) + 0.005 * np.eye(d)
    return U, S


def _pick(B, seam=None):
    """at most 8 inputs: the first, the last, both sides of a chunk seam when there is one, the copy of a training row, random ones"""
    rows = {0, B - 1}
    if B > 37:
        rows.add(37)
    if seam is not None and 0 < seam < B:
        rows.update((seam - 1, seam))
    rest = [int(i) for i in np.random.RandomState(B).permutation(B) if i not in rows]
    return sorted(rows) + rest[:max(0, min(8, B) - len(rows))]


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("N,d", PROP_CASES)
def test_propagation_against_the_generic_route(N, d, B, shared):
    gp, py, x = _prop_gps(N, d)
    U, S = _inputs(x, B, d, N + B)
    Sig = S[0] if shared else S
    up = sk.UncertaintyPropagationApprox(gp)
    assert up._matern52()
    mean, var = up.propagate_GA_many(U, Sig)
    mean_only = up.propagate_mean_many(U, Sig)
    dvh, s2 = up._get_variance_dv_many(U)
    assert np.isfinite(mean).all() and np.isfinite(var).all() and np.isfinite(dvh).all() and np.isfinite(s2).all()
    np.testing.assert_array_equal(mean_only + gp.meant, mean)
    target = s2 + 0.05
    one = np.ones(d)
    sol = IUP(None, gp, None, one, one).get_best_solution_many(U, target)
    worst = [0.0] * 4
    for i in _pick(B):
        Si = Sig if shared else Sig[i]
        # the generic route's single calls: host C / J / H, two sweeps over the factor
        gen = sk.UncertaintyPropagationApprox(py)
        assert gen._generic() and not gen._matern52()
        m1, v1 = gen.propagate_GA(U[i], Si)
        d1 = np.array([gen._get_variance_dv_h(U[i], h) for h in range(d)])
        s1 = gen._get_sigma2(U[i])
        worst = [max(a, b) for a, b in zip(worst, (abs(mean[i] - m1), abs(var[i] - v1), np.abs(dvh[i] - d1).max(), abs(s2[i] - s1)))]
        assert mean[i] == pytest.approx(m1, abs=2 * 1e-9) and var[i] == pytest.approx(v1, abs=2 * 1e-8 * V), i
        np.testing.assert_allclose(dvh[i], d1, rtol=2 * 1e-6, atol=2 * 1e-8 * V, err_msg="input %d" % i)
        assert s2[i] == pytest.approx(s1, abs=2 * 2e-8), i
        # the fused single-input surface is the batch of one
        f1 = sk.UncertaintyPropagationApprox(gp)
        ms, vs = f1.propagate_GA(U[i], Si)
        assert ms == pytest.approx(m1, abs=2 * 1e-9) and vs == pytest.approx(v1, abs=2 * 1e-8 * V), i
        np.testing.assert_allclose([f1._get_variance_dv_h(U[i], h) for h in range(d)], d1, rtol=2 * 1e-6, atol=2 * 1e-8 * V)
        # C_ux / J_ux / H_ux stay host attributes
        assert f1.C_ux.shape == (N,) and f1.J_ux.shape == (N, d, 1) and f1.H_ux.shape == (N, d, d)
        # the inverse propagation: where every dvh_k is safely positive, the closed form of both routes and the single call
        if (d1 > 1e-3).all():
            ref = IUP._closed_form(d1[None], np.array([s1]), one, one, [], target[i:i + 1])[0]
            bound = 1.1 * (2 * 2e-8 / 0.05 + (2e-6 + 2e-8 * V / d1).max())
            assert np.isfinite(sol[i]).all() and (np.abs(sol[i] - ref) <= bound * np.abs(ref)).all(), (i, sol[i], ref)
            single = IUP(target[i], gp, U[i], one, one).get_best_solution()
            gsingle = IUP(target[i], py, U[i], one, one).get_best_solution()
            assert (np.abs(single - gsingle) <= bound * np.abs(gsingle)).all(), (i, single, gsingle)
    _record("propagation N=%d d=%d B=%d %s: worst dmean %.3e dvar %.3e ddvh %.3e dsigma2 %.3e" % ((N, d, B, "shared" if shared else "per-input") + tuple(worst)))


def _raw_approx(gp, U, S, shared):
    U, S = _gpx.f64(U), _gpx.f64(S)
    out = [np.empty(len(U)) for _ in range(4)]
    _gpx.check(_gpx.lib.gpx_matern_propagate_approx_many(gp._dev().handle, _gpx.ptr(U), _gpx.ptr(S), int(shared), len(U), *[_gpx.ptr(o) for o in out]),
               "gpx_matern_propagate_approx_many")
    return out


def _raw_dvh(gp, U):
    U = _gpx.f64(U)
    dvh, s2 = np.empty((len(U), gp.d)), np.empty(len(U))
    _gpx.check(_gpx.lib.gpx_matern_propagate_dvh_many(gp._dev().handle, _gpx.ptr(U), len(U), _gpx.ptr(dvh), _gpx.ptr(s2)), "gpx_matern_propagate_dvh_many")
    return dvh, s2


def test_independence_of_position_split_and_sigma_form():
    """an input's result does not depend on its place in the batch, on the other inputs, or on how Sigma is passed; the split holds bit
    for bit when both calls have more than 32 solver rows (below that the few-right-hand-side solver serves the call)"""
    gp, _py, x = _prop_gps(1500, 8)
    B, d = 130, gp.d
    U, S = _inputs(x, B, d, 77)
    cut = 47
    for raw in (lambda UU, SS: _raw_approx(gp, UU, SS, False), lambda UU, SS: _raw_dvh(gp, UU)):
        one, rev = raw(U, S), raw(U[::-1], S[::-1])
        for a, b in zip(one, rev):
            np.testing.assert_array_equal(a, b[::-1])
        head, tail = raw(U[:cut], S[:cut]), raw(U[cut:], S[cut:])
        for a, h, t in zip(one, head, tail):
            np.testing.assert_array_equal(a, np.concatenate([h, t]))
    shared = _raw_approx(gp, U, S[5], True)
    repeated = _raw_approx(gp, U, np.repeat(S[5][None], B, 0), False)
    for a, b in zip(shared, repeated):
        np.testing.assert_array_equal(a, b)


def test_chunk_seam_of_the_batched_calls():
    """N = 127, d = 8, B = 3300: 33000 Approx rows against the 32768-row chunk (3276 inputs in the first), 56100 dvh rows (1927 a chunk);
    the inputs on both sides of each seam against the generic route, the first chunk's inputs bit for bit a call on them alone"""
    gp, py, x = _prop_gps(127, 8)
    B, d = 3300, 8
    U, S = _inputs(x, B, d, 127 + B)
    out = _raw_approx(gp, U, S[0], True)
    dvh, s2 = _raw_dvh(gp, U)
    first_a, first_d = 32768 // (d + 2), 32768 // (2 * d + 1)
    assert first_a < B and first_d < B and all(np.isfinite(o).all() for o in out) and np.isfinite(dvh).all()
    for a, b in zip(out, _raw_approx(gp, U[:first_a], S[0], True)):
        np.testing.assert_array_equal(a[:first_a], b)
    np.testing.assert_array_equal(dvh[:first_d], _raw_dvh(gp, U[:first_d])[0])
    for i in (first_a - 1, first_a, first_d - 1, first_d):
        gen = sk.UncertaintyPropagationApprox(py)
        m1, v1 = gen.propagate_GA(U[i], S[0])
        assert out[0][i] + gp.meant == pytest.approx(m1, abs=2 * 1e-9) and out[1][i] == pytest.approx(v1, abs=2 * 1e-8 * V), i
        d1 = np.array([gen._get_variance_dv_h(U[i], h) for h in range(d)])
        np.testing.assert_allclose(dvh[i], d1, rtol=2 * 1e-6, atol=2 * 1e-8 * V, err_msg="input %d" % i)


@pytest.mark.parametrize("nu2", NU2)
def test_numerical_hg_fused_against_host_built_nodes(nu2):
    """UncertaintyPropagationNumericalHG on the fused route (gpx_propagate_quadrature_many through handle_gram) against host-built nodes ->
    estimate_many -> gpx_mixture_reduce.  The node coordinates differ by rounding between host and device: the bounds are the parity
    bounds on a predicted row (mean 1e-9, variance 1e-8 v), twice, as tests/test_quadrature.py's seam comparison takes them."""
    x, t, theta = ml.make_case(203, 3)
    gp = sk.GaussianProcess(x, t, _cov(nu2), theta.copy())
    assert gp._route() == "matern"
    rng = np.random.RandomState(8)
    U = 2.0 + 6.0 * rng.uniform(0.0, 1.0, (4, 3))
    Sigma = np.diag([0.09, 0.04, 0.0625])
    Y = np.linspace(-1, 1, 7) + gp._get_mean_t()
    up = sk.UncertaintyPropagationNumericalHG(gp, order=3)
    mean, var, m3, m4 = up.propagate_moments_many(U, Sigma)
    dens = up.propagate_density_many(Y, U, Sigma)
    z, wq = qm.hg_rule(3, 3)
    mu, s2 = gp.estimate_many(qm.nodes_plain(U, qm.hg_root(Sigma), z).reshape(4 * len(wq), 3))
    mom, dd = np.empty((5, 4)), np.empty((4, 7))
    wqa, mua, s2a = _gpx.f64(wq), _gpx.f64(mu), _gpx.f64(s2)
    _gpx.check(_gpx.lib.gpx_mixture_reduce(_gpx.ptr(mua), _gpx.ptr(s2a), _gpx.ptr(wqa), len(wq), 4, _gpx.ptr(_gpx.f64(Y)), 7, 1, 0.0, _gpx.ptr(mom),
                                           _gpx.ptr(dd)), "gpx_mixture_reduce")
    EMU, EVAR = 1e-9, 1e-8
    assert np.all(np.abs(mean - mom[0]) <= 2 * EMU) and np.all(np.abs(var - mom[1]) <= 2 * (2 * EVAR * V + 4 * EMU))
    np.testing.assert_allclose(dens, dd, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(m3, mom[3], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(m4, mom[4], rtol=1e-6, atol=1e-9)
    assert np.all(var > 0) and np.all(np.isfinite(dens))


# ------------------------------------------------------------------------------------------------
# nu = 3/2 and errors
# ------------------------------------------------------------------------------------------------
def _outcome(f):
    try:
        return ("value", np.asarray(f(), dtype=float))
    except Exception as e:  # noqa: BLE001  (the test compares exception TYPES)
        return ("raises", type(e))


def test_three_halves_is_propagated_as_a_generic_operator():
    x, t, theta = ml.make_case(60, 2, seed=123)
    gp = sk.GaussianProcess(x, t, sk.MaternCovariance(1.5), theta.copy())
    py = sk.GaussianProcess(x, t, PyMatern32(), theta.copy())
    assert gp._route() == "matern" and py._route() == "generic"
    xs = ml.make_queries(x, 20, 5)
    for a, b in zip(gp.estimate_many(xs), py.estimate_many(xs)):
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-9 * V)
    u, S = np.array([4.5, 5.25]), np.diag([0.02, 0.03])
    for cls in (sk.UncertaintyPropagationExact, sk.UncertaintyPropagationApprox):
        a = _outcome(lambda: cls(gp).propagate_GA(u, S))
        b = _outcome(lambda: cls(py).propagate_GA(u, S))
        assert a[0] == b[0], (cls.__name__, a, b)
        if a[0] == "value":
            np.testing.assert_allclose(a[1], b[1], rtol=1e-6, atol=1e-8 * V)
        else:
            assert a[1] is b[1], (cls.__name__, a, b)
    assert _outcome(lambda: sk.UncertaintyPropagationApprox(gp).propagate_GA(u, S)) == ("raises", NotImplementedError)
    # the Exact class treats nu = 5/2 the same way
    gp5 = sk.GaussianProcess(x, t, sk.MaternCovariance(2.5), theta.copy())
    py5 = sk.GaussianProcess(x, t, PyMatern(), theta.copy())
    np.testing.assert_allclose(sk.UncertaintyPropagationExact(gp5).propagate_GA(u, S), sk.UncertaintyPropagationExact(py5).propagate_GA(u, S),
                               rtol=1e-6, atol=1e-8 * V)
    # and the fused entry points refuse the handle without touching an output
    out = [np.full(1, 7.25) for _ in range(4)]
    lib = _gpx.lib
    assert lib.gpx_matern_propagate_approx_many(gp._dev().handle, _gpx.ptr(u), _gpx.ptr(S), 1, 1, *[_gpx.ptr(o) for o in out]) == _gpx.GPX_ERR_STATE
    dv = np.full(2, 7.25)
    assert lib.gpx_matern_propagate_dvh_many(gp._dev().handle, _gpx.ptr(u), 1, _gpx.ptr(dv), _gpx.ptr(out[0])) == _gpx.GPX_ERR_STATE
    assert all((o == 7.25).all() for o in out) and (dv == 7.25).all()


def test_state_errors_touch_no_output():
    from skgpuppy_amd.GaussianProcess import _DeviceModel
    import _periodic_ld as pl
    x, t, theta = ml.make_case(130, 2)
    lib = _gpx.lib
    P = _gpx.ptr
    mt = _MaternModel(x, t, theta, 5)
    gm = _DeviceModel(x, t, theta.copy())
    pm = _PeriodicModel(x, t, pl.make_case(130, 2)[2])
    mm = _MatrixModel(ml.kernel_parts(x, x, theta, 5, np.float64)["K"], t)
    u, S = _gpx.f64(x[0]), np.eye(2)

    def fresh():
        return [np.full(300, 7.25) for _ in range(4)]

    # every gpx_matern_* on a Gaussian, periodic or matrix handle
    for h in (gm.handle, pm.handle, mm.handle):
        for call in (lambda o: lib.gpx_matern_predict(h, P(x), 2, P(o[0]), P(o[1])),
                     lambda o: lib.gpx_matern_nll_grad(h, P(o[0])),
                     lambda o: lib.gpx_matern_propagate_approx_many(h, P(u), P(S), 1, 1, P(o[0]), P(o[1]), P(o[2]), P(o[3])),
                     lambda o: lib.gpx_matern_propagate_dvh_many(h, P(u), 1, P(o[0]), P(o[1]))):
            o = fresh()
            assert call(o) == _gpx.GPX_ERR_STATE and "gpx_matern_fit" in _gpx.last_error()
            assert all((a == 7.25).all() for a in o)
    # every Gaussian-only entry point, and the periodic ones, on a Matern handle
    h = mt.handle
    dbl = [ctypes.c_double(7.25) for _ in range(4)]
    ref = [ctypes.byref(c) for c in dbl]
    gauss = (lambda o: lib.gpx_predict(h, P(x), 2, P(o[0]), P(o[1])),
             lambda o: lib.gpx_cjh(h, P(u), P(o[0]), P(o[1]), P(o[2])),
             lambda o: lib.gpx_nll_grad(h, P(o[0])),
             lambda o: lib.gpx_propagate_approx(h, P(u), P(S), *ref),
             lambda o: lib.gpx_propagate_approx_many(h, P(u), P(S), 1, 1, P(o[0]), P(o[1]), P(o[2]), P(o[3])),
             lambda o: lib.gpx_propagate_dvh(h, P(u), P(o[0])),
             lambda o: lib.gpx_propagate_dvh_many(h, P(u), 1, P(o[0]), P(o[1])),
             lambda o: lib.gpx_propagate_exact(h, P(u), P(S), ref[0], ref[1]),
             lambda o: lib.gpx_exact_mean(h, P(u), P(S), ref[0]),
             lambda o: lib.gpx_propagate_exact_many(h, P(u), P(S), 1, 1, P(o[0]), P(o[1])))
    for i, call in enumerate(gauss):
        o = fresh()
        assert call(o) == _gpx.GPX_ERR_STATE and "gpx_matern_" in _gpx.last_error(), i
        assert all((a == 7.25).all() for a in o) and all(c.value == 7.25 for c in dbl), i
    for call in (lambda o: lib.gpx_periodic_predict(h, P(x), 2, P(o[0]), P(o[1])), lambda o: lib.gpx_periodic_nll_grad(h, P(o[0]))):
        o = fresh()
        assert call(o) == _gpx.GPX_ERR_STATE and all((a == 7.25).all() for a in o)
    # what a Matern handle does answer: everything of a matrix handle, gpx_n with its d
    n, d = ctypes.c_int64(), ctypes.c_int()
    assert lib.gpx_n(h, ctypes.byref(n), ctypes.byref(d)) == 0 and (n.value, d.value) == (130, 2)
    assert mt.solve(np.eye(130)[:2]).shape == (2, 130) and np.isfinite(mt.nll()) and mt.jitter() == 0.0
    np.testing.assert_allclose(mt.nll_grad_entry(sk.MaternCovariance()._d_cov_matrix_d_theta(x, theta, 0)), mt.nll_grad()[0], rtol=1e-9)
    # bad arguments: refused with text
    K = np.empty((130, 130))
    hh = ctypes.c_void_p()
    th = P(theta)
    bad = [lib.gpx_matern_gram(P(x), 130, P(x), 130, 2, th, 4, -1, P(K)),
           lib.gpx_matern_gram(P(x), 130, P(x), 130, 2, th, 1, -1, P(K)),
           lib.gpx_matern_gram(P(x), 130, P(x), 130, 0, th, 5, -1, P(K)),
           lib.gpx_matern_gram(P(x), 130, P(x), 130, 65, th, 5, -1, P(K)),
           lib.gpx_matern_gram(None, 130, P(x), 130, 2, th, 5, -1, P(K)),
           lib.gpx_matern_gram(P(x), 130, P(x), 130, 2, None, 5, -1, P(K)),
           lib.gpx_matern_gram(P(x), 0, P(x), 130, 2, th, 5, -1, P(K)),
           lib.gpx_matern_gram(P(x), 130, P(x), 130, 2, th, 5, 4, P(K)),
           lib.gpx_matern_gram(P(x), 130, P(x), 130, 2, th, 5, -2, P(K)),
           lib.gpx_matern_fit(P(x), P(t), 130, 2, th, 2, None, ctypes.byref(hh)),
           lib.gpx_matern_fit(P(x), P(t), 0, 2, th, 5, None, ctypes.byref(hh)),
           lib.gpx_matern_fit(None, P(t), 130, 2, th, 5, None, ctypes.byref(hh)),
           lib.gpx_matern_fit(P(x), P(t), 130, 2, th, 5, None, None),
           lib.gpx_matern_predict(h, None, 2, P(K), P(K)),
           lib.gpx_matern_nll_grad(h, None),
           lib.gpx_matern_nll_grad(None, P(K)),
           lib.gpx_matern_propagate_approx_many(h, None, P(S), 1, 1, P(K), P(K), None, None),
           lib.gpx_matern_propagate_dvh_many(h, P(u), 1, None, None)]
    for i, st in enumerate(bad):
        assert st == _gpx.GPX_ERR_BAD_ARG, (i, st)
    assert _gpx.last_error() and not hh
    assert lib.gpx_matern_predict(h, None, 0, None, None) == 0
    for m in (mt, gm, pm, mm):
        m.close()
