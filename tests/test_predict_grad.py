"""The predictor's input gradients on the device: gpx_predict_mean_grad (mu and grad mu from alpha, no solve), gpx_predict_grad (d + 1 solved
rows a query: mu, sigma^2 and both gradients), GaussianProcess.estimate_many_gradient and UncertaintyPropagationLinear.

(a) the alpha route against the long-double model of tests/_predict_grad_model.py on the device's own alpha, by the project's rule (the bound
    comes from the float64 evaluation of the same case), every (N, d) of both templates, the Gaussian kernel and both Matern nu;
(b) the solver route against the model on the oracle's K^-1 and beta, with the tolerances of tests/test_gpu_parity.py (1e-9 k for means,
    1e-8 v k for variances, k = 10 for metis) times g_k = max(1, w_k max_i |x_ik - u_k|) for grad mu_k and twice that for grad sigma^2_k: the
    J rows are the C row scaled entrywise by at most g_k, and grad sigma^2 carries the factor 2;
(c) one answer: both routes and gpx_predict agree, also at a query bit-equal to a training row;
(d) a query's outputs do not depend on its place in the batch, and a batch of more rows than a chunk is cut between two queries;
(e) periodic and supplied-matrix handles are refused, and their Python route takes central differences;
(f) UncertaintyPropagationLinear against the reference's recorded outputs (tests/golden/linear.npz) and the analytic model.

A Gaussian handle's rows carry no +vt on equality (gpx_predict's are GaussianCovariance.cov_matrix_ij's), a Matern handle's do (gpx_matern_predict):
mean and variance are the handle's own predictor's at every query, and the model is evaluated with the kind's own convention."""
import ctypes

import numpy as np
import pytest

from conftest import GP_CASES, load_golden, torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from oracle import oracle as orc

import _dense_ld as dl
import _predict_grad_model as pg
from _propagate_many_worker import inputs as _inputs

pytestmark = pytest.mark.gpu

GPX_K_GEMM, GPX_K_TRSV, GPX_K_GEMM_SMALL, GPX_K_TRSV_RIDE, GPX_K_GEMM_EMU = 1, 3, 7, 8, 9      # include/gpx.h: the solve classes


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _cov(nu2):
    return sk.GaussianCovariance() if nu2 == 0 else sk.MaternCovariance(nu2 / 2.0)


def mean_grad(h, xs, want_mean=True, want_grad=True):
    xs = _gpx.f64(xs)
    m, d = xs.shape
    mean, g = np.empty(m), np.empty((m, d))
    _gpx.check(_gpx.lib.gpx_predict_mean_grad(h, _gpx.ptr(xs), m, _gpx.ptr(mean) if want_mean else None, _gpx.ptr(g) if want_grad else None),
               "gpx_predict_mean_grad")
    return mean, g


def full_grad(h, xs, want_dmean=True):
    xs = _gpx.f64(xs)
    m, d = xs.shape
    mean, var, dm, dv = np.empty(m), np.empty(m), np.empty((m, d)), np.empty((m, d))
    _gpx.check(_gpx.lib.gpx_predict_grad(h, _gpx.ptr(xs), m, _gpx.ptr(mean), _gpx.ptr(var), _gpx.ptr(dm) if want_dmean else None, _gpx.ptr(dv)),
               "gpx_predict_grad")
    return mean, var, dm, dv


def predict(gp, xs):
    return gp._dev().predict(_gpx.f64(xs))


def _expected(x, theta, alpha, Kinv, U, nu2):
    """the float64 model on a given K^-1 and alpha: (mean, var, dmean, dvar, g_k)"""
    m = pg.mean_grad(x, theta, alpha, U, nu2, dt=np.float64)
    v = pg.var_grad(x, theta, Kinv, U, nu2, dt=np.float64)
    return m["mean"][0], v["var"][0], m["dmean"][0], v["dvar"][0], pg.grad_scale(x, theta, U)


def _assert_parity(what, got, exp, v, k=1.0, factor=1.0):
    """got = (mean, var, dmean, dvar) against exp = (mean, var, dmean, dvar, g) within factor times the tolerances of (b)"""
    mean, var, dm, dv = got
    em, ev, edm, edv, g = exp
    worst = (np.abs(mean - em).max(), np.abs(var - ev).max(), (np.abs(dm - edm) / g).max(), (np.abs(dv - edv) / g).max())
    print("%s: worst dmean %.3e dvar %.3e dgradmean/g %.3e dgradvar/g %.3e" % ((what,) + worst))
    assert np.isfinite(mean).all() and np.isfinite(var).all() and np.isfinite(dm).all() and np.isfinite(dv).all()
    assert worst[0] <= factor * 1e-9 * k and worst[1] <= factor * 1e-8 * v * k, what
    assert worst[2] <= factor * 1e-9 * k and worst[3] <= factor * 2e-8 * v * k, what


# ------------------------------------------------------------------------------------------------
# (a) the alpha route against the long-double model
# ------------------------------------------------------------------------------------------------
A_CASES = [(700, d) for d in (1, 3, 8, 9, 16, 64)] + [(N, d) for N in dl.SMALL_N for d in dl.SMALL_D]
NQ = 20                      # distinct queries a case: between, equal, far, 17 random ones


def _queries(x, theta, seed):
    ins = dl.inputs_u(x, theta, seed)
    rng = np.random.RandomState(seed + 13)
    return np.vstack([ins["between"], ins["equal"], ins["far"], dl._grid(rng.uniform(0, 10, (NQ - 3, x.shape[1])))])


@pytest.mark.parametrize("nu2", pg.KINDS)
@pytest.mark.parametrize("N,d", A_CASES)
def test_alpha_route_against_long_double(N, d, nu2):
    """M = 1 (one query), 17 (a ragged query block) and 200 (more than one block: the 20 distinct queries repeated in a seeded order, each held
    to the model of its source); N = 700 at every d of both templates and the last d, N = 128 / 129 / 200: no padding, 127 padded columns,
    one partial tile"""
    seed = dl.seed_of(N, d)
    x, t, theta = dl.make_case(N, d, seed)
    gp = sk.GaussianProcess(x, t, _cov(nu2), theta.copy())
    h = gp._dev().handle
    alpha = gp._get_beta()
    Q = _queries(x, theta, seed)
    ld = pg.mean_grad(x, theta, alpha, Q, nu2)
    f64 = pg.mean_grad(x, theta, alpha, Q, nu2, dt=np.float64)
    ref = {k: dl.distances(f64[k][0], ld[k][0], ld[k][1]) for k in ld}
    rho = dl.rho_of(ref)
    order = np.random.RandomState(seed + 1).randint(0, NQ, 200)
    order[:NQ] = np.arange(NQ)
    for M in (1, 17, 200):
        src = order[:M]
        mean, g = mean_grad(h, Q[src])
        dist = {"mean": dl.distances(mean, ld["mean"][0][src], ld["mean"][1][src]), "dmean": dl.distances(g, ld["dmean"][0][src], ld["dmean"][1][src])}
        dl.record("alpha route nu2=%d M=%d" % (nu2, M), "N=%d d=%d" % (N, d), rho, dist, ref)
        dl.assert_within(dist, rho, "alpha route N=%d d=%d nu2=%d M=%d" % (N, d, nu2, M))
        # the same mean as the predictor's (two device paths each held to 1e-9)
        pm, _pv = predict(gp, Q[src])
        assert np.abs(mean - pm).max() <= 2e-9, (M, np.abs(mean - pm).max())
        # either output alone
        m_only, _ = mean_grad(h, Q[src], want_grad=False)
        _, g_only = mean_grad(h, Q[src], want_mean=False)
        np.testing.assert_array_equal(m_only, mean)
        np.testing.assert_array_equal(g_only, g)


# ------------------------------------------------------------------------------------------------
# (b) the solver route against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GP_CASES)
def test_solver_route_on_the_fixtures(name):
    g = load_golden(name)
    x, t, theta = np.asarray(g["x"], dtype=float), g["t_raw"], g["theta"]
    gp = sk.GaussianProcess(g["x"], t, sk.GaussianCovariance(), theta.copy())
    og = orc.OracleGP(g["x"], t, theta)
    U = np.array([g["u%d" % i] for i in range(int(g["nu"]))], dtype=float)
    exp = _expected(x, theta, og.beta(), og.Kinv, U, 0)
    _assert_parity("fixture " + name, full_grad(gp._dev().handle, U), exp, np.exp(theta[0]), 10.0 if name == "metis" else 1.0)


_RAGGED = {}


def _ragged(N, nu2=0):
    """the models of tests/test_propagate_many.py's ragged cases (Gaussian), and at N = 127 the same data under both Matern nu"""
    if (N, nu2) not in _RAGGED:
        d = {127: 3, 640: 6, 1500: 8}[N]
        rng = np.random.RandomState(100 + N + d)
        x = rng.uniform(0, 10, (N, d))
        t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
        theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
        if nu2 == 0:
            og = orc.OracleGP(x, t, theta)
        else:
            class Scalar(orc.OracleCovariance):
                cov = sk.MaternCovariance(nu2 / 2.0)

                def __call__(self, xi, xj, th):
                    return self.cov(xi, xj, th)
            og = orc.OracleOperatorGP(x, t, Scalar(), theta)
        _RAGGED[(N, nu2)] = (sk.GaussianProcess(x, t, _cov(nu2), theta.copy()), x, theta, og.beta(), og.Kinv)
    return _RAGGED[(N, nu2)]


@pytest.mark.parametrize("B", [1, 3, 130, 517])
@pytest.mark.parametrize("N", [127, 640, 1500])
def test_solver_route_ragged_batches(N, B):
    """every 37th query a copy of a training row"""
    gp, x, theta, beta, Kinv = _ragged(N)
    U, _S = _inputs(x, B, gp.d, N + B)
    _assert_parity("ragged N=%d B=%d" % (N, B), full_grad(gp._dev().handle, U), _expected(x, theta, beta, Kinv, U, 0), 2.0)


@pytest.mark.parametrize("B", [3, 130])
@pytest.mark.parametrize("nu2", [3, 5])
def test_solver_route_matern(nu2, B):
    """both nu on the solver route (nu = 3/2 has its own radial factors in the build kernel); the copies of training rows carry +vt in C"""
    gp, x, theta, beta, Kinv = _ragged(127, nu2)
    U, _S = _inputs(x, B, gp.d, 127 + B)
    _assert_parity("matern nu2=%d B=%d" % (nu2, B), full_grad(gp._dev().handle, U), _expected(x, theta, beta, Kinv, U, nu2), 2.0)


# ------------------------------------------------------------------------------------------------
# (c) one answer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu2", pg.KINDS)
def test_one_answer(nu2):
    gp, x, theta, beta, Kinv = _ragged(127, nu2)
    h = gp._dev().handle
    U, _S = _inputs(x, 130, gp.d, 127 + 130)          # queries 0, 37, 74, 111: copies of training rows
    mean, var, dm, dv = full_grad(h, U)
    pm, pv = predict(gp, U)
    assert np.abs(mean - pm).max() <= 2e-9 and np.abs(var - pv).max() <= 2 * 1e-8 * 2.0
    am, ag = mean_grad(h, U)
    g = pg.grad_scale(x, theta, U)
    assert (np.abs(dm - ag) / g).max() <= 2e-9 and np.abs(am - mean).max() <= 2e-9
    # dmean_out may be null: the other three outputs are the same bits
    m2, v2, _none, dv2 = full_grad(h, U, want_dmean=False)
    for a, b in ((m2, mean), (v2, var), (dv2, dv)):
        np.testing.assert_array_equal(a, b)
    # at a query bit-equal to a training row: mean and variance are estimate_many's, the gradients finite and the model's
    eq = np.arange(0, 130, 37)
    assert all((x == U[i]).all(1).any() for i in eq)
    em, ev = gp.estimate_many(U[eq])
    assert np.abs(em - (mean[eq] + gp.meant)).max() <= 2e-9 and np.abs(ev - var[eq]).max() <= 2 * 1e-8 * 2.0
    exp = _expected(x, theta, beta, Kinv, U[eq], nu2)
    _assert_parity("equal rows nu2=%d" % nu2, (mean[eq], var[eq], dm[eq], dv[eq]), exp, 2.0)
    if nu2:    # the bump is in C: without it the model's mean is off by vt alpha_i, far beyond the tolerance
        off = pg.mean_grad(x, theta, beta, U[eq], nu2, quirk=False, dt=np.float64)["mean"][0]
        assert np.abs(off - mean[eq]).min() > 1e-6
    # the Python method returns the same numbers, meant added
    r = gp.estimate_many_gradient(U)
    for a, b in zip(r, (mean + gp.meant, var, dm, dv)):
        np.testing.assert_array_equal(a, b)
    r2 = gp.estimate_many_gradient(U, variance=False)
    np.testing.assert_array_equal(r2[0], am + gp.meant)
    np.testing.assert_array_equal(r2[1], ag)
    one = gp.estimate_gradient(U[5])
    assert one[0] == pytest.approx(r[0][5], abs=2e-9) and one[2].shape == (gp.d,) and np.abs(one[3] - dv[5]).max() <= 4e-8 * 2.0 * g[5].max()


# ------------------------------------------------------------------------------------------------
# (d) position independence and the chunk seam
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu2", pg.KINDS)
def test_a_permuted_batch_returns_the_same_bits(nu2):
    gp, x, _theta, _beta, _Kinv = _ragged(127, nu2)
    h = gp._dev().handle
    U, _S = _inputs(x, 130, gp.d, 77)
    perm = np.random.RandomState(5).permutation(130)
    for route in (lambda q: full_grad(h, q), lambda q: mean_grad(h, q)):
        a, b = route(U), route(U[perm])
        for p, q in zip(a, b):
            np.testing.assert_array_equal(p[perm], q)


_SEAM = {}


def _seam_gp():
    if not _SEAM:
        N, d = 127, 8
        rng = np.random.RandomState(100 + N + d)
        x = rng.uniform(0, 10, (N, d))
        t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
        theta = np.log(np.array([2.0, 0.01] + [0.04 * 3.0 / d] * d))
        og = orc.OracleGP(x, t, theta)
        _SEAM["gp"] = (sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy()), x, theta, og.beta(), og.Kinv)
    return _SEAM["gp"]


def test_chunk_seam():
    """N = 127, d = 8, B = 3700: 33300 rows against the 32768-row chunk, 3640 queries in the first chunk"""
    gp, x, theta, beta, Kinv = _seam_gp()
    h = gp._dev().handle
    B, first = 3700, 32768 // 9
    U, _S = _inputs(x, B, 8, 4242)
    out = full_grad(h, U)
    for a in out:
        assert np.isfinite(a).all()
    pick = sorted(set([0, 1, first - 2, first - 1, first, first + 1, B - 2, B - 1] + list(np.random.RandomState(8).randint(0, B, 12))))
    _assert_parity("chunk seam", tuple(a[pick] for a in out), _expected(x, theta, beta, Kinv, U[pick], 0), 2.0)
    alone = full_grad(h, U[:first])
    for a, b in zip(out, alone):
        np.testing.assert_array_equal(a[:first], b)


# ------------------------------------------------------------------------------------------------
# (e) refusals, and the central-difference routes
# ------------------------------------------------------------------------------------------------
class PlainGaussian(sk.GaussianCovariance):
    """the built-in kernel behind the generic route: an overridden matrix builder"""

    def cov_matrix_ij(self, xi, xj, theta):
        return sk.GaussianCovariance.cov_matrix_ij(self, xi, xj, theta)


def _small_case():
    """the case of tests/test_predict_grad_model.py: N = 60, d = 3, v = 2, vt = 0.05, w in [0.3, 0.6]"""
    rng = np.random.RandomState(2214)
    x = pg._grid(rng.uniform(0, 10, (60, 3)))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(60)
    theta = np.log(np.concatenate([[2.0, 0.05], rng.uniform(0.3, 0.6, 3)]))
    return x, t, theta, pg._grid(rng.uniform(2, 8, (5, 3)))


def test_refused_kinds_and_their_python_route():
    x, t, theta, xs = _small_case()
    gen = sk.GaussianProcess(x, t, PlainGaussian(), theta.copy())
    per = sk.GaussianProcess(x, t, sk.PeriodicCovariance(), np.concatenate([theta, np.log(np.full(3, 4.0)), np.log(np.full(3, 0.5))]))
    assert gen._route() == "generic" and per._route() == "periodic"
    for gp, word in ((gen, "gpx_fit_matrix"), (per, "PeriodicCovariance")):
        outs = [np.full(15, 7.25) for _ in range(4)]
        st = _gpx.lib.gpx_predict_grad(gp._dev().handle, _gpx.ptr(xs), 5, *[_gpx.ptr(o) for o in outs])
        assert st == _gpx.GPX_ERR_STATE and word in _gpx.last_error()
        st = _gpx.lib.gpx_predict_mean_grad(gp._dev().handle, _gpx.ptr(xs), 5, _gpx.ptr(outs[0]), _gpx.ptr(outs[1]))
        assert st == _gpx.GPX_ERR_STATE and word in _gpx.last_error()
        for o in outs:
            assert (o == 7.25).all()
    # bad arguments on a good handle: refused before anything is written; m == 0 is fine
    good = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    h = good._dev().handle
    o = [np.full(15, 7.25) for _ in range(4)]
    assert _gpx.lib.gpx_predict_grad(h, _gpx.ptr(xs), -1, *[_gpx.ptr(a) for a in o]) == _gpx.GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_predict_grad(h, None, 5, *[_gpx.ptr(a) for a in o]) == _gpx.GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_predict_grad(h, _gpx.ptr(xs), 5, _gpx.ptr(o[0]), _gpx.ptr(o[1]), _gpx.ptr(o[2]), None) == _gpx.GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_predict_mean_grad(h, _gpx.ptr(xs), 5, None, None) == _gpx.GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_predict_mean_grad(h, _gpx.ptr(xs), 0, None, None) == 0 and _gpx.lib.gpx_predict_grad(h, None, 0, None, None, None, None) == 0
    for a in o:
        assert (a == 7.25).all()
    # the generic route: central differences through one estimate_many call, against the analytic model on the oracle's K^-1 and beta
    og = orc.OracleGP(x, t, theta)
    em, ev, edm, edv, _g = _expected(x, theta, og.beta(), og.Kinv, xs, 0)
    mean, var, dm, dv = gen.estimate_many_gradient(xs)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3)))  # noqa: E731
    print("generic route: central differences against the model: d mean %.3e d var %.3e" % (rel(dm, edm), rel(dv, edv)))
    assert rel(dm, edm) <= 1e-6 and rel(dv, edv) <= 1e-6
    assert np.abs(mean - gen.meant - em).max() <= 1e-9 and np.abs(var - ev).max() <= 2e-8
    m2, dm2 = gen.estimate_many_gradient(xs, variance=False)
    np.testing.assert_array_equal(dm2, dm)
    # and the fused route says the same to the tolerances of (b)
    _assert_parity("fused against the model", full_grad(h, xs), (em, ev, edm, edv, _g), 2.0)
    # the periodic route: its own estimate_many, differenced
    pm, pv, pdm, pdv = per.estimate_many_gradient(xs, h=1e-5)
    e0 = np.zeros(3)
    e0[0] = 1e-5
    (m1, v1), (m0, v0) = per.estimate_many(xs + e0), per.estimate_many(xs - e0)
    assert pdm.shape == pdv.shape == (5, 3) and np.isfinite(pdm).all() and np.isfinite(pdv).all()
    np.testing.assert_allclose(pdm[:, 0], (m1 - m0) / 2e-5, rtol=0, atol=1e-6 * np.abs(pdm).max())
    np.testing.assert_allclose(pdv[:, 0], (v1 - v0) / 2e-5, rtol=0, atol=1e-6 * max(np.abs(pdv).max(), 1e-3))


# ------------------------------------------------------------------------------------------------
# (f) UncertaintyPropagationLinear
# ------------------------------------------------------------------------------------------------
def _launches(h, cls):
    n, ms, w = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_profile_read(h, cls, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w)), "gpx_profile_read")
    return n.value


@pytest.mark.parametrize("name", ["kat1_grid", "n203_d3", "n256_d8"])
def test_linear_against_the_reference(name):
    g, gold = load_golden(name), load_golden("linear")
    x, t, theta = np.asarray(g["x"], dtype=float), g["t_raw"], g["theta"]
    gp = sk.GaussianProcess(g["x"], t, sk.GaussianCovariance(), theta.copy())
    og = orc.OracleGP(g["x"], t, theta)
    up = sk.UncertaintyPropagationLinear(gp)
    nu, nS = int(g["nu"]), int(g["nS"])
    pairs = [(i, j) for i in range(nu) for j in range(nS)]
    U = np.array([g["u%d" % i] for i, _ in pairs], dtype=float)
    S = np.array([g["Sigma%d" % j] for _, j in pairs], dtype=float)
    h = gp._dev().handle
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 2), "gpx_profile_enable")
    _gpx.check(_gpx.lib.gpx_profile_reset(h), "gpx_profile_reset")
    mean, var = up.propagate_GA_many(U, S)
    for cls in (GPX_K_GEMM, GPX_K_TRSV, GPX_K_GEMM_SMALL, GPX_K_TRSV_RIDE, GPX_K_GEMM_EMU):
        assert _launches(h, cls) == 0, cls                      # no call of the class solves anything
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 0), "gpx_profile_enable")
    # the analytic model on the oracle's beta, and the tolerance of (b) carried through sum_k g_k^2 Sigma_kk: 2 |g_k| Sigma_kk per unit of g_k
    m = pg.mean_grad(x, theta, og.beta(), U, 0, dt=np.float64)
    gk, gs = m["dmean"][0], pg.grad_scale(x, theta, U)
    sd = np.diagonal(S, axis1=1, axis2=2)
    k = 1.0
    carried = (2 * np.abs(gk) * sd * 1e-9 * k * gs).sum(1)
    emean, evar = m["mean"][0] + og.meant, (gk * gk * sd).sum(1) + np.exp(theta[1])
    ga, delta = gold["ga_" + name].reshape(-1, 2), gold["delta_" + name].reshape(-1, 2)
    print("linear %s: against the model dmean %.3e dvar %.3e (carried %.3e); against the reference dmean %.3e dvar %.3e (delta_ref %.3e %.3e)"
          % (name, np.abs(mean - emean).max(), np.abs(var - evar).max(), carried.min(), np.abs(mean - ga[:, 0]).max(), np.abs(var - ga[:, 1]).max(),
             delta[:, 0].max(), delta[:, 1].max()))
    assert (np.abs(mean - emean) <= 1e-9 * k).all() and (np.abs(var - evar) <= carried).all()
    assert (np.abs(mean - ga[:, 0]) <= np.maximum(4 * delta[:, 0], 1e-9 * k)).all()
    assert (np.abs(var - ga[:, 1]) <= np.maximum(4 * delta[:, 1], carried)).all()
    # batched equals single, bit for bit; per-input Sigma and shared Sigma agree; the means-only calls; the analytic _derivative
    for i in range(len(pairs)):
        m1, v1 = up.propagate_GA(U[i], S[i])
        assert m1 == mean[i] and v1 == var[i]
        assert up.propagate_mean(U[i], S[i]) == mean[i]
    ms, vs = up.propagate_GA_many(U, S[0])
    same = [i for i, (_iu, j) in enumerate(pairs) if j == 0]
    np.testing.assert_array_equal(ms, mean)
    np.testing.assert_array_equal(vs[same], var[same])
    np.testing.assert_array_equal(up.propagate_mean_many(U, S) + gp.meant, mean)
    d0 = up._derivative(U[0], 0)
    assert d0 == mean_grad(h, U[:1])[1][0, 0] and abs(d0 - gk[0, 0]) <= 1e-9 * gs[0, 0]
