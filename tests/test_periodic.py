"""PeriodicCovariance on the device (csrc/periodic.hip; gpx_periodic_gram / _fit / _predict / _nll_grad and the Python classes on top)
against the long-double model of tests/_periodic_ld.py, the golden file of the genuine reference (tests/golden/periodic.npz) and the
generic route on the NumPy restatement's K.

Bounds (none fitted to a device result; tests/_periodic_ld.py states the rules):
  Gram and derivative entries: 8 * max(rho_K, 4) units of u K (1 + q), rho_K the float64 restatement's own worst error over all Gram cases;
  gradient: every one of the 3 d + 2 sums on the scale of its absolute terms, 32 * max(rho_ref, 1000 u), from the device's own K^-1 and alpha;
  fit / solve / predict: SURVEY 8a -- rtol 1e-6 / atol 1e-9 v for predictions, 1e-9 relative for nll and log det.
GPX_PERIODIC_RECORD=<file> appends the measured worst ratios (profiles/r16_periodic.txt holds a run's)."""
import ctypes
import functools
import os
import pickle

import numpy as np
import pytest

from conftest import load_golden

import _periodic_ld as pl

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from skgpuppy_amd.Covariance import _MatrixModel, _PeriodicModel

pytestmark = pytest.mark.gpu
V, VT = 2.0, 0.01


def _record(line):
    print(line)
    path = os.environ.get("GPX_PERIODIC_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _gram(xi, n1, xj, n2, d, theta, deriv=-1, out=None):
    """gpx_periodic_gram on raw pointers (ints: device pointers)"""
    K = np.empty((n1, n2)) if out is None else out
    as_ptr = lambda a: ctypes.c_void_p(a) if isinstance(a, int) else _gpx.ptr(a)  # noqa: E731
    st = _gpx.lib.gpx_periodic_gram(as_ptr(xi), n1, as_ptr(xj), n2, d, _gpx.ptr(_gpx.f64(theta)), deriv, as_ptr(K))
    _gpx.check(st, "gpx_periodic_gram")
    return K


@functools.lru_cache(maxsize=None)
def rho_K():
    worst = 0.0
    for n1, n2 in pl.GRAM_SHAPES:
        for d in pl.D_ALL:
            xi, xj, theta = pl.make_gram_case(n1, n2, d)
            worst = max(worst, float(pl.gram_units(pl.kernel_parts(xi, xj, theta, np.float64)["K"], _ld(n1, n2, d)).max()))
    _record("rho_K (float64 restatement, all Gram cases) = %.3e -> bound %.3e units of u K (1 + q)" % (worst, pl.gram_bound(worst)))
    return worst


@functools.lru_cache(maxsize=None)
def _ld(n1, n2, d):
    xi, xj, theta = pl.make_gram_case(n1, n2, d)
    return pl.kernel_parts(xi, xj, theta)


# ------------------------------------------------------------------------------------------------
# Gram
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", pl.D_ALL)
@pytest.mark.parametrize("n1,n2", pl.GRAM_SHAPES)
def test_gram_against_the_model(n1, n2, d):
    xi, xj, theta = pl.make_gram_case(n1, n2, d)
    ld = _ld(n1, n2, d)
    K = _gram(xi, n1, xj, n2, d, theta)
    units = pl.gram_units(K, ld)
    lim = pl.gram_bound(rho_K())
    _record("gram (%d, %d) d=%d: worst %.3f units = %.4f of the bound %.2f" % (n1, n2, d, units.max(), units.max() / lim, lim))
    assert np.all(units <= lim), (units.max(), lim)
    # the quirk: rows of xi that equal a row of xj carry exactly +vt on top of v exp(-0) = v
    eq = ld["eq"]
    assert eq.sum() >= (n1 > 3)
    assert np.all(K[eq] == K[eq][:1]) and np.all(np.abs(K[eq] - (V + VT)) <= 4 * pl.U * (V + VT))
    # the class's accessor is the same call
    np.testing.assert_array_equal(sk.PeriodicCovariance().cov_matrix_ij(xi, xj, theta), K)


@pytest.mark.parametrize("d", pl.D_ALL)
def test_gram_bit_equalities(d):
    import torch
    x, _t, theta = pl.make_case(257, d)
    x[200] = x[17]                                                       # a duplicate training row
    K = _gram(x, 257, x, 257, d, theta)
    np.testing.assert_array_equal(K, K.T)                                # K_ij == K_ji: the fit never computes the upper half
    assert K[200, 17] == K[0, 0] and K[17, 200] == K[0, 0] and np.all(np.diag(K) == K[0, 0]) and abs(K[0, 0] - (V + VT)) <= 4 * pl.U * (V + VT)
    xj = pl.make_case(130, d, seed=5)[0]
    full = _gram(x, 257, xj, 130, d, theta)
    for a, b in ((0, 1), (63, 130), (129, 257)):                         # rows a:b of a call equal a call on rows a:b
        np.testing.assert_array_equal(_gram(np.ascontiguousarray(x[a:b]), b - a, xj, 130, d, theta), full[a:b])
    xd, xjd = torch.from_numpy(x).cuda(), torch.from_numpy(xj).cuda()    # host and device pointers
    outd = torch.empty((257, 130), dtype=torch.float64, device="cuda")
    _gram(xd.data_ptr(), 257, xjd.data_ptr(), 130, d, theta, out=outd.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(outd.cpu().numpy(), full)


@pytest.mark.parametrize("d", pl.D_ALL)
def test_every_derivative_against_the_model(d):
    n1, n2 = (130, 257) if d <= 3 else (64, 129)
    xi, xj, theta = pl.make_gram_case(n1, n2, d)
    ld = pl.kernel_parts(xi, xj, theta, keep=True)
    lim = pl.gram_bound(rho_K())
    cov = sk.PeriodicCovariance()
    worst = 0.0
    for j in range(2 + 3 * d):
        dK = cov._d_cov_matrix_d_theta_ij(xi, xj, theta, j)
        units = pl.deriv_units(dK, ld, theta, j)
        worst = max(worst, float(units.max()))
        assert np.all(units <= lim), (j, units.max(), lim)
    _record("deriv (%d, %d) d=%d: worst %.3f units = %.4f of the bound" % (n1, n2, d, worst, worst / lim))
    dvt = cov._d_cov_matrix_d_theta_ij(xi, xj, theta, 1)
    assert np.all(dvt[~ld["eq"]] == 0) and np.all(dvt[ld["eq"]] == dvt[ld["eq"]][:1]) and np.all(np.abs(dvt[ld["eq"]] - VT) <= 4 * pl.U * VT)


# ------------------------------------------------------------------------------------------------
# fit, solve, predict
# ------------------------------------------------------------------------------------------------
def _golden_case(N, d):
    g = load_golden("periodic")
    key = "c%d_%d_" % (N, d)
    return {k[len(key):]: v for k, v in g.items() if k.startswith(key)}


@pytest.mark.parametrize("N,d", pl.FIT_CASES)
def test_fit_solve_predict(N, d):
    x, t, theta = pl.make_case(N, d)
    xs = pl.make_queries(x, 64, pl.seed_of(N, d) + 1)
    cov = sk.PeriodicCovariance()
    gp = sk.GaussianProcess(x, t, cov, theta.copy())
    assert gp._route() == "periodic"
    mean, var = gp.estimate_many(xs)
    # the generic route on the NumPy restatement's K: gpx_fit_matrix / gpx_predict_kv
    Knp = pl.kernel_parts(x, x, theta, np.float64)["K"]
    kv = pl.kernel_parts(xs, x, theta, np.float64)["K"]
    mm = _MatrixModel(Knp, gp.t)
    gm, gv = mm.predict_kv(kv, np.full(len(xs), V + VT))
    kscale = np.abs(mm.kinv()).max()
    np.testing.assert_allclose(gp.Kinv, mm.kinv(), rtol=1e-6, atol=1e-7 * kscale)
    np.testing.assert_allclose(gp._get_beta(), mm.alpha(), rtol=1e-6, atol=1e-8 * np.abs(mm.alpha()).max())
    np.testing.assert_allclose(mean, gm + gp.meant, rtol=1e-6, atol=1e-9 * V)
    np.testing.assert_allclose(var, gv, rtol=1e-6, atol=1e-9 * V)
    for q in (0, 3):                                                    # (query 3 equals a training row)
        m0, v0 = gp.estimate(xs[q])
        np.testing.assert_allclose([m0, v0], [mean[q], var[q]], rtol=1e-6, atol=1e-9 * V)
    nll = cov._negativeloglikelihood(x, gp.t, theta)
    np.testing.assert_allclose(nll, mm.nll(), rtol=1e-9)
    np.testing.assert_allclose(nll, pl.nll(Knp, gp.t), rtol=1e-9)
    np.testing.assert_allclose(cov._log_det_cov_matrix(x, theta), mm.logdet(), rtol=1e-9)
    np.testing.assert_allclose(cov.inv_cov_matrix(x, theta), mm.kinv(), rtol=1e-6, atol=1e-7 * kscale)
    assert gp._dev().jitter() == 0.0
    if (N, d) in pl.GOLDEN_CASES:
        c = _golden_case(N, d)
        np.testing.assert_allclose(cov.cov_matrix(x, theta), c["K"], rtol=1e-12)
        np.testing.assert_allclose(gp._get_beta(), c["beta"], rtol=1e-6, atol=1e-8 * np.abs(c["beta"]).max())
        np.testing.assert_allclose(mean, c["mean"], rtol=1e-6, atol=1e-9 * V)
        np.testing.assert_allclose(var, c["var"], rtol=1e-6, atol=1e-9 * V)
        np.testing.assert_allclose(nll, float(c["nll"]), rtol=1e-9)
        np.testing.assert_allclose(cov._d_nll_d_theta(x, gp.t, theta), c["grad"], rtol=1e-6, atol=1e-7)
        sub = x[:40]
        for j in range(len(theta)):
            np.testing.assert_allclose(cov._d_cov_matrix_d_theta_ij(sub, sub, theta, j), c["dK"][j], rtol=1e-11, atol=1e-15)
    mm.close()


def _chol_of(handle, n):
    out = np.empty((n, n))
    _gpx.check(_gpx.lib.gpx_chol(handle, _gpx.ptr(out)), "gpx_chol")
    return out


def test_fit_matrix_of_the_device_gram_is_the_fit():
    """gpx_fit_matrix on gpx_periodic_gram's matrix gives gpx_periodic_fit's factor bit for bit (the periodic twin of
    test_backward_error.py's test of that name).  N = 1153 pads to 1280, the smallest shape whose assembly is split: the first outer
    panel's 1024 columns, then the rest with 129 real rows in a 256-row padded grid that starts off the origin of the buffer."""
    N, d = 1153, 3
    x, t, theta = pl.make_case(N, d)
    K = _gram(x, N, x, N, d, theta)
    gp = sk.GaussianProcess(x, t, sk.PeriodicCovariance(), theta.copy())
    assert gp._route() == "periodic"
    L1 = _chol_of(gp._dev().handle, N)
    assert gp._dev().jitter() == 0.0
    gp._dev().close()
    m = _MatrixModel(K, None)
    L2 = _chol_of(m.handle, N)
    assert m.jitter() == 0.0
    m.close()
    assert np.array_equal(L1, L2), np.abs(L1 - L2).max()


def test_batch_place_and_chunking_do_not_change_a_query(monkeypatch):
    """2049 + 3 queries at N = 130 in chunks of 1024 (GPX_PERIODIC_CHUNK, read at call time) against the same queries one at a time and
    reversed, bit for bit"""
    x, t, theta = pl.make_case(130, 1)
    xs = pl.make_queries(x, 2049 + 3, 77)
    model = _PeriodicModel(x, t, theta)
    monkeypatch.setenv("GPX_PERIODIC_CHUNK", "1024")
    mean, var = model.predict(xs)
    rm, rv = model.predict(np.ascontiguousarray(xs[::-1]))
    np.testing.assert_array_equal(rm[::-1], mean)
    np.testing.assert_array_equal(rv[::-1], var)
    monkeypatch.delenv("GPX_PERIODIC_CHUNK")
    wm, wv = model.predict(xs)                                           # one chunk
    np.testing.assert_array_equal(wm, mean)
    np.testing.assert_array_equal(wv, var)
    one_m, one_v = np.empty_like(mean), np.empty_like(var)
    for i in range(len(xs)):
        a, b = model.predict(xs[i:i + 1])
        one_m[i], one_v[i] = a[0], b[0]
    np.testing.assert_array_equal(one_m, mean)
    np.testing.assert_array_equal(one_v, var)
    model.close()


# ------------------------------------------------------------------------------------------------
# gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", pl.D_ALL)
@pytest.mark.parametrize("N", pl.GRAD_N)
def test_gradient_against_the_model(N, d):
    x, t, theta = pl.make_case(N, d)
    model = _PeriodicModel(x, t, theta)
    g1, g2 = model.nll_grad(), model.nll_grad()
    np.testing.assert_array_equal(g1, g2)                                # fixed-order reduction
    Kinv, alpha = model.kinv(), model.alpha()
    model.close()
    want, scale = pl.grad(x, theta, Kinv, alpha)
    ref, _ = pl.grad(x, theta, Kinv, alpha, np.float64)
    rho = float(pl.distances(ref, want, scale).max())
    dist = pl.distances(g1, want, scale)
    _record("grad N=%d d=%d: rho_ref %.3e bound %.3e device worst %.3e = %.5f of the bound" % (N, d, rho, pl.bound(rho), dist.max(), dist.max() / pl.bound(rho)))
    pl.assert_within({"grad": dist}, rho, "gpx_periodic_nll_grad N=%d d=%d" % (N, d))
    if (N, d) in pl.GOLDEN_CASES:
        np.testing.assert_allclose(g1, _golden_case(N, d)["grad"], rtol=1e-6, atol=1e-7)


def test_gradient_against_golden():
    for N, d in pl.GOLDEN_CASES:
        c = _golden_case(N, d)
        model = _PeriodicModel(c["x"], c["t"], c["theta"])
        np.testing.assert_allclose(model.nll_grad(), c["grad"], rtol=1e-6, atol=1e-7)
        model.close()


# ------------------------------------------------------------------------------------------------
# jitter retry, ML fit
# ------------------------------------------------------------------------------------------------
def test_jitter_retry():
    x = (0.01 * np.arange(256.0))[:, None]
    theta = np.array([np.log(2.0), -np.inf, np.log(0.05), np.log(3.0), np.log(1.0)])
    t = np.sin(x[:, 0])
    t = t - t.mean()
    Knp = pl.kernel_parts(x, x, theta, np.float64)["K"]
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(Knp)
    np.linalg.cholesky(Knp + 1e-5 * np.eye(256))
    pm, mm = _PeriodicModel(x, t, theta), _MatrixModel(Knp, t)
    assert pm.jitter() == 1e-5 and mm.jitter() == 1e-5
    xs = np.linspace(0.0, 2.56, 50)[:, None]
    kv = pl.kernel_parts(xs, x, theta, np.float64)["K"]
    m1, v1 = pm.predict(xs)
    m2, v2 = mm.predict_kv(kv, np.full(50, V))
    np.testing.assert_allclose(m1, m2, rtol=1e-6, atol=1e-6)             # (cond (K + 1e-5 I) ~ 1e8: the two factor different roundings of K)
    np.testing.assert_allclose(v1, v2, rtol=1e-6, atol=1e-7 * V)
    pm.close()
    mm.close()


def test_ml_fit():
    """GaussianProcess(x, t, PeriodicCovariance()) without theta: L-BFGS-B on the fused NLL / gradient, judged by the NumPy restatement
    (the criteria of the generic route's ML test)"""
    rng = np.random.RandomState(11)
    x = np.sort(rng.uniform(0, 10, 60))[:, None]
    t = np.sin(2 * np.pi * x[:, 0] / 2.5) + 0.1 * rng.randn(60)
    cov = sk.PeriodicCovariance()
    gp = sk.GaussianProcess(x, t, cov)

    def judge(theta):
        K = pl.kernel_parts(x, x, theta, np.float64)["K"]
        Kinv = np.linalg.inv(K)
        g, _ = pl.grad(x, theta, Kinv, Kinv.dot(gp.t), np.float64)
        return pl.nll(K, gp.t), g

    nll0, _g0 = judge(cov.get_theta(x, gp.t))
    nll1, g1 = judge(gp.theta_min)
    assert nll1 < nll0 - 1.0, (nll0, nll1)
    assert np.abs(g1).max() < 5e-2 * max(1.0, abs(nll1)), (g1, nll1)


# ------------------------------------------------------------------------------------------------
# edges
# ------------------------------------------------------------------------------------------------
def test_state_errors_and_bad_arguments():
    x, t, theta = pl.make_case(130, 2)
    lib = _gpx.lib
    pm = _PeriodicModel(x, t, theta)
    out, g = np.empty(4), np.empty(8)
    u = _gpx.f64(x[0])
    for st in (lib.gpx_predict(pm.handle, _gpx.ptr(x), 2, _gpx.ptr(out), _gpx.ptr(out[2:])),
               lib.gpx_cjh(pm.handle, _gpx.ptr(u), _gpx.ptr(np.empty(130)), None, None),
               lib.gpx_nll_grad(pm.handle, _gpx.ptr(g))):
        assert st == _gpx.GPX_ERR_STATE and "gpx_periodic" in _gpx.last_error()
    n, d = ctypes.c_int64(), ctypes.c_int()
    assert lib.gpx_n(pm.handle, ctypes.byref(n), ctypes.byref(d)) == 0 and (n.value, d.value) == (130, 2)
    # everything a matrix handle answers
    assert pm.solve(np.eye(130)[:2]).shape == (2, 130) and np.isfinite(pm.nll()) and pm.jitter() == 0.0
    np.testing.assert_allclose(pm.nll_grad_entry(sk.PeriodicCovariance()._d_cov_matrix_d_theta(x, theta, 0)), pm.nll_grad()[0], rtol=1e-9)
    from skgpuppy_amd.GaussianProcess import _DeviceModel
    gm = _DeviceModel(x, t, theta[:4].copy())
    mm = _MatrixModel(pl.kernel_parts(x, x, theta, np.float64)["K"], t)
    for h in (gm.handle, mm.handle):
        assert lib.gpx_periodic_predict(h, _gpx.ptr(x), 2, _gpx.ptr(out), _gpx.ptr(out[2:])) == _gpx.GPX_ERR_STATE
        assert "gpx_periodic_fit" in _gpx.last_error()
        assert lib.gpx_periodic_nll_grad(h, _gpx.ptr(g)) == _gpx.GPX_ERR_STATE
    gm.close()
    mm.close()
    # bad arguments: refused with text
    h = ctypes.c_void_p()
    K = np.empty((130, 130))
    th = _gpx.ptr(theta)
    bad = [lib.gpx_periodic_gram(_gpx.ptr(x), 130, _gpx.ptr(x), 130, 0, th, -1, _gpx.ptr(K)),
           lib.gpx_periodic_gram(_gpx.ptr(x), 130, _gpx.ptr(x), 130, 65, th, -1, _gpx.ptr(K)),
           lib.gpx_periodic_gram(None, 130, _gpx.ptr(x), 130, 2, th, -1, _gpx.ptr(K)),
           lib.gpx_periodic_gram(_gpx.ptr(x), 130, _gpx.ptr(x), 130, 2, None, -1, _gpx.ptr(K)),
           lib.gpx_periodic_gram(_gpx.ptr(x), 0, _gpx.ptr(x), 130, 2, th, -1, _gpx.ptr(K)),
           lib.gpx_periodic_gram(_gpx.ptr(x), 130, _gpx.ptr(x), 130, 2, th, 8, _gpx.ptr(K)),
           lib.gpx_periodic_gram(_gpx.ptr(x), 130, _gpx.ptr(x), 130, 2, th, -2, _gpx.ptr(K)),
           lib.gpx_periodic_fit(_gpx.ptr(x), _gpx.ptr(t), 0, 2, th, None, ctypes.byref(h)),
           lib.gpx_periodic_fit(None, _gpx.ptr(t), 130, 2, th, None, ctypes.byref(h)),
           lib.gpx_periodic_fit(_gpx.ptr(x), _gpx.ptr(t), 130, 65, th, None, ctypes.byref(h)),
           lib.gpx_periodic_fit(_gpx.ptr(x), _gpx.ptr(t), 130, 2, th, None, None),
           lib.gpx_periodic_predict(pm.handle, None, 2, _gpx.ptr(out), _gpx.ptr(out[2:])),
           lib.gpx_periodic_predict(pm.handle, _gpx.ptr(x), -1, _gpx.ptr(out), _gpx.ptr(out[2:])),
           lib.gpx_periodic_nll_grad(pm.handle, None),
           lib.gpx_periodic_nll_grad(None, _gpx.ptr(g))]
    for i, st in enumerate(bad):
        assert st == _gpx.GPX_ERR_BAD_ARG, (i, st)
    assert _gpx.last_error() and not h
    # m = 0 is a no-op: nothing is written, nothing is launched
    lib.gpx_profile_enable(pm.handle, 2)
    lib.gpx_profile_reset(pm.handle)
    assert lib.gpx_periodic_predict(pm.handle, None, 0, None, None) == 0
    launches, ms, work = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    for cls in range(10):
        assert lib.gpx_profile_read(pm.handle, cls, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work)) == 0 and launches.value == 0
    # the Gram and the gradient pass show up in their classes
    pm.predict(x[:5])
    pm.nll_grad()
    assert lib.gpx_profile_read(pm.handle, _gpx.K_GRAM, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work)) == 0
    assert launches.value == 1 and work.value == 8.0 * 128 * 256
    assert lib.gpx_profile_read(pm.handle, _gpx.K_QUAD, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work)) == 0
    assert launches.value >= 1 and ms.value > 0
    pm.close()


class PyPeriodic(sk.Covariance):
    """the same kernel restated on the generic base class: every matrix comes from N^2 Python calls"""
    __call__ = sk.PeriodicCovariance.__call__
    _split = staticmethod(sk.PeriodicCovariance._split)
    get_theta = sk.PeriodicCovariance.get_theta


class OwnCross(sk.PeriodicCovariance):
    def cov_matrix_ij(self, xi, xj, theta):
        return sk.Covariance.cov_matrix_ij(self, xi, xj, theta)


def _outcome(f):
    try:
        return ("value", np.asarray(f(), dtype=float))
    except Exception as e:  # noqa: BLE001  (the test compares exception TYPES)
        return ("raises", type(e))


def test_python_behaviour():
    x, t, theta = pl.make_case(60, 2, seed=123)
    xs = pl.make_queries(x, 20, 5)
    gp = sk.GaussianProcess(x, t, sk.PeriodicCovariance(), theta.copy())
    mean, var = gp.estimate_many(xs)
    gp.cov._negativeloglikelihood(x, gp.t, theta)                        # (a live handle in the operator's cache as well)
    gp2 = pickle.loads(pickle.dumps(gp))
    assert gp2._model is None and not hasattr(gp2.cov, "_ml_cache")
    m2, v2 = gp2.estimate_many(xs)
    np.testing.assert_array_equal(m2, mean)
    np.testing.assert_array_equal(v2, var)
    # a subclass that overrides a matrix builder takes the generic route, with the same numbers to rounding
    own = sk.GaussianProcess(x, t, OwnCross(), theta.copy())
    assert own._route() == "generic" and gp._route() == "periodic"
    mo, vo = own.estimate_many(xs)
    np.testing.assert_allclose(mo, mean, rtol=1e-6, atol=1e-9 * V)
    np.testing.assert_allclose(vo, var, rtol=1e-6, atol=1e-9 * V)
    np.testing.assert_allclose(own.cov._d_nll_d_theta(x, own.t, theta), gp.cov._d_nll_d_theta(x, gp.t, theta), rtol=1e-5, atol=1e-6)
    # the propagation classes treat a periodic GP as they treat a generic-route GP
    py = sk.GaussianProcess(x, t, PyPeriodic(), theta.copy())
    assert py._route() == "generic"
    u, S = np.array([4.5, 5.25]), np.diag([0.02, 0.03])
    for cls in (sk.UncertaintyPropagationExact, sk.UncertaintyPropagationApprox):
        a = _outcome(lambda: cls(gp).propagate_GA(u, S))
        b = _outcome(lambda: cls(py).propagate_GA(u, S))
        assert a[0] == b[0], (cls.__name__, a, b)
        if a[0] == "value":
            np.testing.assert_allclose(a[1], b[1], rtol=1e-6, atol=1e-8 * V)
        else:
            assert a[1] is b[1], (cls.__name__, a, b)


def test_predict_from_five_slabs_on():
    """N = 5200 (six slabs of 1024 columns): gpx_periodic_predict shares estimate_many's solver, which from five slabs on is left-looking
    with emulated updates from K = 4096 and needs a bound on every solved row -- sqrt(v + vt) here, the equality quirk included.  Against
    NumPy's Cholesky of the restatement's K on SURVEY 8a's bounds; 300 queries, one of them a training row."""
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    N, d, m = 5200, 2, 300
    x, t, theta = pl.make_case(N, d)
    xs = pl.make_queries(x, m, 31)
    model = _PeriodicModel(x, t, theta)
    mean, var = model.predict(xs)
    assert model.jitter() == 0.0
    model.close()
    K = pl.kernel_parts(x, x, theta, np.float64)["K"]
    kv = pl.kernel_parts(xs, x, theta, np.float64)["K"]
    c = cho_factor(K, lower=True)
    z = solve_triangular(c[0], kv.T, lower=True)
    np.testing.assert_allclose(mean, kv.dot(cho_solve(c, t)), rtol=1e-6, atol=1e-9 * V)
    np.testing.assert_allclose(var, (V + VT) - (z * z).sum(0), rtol=1e-6, atol=1e-9 * V)
