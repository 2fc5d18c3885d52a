"""Covariance operator interface -- host-side mirror of skgpuppy/Covariance.py for the hot path.

`Covariance` is the reference's operator interface (skgpuppy/Covariance.py:111-359); only
`GaussianCovariance` (:435-689) is on the accelerated path.  Matrix-sized work (cov_matrix_ij,
cov_matrix, inv_cov_matrix) is done by libgpx on the GPU; the scalar accessors (__call__, get_theta,
get_Jacobian, get_Hessian: O(d^2) per call) are plain host arithmetic exactly as the reference defines
them -- their batched forms are gpx_cjh / the fused device kernels.
"""
import ctypes

import numpy as np

from . import _gpx


def tracedot(A, B):
    """trace(dot(A, B))  (skgpuppy/Covariance.py:101-109)."""
    return np.dot(np.ravel(np.asarray(A).T), np.ravel(B))


class _MatrixModel(object):
    """Owner of one gpx_handle built from a SUPPLIED covariance matrix (gpx_fit_matrix): the device route of the generic operator
    interface -- Cholesky factor of the operator's own cov_matrix(x, theta) (+1e-5 I retry), alpha, lazily K^-1."""

    def __init__(self, K, t_centered):
        K = _gpx.f64(K)
        if K.ndim != 2 or K.shape[0] != K.shape[1]:
            raise ValueError("cov_matrix must return a square matrix, got shape %r" % (K.shape,))
        self.n, self.d = K.shape[0], 0
        t = np.zeros(self.n) if t_centered is None else _gpx.f64(t_centered)
        if t.shape != (self.n,):
            raise ValueError("t must have %d entries" % self.n)
        self._h = ctypes.c_void_p()
        _gpx.check(_gpx.lib.gpx_fit_matrix(_gpx.ptr(K), _gpx.ptr(t), self.n, None, ctypes.byref(self._h)), "gpx_fit_matrix")

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("device model already released")
        return self._h

    def close(self, _free=_gpx.lib.gpx_free, _null=ctypes.c_void_p):
        if getattr(self, "_h", None):
            _free(self._h)
            self._h = _null()

    __del__ = close

    def predict_kv(self, kv, kdiag):
        kv = _gpx.f64(np.atleast_2d(kv))
        kdiag = _gpx.f64(np.atleast_1d(kdiag))
        m = kv.shape[0]
        if kv.shape[1] != self.n or kdiag.shape != (m,):
            raise ValueError("kv must be (m, %d) and kdiag (m,)" % self.n)
        mean = np.empty(m)
        var = np.empty(m)
        _gpx.check(_gpx.lib.gpx_predict_kv(self.handle, _gpx.ptr(kv), m, _gpx.ptr(kdiag), _gpx.ptr(mean), _gpx.ptr(var)), "gpx_predict_kv")
        return mean, var

    def alpha(self):
        out = np.empty(self.n)
        _gpx.check(_gpx.lib.gpx_alpha(self.handle, _gpx.ptr(out)), "gpx_alpha")
        return out

    def solve(self, B):
        B = _gpx.f64(np.atleast_2d(B))
        kb = np.empty_like(B)
        _gpx.check(_gpx.lib.gpx_solve(self.handle, _gpx.ptr(B), B.shape[0], None, _gpx.ptr(kb)), "gpx_solve")
        return kb

    def kinv(self):
        out = np.empty((self.n, self.n))
        _gpx.check(_gpx.lib.gpx_kinv(self.handle, _gpx.ptr(out)), "gpx_kinv")
        return out

    def logdet(self):
        v = ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_logdet(self.handle, ctypes.byref(v)), "gpx_logdet")
        return v.value

    def nll(self):
        v = ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_nll(self.handle, ctypes.byref(v)), "gpx_nll")
        return v.value

    def nll_grad_entry(self, dK):
        dK = _gpx.f64(dK)
        if dK.shape != (self.n, self.n):
            raise ValueError("_d_cov_matrix_d_theta must return an (%d, %d) matrix" % (self.n, self.n))
        v = ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_nll_grad_matrix(self.handle, _gpx.ptr(dK), ctypes.byref(v)), "gpx_nll_grad_matrix")
        return v.value

    def jitter(self):
        v = ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_jitter_used(self.handle, ctypes.byref(v)), "gpx_jitter_used")
        return v.value


class Covariance(object):
    """Superclass for all covariance functions (skgpuppy/Covariance.py:111-359): the interface GaussianProcess talks to.

    As in the reference the base class is GENERIC: a subclass that implements `__call__` (and `get_theta` for the ML fit)
    gets cov_matrix_ij / cov_matrix from it, and inv_cov_matrix, the likelihood and its gradient from those -- the matrix-sized
    algebra (factorisation with the +1e-5 I retry, inverse, log det, quadratic forms, trace terms) runs on the GPU on the
    operator's own matrices (gpx_fit_matrix and friends); only the entry-wise evaluation of a user's Python kernel is host work,
    as it is in the reference."""

    def __init__(self):
        pass

    def __call__(self, xi, xj, theta):
        raise NotImplementedError

    def get_theta(self, x, t):
        raise NotImplementedError

    def cov_matrix_ij(self, xi, xj, theta):
        """N1 x N2 matrix of the operator's own scalar kernel (Covariance.py:137-152)"""
        ni, nj = len(xi), len(xj)
        K = np.zeros((ni, nj))
        for i in range(ni):
            for j in range(nj):
                K[i, j] = self(xi[i], xj[j], theta)
        return K

    def cov_matrix(self, x, theta):
        # (Covariance.py:155-164)
        return self.cov_matrix_ij(x, x, theta)

    def inv_cov_matrix(self, x, theta, cov_matrix=None):
        """inverse of the operator's own cov_matrix(x, theta), or of `cov_matrix` when given (Covariance.py:167-187).  The reference
        LU-inverts and falls back to chol(K + 1e-5 I) when that raises; here K is Cholesky-factored on the GPU with the same
        single +1e-5 I retry and K^-1 = L^-T L^-1."""
        if cov_matrix is not None:
            K = _gpx.f64(cov_matrix)
            if K.ndim != 2 or K.shape[0] != K.shape[1]:
                raise ValueError("cov_matrix must be square")
            out = np.empty_like(K)
            _gpx.check(_gpx.lib.gpx_spd_inverse(_gpx.ptr(K), K.shape[0], _gpx.ptr(out), None), "gpx_spd_inverse")
            return out
        model = _MatrixModel(np.array(self.cov_matrix(x, theta)), None)
        try:
            return model.kinv()
        finally:
            model.close()

    def get_Hessian(self, u, xi, theta):
        raise NotImplementedError

    def get_Jacobian(self, u, xi, theta):
        raise NotImplementedError

    # ---- hyper-parameter maximum likelihood ("next" row f1; skgpuppy/Covariance.py:189-337) ----------------
    def _matrix_model_at(self, x, t, theta):
        """device model of the operator's own cov_matrix(x, theta) with targets t, kept for the next call at the same theta
        (L-BFGS-B asks for the value and the gradient one after the other)"""
        th = np.array(theta, dtype=float)
        ta = None if t is None else _gpx.f64(t)
        key = (id(x), np.shape(x), None if ta is None else ta.tobytes(), th.tobytes())
        cached = getattr(self, "_mm_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        if cached is not None:
            cached[1].close()
        self._mm_cache = None
        model = _MatrixModel(np.array(self.cov_matrix(x, theta)), ta)
        self._mm_cache = (key, model)
        return model

    def _fitted_model_at(self, x, t, theta, check_theta, build):
        """the fused classes' device model build(x, t, theta) fitted at theta, cached on (x, t, theta) identity/bytes: L-BFGS-B asks
        for the value and the gradient at the same theta in two separate calls.  The cache is cleared before the new fit: a
        constructor that raises leaves no closed model behind."""
        xa = _gpx.f64(x)
        ta = _gpx.f64(t)
        th = check_theta(theta, xa.shape[1]).copy()
        key = (xa.ctypes.data if xa is x else id(x), xa.shape, ta.tobytes(), th.tobytes())
        cached = getattr(self, "_ml_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        if cached is not None:
            cached[1].close()
        self._ml_cache = None
        model = build(xa, ta, th)
        self._ml_cache = (key, model)
        return model

    def _log_det_cov_matrix(self, x, theta):
        """log det of cov_matrix(x, theta) (Covariance.py:189-195: numpy slogdet); here 2 sum log diag of its Cholesky factor,
        computed on the GPU from the operator's own matrix"""
        return self._matrix_model_at(x, None, theta).logdet()

    def _d_cov_d_theta(self, xi, xj, theta, j):
        """central difference of the scalar kernel in theta_j, eps = 1e-5 (Covariance.py:219-233)"""
        eps = 1e-5
        d = np.zeros(len(theta))
        d[j] = eps
        return (self(xi, xj, theta + d) - self(xi, xj, theta - d)) / (2 * eps)

    def _d_cov_matrix_d_theta_ij(self, xi, xj, theta, j):
        """entry-wise _d_cov_d_theta (Covariance.py:236-253); GaussianCovariance overrides it with the closed form"""
        ni, nj = len(xi), len(xj)
        K = np.zeros((ni, nj))
        for i1 in range(ni):
            for i2 in range(nj):
                K[i1, i2] = self._d_cov_d_theta(xi[i1], xj[i2], theta, j)
        return K

    def _d_cov_matrix_d_theta(self, x, theta, j):
        # (Covariance.py:256-265)
        return self._d_cov_matrix_d_theta_ij(x, x, theta, j)

    def _negativeloglikelihood(self, x, t, theta):
        """N/2 log 2pi + 1/2 log det K + 1/2 t^T K^-1 t for the operator's own K (Covariance.py:197-216): factorisation, log det and
        the quadratic form on the GPU; 1e20 when K cannot be factored, like the reference's except branch."""
        try:
            return self._matrix_model_at(x, t, theta).nll()
        except (np.linalg.LinAlgError, RuntimeWarning, ZeroDivisionError, ValueError):
            return 1.0e+20

    def _d_nll_d_theta(self, x, t, theta):
        """gradient of the NLL from the operator's own derivative matrices (Covariance.py:266-282): entry j is
        1/2 tr(K^-1 dK_j) - 1/2 alpha^T dK_j alpha, one fused device pass over K^-1 and dK_j each"""
        model = self._matrix_model_at(x, t, theta)
        return np.array([model.nll_grad_entry(self._d_cov_matrix_d_theta(x, theta, j)) for j in range(len(theta))])

    def _nll_function(self, x, t):
        # (Covariance.py:284-297)
        def nll(theta):
            return self._negativeloglikelihood(x, t, theta)
        return nll

    def _gradient_function(self, x, t):
        # (Covariance.py:299-312): retried at 0.999 theta when the factorisation fails
        def gradient(theta):
            try:
                gr = self._d_nll_d_theta(x, t, theta)
            except np.linalg.LinAlgError:
                gr = self._d_nll_d_theta(x, t, theta * 0.999)
            return gr
        return gradient

    def ml_estimate(self, x, t):
        """maximum-likelihood theta by L-BFGS-B with the analytic gradient (Covariance.py:314-337, which goes
        through Utilities.minimize(method=["l_bfgs_b"]) = scipy's fmin_l_bfgs_b with default settings)."""
        from scipy.optimize import fmin_l_bfgs_b
        theta_start = self.get_theta(x, t)
        func = self._nll_function(x, t)
        fprime = self._gradient_function(x, t)
        theta_min = fmin_l_bfgs_b(func, theta_start, bounds=None, approx_grad=False, fprime=fprime)
        return np.array(theta_min[0])

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_mm_cache", None)     # device handles never enter a pickle
        state.pop("_ml_cache", None)
        return state


def _theta(theta, d):
    th = _gpx.f64(theta)
    if th.ndim != 1 or th.shape[0] != d + 2:
        raise ValueError("theta must have 2 + d = %d entries, got shape %r" % (d + 2, th.shape))
    return th


class GaussianCovariance(Covariance):
    """ARD squared-exponential kernel, theta = (log v, log vt, log w_1..w_d)
    (skgpuppy/Covariance.py:435-689).

    The matrix methods are the fused HIP path (Gram kernel, Cholesky on the Gram tiles, one-pass likelihood gradient).  A user
    subclass that overrides one of the matrix builders keeps the reference's semantics -- cov_matrix is cov_matrix_ij + vt I,
    inv_cov_matrix / the likelihood / its gradient are built on whatever those return -- by falling back to the generic
    device route of `Covariance` (`_fused()` decides per instance)."""

    _MATRIX_METHODS = ("cov_matrix_ij", "cov_matrix", "inv_cov_matrix", "_d_cov_matrix_d_theta", "_d_cov_matrix_d_theta_ij",
                       "_log_det_cov_matrix")

    def _fused(self):
        """True when every matrix-defining method of this instance is GaussianCovariance's own"""
        cls = type(self)
        return cls is GaussianCovariance or all(getattr(cls, m) is getattr(GaussianCovariance, m) for m in self._MATRIX_METHODS)

    def __call__(self, xi, xj, theta):
        # scalar kernel incl. the "+vt iff xi == xj elementwise" hack (Covariance.py:440-451)
        xi = np.asarray(xi)
        xj = np.asarray(xj)
        with np.errstate(divide="ignore"):
            v = np.exp(theta[0])
            vt = np.exp(theta[1])
            w = np.exp(np.asarray(theta[2:], dtype=float))
        diff = xi - xj
        return v * np.exp(-0.5 * np.dot(diff, w * diff)) + (vt if (xi == xj).all() else 0)

    def get_theta(self, x, t):
        # initial guess for the hyper-parameter search (Covariance.py:453-459)
        n, d = np.shape(x)
        theta = np.ones(2 + d)
        theta[0] = np.log(np.var(t)) if t is not None else 1
        theta[1] = np.log(np.var(t) / 4) if t is not None else 1
        theta[2:] = -2 * np.log((np.max(x, 0) - np.min(x, 0)) / 2.0)
        return theta

    def _gram(self, xi, xj, theta, add_diag):
        a = _gpx.f64(xi)
        b = a if xj is xi else _gpx.f64(xj)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
            raise ValueError("inputs must be (n, d) arrays with equal d")
        th = _theta(theta, a.shape[1])
        K = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
        if K.size:
            st = _gpx.lib.gpx_gram(_gpx.ptr(a), a.shape[0], _gpx.ptr(b), b.shape[0], a.shape[1], _gpx.ptr(th),
                                   float(add_diag), _gpx.ptr(K))
            _gpx.check(st, "gpx_gram")
        return K

    def cov_matrix_ij(self, xi, xj, theta):
        """N1 x N2 cross-covariance without the noise term (Covariance.py:466-483) -- HIP Gram kernel."""
        return self._gram(xi, xj, theta, 0.0)

    def cov_matrix(self, x, theta):
        """cov_matrix_ij(x, x) + vt I (Covariance.py:461-464); the diagonal add is fused in the kernel."""
        with np.errstate(divide="ignore"):
            vt = float(np.exp(theta[1]))
        if type(self).cov_matrix_ij is not GaussianCovariance.cov_matrix_ij:     # a subclass's own cross-covariance
            return np.asarray(self.cov_matrix_ij(x, x, theta), dtype=float) + vt * np.eye(np.shape(x)[0])
        return self._gram(x, x, theta, vt)

    def inv_cov_matrix(self, x, theta, cov_matrix=None):
        """K^-1 (Covariance.py:167-187).  The reference LU-inverts; here K is Cholesky-factored on the GPU
        (with the reference's +1e-5 I retry on a non-PD pivot) and K^-1 = L^-T L^-1."""
        if cov_matrix is not None or not self._fused():
            return Covariance.inv_cov_matrix(self, x, theta, cov_matrix)
        from .GaussianProcess import _DeviceModel
        xa = _gpx.f64(x)
        model = _DeviceModel(xa, np.zeros(xa.shape[0]), _theta(theta, xa.shape[1]))
        try:
            return model.kinv()
        finally:
            model.close()

    def _log_det_cov_matrix(self, x, theta):
        """log det (K + vt I) (Covariance.py:189-195) from the Cholesky factor of a device fit"""
        if not self._fused():
            return Covariance._log_det_cov_matrix(self, x, theta)
        from .GaussianProcess import _DeviceModel
        xa = _gpx.f64(x)
        model = _DeviceModel(xa, np.zeros(xa.shape[0]), _theta(theta, xa.shape[1]))
        try:
            return model.logdet()
        finally:
            model.close()

    def _d_cov_d_theta(self, xi, xj, theta, j):
        """d k(xi, xj) / d theta_j in closed form (Covariance.py:485-503); theta is the LOG of (v, vt, w): j = 0 -> the
        noise-free kernel, j = 1 -> vt iff xi == xj elementwise, j >= 2 -> -1/2 (dx_k)^2 w_k k"""
        xi = np.asarray(xi, dtype=float)
        xj = np.asarray(xj, dtype=float)
        diff = xi - xj
        with np.errstate(divide="ignore"):
            v = np.exp(theta[0])
            vt = np.exp(theta[1])
            w = np.exp(np.asarray(theta[2:], dtype=float))
        kf = v * np.exp(-0.5 * np.dot(diff, w * diff))
        if j == 0:
            return kf
        if j == 1:
            return vt if (xi == xj).all() else 0
        return -0.5 * diff[j - 2] ** 2 * kf * w[j - 2]

    def _d_cov_matrix_d_theta(self, x, theta, j):
        # (Covariance.py:505-512)
        if j == 1:
            with np.errstate(divide="ignore"):
                return np.eye(np.shape(x)[0]) * np.exp(theta[1])
        return self._d_cov_matrix_d_theta_ij(x, x, theta, j)

    def _d_cov_matrix_d_theta_ij(self, xi, xj, theta, j, Cov=None):
        """derivative Gram d K_ij / d theta_j (Covariance.py:605-657): the noise-free Gram from the HIP kernel (or `Cov` when
        the caller has it), scaled entry-wise by -1/2 w_k (xi_k - xj_k)^2 for j = k + 2.  An accessor: the likelihood gradient
        itself never forms these matrices (nll_grad_kernel)."""
        a = _gpx.f64(xi)
        b = _gpx.f64(xj)
        if j == 1:
            return np.zeros((a.shape[0], b.shape[0]))
        # (the reference recomputes the built-in Gram inline here, :622-633 -- also for a subclass with its own cov_matrix_ij)
        K = np.asarray(Cov, dtype=float) if Cov is not None else GaussianCovariance.cov_matrix_ij(self, a, b, theta)
        if j == 0:
            return K
        w = np.exp(np.asarray(theta[2:], dtype=float))
        dk = a[:, j - 2][:, None] - b[:, j - 2][None, :]
        return -0.5 * K * (dk * dk) * w[j - 2]

    def _model_at(self, x, t, theta):
        from .GaussianProcess import _DeviceModel
        return self._fitted_model_at(x, t, theta, _theta, _DeviceModel)

    def _negativeloglikelihood(self, x, t, theta):
        """N/2 log 2pi + 1/2 log det K + 1/2 t^T K^-1 t on the GPU (Covariance.py:197-216); 1e20 when K cannot be
        factored, like the reference's except branch."""
        if not self._fused():
            return Covariance._negativeloglikelihood(self, x, t, theta)
        try:
            model = self._model_at(x, t, theta)
            out = ctypes.c_double()
            _gpx.check(_gpx.lib.gpx_nll(model.handle, ctypes.byref(out)), "gpx_nll")
            return out.value
        except (np.linalg.LinAlgError, ValueError, ZeroDivisionError):
            return 1.0e+20

    def _d_nll_d_theta(self, x, t, theta):
        """gradient of the NLL (Covariance.py:266-282 with the derivative Grams of :505-512, :605-657): one fused
        pass over K^-1 on the GPU instead of 2+d derivative matrices."""
        if not self._fused():
            return Covariance._d_nll_d_theta(self, x, t, theta)
        model = self._model_at(x, t, theta)
        g = np.empty(len(theta))
        _gpx.check(_gpx.lib.gpx_nll_grad(model.handle, _gpx.ptr(g)), "gpx_nll_grad")
        return g

    def get_Hessian(self, u, xi, theta):
        # (Covariance.py:660-674)
        with np.errstate(divide="ignore"):
            v = np.exp(theta[0])
            w = np.exp(np.asarray(theta[2:], dtype=float))
        diff = np.asarray(xi, dtype=float) - np.asarray(u, dtype=float)
        e = v * np.exp(-0.5 * np.dot(diff, w * diff))
        wd = diff * w
        return (np.outer(wd, wd) - np.diag(w)) * e

    def get_Jacobian(self, u, xi, theta):
        # (Covariance.py:676-689): -(xi-u) w c as a (d,1) column
        with np.errstate(divide="ignore"):
            v = np.exp(theta[0])
            w = np.exp(np.asarray(theta[2:], dtype=float))
        diff = np.asarray(xi, dtype=float) - np.asarray(u, dtype=float)
        e = v * np.exp(-0.5 * np.dot(diff, w * diff))
        return np.atleast_2d(-diff * w * e).T


def _periodic_theta(theta, d):
    th = _gpx.f64(theta)
    if th.ndim != 1 or th.shape[0] != 2 + 3 * d:
        raise ValueError("theta must have 2 + 3 d = %d entries, got shape %r" % (2 + 3 * d, th.shape))
    return th


class _RawInputModel(_MatrixModel):
    """Owner of one gpx_periodic_fit / gpx_matern_fit handle: K of a kernel on the raw inputs assembled and factored on the device.
    Everything a matrix model answers, plus the kernel's own prediction and likelihood gradient.  A kind names its entry points
    (gpx_<_KIND>_fit / _predict / _nll_grad) and its theta checker; `extra`: what its fit takes after theta."""

    _KIND = None
    _check_theta = None

    def __init__(self, x, t_centered, theta, *extra):
        x = _gpx.f64(x)
        if x.ndim != 2:
            raise ValueError("x must be an (n, d) array")
        self.n, self.d = x.shape
        theta = self._check_theta(theta, self.d)
        self._ntheta = theta.shape[0]
        t = np.zeros(self.n) if t_centered is None else _gpx.f64(t_centered)
        if t.shape != (self.n,):
            raise ValueError("t must have %d entries" % self.n)
        self._h = ctypes.c_void_p()
        self._call("fit", _gpx.ptr(x), _gpx.ptr(t), self.n, self.d, _gpx.ptr(theta), *(extra + (None, ctypes.byref(self._h))))

    def _call(self, what, *args):
        name = "gpx_%s_%s" % (self._KIND, what)
        _gpx.check(getattr(_gpx.lib, name)(*args), name)

    def predict(self, xs):
        m = xs.shape[0]
        mean = np.empty(m)
        var = np.empty(m)
        self._call("predict", self.handle, _gpx.ptr(xs), m, _gpx.ptr(mean), _gpx.ptr(var))
        return mean, var

    def nll_grad(self):
        g = np.empty(self._ntheta)
        self._call("nll_grad", self.handle, _gpx.ptr(g))
        return g


class _PeriodicModel(_RawInputModel):
    _KIND, _check_theta = "periodic", staticmethod(_periodic_theta)


class _MaternModel(_RawInputModel):
    """nu2 = 2 nu.  For nu = 5/2 the handle also serves the batched propagation calls that UncertaintyPropagationApprox makes on it."""
    _KIND, _check_theta = "matern", staticmethod(_theta)

    def __init__(self, x, t_centered, theta, nu2):
        self.nu2 = int(nu2)
        _RawInputModel.__init__(self, x, t_centered, theta, self.nu2)


class _RawInputCovariance(Covariance):
    """What PeriodicCovariance and MaternCovariance share: the matrix methods of a kernel built on the base class's conventions --
    cov_matrix AND cov_matrix_ij carry the +vt on exact equality -- as the fused HIP path (the kind's Gram kernel on the raw inputs,
    Cholesky on the Gram tiles, one-pass likelihood gradient).  A subclass that overrides one of the matrix builders falls back to the
    generic device route of `Covariance` (`_fused()` decides per instance), as for GaussianCovariance.  A kind names its device model
    (`_MODEL`, whose theta checker and gpx_<kind>_gram it uses) and what its entry points take after theta (`_extra`)."""

    _MATRIX_METHODS = GaussianCovariance._MATRIX_METHODS
    _MODEL = None

    def _extra(self):
        return ()

    def _fused(self):
        """True when every matrix-defining method of this instance is the fused one of this base"""
        cls = type(self)
        return all(getattr(cls, m) is getattr(_RawInputCovariance, m) for m in self._MATRIX_METHODS)

    def _new_model(self, x, t, theta):
        return self._MODEL(x, t, theta, *self._extra())

    def _gram(self, xi, xj, theta, deriv):
        a = _gpx.f64(xi)
        b = a if xj is xi else _gpx.f64(xj)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
            raise ValueError("inputs must be (n, d) arrays with equal d")
        th = self._MODEL._check_theta(theta, a.shape[1])
        K = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
        if K.size:
            name = "gpx_%s_gram" % self._MODEL._KIND
            _gpx.check(getattr(_gpx.lib, name)(_gpx.ptr(a), a.shape[0], _gpx.ptr(b), b.shape[0], a.shape[1], _gpx.ptr(th),
                                               *(self._extra() + (int(deriv), _gpx.ptr(K)))), name)
        return K

    def cov_matrix_ij(self, xi, xj, theta):
        """N1 x N2 matrix of the kernel, +vt wherever two rows are equal (Covariance.py:137-152 over the scalar kernel) -- HIP Gram
        kernel."""
        return self._gram(xi, xj, theta, -1)

    def cov_matrix(self, x, theta):
        # (Covariance.py:155-164): cov_matrix_ij(x, x) -- a subclass's own cross-covariance if it has one
        return self.cov_matrix_ij(x, x, theta)

    def _d_cov_matrix_d_theta_ij(self, xi, xj, theta, j):
        """d K / d theta_j entry-wise (Covariance.py:236-253 over _d_cov_d_theta) from the kernel's derivative variant.  An accessor:
        the likelihood gradient never forms these matrices (periodic_nll_grad_kernel, matern_nll_grad_kernel)."""
        if not 0 <= j < len(theta):
            raise ValueError("j must be in [0, %d)" % len(theta))
        return self._gram(xi, xj, theta, j)

    def _d_cov_matrix_d_theta(self, x, theta, j):
        # (Covariance.py:256-265)
        return self._d_cov_matrix_d_theta_ij(x, x, theta, j)

    def inv_cov_matrix(self, x, theta, cov_matrix=None):
        """K^-1 (Covariance.py:167-187) from a device fit: K never leaves the device"""
        if cov_matrix is not None or not self._fused():
            return Covariance.inv_cov_matrix(self, x, theta, cov_matrix)
        model = self._new_model(x, None, theta)
        try:
            return model.kinv()
        finally:
            model.close()

    def _log_det_cov_matrix(self, x, theta):
        """log det K (Covariance.py:189-195) from the Cholesky factor of a device fit"""
        if not self._fused():
            return Covariance._log_det_cov_matrix(self, x, theta)
        model = self._new_model(x, None, theta)
        try:
            return model.logdet()
        finally:
            model.close()

    def _model_at(self, x, t, theta):
        return self._fitted_model_at(x, t, theta, self._MODEL._check_theta, self._new_model)

    def _negativeloglikelihood(self, x, t, theta):
        """N/2 log 2pi + 1/2 log det K + 1/2 t^T K^-1 t on the GPU (Covariance.py:197-216); 1e20 when K cannot be factored, like the
        reference's except branch."""
        if not self._fused():
            return Covariance._negativeloglikelihood(self, x, t, theta)
        try:
            return self._model_at(x, t, theta).nll()
        except (np.linalg.LinAlgError, ValueError, ZeroDivisionError):
            return 1.0e+20

    def _d_nll_d_theta(self, x, t, theta):
        """gradient of the NLL (Covariance.py:266-282): one fused pass over K^-1 on the GPU instead of one derivative matrix per
        parameter evaluated entry by entry in Python."""
        if not self._fused():
            return Covariance._d_nll_d_theta(self, x, t, theta)
        return self._model_at(x, t, theta).nll_grad()


class PeriodicCovariance(_RawInputCovariance):
    """ARD squared exponential times a periodic factor per dimension, theta = (log v, log vt, log w_1..d, log p_1..d, log w2_1..d)
    (skgpuppy/Covariance.py:361-433):  k(xi, xj) = v exp(-1/2 sum_k [w_k delta_k^2 + w2_k sin^2(pi delta_k / p_k)]) + (vt iff xi == xj).

    The reference class defines the scalar kernel, its theta derivatives and get_theta only and inherits every matrix method from the
    base class -- so cov_matrix AND cov_matrix_ij carry the +vt on exact equality (also for a query that equals a training row), and
    duplicate training rows make K singular.  Here the matrix methods are the fused HIP path (periodic_gram_kernel, Cholesky on the
    Gram tiles, one-pass likelihood gradient) with those semantics; a subclass that overrides one of the matrix builders falls back to
    the generic device route of `Covariance` (`_fused()`), as for GaussianCovariance.  Like the reference's it offers no Jacobian /
    Hessian: the propagation classes treat it as any generic operator."""

    _MODEL = _PeriodicModel

    @staticmethod
    def _split(xi, theta):
        d, = np.shape(xi)
        with np.errstate(divide="ignore"):
            v = np.exp(theta[0])
            vt = np.exp(theta[1])
            w = np.exp(np.asarray(theta[2:2 + d], dtype=float))
            p = np.exp(np.asarray(theta[2 + d:2 + 2 * d], dtype=float))
            w2 = np.exp(np.asarray(theta[2 + 2 * d:], dtype=float))
        return d, v, vt, w, p, w2

    def __call__(self, xi, xj, theta):
        # (Covariance.py:369-386), the "+vt iff xi == xj elementwise" hack included
        xi = np.asarray(xi)
        xj = np.asarray(xj)
        d, v, vt, w, p, w2 = self._split(xi, theta)
        diff = xi - xj
        return v * np.exp(-0.5 * ((np.sin(np.pi / p * diff) ** 2 * w2).sum() + np.dot(diff.T, w * diff))) + (vt if (xi == xj).all() else 0)

    def get_theta(self, x, t):
        # (Covariance.py:388-396)
        n, d = np.shape(x)
        theta = np.ones(2 + 3 * d)
        theta[0] = np.log(np.var(t)) if t is not None else 1
        theta[1] = np.log(np.var(t) / 100) if t is not None else 1
        theta[2:2 + d] = -2 * np.log((np.max(x, 0) - np.min(x, 0)) / 2.0)
        theta[2 + d:2 + 2 * d] = np.ones(d)
        theta[2 + 2 * d:] = -2 * np.log((np.max(x, 0) - np.min(x, 0)) / 2.0) + np.log(100)
        return theta

    def _d_cov_d_theta(self, xi, xj, theta, j):
        # (Covariance.py:399-433): theta is the LOG of the parameters
        xi = np.asarray(xi)
        xj = np.asarray(xj)
        d, v, vt, w, p, w2 = self._split(xi, theta)
        diff = xi - xj
        if j == 1:
            return vt if (xi == xj).all() else 0
        kf = v * np.exp(-0.5 * ((np.sin(np.pi / p * diff) ** 2 * w2).sum() + np.dot(diff.T, w * diff)))
        if j == 0:
            return kf
        if j < 2 + d:
            return -0.5 * (diff[j - 2] ** 2 * w[j - 2]) * kf
        if j < 2 + 2 * d:
            i = j - (2 + d)
            return np.pi * diff[i] * w2[i] / p[i] * np.sin(np.pi / p[i] * diff[i]) * np.cos(np.pi / p[i] * diff[i]) * kf
        if j < 2 + 3 * d:
            i = j - (2 + 2 * d)
            return -0.5 * (np.sin(np.pi / p[i] * diff[i]) ** 2 * w2[i]) * kf
        return None


class MaternCovariance(_RawInputCovariance):
    """ARD Matern kernel with nu = 3/2 or 5/2, theta = (log v, log vt, log w_1..d) as for GaussianCovariance.  With delta = xi - xj,
    q = sum_k w_k delta_k^2 and s = sqrt(2 nu q):
        nu = 5/2:  k = v (1 + s + s^2 / 3) exp(-s)        nu = 3/2:  k = v (1 + s) exp(-s)        (+ vt iff xi == xj elementwise).

    Built on the base class's conventions, like PeriodicCovariance: cov_matrix AND cov_matrix_ij carry the +vt on exact equality (also
    for a query that equals a training row) and duplicate training rows make K singular.  The matrix methods are the fused HIP path
    (matern_gram_kernel, Cholesky on the Gram tiles, one-pass likelihood gradient); a subclass that overrides one of the matrix
    builders falls back to the generic device route of `Covariance` (`_fused()`).  nu = 5/2 is twice differentiable and offers
    get_Jacobian / get_Hessian, so UncertaintyPropagationApprox and the inverse propagation run fused on the device for it; nu = 3/2
    (no Hessian at the origin) is propagated as any generic operator without derivatives."""

    _MODEL = _MaternModel

    def __init__(self, nu=2.5):
        Covariance.__init__(self)
        if nu not in (1.5, 2.5):
            raise ValueError("nu must be 1.5 or 2.5, got %r" % (nu,))
        self.nu = float(nu)

    @property
    def _nu2(self):
        return int(round(2 * self.nu))

    def _extra(self):
        return (self._nu2,)

    def _radial(self, diff, theta):
        """(s, v exp(-s), w) at the difference diff"""
        with np.errstate(divide="ignore"):
            v = np.exp(theta[0])
            w = np.exp(np.asarray(theta[2:], dtype=float))
        s = np.sqrt(self._nu2 * np.dot(diff, w * diff))
        return s, v * np.exp(-s), w

    def _kf_g(self, s, e):
        """the noise-free kernel and the factor G of its first derivatives"""
        if self._nu2 == 5:
            return e * (1.0 + s + s * s / 3.0), (5.0 / 3.0) * e * (1.0 + s)
        return e * (1.0 + s), 3.0 * e

    def __call__(self, xi, xj, theta):
        xi = np.asarray(xi)
        xj = np.asarray(xj)
        with np.errstate(divide="ignore"):
            vt = np.exp(theta[1])
        s, e, _w = self._radial(xi - xj, theta)
        return self._kf_g(s, e)[0] + (vt if (xi == xj).all() else 0)

    get_theta = GaussianCovariance.get_theta

    def _d_cov_d_theta(self, xi, xj, theta, j):
        """d k(xi, xj) / d theta_j in closed form; theta is the LOG of (v, vt, w): j = 0 -> the noise-free kernel, j = 1 -> vt iff
        xi == xj elementwise, j = 2 + k -> -1/2 w_k delta_k^2 G (no division by s)"""
        xi = np.asarray(xi, dtype=float)
        xj = np.asarray(xj, dtype=float)
        if j == 1:
            with np.errstate(divide="ignore"):
                return np.exp(theta[1]) if (xi == xj).all() else 0
        diff = xi - xj
        s, e, w = self._radial(diff, theta)
        kf, g = self._kf_g(s, e)
        if j == 0:
            return kf
        return -0.5 * w[j - 2] * diff[j - 2] ** 2 * g

    def get_Jacobian(self, u, xi, theta):
        """nu = 5/2: -(xi - u) w G as a (d, 1) column, GaussianCovariance.get_Jacobian's convention"""
        if self._nu2 != 5:
            return Covariance.get_Jacobian(self, u, xi, theta)
        diff = np.asarray(xi, dtype=float) - np.asarray(u, dtype=float)
        s, e, w = self._radial(diff, theta)
        return np.atleast_2d(-diff * w * self._kf_g(s, e)[1]).T

    def get_Hessian(self, u, xi, theta):
        """nu = 5/2: (5/3) v exp(-s) [5 (w diff)(w diff)^T - diag(w) (1 + s)]"""
        if self._nu2 != 5:
            return Covariance.get_Hessian(self, u, xi, theta)
        diff = np.asarray(xi, dtype=float) - np.asarray(u, dtype=float)
        s, e, w = self._radial(diff, theta)
        wd = diff * w
        return (5.0 / 3.0) * e * (5.0 * np.outer(wd, wd) - np.diag(w) * (1.0 + s))


class _SPGPDeviceModel(object):
    """Owner of one gpx_spgp handle: K_NM, chol(K_M + 1e-5 I), Lambda and chol(B + 1e-5 I) resident in HBM."""

    def __init__(self, x, t_centered, theta_gc, xb):
        self.n, self.d = x.shape
        self.m = xb.shape[0]
        self._h = ctypes.c_void_p()
        st = _gpx.lib.gpx_spgp_fit(_gpx.ptr(x), _gpx.ptr(t_centered), self.n, self.d, _gpx.ptr(theta_gc), _gpx.ptr(xb),
                                   self.m, ctypes.byref(self._h))
        _gpx.check(st, "gpx_spgp_fit")

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("device model already released")
        return self._h

    def close(self, _free=_gpx.lib.gpx_spgp_free, _null=ctypes.c_void_p):
        if getattr(self, "_h", None):
            _free(self._h)
            self._h = _null()

    __del__ = close

    def predict(self, xs):
        k = xs.shape[0]
        mean = np.empty(k)
        var = np.empty(k)
        _gpx.check(_gpx.lib.gpx_spgp_predict(self.handle, _gpx.ptr(xs), k, _gpx.ptr(mean), _gpx.ptr(var)), "gpx_spgp_predict")
        return mean, var

    def nll(self):
        out = ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_spgp_nll(self.handle, ctypes.byref(out)), "gpx_spgp_nll")
        return out.value

    def nll_grad(self):
        out = np.empty(2 + self.d + self.m * self.d)
        _gpx.check(_gpx.lib.gpx_spgp_nll_grad(self.handle, _gpx.ptr(out)), "gpx_spgp_nll_grad")
        return out

    def split(self):
        """K-chunks of this model's rank-N products (0: one plain launch each)"""
        out = ctypes.c_int()
        _gpx.check(_gpx.lib.gpx_spgp_split(self.handle, ctypes.byref(out)), "gpx_spgp_split")
        return out.value

    def dense(self, which):
        out = np.empty((self.n, self.n))
        _gpx.check(_gpx.lib.gpx_spgp_dense(self.handle, which, _gpx.ptr(out)), "gpx_spgp_dense")
        return out

    def kinv(self):
        return self.dense(1)

    def cross(self, xi, xj):
        out = np.empty((xi.shape[0], xj.shape[0]))
        if out.size:
            _gpx.check(_gpx.lib.gpx_spgp_cross(self.handle, _gpx.ptr(xi), xi.shape[0], _gpx.ptr(xj), xj.shape[0], _gpx.ptr(out)),
                       "gpx_spgp_cross")
        return out


class SPGPCovariance(Covariance):
    """Snelson's sparse pseudo-input covariance ("next" row f3; skgpuppy/Covariance.py:692-1019).

    theta = (log v, log vt, log w_1..w_d, the m pseudo-inputs flattened row-major).  Like the reference's it offers no
    Jacobian/Hessian; uncertainty propagation of the fitted model goes through GaussianProcess.pseudo_gp(), the model as a dense GP over
    its m pseudo-inputs (O(m^2) per input, no N x N matrix).  Fit, prediction and Snelson's likelihood are O(N m^2) on the GPU;
    cov_matrix / inv_cov_matrix materialise the reference's N x N matrices for small N only."""

    def __init__(self, m):
        self.m = m
        self.cov = GaussianCovariance()

    def _split(self, theta, d):
        th = _gpx.f64(theta)
        if th.ndim != 1 or th.shape[0] != 2 + d + self.m * d:
            raise ValueError("theta must have 2 + d + m*d = %d entries, got shape %r" % (2 + d + self.m * d, th.shape))
        return np.ascontiguousarray(th[:2 + d]), np.ascontiguousarray(np.reshape(th[2 + d:], (self.m, d)))

    def _model(self, x, t, theta):
        xa = _gpx.f64(x)
        if xa.ndim != 2:
            raise ValueError("x must be an (n, d) array")
        tg, xb = self._split(theta, xa.shape[1])
        ta = np.zeros(xa.shape[0]) if t is None else _gpx.f64(t)
        return _SPGPDeviceModel(xa, ta, tg, xb)

    def __call__(self, xi, xj, theta):
        # (Covariance.py:708-732): the full kernel on the diagonal, the low-rank one elsewhere
        xi = np.asarray(xi)
        xj = np.asarray(xj)
        d = np.shape(xi)[0]
        if (xi == xj).all():
            return self.cov(xi, xj, theta[0:2 + d])
        return self.cov_matrix_ij(np.atleast_2d(xi), np.atleast_2d(xj), theta)[0, 0]

    def get_theta(self, x, t):
        # (Covariance.py:734-741): GaussianCovariance start + m training rows drawn at random as pseudo-inputs
        n, d = np.shape(x)
        theta = np.ones(2 + d + self.m * d)
        theta[0:2 + d] = self.cov.get_theta(x, t)
        theta[2 + d:] = np.reshape(np.asarray(x)[np.random.randint(n, size=self.m), :], self.m * d)
        return theta

    def cov_matrix_ij(self, xi, xj, theta):
        """Q_ij = K_iM (K_M + 1e-5 I)^-1 K_Mj (Covariance.py:743-763).  Depends on theta only through the pseudo-inputs'
        factor: the device model behind it is fitted on the M pseudo-inputs themselves (O(M^3), not a fit of xi) and kept
        for the next call with the same theta."""
        a = _gpx.f64(xi)
        b = _gpx.f64(xj)
        th = _gpx.f64(theta)
        key = th.tobytes()
        cached = getattr(self, "_cross_model", None)
        if cached is None or cached[0] != key:
            if cached is not None:
                cached[1].close()
            _tg, xb = self._split(th, a.shape[1])
            cached = (key, self._model(xb, None, th))
            self._cross_model = cached
        return cached[1].cross(a, b)

    def cov_matrix(self, x, theta):
        """Q_N + diag(K_N - Q_N) + vt I (Covariance.py:814-833); shares the device model of (x, theta) with inv_cov_matrix."""
        return self._fit_model(x, None, theta).dense(0)

    def inv_cov_matrix(self, x, theta, cov_matrix=None):
        """the Woodbury inverse (Covariance.py:835-863); `cov_matrix` is ignored as in the reference."""
        return self._fit_model(x, None, theta).dense(1)

    @staticmethod
    def _signature(a):
        """content signature of an array: shape, dtype and a hash of ALL its bytes (xxh3 at several GB/s, crc32 otherwise: a few
        ms for C5's 16 MB of inputs next to a 40 ms fit).  A sampled hash (round 3) missed in-place edits of a few rows and
        handed back a stale device model."""
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        buf = memoryview(a).cast("B")
        try:
            import xxhash
            digest = xxhash.xxh3_64_intdigest(buf)
        except ImportError:
            import zlib
            digest = zlib.crc32(buf)
        return (a.shape, a.dtype.str, digest)

    def _fit_model(self, x, t, theta):
        """the device model of (x, t, theta), kept until the next different request: L-BFGS asks for the likelihood and
        its gradient at the same theta, one after the other.  The key is the CONTENT of x, t and theta (hashed in full); `clear_cache()` releases the device buffers, and `ml_estimate` does so when it is done."""
        key = (self._signature(x), self._signature(t), _gpx.f64(theta).tobytes())
        cached = getattr(self, "_fit_cache", None)
        if cached is None or cached[0] != key:
            if cached is not None:
                cached[1].close()
            self._fit_cache = None
            cached = (key, self._model(x, t, theta))
            self._fit_cache = cached
        return cached[1]

    def clear_cache(self):
        """release the cached device models (K_NM, Z, W^T and the M x M buffers: about 3 N M doubles)"""
        for name in ("_fit_cache", "_cross_model"):
            cached = getattr(self, name, None)
            if cached is not None:
                cached[1].close()
            setattr(self, name, None)

    close = clear_cache

    def ml_estimate(self, x, t):
        try:
            return Covariance.ml_estimate(self, x, t)
        finally:
            self.clear_cache()

    def _negativeloglikelihood(self, x, t, theta):
        """Snelson's O(N m^2) likelihood (Covariance.py:981-1019); raises LinAlgError like the reference's Cholesky."""
        return self._fit_model(x, t, theta).nll()

    def _d_nll_d_theta(self, x, t, theta):
        """analytic gradient of Snelson's likelihood in O(N m^2) on the GPU (gpx_spgp_nll_grad).  The reference's own
        (Covariance.py:906-979) differentiates the dense N x N likelihood at O(N^2 m) per parameter and is itself only
        checked against central differences (skgpuppy/tests/tests.py:538-565)."""
        return self._fit_model(x, t, theta).nll_grad()

    def __getstate__(self):
        state = Covariance.__getstate__(self)
        state.pop("_cross_model", None)          # device handles never enter a pickle
        state.pop("_fit_cache", None)
        return state
