"""Uncertainty propagation -- host-side mirror of skgpuppy/UncertaintyPropagation.py (Approx, Exact).

The reference swaps its pure-Python classes for the compiled Cython twins at import
(skgpuppy/UncertaintyPropagation.py:10-21,244); this module is the third backend: same class names and
methods, the O(N^2) loops K1..K8 run as HIP kernels on the handle of the GaussianProcess.
"""
import ctypes
import math

import numpy as np

from . import _gpx

weaving = False     # the reference's module flags; neither native CPU backend exists here
cython = False
hip = True


class UncertaintyPropagationGA(object):
    """Superclass (UncertaintyPropagation.py:55-85)."""

    def __init__(self, gp):
        self.gp = gp

    def propagate_mean(self, u, Sigma_x):
        return 0

    def propagate_GA(self, u, Sigma_x):
        return 0, 0

    # argument forms of the many-input calls of both subclasses: U (B, d); Sigma_x (d, d) for every input, or (B, d, d)
    def _many_args(self, U, Sigma_x):
        d = self.gp.d
        UU = _gpx.f64(U)
        S = _gpx.f64(Sigma_x)
        if UU.ndim != 2 or UU.shape[1] != d:
            raise ValueError("U must be (B, %d), got %s" % (d, UU.shape))
        if S.shape != (d, d) and S.shape != (len(UU), d, d):
            raise ValueError("Sigma_x must be (%d, %d) or (%d, %d, %d), got %s" % (d, d, len(UU), d, d, S.shape))
        return UU, S


def _u_sigma(gp, u, Sigma_x):
    uu = _gpx.f64(u)
    S = _gpx.f64(Sigma_x)
    if uu.shape != (gp.d,) or S.shape != (gp.d, gp.d):
        raise ValueError("u must be (%d,) and Sigma_x (%d, %d)" % (gp.d, gp.d, gp.d))
    return uu, S


class UncertaintyPropagationApprox(UncertaintyPropagationGA):
    """Girard's approximate Gaussian-approximation moments (UncertaintyPropagation.py:386-630 /
    UncertaintyPropagation2.pyx:189-380).

    With the built-in GaussianCovariance everything runs fused on the device handle (C / J / tr built by a kernel, one pass
    K^-1 [C, J_1..J_d] or two sweeps over the factor, dot products); with MaternCovariance(2.5) every sum comes from the batched
    gpx_matern_propagate_* calls, a single input as a batch of one.  With any other operator (the generic route of
    GaussianProcess) C_ux / J_ux / H_ux come from the operator's own __call__ / get_Jacobian / get_Hessian -- 3N host calls,
    as in the reference (:504-510) -- and the reference's N^2 double loops become two device sweeps over the factor
    (gpx_solve) plus O(N d) dot products."""

    def __init__(self, gp):
        UncertaintyPropagationGA.__init__(self, gp)
        self.v = self.gp._get_v()
        self.Winv = self.gp._get_W_inv()
        self.u = None
        self._cjh = None
        self._kv = None            # generic route: K^-1 [C, J_1..J_d] of the cached u

    def _generic(self):
        return self.gp._route() != "gaussian"

    def _matern52(self):
        """MaternCovariance(2.5) on its fused route: every sum comes from the gpx_matern_propagate_* calls (a single input is a batch
        of one); C_ux / J_ux / H_ux stay host attributes built from the scalar methods.  nu = 3/2 has no Hessian: generic."""
        return self.gp._route() == "matern" and self.gp.cov._nu2 == 5

    def _new_u(self, u, uu):
        if self.u is None or (np.asarray(self.u) != uu).any():
            self.u = u               # stored by reference like UncertaintyPropagation.py:500
            self._cjh = None
            self._kv = None

    def _parts(self, u, Sigma_x):
        uu, S = _u_sigma(self.gp, u, Sigma_x)
        self._new_u(u, uu)
        if self._matern52():
            return tuple(float(o[0]) for o in self._parts_many(uu[None, :], S))
        if self._generic():
            return self._parts_generic(S)
        out = [ctypes.c_double() for _ in range(4)]
        st = _gpx.lib.gpx_propagate_approx(self.gp._dev().handle, _gpx.ptr(uu), _gpx.ptr(S),
                                           *[ctypes.byref(o) for o in out])
        _gpx.check(st, "gpx_propagate_approx")
        mean, var, sigma2, rest = [o.value for o in out]
        return mean, var, sigma2, rest

    # ---- generic operators ---------------------------------------------------------------------------------------
    def _kinv_rows(self):
        """K^-1 [C, J_1..J_d] for the cached u: two sweeps over the factor on the device"""
        if self._kv is None:
            C, J, _H = self._fetch_cjh()
            self._kv = self.gp._dev().solve(np.vstack([C[None, :], J[:, :, 0].T]))
        return self._kv

    @staticmethod
    def _quadratic_parts(cuu, beta, C, J, H, S, KC, KJ, Ktr=None):
        """(mean without meant, sigma2, variance2 + variance3) from the vectors and their products with K^-1
        (UncertaintyPropagation.py:397-408, :412-433, :435-481); KC = Kinv C, KJ[k] = Kinv J_k, Ktr = Kinv tr (None: Kinv is
        symmetric, C.Ktr = tr.KC)"""
        trace = np.einsum("iab,ba->i", H, S)                    # tracedot(H_i, Sigma_x)
        mean = np.dot(beta, C) + 0.5 * np.dot(beta, trace)
        sigma2 = cuu - np.dot(C, KC)
        sd = np.diag(S)
        var2 = -sum(sd[k] * (np.dot(J[:, k, 0], KJ[k]) - np.dot(beta, J[:, k, 0]) ** 2) for k in range(len(sd)))
        var3 = -np.dot(trace, KC) if Ktr is None else -0.5 * (np.dot(C, Ktr) + np.dot(trace, KC))
        return mean, sigma2, var2 + var3

    def _parts_generic(self, S):
        C, J, H = self._fetch_cjh()
        kv = self._kinv_rows()
        mean, sigma2, rest = self._quadratic_parts(self.gp._covariance(self.u, self.u), self.gp._get_beta(), C, J, H, S, kv[0], kv[1:])
        return mean, sigma2 + rest, sigma2, rest

    def _fetch_cjh(self):
        if self._cjh is None:
            if self.u is None:
                raise AttributeError("C_ux/J_ux/H_ux exist only after a propagate call (as in the reference)")
            gp = self.gp
            if self._generic():
                # (UncertaintyPropagation.py:504-510): the operator's own scalar kernel, Jacobian and Hessian per training point
                x, u = gp.x, self.u
                n = len(x)
                self._cjh = (np.array([gp._covariance(u, x[i]) for i in range(n)], dtype=float),
                             np.array([gp._get_Jacobian(u, x[i]) for i in range(n)], dtype=float).reshape(n, gp.d, 1),
                             np.array([gp._get_Hessian(u, x[i]) for i in range(n)], dtype=float))
                return self._cjh
            uu = _gpx.f64(self.u)
            C = np.empty(gp.n)
            J = np.empty((gp.n, gp.d))
            H = np.empty((gp.n, gp.d, gp.d))
            st = _gpx.lib.gpx_cjh(gp._dev().handle, _gpx.ptr(uu), _gpx.ptr(C), _gpx.ptr(J), _gpx.ptr(H))
            _gpx.check(st, "gpx_cjh")
            self._cjh = (C, J.reshape(gp.n, gp.d, 1), H)
        return self._cjh

    # the pure-Python reference exposes these caches as attributes (UncertaintyPropagation.py:501-510)
    @property
    def C_ux(self):
        return self._fetch_cjh()[0]

    @property
    def J_ux(self):
        return self._fetch_cjh()[1]

    @property
    def H_ux(self):
        return self._fetch_cjh()[2]

    def propagate_mean(self, u, Sigma_x):
        # (UncertaintyPropagation.py:397-408): beta.C + 1/2 beta.tr(H Sigma)
        return np.float64(self._parts(u, Sigma_x)[0])

    def propagate_GA(self, u, Sigma_x):
        # (UncertaintyPropagation.py:490-523)
        mean, var, _s2, _rest = self._parts(u, Sigma_x)
        return np.float64(mean + self.gp._get_mean_t()), np.float64(var)

    # ---- many inputs in one call (no reference counterpart: what a caller's loop over propagate_GA computes) ----
    def _parts_many(self, U, Sigma_x):
        """(mean without meant, variance, sigma2, rest), each [B].  Built-in kernel: ONE gpx_propagate_approx_many call -- every
        input's C, tr, J_1..J_d are d + 2 rows of the many-right-hand-side solve behind estimate_many; K^-1 is not built and the
        single-input caches (self.u, C_ux, ...) are not touched.  Generic route (any other Covariance, SPGP): a loop over the
        single-input path on a fresh instance -- correct, not accelerated."""
        UU, S = self._many_args(U, Sigma_x)
        B = len(UU)
        shared = S.ndim == 2
        out = [np.empty(B) for _ in range(4)]
        if self._matern52():
            st = _gpx.lib.gpx_matern_propagate_approx_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(S), int(shared), B,
                                                           *[_gpx.ptr(o) for o in out])
            _gpx.check(st, "gpx_matern_propagate_approx_many")
            return out
        if self._generic():
            one = type(self)(self.gp)
            for i in range(B):
                parts = one._parts(UU[i], S if shared else S[i])
                for o, p in zip(out, parts):
                    o[i] = p
            return out
        st = _gpx.lib.gpx_propagate_approx_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(S), int(shared), B,
                                                *[_gpx.ptr(o) for o in out])
        _gpx.check(st, "gpx_propagate_approx_many")
        return out

    def propagate_mean_many(self, U, Sigma_x):
        """propagate_mean for the rows of U (B, d); Sigma_x (d, d) for all of them or (B, d, d): means [B] WITHOUT meant"""
        return self._parts_many(U, Sigma_x)[0]

    def propagate_GA_many(self, U, Sigma_x):
        """propagate_GA for the rows of U (B, d); Sigma_x (d, d) for all of them or (B, d, d): (means [B] with meant, variances [B])"""
        mean, var, _s2, _rest = self._parts_many(U, Sigma_x)
        return mean + self.gp._get_mean_t(), var

    # The three quadratic-form helpers of the reference (UncertaintyPropagation.py:412-488 / UncertaintyPropagation2.pyx:221-299)
    # take explicit Kinv / x / beta / C_ux / J_ux / H_ux arrays.  Called the way the reference itself calls them -- with the fitted
    # GP's own Kinv and the caches of the last propagation (or with nothing) -- the sums come from the device cache of `u`.  Any
    # OTHER array is honoured: the vectors are taken from the arguments and their products with the explicit matrix run on the
    # device (gpx_symv), so a caller that passes a different Kinv gets that Kinv's numbers, as in the reference.
    def _is_own(self, Kinv=None, beta=None, C_ux=None, J_ux=None, H_ux=None):
        gp = self.gp
        cj = self._cjh if self._cjh is not None else (None, None, None)
        return ((Kinv is None or Kinv is gp._Kinv) and beta is None and (C_ux is None or C_ux is cj[0]) and
                (J_ux is None or J_ux is cj[1]) and (H_ux is None or H_ux is cj[2]))

    def _explicit_parts(self, u, Sigma_x, Kinv, beta, C_ux, J_ux, H_ux):
        gp = self.gp
        uu, S = _u_sigma(gp, u, Sigma_x)
        self._new_u(u, uu)
        C = np.asarray(C_ux if C_ux is not None else self.C_ux, dtype=float).reshape(gp.n)
        J = np.asarray(J_ux if J_ux is not None else self.J_ux, dtype=float).reshape(gp.n, gp.d, 1)
        H = np.asarray(H_ux if H_ux is not None else self.H_ux, dtype=float).reshape(gp.n, gp.d, gp.d)
        b = np.asarray(beta if beta is not None else gp._get_beta(), dtype=float).reshape(gp.n)
        trace = np.einsum("iab,ba->i", H, S)
        V = _gpx.f64(np.vstack([C[None, :], trace[None, :], J[:, :, 0].T]))
        if Kinv is None or Kinv is gp._Kinv:
            KV = gp._dev().solve(V)                              # the model's own K^-1: two sweeps over its factor
        else:
            M = _gpx.f64(Kinv)
            if M.shape != (gp.n, gp.n):
                raise ValueError("Kinv must be (%d, %d)" % (gp.n, gp.n))
            KV = np.empty_like(V)
            _gpx.check(_gpx.lib.gpx_symv(_gpx.ptr(M), gp.n, _gpx.ptr(V), V.shape[0], _gpx.ptr(KV)), "gpx_symv")
        # (a pseudo-input model's _covariance is the plain kernel: its prior variance v + vt is stated apart)
        cuu = gp._prior_variance(u) if getattr(gp, "_pseudo", False) else gp._covariance(u, u)
        return self._quadratic_parts(cuu, b, C, J, H, S, KV[0], KV[2:], KV[1])

    def _get_sigma2(self, u, Kinv=None, x=None, C_ux=None, J_ux=None, H_ux=None):
        """C(u,u) - C^T K^-1 C  (UncertaintyPropagation.py:412-433); needs no Sigma_x"""
        Z = np.zeros((self.gp.d, self.gp.d))
        if self._is_own(Kinv, None, C_ux, J_ux, H_ux):
            return self._parts(u, Z)[2]
        return self._explicit_parts(u, Z, Kinv, None, C_ux, J_ux, H_ux)[1]

    def _get_variance_rest(self, u, Sigma_x, Kinv=None, x=None, beta=None, C_ux=None, J_ux=None, H_ux=None):
        """variance2 + variance3  (UncertaintyPropagation.py:435-481)"""
        if self._is_own(Kinv, beta, C_ux, J_ux, H_ux):
            return self._parts(u, Sigma_x)[3]
        return self._explicit_parts(u, Sigma_x, Kinv, beta, C_ux, J_ux, H_ux)[2]

    def _get_sigma2_and_variance_rest(self, u, Sigma_x, Kinv=None, x=None, beta=None):
        """(UncertaintyPropagation.py:483-488)"""
        if self._is_own(Kinv, beta):
            _m, _var, sigma2, rest = self._parts(u, Sigma_x)
            return sigma2, rest
        _m, sigma2, rest = self._explicit_parts(u, Sigma_x, Kinv, beta, None, None, None)
        return sigma2, rest

    def _getFactor(self, u, Sigma_x, v):
        # (UncertaintyPropagation.py:526-560)
        _m, _var, sigma2, rest = self._parts(u, Sigma_x)
        return (v - sigma2) / rest

    def _get_variance_dv_h(self, u, h):
        # (UncertaintyPropagation.py:564-630); all d values come out of one device call
        uu = _gpx.f64(u)
        self._new_u(u, uu)
        if self._matern52():
            return self._get_variance_dv_many(uu[None, :])[0][0, h]
        if self._generic():
            C, J, H = self._fetch_cjh()
            kv = self._kinv_rows()
            beta = self.gp._get_beta()
            v2 = -(np.dot(J[:, h, 0], kv[1 + h]) - np.dot(beta, J[:, h, 0]) ** 2)
            return v2 - np.dot(kv[0], H[:, h, h])
        out = np.empty(self.gp.d)
        st = _gpx.lib.gpx_propagate_dvh(self.gp._dev().handle, _gpx.ptr(uu), _gpx.ptr(out))
        _gpx.check(st, "gpx_propagate_dvh")
        return out[h]

    def _get_variance_dv_many(self, U):
        """(dvh [B, d], sigma2 [B]): _get_variance_dv_h for every h and _get_sigma2 for the rows of U (B, d) -- all the closed form of
        InverseUncertaintyPropagationApprox needs (the variance rest of a diagonal Sigma = diag(s) is sum_k s_k dvh_k).  Built-in kernel:
        ONE gpx_propagate_dvh_many call -- every input's C, J_1..J_d, H_11..H_dd are 2 d + 1 rows of the many-right-hand-side solve
        behind estimate_many; K^-1 is not built and the single-input caches (self.u, C_ux, ...) are not touched.  Generic route (any other
        Covariance, SPGP): a loop over the single-input path on a fresh instance -- correct, not accelerated."""
        d = self.gp.d
        UU, _S = self._many_args(U, np.zeros((d, d)))
        B = len(UU)
        dvh, sigma2 = np.empty((B, d)), np.empty(B)
        if self._matern52():
            st = _gpx.lib.gpx_matern_propagate_dvh_many(self.gp._dev().handle, _gpx.ptr(UU), B, _gpx.ptr(dvh), _gpx.ptr(sigma2))
            _gpx.check(st, "gpx_matern_propagate_dvh_many")
            return dvh, sigma2
        if self._generic() or getattr(self.gp, "_pseudo", False):
            # (a PseudoInputGP: the batched call has no K^-1 form -- the single-input device call, one input after the other)
            one = type(self)(self.gp)
            for i in range(B):
                for h in range(d):
                    dvh[i, h] = one._get_variance_dv_h(UU[i], h)
                sigma2[i] = one._get_sigma2(UU[i])
            return dvh, sigma2
        st = _gpx.lib.gpx_propagate_dvh_many(self.gp._dev().handle, _gpx.ptr(UU), B, _gpx.ptr(dvh), _gpx.ptr(sigma2))
        _gpx.check(st, "gpx_propagate_dvh_many")
        return dvh, sigma2


class UncertaintyPropagationLinear(UncertaintyPropagationGA):
    """First-order (delta-method) propagation (UncertaintyPropagation.py:213-242): mean = mu(u), variance = sum_k g_k^2 Sigma_kk + vt with
    g = d mu / d u -- the DIAGONAL of Sigma_x only, plus vt, as the reference has it.

    The reference takes g by central differences of gp(x)[0], 2 d calls of estimate per input.  With the built-in Gaussian and Matern
    kernels g is the closed-form sum over alpha (GaussianProcess.estimate_many_gradient(variance=False), gpx_predict_mean_grad): one
    fused pass over the B x N pairs for a whole batch and no solve at all.  Every other route takes the reference's differences, batched
    into one estimate_many call."""

    def _mean_grad(self, U):
        """(mean WITHOUT meant [B], g [B, d])"""
        gp = self.gp
        if gp._route() in ("gaussian", "matern"):
            UU = _gpx.f64(U)
            mean, g = np.empty(len(UU)), np.empty(UU.shape)
            _gpx.check(_gpx.lib.gpx_predict_mean_grad(gp._dev().handle, _gpx.ptr(UU), len(UU), _gpx.ptr(mean), _gpx.ptr(g)), "gpx_predict_mean_grad")
            return mean, g
        mean, g = gp.estimate_many_gradient(U, variance=False)
        return mean - gp._get_mean_t(), g

    def _derivative(self, x, i, d=1e-5):
        """d mu / d x_i at x (UncertaintyPropagation.py:214-227): analytic on the fused routes (d is not used there), the reference's
        central difference of step d otherwise"""
        return np.float64(self.gp.estimate_many_gradient(np.atleast_2d(_gpx.f64(x)), variance=False, h=d)[1][0, i])

    def propagate_mean(self, u, Sigma_x):
        # (UncertaintyPropagation.py:229-231): gp(u)[0], meant included
        uu, _S = _u_sigma(self.gp, u, Sigma_x)
        return np.float64(self._mean_grad(uu[None, :])[0][0] + self.gp._get_mean_t())

    def propagate_GA(self, u, Sigma_x):
        # (UncertaintyPropagation.py:233-242)
        uu, S = _u_sigma(self.gp, u, Sigma_x)
        mean, var = self.propagate_GA_many(uu[None, :], S)
        return np.float64(mean[0]), np.float64(var[0])

    # ---- many inputs in one call ----
    def propagate_mean_many(self, U, Sigma_x):
        """propagate_mean for the rows of U (B, d); Sigma_x (d, d) for all of them or (B, d, d): means [B] WITHOUT meant"""
        UU, _S = self._many_args(U, Sigma_x)
        return self._mean_grad(UU)[0]

    def propagate_GA_many(self, U, Sigma_x):
        """propagate_GA for the rows of U (B, d); Sigma_x (d, d) for all of them or (B, d, d): (means [B] with meant, variances [B])"""
        UU, S = self._many_args(U, Sigma_x)
        mean, g = self._mean_grad(UU)
        sd = np.diagonal(S, axis1=-2, axis2=-1)             # (d,) or (B, d)
        var = np.zeros(len(UU))
        for k in range(UU.shape[1]):                        # the reference's order of the sum (:236-238), then + vt (:240)
            var = var + g[:, k] ** 2 * (sd[k] if S.ndim == 2 else sd[:, k])
        return mean + self.gp._get_mean_t(), var + self.gp._get_vt()


class _ExplicitInverse(object):
    """Owner of one gpx_kinv_model: an explicit K^-1 / beta resident in HBM (gpx.h)."""

    def __init__(self, Kinv, beta, n):
        self._h = ctypes.c_void_p()
        _gpx.check(_gpx.lib.gpx_kinv_model_create(_gpx.ptr(Kinv), _gpx.ptr(beta), n, ctypes.byref(self._h)), "gpx_kinv_model_create")

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("explicit-inverse model already released")
        return self._h

    def close(self, _free=_gpx.lib.gpx_kinv_model_free, _null=ctypes.c_void_p):
        if getattr(self, "_h", None):
            _free(self._h)
            self._h = _null()

    __del__ = close


class UncertaintyPropagationExact(UncertaintyPropagationGA):
    """Girard's exact Gaussian-approximation moments (UncertaintyPropagation.py:246-379 /
    UncertaintyPropagation2.pyx:57-184)."""

    # scalar correction factors of Girard's exact moments -- O(d^2) host arithmetic exactly as the reference defines them
    # (UncertaintyPropagation.py:247-266, :292-321); their N and N^2-fold evaluation is the device kernels' job
    def _prepare_C_corr(self, D):
        I = np.eye(D)
        self.Deltainv = self.Winv - np.diag(np.array([self.Winv[i][i] / (1 + self.Winv[i][i] * self.Sigma_x[i][i]) for i in range(D)]))
        self.normalize_C_corr = 1 / np.sqrt(np.linalg.det(I + self.Winv * self.Sigma_x))

    def _get_C_corr(self, u, xi):
        diff = np.asarray(u, dtype=float) - np.asarray(xi, dtype=float)
        return self.normalize_C_corr * np.exp(0.5 * (np.dot(diff.T, np.dot(self.Deltainv, diff))))

    def _prepare_C_corr2(self, D):
        I = np.eye(D)
        W = np.diag(np.array([1 / self.Winv[i][i] for i in range(D)]))
        self.LambdaInv = 2 * self.Winv - np.linalg.inv(0.5 * W + self.Sigma_x)
        self.normalize_C_corr2 = 1 / np.sqrt(np.linalg.det(2 * self.Winv * self.Sigma_x + I))

    def _get_C_corr2(self, u, x):
        diff = np.asarray(u, dtype=float) - np.asarray(x, dtype=float)
        return self.normalize_C_corr2 * np.exp(0.5 * (np.dot(diff.T, np.dot(self.LambdaInv, diff))))

    def _set_constants(self, u, Sigma_x):
        # attributes the reference's propagate_* leave behind (UncertaintyPropagation.py:279-283, :326-334)
        self.Winv = self.gp._get_W_inv()
        self.Sigma_x = Sigma_x
        with np.errstate(all="ignore"):
            self._prepare_C_corr(len(u))
            self._prepare_C_corr2(len(u))

    def _generic_moments(self, u, Sigma_x, C_ux, want_var):
        """Any operator but the fused built-in kernel (a from-scratch Covariance, a subclass that overrides a matrix builder, SPGP):
        the reference's class talks to the GP only through _get_beta / _get_W_inv / _inv_cov_matrix / _covariance / x
        (UncertaintyPropagation.py:269-290, :323-379), so it returns numbers for such a GP -- Girard's correction factors built from
        theta[2:2+d], applied to the operator's own C(u, x_i).  C_ux comes from the operator's scalar kernel on the host (N calls, as
        in the reference), the N and N^2 sums run on the device over the model's K^-1 (gpx_propagate_exact_matrix)."""
        gp = self.gp
        uu, S = _u_sigma(gp, u, Sigma_x)
        x = _gpx.f64(gp.x)
        if C_ux is None:
            C_ux = np.array([gp._covariance(u, gp.x[i]) for i in range(gp.n)])
        C = _gpx.f64(C_ux).reshape(gp.n)
        w = _gpx.f64(np.diag(self.Winv))
        pseudo = getattr(gp, "_pseudo", False)              # (a PseudoInputGP with a caller's C_ux: its P and beta as an explicit model)
        cuu = float(gp._prior_variance(u) if pseudo else gp._covariance(u, u)) if want_var else 0.0
        mean, var = ctypes.c_double(), ctypes.c_double()
        pvar = ctypes.byref(var) if want_var else None      # mean only: the library neither builds nor reads K^-1
        if gp._route() in ("generic", "gaussian", "periodic", "matern") and not pseudo:
            # (any fitted handle: a gpx_fit_matrix one, a gpx_periodic_fit one -- the reference has no input derivatives for that kernel,
            # it is propagated as any generic operator --, a gpx_matern_fit one likewise, or -- a caller-supplied C_ux on the built-in route -- the gpx_fit one)
            st = _gpx.lib.gpx_propagate_exact_matrix(gp._dev().handle, None, None, _gpx.ptr(x), gp.n, gp.d, _gpx.ptr(w), _gpx.ptr(C),
                                                     _gpx.ptr(uu), _gpx.ptr(S), cuu, ctypes.byref(mean), pvar)
        else:
            # (SPGP: the model's dense K^-1 -- what the reference's class reads through _inv_cov_matrix -- and beta = Kinv t: kept on the
            # device across calls, uploaded once per Kinv array: gpx_kinv_model_*)
            st = _gpx.lib.gpx_propagate_exact_model(self._explicit_model(gp), _gpx.ptr(x), gp.d, _gpx.ptr(w), _gpx.ptr(C), _gpx.ptr(uu),
                                                    _gpx.ptr(S), cuu, ctypes.byref(mean), pvar)
        _gpx.check(st, "gpx_propagate_exact_matrix")
        return mean.value, var.value

    def _explicit_model(self, gp):
        """device copy of the GP's dense Kinv attribute and beta (padded, symmetrised), rebuilt only when the GP holds another Kinv array"""
        Kinv = gp._inv_cov_matrix()
        key = (id(Kinv), Kinv.__array_interface__["data"][0], Kinv.shape)
        cached = getattr(self, "_kinv_model", None)
        if cached is not None and cached[0] == key:
            return cached[1].handle
        self._release_explicit_model()
        self._kinv_model = (key, _ExplicitInverse(_gpx.f64(Kinv), _gpx.f64(gp._get_beta()), gp.n), Kinv)   # (Kinv kept alive: its id is the key)
        return self._kinv_model[1].handle

    def _release_explicit_model(self):
        cached = getattr(self, "_kinv_model", None)
        if cached is not None:
            cached[1].close()
            self._kinv_model = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_kinv_model", None)          # device handles never enter a pickle
        return state

    def propagate_mean(self, u, Sigma_x, C_ux=None):
        # (UncertaintyPropagation.py:269-290).  A caller-supplied C_ux is USED, as in the reference's class (sum_i beta_i C_ux_i corr_i):
        # on the built-in route too it goes through gpx_propagate_exact_matrix on the fitted handle; without one the device builds
        # C(u, x_i) itself (gpx_exact_mean).
        self._set_constants(u, np.asarray(Sigma_x, dtype=float))
        if self.gp._route() != "gaussian" or C_ux is not None:
            return np.float64(self._generic_moments(u, Sigma_x, C_ux, False)[0])
        uu, S = _u_sigma(self.gp, u, Sigma_x)
        out = ctypes.c_double()
        st = _gpx.lib.gpx_exact_mean(self.gp._dev().handle, _gpx.ptr(uu), _gpx.ptr(S), ctypes.byref(out))
        _gpx.check(st, "gpx_exact_mean")
        return np.float64(out.value)

    def propagate_GA(self, u, Sigma_x):
        # (UncertaintyPropagation.py:323-379)
        uu, S = _u_sigma(self.gp, u, Sigma_x)
        self._set_constants(uu, S)
        if self.gp._route() != "gaussian":
            mean, var = self._generic_moments(u, Sigma_x, None, True)
            return np.float64(mean + self.gp._get_mean_t()), np.float64(var)
        mean, var = ctypes.c_double(), ctypes.c_double()
        st = _gpx.lib.gpx_propagate_exact(self.gp._dev().handle, _gpx.ptr(uu), _gpx.ptr(S), ctypes.byref(mean),
                                          ctypes.byref(var))
        _gpx.check(st, "gpx_propagate_exact")
        return np.float64(mean.value + self.gp._get_mean_t()), np.float64(var.value)

    # ---- many inputs in one call (no reference counterpart: what a caller's loop over propagate_GA computes) ----
    def _moments_many(self, U, Sigma_x, want_var):
        """(means without meant, variances or None), each [B].  Built-in kernel: ONE gpx_propagate_exact_many call -- for the inputs that
        share a Sigma the double sum is the quadratic form h^T M h with M = (Kinv - beta beta^T) o E built once (gpx.h); with
        want_var = False K^-1 is neither built nor read.  Any other route (a generic operator, SPGP): a loop over the single-input path on
        a fresh instance -- correct, not accelerated.  Neither sets Winv, Sigma_x, Deltainv, LambdaInv or the normalisers on this instance."""
        UU, S = self._many_args(U, Sigma_x)
        B = len(UU)
        shared = S.ndim == 2
        mean, var = np.empty(B), (np.empty(B) if want_var else None)
        if self.gp._route() != "gaussian":
            one = type(self)(self.gp)
            for i in range(B):
                Si = S if shared else S[i]
                one._set_constants(UU[i], Si)                    # what propagate_GA / propagate_mean do first
                m, v = one._generic_moments(UU[i], Si, None, want_var)
                mean[i] = m
                if want_var:
                    var[i] = v
            return mean, var
        st = _gpx.lib.gpx_propagate_exact_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(S), int(shared), B, _gpx.ptr(mean),
                                               _gpx.ptr(var) if want_var else None)
        _gpx.check(st, "gpx_propagate_exact_many")
        return mean, var

    def propagate_mean_many(self, U, Sigma_x):
        """propagate_mean for the rows of U (B, d); Sigma_x (d, d) for all of them or (B, d, d): means [B] WITHOUT meant"""
        return self._moments_many(U, Sigma_x, False)[0]

    def propagate_GA_many(self, U, Sigma_x):
        """propagate_GA for the rows of U (B, d); Sigma_x (d, d) for all of them or (B, d, d): (means [B] with meant, variances [B])"""
        mean, var = self._moments_many(U, Sigma_x, True)
        return mean + self.gp._get_mean_t(), var

    # ---- the moments with their gradients in u and in the diagonal of Sigma_x (no reference counterpart: the gradient whose absence makes
    # the reference's exact inverse solver derivative-free, InverseUncertaintyPropagation.py:103-104) ----
    def propagate_GA_gradient_many(self, U, Sigma_x, h=1e-5):
        """(mean + meant [B], var [B], d mean / d u [B, d], d var / d u [B, d], d mean / d v [B, d], d var / d v [B, d]) for the rows of
        U (B, d), v_k = Sigma_x[k, k] with every other entry of Sigma_x held fixed; Sigma_x (d, d) for all inputs or (B, d, d).

        Route "gaussian" (pseudo_gp() included) is fused: ONE gpx_propagate_exact_grad_many call, closed form (gpx.h); h is not used.  Every
        other route takes central differences through propagate_GA_many, one call per distinct Sigma: the B inputs and their 2 d B shifts by
        h along each coordinate under Sigma_x, then per k the B inputs under Sigma_x -+ h v_k e_k e_k^T (a relative step; h itself where
        v_k = 0).  Neither sets Winv, Sigma_x, Deltainv, LambdaInv or the normalisers on this instance."""
        UU, S = self._many_args(U, Sigma_x)
        B, d = UU.shape
        meant = self.gp._get_mean_t()
        if self.gp._route() == "gaussian":
            mean, var = np.empty(B), np.empty(B)
            g = [np.empty((B, d)) for _ in range(4)]
            st = _gpx.lib.gpx_propagate_exact_grad_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(S), int(S.ndim == 2), B, _gpx.ptr(mean),
                                                        _gpx.ptr(var), *[_gpx.ptr(a) for a in g])
            _gpx.check(st, "gpx_propagate_exact_grad_many")
            return (mean + meant, var) + tuple(g)
        # rows [0, B): the inputs; then per k the B inputs moved by -h and the B moved by +h along k
        pts = np.concatenate([UU[None]] + [UU[None] + s * h * np.eye(d)[k] for k in range(d) for s in (-1.0, 1.0)]).reshape(-1, d)
        mu, var = self.propagate_GA_many(pts, S if S.ndim == 2 else np.tile(S, (2 * d + 1, 1, 1)))
        mu, var = np.asarray(mu).reshape(2 * d + 1, B), np.asarray(var).reshape(2 * d + 1, B)
        dmu, dvu = ((mu[2::2] - mu[1::2]) / (2.0 * h)).T, ((var[2::2] - var[1::2]) / (2.0 * h)).T
        dmv, dvv = np.empty((B, d)), np.empty((B, d))
        for k in range(d):
            vk = S[..., k, k]
            step = np.where(vk != 0, h * np.abs(vk), h)
            side = []
            for s in (-1.0, 1.0):
                Sk = S.copy()
                Sk[..., k, k] = vk + s * step
                side.append(self.propagate_GA_many(UU, Sk))
            dmv[:, k] = (side[1][0] - side[0][0]) / (2.0 * step)
            dvv[:, k] = (side[1][1] - side[0][1]) / (2.0 * step)
        return mu[0], var[0], dmu, dvu, dmv, dvv

    def propagate_GA_gradient(self, u, Sigma_x, h=1e-5):
        """single-input twin of propagate_GA_gradient_many: scalars for mean and var, [d] for the four gradients"""
        uu, S = _u_sigma(self.gp, u, Sigma_x)
        return tuple(o[0] for o in self.propagate_GA_gradient_many(uu[None], S, h))


# ---- the numerical family (UncertaintyPropagation.py:28-52, :90-162) ---------------------------------------------------------------
class UncertaintyPropagation(object):
    """Superclass of the propagators that return the output density itself (UncertaintyPropagation.py:28-52)."""

    def propagate(self, y, u, Sigma_x):
        """p(y) under x ~ N(u, Sigma_x) (Girard 2004, p. 32)"""

    def propagate_many(self, yvec, u, Sigma_x):
        return np.array([self.propagate(y, u, Sigma_x) for y in yvec])


MAX_NODES = 1 << 22


class _MixturePropagation(UncertaintyPropagationGA, UncertaintyPropagation):
    """What UncertaintyPropagationNumericalHG and UncertaintyPropagationMC share: under x ~ N(u, Sigma_x) the output is the mixture
    p(y) = sum_s wq_s N(y; mu(x_s), sigma^2(x_s)) over the nodes x_s = u + A z_s of a rule (z [S, d], wq [S]) and a square root A of the
    input covariance.  The reference evaluates gp(x_s) in S Python calls per expectation; here the nodes of ALL inputs are rows of ONE
    many-row solve (estimate_many's) and one reduction kernel returns, per input, the mean, the variance and the third and fourth central
    moments of the mixture, and its density at any number of y.

    Built-in Gaussian, periodic and Matern kernels: gpx_propagate_quadrature_many -- nodes, mu and sigma^2 never leave the device.  Every other route
    (a generic operator, SPGP): the nodes are built on the host, gp.estimate_many evaluates them, gpx_mixture_reduce reduces its output."""

    def __init__(self, gp):
        if getattr(gp, "_pseudo", False):
            raise TypeError("%s evaluates the predictor at its nodes: pass the SPGP GaussianProcess itself (the PseudoInputGP's parent), "
                            "whose estimate_many serves it" % type(self).__name__)
        UncertaintyPropagationGA.__init__(self, gp)

    def _rule(self, d):
        raise NotImplementedError

    def _root(self, S):
        raise NotImplementedError

    def _reduce(self, U, Sigma_x, Y=None):
        """(mom [5, B] = mean WITH meant | var | E[sigma^2] | m3 | m4, dens [B, ny] or None)"""
        gp = self.gp
        UU, S = self._many_args(U, Sigma_x)
        B, d = UU.shape
        shared = S.ndim == 2
        A = _gpx.f64(self._root(S) if shared else np.stack([self._root(Si) for Si in S]).reshape(B, d, d))
        z, wq = self._rule(d)
        z, wq = _gpx.f64(z), _gpx.f64(wq)
        ns = len(wq)
        ny, yshared, YY = 0, 1, None
        if Y is not None:
            YY = _gpx.f64(Y)
            if YY.ndim == 1:
                ny = len(YY)
            elif YY.ndim == 2 and YY.shape[0] == B:
                ny, yshared = YY.shape[1], 0
            else:
                raise ValueError("Y must be (ny,) or (%d, ny), got %s" % (B, YY.shape))
        mom = np.empty((5, B))
        dens = np.empty((B, ny)) if ny else None
        yp = _gpx.ptr(YY) if ny else None
        dp = _gpx.ptr(dens) if ny else None
        meant = float(gp._get_mean_t())
        if gp._route() in ("gaussian", "periodic", "matern"):
            st = _gpx.lib.gpx_propagate_quadrature_many(gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(A), int(shared), B, _gpx.ptr(z), _gpx.ptr(wq),
                                                        ns, yp, ny, yshared, meant, _gpx.ptr(mom), dp)
            _gpx.check(st, "gpx_propagate_quadrature_many")
            mom[0] += meant
        else:
            # the model's own estimate_many output (its means carry meant: no shift)
            X = UU[:, None, :] + (z.dot(A.T)[None] if shared else np.einsum("ike,se->isk", A, z))
            mu, var = gp.estimate_many(X.reshape(B * ns, d))
            mu, var = _gpx.f64(mu), _gpx.f64(var)
            st = _gpx.lib.gpx_mixture_reduce(_gpx.ptr(mu), _gpx.ptr(var), _gpx.ptr(wq), ns, B, yp, ny, yshared, 0.0, _gpx.ptr(mom), dp)
            _gpx.check(st, "gpx_mixture_reduce")
        return mom, dens

    # ---- the reference's surface ----
    def propagate_mean(self, u, Sigma_x):
        """E[mu(x)], meant included (the reference averages gp(x)[0])"""
        return np.float64(self._reduce(np.atleast_2d(_gpx.f64(u)), Sigma_x)[0][0, 0])

    def propagate_GA(self, u, Sigma_x):
        mom, _ = self._reduce(np.atleast_2d(_gpx.f64(u)), Sigma_x)
        return np.float64(mom[0, 0]), np.float64(mom[1, 0])

    def propagate(self, y, u, Sigma_x):
        return np.float64(self.propagate_many([y], u, Sigma_x)[0])

    def propagate_many(self, yvec, u, Sigma_x):
        """the density at every y of yvec: one device call (the reference: len(yvec) S calls of gp(x))"""
        return self._reduce(np.atleast_2d(_gpx.f64(u)), Sigma_x, _gpx.f64(yvec).reshape(-1))[1][0]

    # ---- many inputs in one call ----
    def propagate_GA_many(self, U, Sigma_x):
        """(means [B] with meant, variances [B]) for the rows of U (B, d); Sigma_x (d, d) for all of them or (B, d, d)"""
        mom, _ = self._reduce(U, Sigma_x)
        return mom[0], mom[1]

    def propagate_moments_many(self, U, Sigma_x):
        """(mean with meant, variance, third central moment, fourth central moment), each [B]"""
        mom, _ = self._reduce(U, Sigma_x)
        return mom[0], mom[1], mom[3], mom[4]

    def propagate_density_many(self, Y, U, Sigma_x):
        """densities [B, ny] at Y (ny,) -- the same y for every input -- or (B, ny)"""
        return self._reduce(U, Sigma_x, Y)[1]


class UncertaintyPropagationNumericalHG(_MixturePropagation):
    """Gauss-Hermite quadrature (UncertaintyPropagation.py:135-162, Utilities.py:144-167): the tensor grid of
    numpy.polynomial.hermite.hermgauss(order) in itertools.product order, wq = prod w / pi^(d/2), order = 4 as the reference fixes it.

    full_sigma=False is the reference's rule EXACTLY: x_s = u + sqrt(2) diag(sqrt(Sigma_kk)) z_s -- it reads the diagonal of Sigma_x and
    ignores every off-diagonal entry (Utilities.py:157), so correlated inputs are propagated as if independent.  full_sigma=True takes
    A = sqrt(2) chol(Sigma_x) instead, the rule for the covariance as given.  order^d may not exceed 2^22 nodes."""

    def __init__(self, gp, order=4, full_sigma=False):
        _MixturePropagation.__init__(self, gp)
        self.order = int(order)
        self.full_sigma = bool(full_sigma)
        if self.order < 1:
            raise ValueError("order must be >= 1")

    def _rule(self, d):
        if self.order ** d > MAX_NODES:
            raise ValueError("order %d in %d dimensions is %d nodes (more than %d)" % (self.order, d, self.order ** d, MAX_NODES))
        x, w = np.polynomial.hermite.hermgauss(self.order)
        # w / sqrt(pi) per axis, with the weights' own sum for sqrt(pi) (they are equal in exact arithmetic; hermgauss's sum is off by up to
        # 2.5 u, which the d-fold product multiplies): wq then sums to 1 within 4 u for every order <= 8, d <= 4
        w = w / math.fsum(w)
        z = np.stack(np.meshgrid(*([x] * d), indexing="ij"), -1).reshape(-1, d)          # itertools.product(x, repeat=d) order
        ws = np.stack(np.meshgrid(*([w] * d), indexing="ij"), -1).reshape(-1, d)
        return z, ws.prod(axis=1)

    def _root(self, S):
        if self.full_sigma:
            return np.sqrt(2.0) * np.linalg.cholesky(S)
        return np.diag(np.sqrt(np.diag(S)) * np.sqrt(2.0))


class UncertaintyPropagationMC(_MixturePropagation):
    """Monte-Carlo integration (UncertaintyPropagation.py:90-132, Utilities.py:172-185): z = standard_normal((n, d)) from
    RandomState(seed), or from numpy's global state when seed is None (as the reference, so numpy.random.seed governs it), wq = 1 / n,
    x_s = u + A z_s with A = chol(Sigma_x) (the symmetric square root when Sigma_x is singular).

    ONE sample set per call serves the mean, the variance and the density, and every input of a batch.  The reference draws three
    independent sets inside propagate_GA (and its sampler is SVD-based): results are statistically equivalent, not sample-identical."""

    def __init__(self, gp, n=1000, seed=None):
        _MixturePropagation.__init__(self, gp)
        self.n = int(n)
        self.seed = seed
        if self.n < 1:
            raise ValueError("n must be >= 1")

    def _rule(self, d):
        if self.n > MAX_NODES:
            raise ValueError("n = %d is more than %d nodes" % (self.n, MAX_NODES))
        rng = np.random if self.seed is None else np.random.RandomState(self.seed)
        return rng.standard_normal((self.n, d)), np.full(self.n, 1.0 / self.n)

    def _root(self, S):
        try:
            return np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            lam, V = np.linalg.eigh(0.5 * (S + S.T))
            return (V * np.sqrt(np.maximum(lam, 0.0))).dot(V.T)
