"""Which input's uncertainty produces the output variance: the variance decomposition of the GP predictor mean under independent
Gaussian inputs x_k ~ N(u_k, s_k), in closed form for the ARD squared-exponential kernel (gpx_sensitivity_many; include/gpx.h carries
the formulas).  No reference counterpart: the reference's nearest code is the nquad / Hermite-Gauss cross-check of
skgpuppy/UncertaintyPropagation.py:135-210.

  V        = Var(mu(x))                       the variance of the predictor mean (the beta beta^T part of Girard's exact variance)
  first_k  = Var_{x_k}(E[mu | x_k])           what x_k's uncertainty produces on its own
  total_k  = E[Var_{x_k}(mu | x_~k)]          what is left when everything but x_k is known: first_k plus every interaction with x_k
  sum_k first_k <= V <= sum_k total_k;  the Sobol indices are first / V and total / V.
  second_kl = V_kl - first_k - first_l        with WHICH other input x_k interacts (second_order*; gpx_sensitivity_second_many)
  D_S, Sh_k                                   EVERY interaction order and the Shapley effects, sum_k Sh_k = V, for up to ten uncertain
                                              inputs (anova*, shapley*, closed_variance; gpx_sensitivity_anova_many)
  posterior=True                              the same terms of the GP f itself, in posterior expectation: each plus the term of the
                                              posterior residual (variances*, indices*; gpx_sensitivity_post_many, reads K^-1)
  C = E[grad f grad f^T]                      which DIRECTIONS matter: the active-subspace matrix, its diagonal the DGSM nu_k with
                                              total_k <= s_k nu_k (gradient_moments*, dgsm*, active_subspace; gpx_sensitivity_gradient_many)

The call reads (x, beta, v, w) alone -- no K^-1, no factor, no solve: a GaussianProcess on the fused GaussianCovariance route costs N^2 d
per input, a PseudoInputGP (GaussianProcess.pseudo_gp() of an SPGP model) m^2 d.  Setting all but one Sigma_kk to zero in propagate_GA is
NOT first_k: that pins the other inputs at u instead of averaging over them.

SensitivityAnalysis(gp, distribution="uniform") reads the same (u, Sigma_x) as the centre and the variance of independent UNIFORM inputs,
x_k ~ U(u_k - sqrt(3 s_k), u_k + sqrt(3 s_k)) -- the design-box setting of global sensitivity analysis (gpx_sensitivity_box_many); the
*_box methods take the bounds themselves, whatever the distribution argument; second_order_box* are the pair interactions over such a box
(gpx_sensitivity_box_second_many)."""
import numpy as np

from . import _gpx
from .GaussianProcess import GaussianProcess, PseudoInputGP


class SensitivityAnalysis(object):
    """SensitivityAnalysis(gp): gp a GaussianProcess with a fused GaussianCovariance, or a PseudoInputGP."""

    def __init__(self, gp, distribution="gaussian"):
        if distribution not in ("gaussian", "uniform"):
            raise ValueError("distribution must be 'gaussian' or 'uniform', got %r" % (distribution,))
        self.distribution = distribution
        served = isinstance(gp, PseudoInputGP) or (isinstance(gp, GaussianProcess) and gp._route() == "gaussian")
        if not served:
            route = gp._route() if isinstance(gp, GaussianProcess) else type(gp).__name__
            raise TypeError("SensitivityAnalysis serves a GaussianProcess whose cov is a (fused) GaussianCovariance, or a PseudoInputGP "
                            "(GaussianProcess.pseudo_gp() of an SPGP model): the closed form is the ARD squared-exponential kernel's; got %r" % (route,))
        self.gp = gp

    @staticmethod
    def _variances_of(Sigma_x, d, b=None):
        """The input variances of Sigma_x as an array: [d] (one input, or one set for all b inputs) or [b, d].  Accepted: a vector [d], a
        diagonal matrix [d, d], and with b given also [b, d] and [b, d, d].  With b == d a 2-D array is ambiguous (a matrix or b rows of
        variances) and refused: pass the vector [d] or the [b, d, d] form.  ValueError for any other shape, a non-zero off-diagonal entry (the
        decomposition needs independent inputs), a negative or a non-finite variance.  Needs no device."""
        S = np.asarray(Sigma_x, dtype=np.float64)
        if S.ndim == 1 and S.shape == (d,):
            out = S
        elif S.ndim == 2 and S.shape == (d, d) and (b is None or b != d):
            out = SensitivityAnalysis._diagonal_of(S, d)
        elif b is not None and S.ndim == 2 and S.shape == (b, d) and b != d:
            out = S
        elif b is not None and S.ndim == 2 and S.shape == (d, d):
            raise ValueError("Sigma_x of shape (%d, %d) with b == d is either one matrix or b rows of variances: pass the vector [d] or the "
                             "[b, d, d] form" % (d, d))
        elif b is not None and S.ndim == 3 and S.shape == (b, d, d):
            out = np.stack([SensitivityAnalysis._diagonal_of(S[i], d) for i in range(b)]) if b else np.empty((0, d))
        else:
            forms = "[%d] or [%d, %d]" % (d, d, d) + ("" if b is None else ", [%d, %d] or [%d, %d, %d]" % (b, d, b, d, d))
            raise ValueError("Sigma_x of shape %r: expected %s" % (S.shape, forms))
        if not np.all(np.isfinite(out)) or np.any(out < 0):
            raise ValueError("the input variances must be finite and >= 0")
        return np.ascontiguousarray(out, dtype=np.float64)

    @staticmethod
    def _diagonal_of(S, d):
        off = S[~np.eye(d, dtype=bool)]
        if np.any(off != 0) or np.any(np.isnan(off)):
            raise ValueError("Sigma_x has a non-zero off-diagonal entry: the variance decomposition needs independent inputs")
        return np.array(np.diagonal(S))

    def _many(self, U, Sigma_x, want_total=True, posterior=False):
        """(mean WITHOUT meant [b], V [b], first [b, d], total [b, d] or None); posterior: V, first and total of the GP itself in posterior
        expectation, the mean part plus the posterior part of ONE gpx_sensitivity_post_many call"""
        if posterior and self.distribution != "gaussian":
            raise NotImplementedError("posterior=True: the closed form serves distribution='gaussian' (the Gaussian law) only, not %r"
                                      % (self.distribution,))
        d = self.gp.d
        UU = _gpx.f64(U)
        if UU.ndim != 2 or UU.shape[1] != d:
            raise ValueError("U must be (b, %d)" % d)
        b = len(UU)
        s = self._variances_of(Sigma_x, d, b)
        if self.distribution == "uniform":
            half = np.sqrt(3.0 * s)                              # a uniform law of variance s has half-width sqrt(3 s)
            return self._box_many(UU - half, UU + half, want_total)[:4]
        mean, V, first = np.empty(b), np.empty(b), np.empty((b, d))
        total = np.empty((b, d)) if want_total else None
        if posterior:
            vp, fp = np.empty(b), np.empty((b, d))
            tp = np.empty((b, d)) if want_total else None
            st = _gpx.lib.gpx_sensitivity_post_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(s), int(s.ndim == 1), b, _gpx.ptr(mean), _gpx.ptr(V),
                                                    _gpx.ptr(first), _gpx.ptr(total) if want_total else None, _gpx.ptr(vp), _gpx.ptr(fp),
                                                    _gpx.ptr(tp) if want_total else None)
            _gpx.check(st, "gpx_sensitivity_post_many")
            return mean, V + vp, first + fp, (total + tp if want_total else None)
        st = _gpx.lib.gpx_sensitivity_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(s), int(s.ndim == 1), b, _gpx.ptr(mean), _gpx.ptr(V),
                                           _gpx.ptr(first), _gpx.ptr(total) if want_total else None)
        _gpx.check(st, "gpx_sensitivity_many")
        return mean, V, first, total

    def _box_many(self, LO, HI, want_total=True, want_quad=False):
        """(mean WITHOUT meant [b], V [b], first [b, d], total [b, d] or None, quad [b] or None) under x_k ~ U(LO_k, HI_k): the bounds as
        given, [b, d] each or one [d] for all rows of the other"""
        d = self.gp.d
        lo, hi = _gpx.f64(LO), _gpx.f64(HI)
        shared = lo.ndim == 1 and hi.ndim == 1
        if not shared:
            lo, hi = (_gpx.f64(a) for a in np.broadcast_arrays(np.atleast_2d(lo), np.atleast_2d(hi)))
        if lo.shape != hi.shape or lo.shape[-1] != d:
            raise ValueError("lo and hi must be (b, %d) or (%d,), got %s and %s" % (d, d, lo.shape, hi.shape))
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
            raise ValueError("the bounds must be finite with lo <= hi")
        b = 1 if shared else len(lo)
        mean, V, first = np.empty(b), np.empty(b), np.empty((b, d))
        total = np.empty((b, d)) if want_total else None
        quad = np.empty(b) if want_quad else None
        st = _gpx.lib.gpx_sensitivity_box_many(self.gp._dev().handle, _gpx.ptr(lo), _gpx.ptr(hi), int(shared), b, _gpx.ptr(mean), _gpx.ptr(V),
                                               _gpx.ptr(first), _gpx.ptr(total) if want_total else None, _gpx.ptr(quad) if want_quad else None)
        _gpx.check(st, "gpx_sensitivity_box_many")
        return mean, V, first, total, quad

    def variances_box_many(self, LO, HI):
        """(means with meant [b], V [b], first [b, d], total [b, d]) under x_k ~ U(LO_ik, HI_ik) for the rows of LO, HI (b, d)"""
        mean, V, first, total, _q = self._box_many(LO, HI)
        return mean + self.gp._get_mean_t(), V, first, total

    def variances_box(self, lo, hi):
        """(mean with meant, V, first [d], total [d]) under x_k ~ U(lo_k, hi_k); lo_k == hi_k pins the coordinate"""
        d = self.gp.d
        mean, V, first, total, _q = self._box_many(_gpx.f64(lo).reshape(1, d), _gpx.f64(hi).reshape(1, d))
        return np.float64(mean[0] + self.gp._get_mean_t()), np.float64(V[0]), first[0], total[0]

    def indices_box_many(self, LO, HI):
        """(first / V, total / V), each [b, d]; zeros where V == 0"""
        _mean, V, first, total, _q = self._box_many(LO, HI)
        return self._ratio(first, V), self._ratio(total, V)

    def indices_box(self, lo, hi):
        """(first / V, total / V), each [d]; zeros where V == 0"""
        d = self.gp.d
        f, t = self.indices_box_many(_gpx.f64(lo).reshape(1, d), _gpx.f64(hi).reshape(1, d))
        return f[0], t[0]

    # ---- second order over a box (gpx_sensitivity_box_second_many); whatever the distribution argument, as the *_box methods above ----
    def _box_bounds(self, LO, HI):
        """(lo, hi) as [b, d] float64 after the checks of _box_many"""
        d = self.gp.d
        lo, hi = (_gpx.f64(a) for a in np.broadcast_arrays(np.atleast_2d(_gpx.f64(LO)), np.atleast_2d(_gpx.f64(HI))))
        if lo.ndim != 2 or lo.shape[-1] != d:
            raise ValueError("lo and hi must be (b, %d) or (%d,), got %s" % (d, d, lo.shape))
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
            raise ValueError("the bounds must be finite with lo <= hi")
        return lo, hi

    def second_order_box_many(self, LO, HI):
        """second [b, d, d] under x_k ~ U(LO_ik, HI_ik): second[i, k, l] = V^closed_{kl} - first_k - first_l of variances_box_many;
        symmetric, zero on the diagonal and in the rows and columns of a pinned coordinate (LO == HI)"""
        lo, hi = self._box_bounds(LO, HI)
        second = np.empty((len(lo), self.gp.d, self.gp.d))
        st = _gpx.lib.gpx_sensitivity_box_second_many(self.gp._dev().handle, _gpx.ptr(lo), _gpx.ptr(hi), 0, len(lo), _gpx.ptr(second))
        _gpx.check(st, "gpx_sensitivity_box_second_many")
        return second

    def second_order_box(self, lo, hi):
        """second [d, d] under x_k ~ U(lo_k, hi_k)"""
        d = self.gp.d
        return self.second_order_box_many(_gpx.f64(lo).reshape(1, d), _gpx.f64(hi).reshape(1, d))[0]

    def second_order_indices_box_many(self, LO, HI):
        """second / V [b, d, d] with V of variances_box_many; zeros where V == 0"""
        lo, hi = self._box_bounds(LO, HI)
        second = self.second_order_box_many(lo, hi)
        V = self._box_many(lo, hi, want_total=False)[1]
        return self._ratio(second.reshape(len(V), -1), V).reshape(second.shape)

    def second_order_indices_box(self, lo, hi):
        """second / V [d, d]; zeros where V == 0"""
        d = self.gp.d
        return self.second_order_indices_box_many(_gpx.f64(lo).reshape(1, d), _gpx.f64(hi).reshape(1, d))[0]

    def variances_many(self, U, Sigma_x, posterior=False):
        """(means with meant [b], V [b], first [b, d], total [b, d]) for the rows of U (b, d); Sigma_x: [d] or a diagonal [d, d] for all of
        them, or [b, d] / diagonal [b, d, d].  posterior=True: the terms of the GP f itself in posterior expectation, E*[Var f], E*[first_k
        of f], E*[total_k of f] (Oakley and O'Hagan 2004): the terms of the mean plus those of the posterior residual, which are what the
        plug-in terms miss where the emulator is uncertain (reads K^-1; Gaussian inputs only)."""
        mean, V, first, total = self._many(U, Sigma_x, posterior=posterior)
        return mean + self.gp._get_mean_t(), V, first, total

    def variances(self, u, Sigma_x, posterior=False):
        """(mean with meant, V, first [d], total [d]) at one input u [d]; Sigma_x: the variances [d] or a diagonal [d, d]"""
        d = self.gp.d
        s = self._variances_of(Sigma_x, d)
        mean, V, first, total = self._many(_gpx.f64(u).reshape(1, d), s, posterior=posterior)
        return np.float64(mean[0] + self.gp._get_mean_t()), np.float64(V[0]), first[0], total[0]

    @staticmethod
    def _ratio(part, V):
        out = np.zeros_like(part)
        live = V != 0
        out[live] = part[live] / V[live][..., None]
        return out

    def indices_many(self, U, Sigma_x, posterior=False):
        """(first / V, total / V), each [b, d]; zeros where V == 0.  posterior=True: the ratios of the posterior EXPECTATIONS of
        variances_many(posterior=True) -- Oakley and O'Hagan's estimate of the indices of f, not the expectation of the ratio."""
        _mean, V, first, total = self._many(U, Sigma_x, posterior=posterior)
        return self._ratio(first, V), self._ratio(total, V)

    def indices(self, u, Sigma_x, posterior=False):
        """(first / V, total / V), each [d]; zeros where V == 0"""
        d = self.gp.d
        f, t = self.indices_many(_gpx.f64(u).reshape(1, d), self._variances_of(Sigma_x, d), posterior)
        return f[0], t[0]

    # ---- second order: with WHICH other input x_k interacts (gpx_sensitivity_second_many) ----
    def second_order_many(self, U, Sigma_x):
        """second [b, d, d]: second[i, k, l] = the variance of the ANOVA term of mu in (x_k, x_l) at input i = V^closed_{kl} - first_k -
        first_l; symmetric, zero on the diagonal and in the rows and columns of a coordinate without variance.  Gaussian inputs only."""
        if self.distribution != "gaussian":
            raise NotImplementedError("second_order*: the closed form serves distribution='gaussian' (the Gaussian law) only, not %r"
                                      % (self.distribution,))
        d = self.gp.d
        UU = _gpx.f64(U)
        if UU.ndim != 2 or UU.shape[1] != d:
            raise ValueError("U must be (b, %d)" % d)
        b = len(UU)
        s = self._variances_of(Sigma_x, d, b)
        second = np.empty((b, d, d))
        st = _gpx.lib.gpx_sensitivity_second_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(s), int(s.ndim == 1), b, _gpx.ptr(second))
        _gpx.check(st, "gpx_sensitivity_second_many")
        return second

    def second_order(self, u, Sigma_x):
        """second [d, d] at one input u [d]; Sigma_x: the variances [d] or a diagonal [d, d]"""
        d = self.gp.d
        return self.second_order_many(_gpx.f64(u).reshape(1, d), self._variances_of(Sigma_x, d))[0]

    def second_order_indices_many(self, U, Sigma_x):
        """second / V [b, d, d] with V of variances_many; zeros where V == 0"""
        second = self.second_order_many(U, Sigma_x)
        _mean, V, _first, _total = self._many(U, Sigma_x, want_total=False)
        return self._ratio(second.reshape(len(V), -1), V).reshape(second.shape)

    def second_order_indices(self, u, Sigma_x):
        """second / V [d, d]; zeros where V == 0"""
        d = self.gp.d
        return self.second_order_indices_many(_gpx.f64(u).reshape(1, d), self._variances_of(Sigma_x, d))[0]

    # ---- every interaction order: the full ANOVA decomposition and the Shapley effects (gpx_sensitivity_anova_many) ----
    def _anova_terms(self, U, Sigma_x):
        """(terms [b, 2^na_max] by mask, active: b lists of the uncertain coordinates in increasing order): terms[i, mask] = D_S of input i
        with bit q of mask the coordinate active[i][q]; the raw call's bits"""
        if self.distribution != "gaussian":
            raise NotImplementedError("anova*, shapley*, closed_variance: the closed form serves distribution='gaussian' (the Gaussian law) "
                                      "only, not %r" % (self.distribution,))
        d = self.gp.d
        UU = _gpx.f64(U)
        if UU.ndim != 2 or UU.shape[1] != d:
            raise ValueError("U must be (b, %d)" % d)
        b = len(UU)
        s = self._variances_of(Sigma_x, d, b)
        rows = s[None, :] if s.ndim == 1 else s
        active = [[int(k) for k in np.flatnonzero(rows[0 if s.ndim == 1 else i] > 0)] for i in range(b)]
        na = max([len(a) for a in active] + [0])
        if na > _gpx.GPX_ANOVA_MAX_ACTIVE:
            raise ValueError("%d uncertain coordinates: the full decomposition serves at most GPX_ANOVA_MAX_ACTIVE = %d per input"
                             % (na, _gpx.GPX_ANOVA_MAX_ACTIVE))
        terms = np.empty((b, 1 << na))
        st = _gpx.lib.gpx_sensitivity_anova_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(s), int(s.ndim == 1), b, _gpx.ptr(terms), 1 << na)
        _gpx.check(st, "gpx_sensitivity_anova_many")
        return terms, active

    def anova_many(self, U, Sigma_x):
        """b dicts {tuple of coordinate indices: D_S} over the non-empty subsets S of each input's uncertain coordinates: D_S is the variance
        of the ANOVA component of mu in x_S.  D_(k,) = first_k, D_(k, l) = second_kl, the values sum to V, those with k in S to total_k.  At
        most GPX_ANOVA_MAX_ACTIVE uncertain coordinates per input.  Gaussian inputs only."""
        terms, active = self._anova_terms(U, Sigma_x)
        return [{tuple(a[q] for q in range(len(a)) if mask >> q & 1): terms[i, mask] for mask in range(1, 1 << len(a))}
                for i, a in enumerate(active)]

    def anova(self, u, Sigma_x):
        """{tuple of coordinate indices: D_S} at one input u [d]; Sigma_x: the variances [d] or a diagonal [d, d]"""
        d = self.gp.d
        return self.anova_many(_gpx.f64(u).reshape(1, d), self._variances_of(Sigma_x, d))[0]

    def shapley_many(self, U, Sigma_x):
        """Sh [b, d]: the Shapley effects Sh_k = sum_{S contains k} D_S / |S| (Owen 2014), one attribution per input with sum_k Sh_k = V;
        0.0 for a coordinate without variance.  The masks are summed in ascending order."""
        terms, active = self._anova_terms(U, Sigma_x)
        out = np.zeros((len(active), self.gp.d))
        for i, a in enumerate(active):
            for mask in range(1, 1 << len(a)):
                share = terms[i, mask] / bin(mask).count("1")
                for q, k in enumerate(a):
                    if mask >> q & 1:
                        out[i, k] += share
        return out

    def shapley(self, u, Sigma_x):
        """Sh [d] at one input u [d]"""
        d = self.gp.d
        return self.shapley_many(_gpx.f64(u).reshape(1, d), self._variances_of(Sigma_x, d))[0]

    def closed_variance(self, u, Sigma_x, subset):
        """V^closed_S = Var(E[mu | x_S]) = sum of D_T over the non-empty T inside `subset` (coordinate indices; one without variance adds
        nothing), the masks in ascending order"""
        d = self.gp.d
        subset = set(int(k) for k in subset)
        if not all(0 <= k < d for k in subset):
            raise ValueError("subset must hold coordinate indices in [0, %d)" % d)
        terms, active = self._anova_terms(_gpx.f64(u).reshape(1, d), self._variances_of(Sigma_x, d))
        inside = sum(1 << q for q, k in enumerate(active[0]) if k in subset)
        return np.float64(sum(terms[0, mask] for mask in range(1, 1 << len(active[0])) if mask & ~inside == 0))

    # ---- which DIRECTIONS matter: the second moment of the gradient, the active-subspace matrix (gpx_sensitivity_gradient_many) ----
    def gradient_moments_many(self, U, Sigma_x, posterior=False):
        """(gmean [b, d], C [b, d, d]): gmean = E[grad mu(x)], C = E[grad mu grad mu^T] of the predictor mean, or with posterior=True the
        posterior expectation E[grad f grad f^T] = that plus E[Cov grad f] (reads K^-1; Wycoff, Binois and Wild 2021).  C is symmetric; the
        covariance of grad mu is C - gmean gmean^T.  Gaussian inputs only."""
        if self.distribution != "gaussian":
            raise NotImplementedError("gradient_moments*, dgsm*, active_subspace: the closed form serves distribution='gaussian' (the Gaussian "
                                      "law) only, not %r" % (self.distribution,))
        d = self.gp.d
        UU = _gpx.f64(U)
        if UU.ndim != 2 or UU.shape[1] != d:
            raise ValueError("U must be (b, %d)" % d)
        b = len(UU)
        s = self._variances_of(Sigma_x, d, b)
        gmean, cmean = np.empty((b, d)), np.empty((b, d, d))
        cpost = np.empty((b, d, d)) if posterior else None
        st = _gpx.lib.gpx_sensitivity_gradient_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(s), int(s.ndim == 1), b, _gpx.ptr(gmean),
                                                    _gpx.ptr(cmean), _gpx.ptr(cpost) if posterior else None)
        _gpx.check(st, "gpx_sensitivity_gradient_many")
        return gmean, (cmean + cpost if posterior else cmean)

    def gradient_moments(self, u, Sigma_x, posterior=False):
        """(gmean [d], C [d, d]) at one input u [d]; Sigma_x: the variances [d] or a diagonal [d, d]"""
        d = self.gp.d
        g, C = self.gradient_moments_many(_gpx.f64(u).reshape(1, d), self._variances_of(Sigma_x, d), posterior)
        return g[0], C[0]

    def dgsm_many(self, U, Sigma_x, posterior=False):
        """nu [b, d] = the diagonal of C: the derivative-based global sensitivity measures; total_k <= s_k nu_k (Gaussian Poincare)"""
        return np.array(np.diagonal(self.gradient_moments_many(U, Sigma_x, posterior)[1], axis1=1, axis2=2))

    def dgsm(self, u, Sigma_x, posterior=False):
        """nu [d] at one input u [d]"""
        return np.array(np.diagonal(self.gradient_moments(u, Sigma_x, posterior)[1]))

    def active_subspace(self, u, Sigma_x, posterior=True):
        """(eigenvalues [d] in descending order, eigenvectors [d, d] as columns) of C at one input u [d]: the leading columns span the
        directions along which the GP varies most under the input law"""
        lam, vec = np.linalg.eigh(self.gradient_moments(u, Sigma_x, posterior)[1])
        return lam[::-1].copy(), vec[:, ::-1].copy()
