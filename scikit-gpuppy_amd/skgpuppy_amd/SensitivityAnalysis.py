"""Which input's uncertainty produces the output variance: the variance decomposition of the GP predictor mean under independent
Gaussian inputs x_k ~ N(u_k, s_k), in closed form for the ARD squared-exponential kernel (gpx_sensitivity_many; include/gpx.h carries
the formulas).  No reference counterpart: the reference's nearest code is the nquad / Hermite-Gauss cross-check of
skgpuppy/UncertaintyPropagation.py:135-210.

  V        = Var(mu(x))                       the variance of the predictor mean (the beta beta^T part of Girard's exact variance)
  first_k  = Var_{x_k}(E[mu | x_k])           what x_k's uncertainty produces on its own
  total_k  = E[Var_{x_k}(mu | x_~k)]          what is left when everything but x_k is known: first_k plus every interaction with x_k
  sum_k first_k <= V <= sum_k total_k;  the Sobol indices are first / V and total / V.

The call reads (x, beta, v, w) alone -- no K^-1, no factor, no solve: a GaussianProcess on the fused GaussianCovariance route costs N^2 d
per input, a PseudoInputGP (GaussianProcess.pseudo_gp() of an SPGP model) m^2 d.  Setting all but one Sigma_kk to zero in propagate_GA is
NOT first_k: that pins the other inputs at u instead of averaging over them."""
import numpy as np

from . import _gpx
from .GaussianProcess import GaussianProcess, PseudoInputGP


class SensitivityAnalysis(object):
    """SensitivityAnalysis(gp): gp a GaussianProcess with a fused GaussianCovariance, or a PseudoInputGP."""

    def __init__(self, gp):
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

    def _many(self, U, Sigma_x, want_total=True):
        """(mean WITHOUT meant [b], V [b], first [b, d], total [b, d] or None)"""
        d = self.gp.d
        UU = _gpx.f64(U)
        if UU.ndim != 2 or UU.shape[1] != d:
            raise ValueError("U must be (b, %d)" % d)
        b = len(UU)
        s = self._variances_of(Sigma_x, d, b)
        mean, V, first = np.empty(b), np.empty(b), np.empty((b, d))
        total = np.empty((b, d)) if want_total else None
        st = _gpx.lib.gpx_sensitivity_many(self.gp._dev().handle, _gpx.ptr(UU), _gpx.ptr(s), int(s.ndim == 1), b, _gpx.ptr(mean), _gpx.ptr(V),
                                           _gpx.ptr(first), _gpx.ptr(total) if want_total else None)
        _gpx.check(st, "gpx_sensitivity_many")
        return mean, V, first, total

    def variances_many(self, U, Sigma_x):
        """(means with meant [b], V [b], first [b, d], total [b, d]) for the rows of U (b, d); Sigma_x: [d] or a diagonal [d, d] for all of
        them, or [b, d] / diagonal [b, d, d]"""
        mean, V, first, total = self._many(U, Sigma_x)
        return mean + self.gp._get_mean_t(), V, first, total

    def variances(self, u, Sigma_x):
        """(mean with meant, V, first [d], total [d]) at one input u [d]; Sigma_x: the variances [d] or a diagonal [d, d]"""
        d = self.gp.d
        s = self._variances_of(Sigma_x, d)
        mean, V, first, total = self._many(_gpx.f64(u).reshape(1, d), s)
        return np.float64(mean[0] + self.gp._get_mean_t()), np.float64(V[0]), first[0], total[0]

    @staticmethod
    def _ratio(part, V):
        out = np.zeros_like(part)
        live = V != 0
        out[live] = part[live] / V[live][..., None]
        return out

    def indices_many(self, U, Sigma_x):
        """(first / V, total / V), each [b, d]; zeros where V == 0"""
        _mean, V, first, total = self._many(U, Sigma_x)
        return self._ratio(first, V), self._ratio(total, V)

    def indices(self, u, Sigma_x):
        """(first / V, total / V), each [d]; zeros where V == 0"""
        d = self.gp.d
        f, t = self.indices_many(_gpx.f64(u).reshape(1, d), self._variances_of(Sigma_x, d))
        return f[0], t[0]
