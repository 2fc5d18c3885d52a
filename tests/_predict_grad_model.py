"""A long-double model of the predictor's input gradients (scikit-gpuppy_amd/csrc/predict_grad.hip; gpx_predict_mean_grad, gpx_predict_grad),
for the Gaussian kernel and Matern 3/2 and 5/2.  Host only.

With delta = x_i - u (DIRECT differences of the raw inputs), q_i = sum_k w_k delta_k^2 and the radial factors of the kernel
  nu2 = 0 (Gaussian): c = g = v exp(-q / 2)
  nu2 = 5: s = sqrt(5 q), c = v (1 + s + s^2 / 3) exp(-s), g = (5/3) v (1 + s) exp(-s)        nu2 = 3: s = sqrt(3 q), c = v (1 + s) exp(-s), g = 3 v exp(-s)
the noise-free kernel has d c_i / d u_k = +w_k delta_k g_i, and
  mu       = sum_i C_i alpha_i                         grad mu_k      = sum_i w_k delta_k g_i alpha_i                       (from a given alpha)
  sigma^2  = (v + vt) - sum_ij C_i Kinv_ij C_j         grad sigma^2_k = -2 sum_ij C_i Kinv_ij w_k delta_jk g_j              (from a given K^-1)
C_i = c_i + vt iff x_i == u elementwise when `quirk` holds -- the rows of a Matern handle (gpx_matern_predict), not those of a Gaussian one
(gpx_predict: GaussianCovariance.cov_matrix_ij has no such term); `quirk=None` takes the kind's own.  No derivative carries vt.

Every function takes `dt` (np.longdouble: the model; np.float64: the plain evaluation rho_ref is measured on), the parameters are exp(theta)
in float64 -- what the device holds -- then widened, and every sum comes back as (values, absolute scales), the scale being the sum of the
absolute values of its terms (a combined value: the same combination of its parts' scales).  The rule is tests/_dense_ld.py's, imported.

`defect=` plants one of DEFECTS in an evaluation (meant for dt = np.float64): "sign" the gradients negated (the reference's get_Jacobian
convention taken for the derivative), "half" the factor 2 of grad sigma^2 missing, "now" w_k missing, "vt" the noise term treated as part of the
differentiable kernel (g + vt in every derivative)."""
import numpy as np

from _dense_ld import FLOOR, LD, MARGIN, assert_within, distances, rho_of  # noqa: F401  (the project's one rule: imported, not copied)
from _spgp_ld import _grid, bound  # noqa: F401

KINDS = (0, 3, 5)                       # nu2: 0 = the Gaussian kernel
DEFECTS = ("sign", "half", "now", "vt")


def params(theta, d, dt=LD):
    """(v, vt, w): exp(theta) in float64, then widened"""
    th = np.asarray(theta, dtype=np.float64)
    with np.errstate(divide="ignore"):
        e = np.exp(th)
    return dt(e[0]), dt(e[1]), e[2:2 + d].astype(dt)


def radial(q, v, nu2, dt=LD):
    """(c, g) at q"""
    if nu2 == 0:
        c = v * np.exp(-q / 2)
        return c, c
    s = np.sqrt(dt(nu2) * q)
    e = v * np.exp(-s)
    if nu2 == 5:
        return e * (1 + s + s * s / 3), dt(5) / 3 * e * (1 + s)
    return e * (1 + s), 3 * e


def rows(x, theta, U, nu2, quirk=None, dt=LD, defect=None):
    """(C [M, N], dC [M, d, N] = d c_i / d u_k, v + vt) for the queries U [M, d]"""
    xr, ur = np.asarray(x, dtype=np.float64), np.atleast_2d(np.asarray(U, dtype=np.float64))
    d = xr.shape[1]
    v, vt, w = params(theta, d, dt)
    quirk = (nu2 != 0) if quirk is None else quirk
    delta = xr.astype(dt)[None, :, :] - ur.astype(dt)[:, None, :]                 # [M, N, d]
    q = (w * delta * delta).sum(2)
    c, g = radial(q, v, nu2, dt)
    same = (xr[None, :, :] == ur[:, None, :]).all(2)
    C = c + (vt * same.astype(dt) if quirk else 0)
    if defect == "vt":
        g = g + vt
    wk = np.ones(d, dt) if defect == "now" else w
    dC = np.transpose(wk * delta, (0, 2, 1)) * g[:, None, :]
    if defect == "sign":
        dC = -dC
    return C, dC, v + vt


def mean_grad(x, theta, alpha, U, nu2, quirk=None, dt=LD, defect=None):
    """{"mean": ([M], scales), "dmean": ([M, d], scales)} from a given alpha (mean WITHOUT meant)"""
    C, dC, _k = rows(x, theta, U, nu2, quirk, dt, defect)
    al = np.asarray(alpha).astype(dt)
    return {"mean": (C.dot(al), np.abs(C).dot(np.abs(al))), "dmean": (dC.dot(al), np.abs(dC).dot(np.abs(al)))}


def var_grad(x, theta, Kinv, U, nu2, quirk=None, dt=LD, defect=None):
    """{"var": ([M], scales), "dvar": ([M, d], scales)} from a given K^-1"""
    C, dC, kuu = rows(x, theta, U, nu2, quirk, dt, defect)
    Ki = np.asarray(Kinv).astype(dt)
    KC, aKC = C.dot(Ki), np.abs(C).dot(np.abs(Ki))                                # [M, N] (Kinv symmetric to rounding: row form)
    two = dt(1) if defect == "half" else dt(2)
    return {"var": (kuu - (KC * C).sum(1), np.abs(kuu) + (aKC * np.abs(C)).sum(1)),
            "dvar": (-two * np.einsum("mj,mkj->mk", KC, dC), 2 * np.einsum("mj,mkj->mk", aKC, np.abs(dC)))}


def grad_scale(x, theta, U):
    """g_k = max(1, w_k max_i |x_ik - u_k|) [M, d]: the J rows are the C row scaled entrywise by factors of at most g_k"""
    xr, ur = np.asarray(x, dtype=np.float64), np.atleast_2d(np.asarray(U, dtype=np.float64))
    _v, _vt, w = params(theta, xr.shape[1], np.float64)
    return np.maximum(1.0, w * np.abs(xr[None, :, :] - ur[:, None, :]).max(1))
