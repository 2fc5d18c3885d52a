"""Exact translations of the seeded cases, and the float64 restatement of what the dense Gaussian path computes from prescaled inputs
away from the origin (tests/test_shifted_inputs.py, tests/test_shift_model.py).  Host only.

Every seeded input of the suite lives on the 2^-20 grid in [0, 10]^d (far inputs: below 2^14), so x + 2^10 and x + 2^17 are exact in
float64 and so is every difference of two translated coordinates.  shifted() translates a case and asserts that.  The long-double models
(_dense_ld, _matern_ld, _periodic_ld, _rows_ld, ..) take direct differences of the inputs: on a translated case they return the values of
the case as seeded, bit for bit, which therefore are the truth for the translated case too.

The dense Gaussian path does not see differences first: the fit scales every coordinate by fl(sqrt(w_k)) (launch_scale_rows, fit.hip) and
gram_kernel / nll_grad_kernel / the predictor's query rows difference the scaled coordinates.  restated_grad() says that in NumPy float64
(NOT the code under test): a = fl(fl(sqrt(w)) (x + s)), e_k = a_ik - a_jk, q = sum_k e_k^2, Kf = v exp(-q / 2), the sums of
_dense_ld.grad_sums with e_k^2 for w_k (x_ik - x_jk)^2.  What this costs is bounded by _dense_ld.prescale_loss, which _dense_ld.grad_loss sums
into an absolute allowance per gradient entry: nothing here is fitted to a device result.

Two yardsticks hold gpx_nll_grad, and the seeded defects are planted in the first one's reference, on the d + 2 values the device returns:
  against the restatement   |g - restated_grad| on the PLAIN scales of _dense_ld.grad under the plain rule, no allowance: the device and
                            the restatement do the same arithmetic on the same scaled coordinates, K^-1 and alpha and differ by the order
                            of their sums and the last bits of exp, which is what FLOOR is for.  This is the comparison with power: an
                            arithmetic that loses more than differencing the scaled coordinates does shows here undiluted.
  against long double       |g - model| less grad_loss on the same scales: the loss that is left is linear in the offset and bounded.

`defect=` plants one of DEFECTS in the restatement (tests/test_shift_model.py):
  "expanded"  q and every e_k^2 from expanded squares, a_k^2 + b_k^2 - 2 a_k b_k: the rounding error is u |a|^2, quadratic in the offset
  "sqrt32"    sqrt(w_k) rounded to float32 before the scaling (a relative 6e-8 in w: seen at every shift)
  "scaled32"  the scaled coordinate rounded to float32: an absolute 6e-8 sqrt(w) |x| in every coordinate, growing with the offset
  "eq_scaled" rows_c(): the equality that decides the +vt of a C row taken on the scaled coordinates instead of the raw ones"""
import numpy as np

import _dense_ld as dl
from _gauss_ld import OFFSET  # noqa: F401  (2^10: imported, not copied)
from _spgp_ld import SHIFT    # noqa: F401  (2^17)

SHIFTS = (OFFSET, SHIFT)
COORDINATES = ("x", "xi", "xj", "xs", "U", "u")          # the entries of a case that are points of the input space
DEFECTS = ("expanded", "sqrt32", "scaled32", "eq_scaled")


def translate(a, s):
    """a + s, asserted exact: (a + s) - s == a elementwise (test_spgp_bounds.Case.shifted's check)"""
    a = np.asarray(a, dtype=np.float64)
    b = a + s
    np.testing.assert_array_equal(b - s, a)
    return b


def shifted(case, s):
    """the case {name: array, or {name: array} for a family of inputs} with s added to every coordinate of its COORDINATES and nothing else"""
    out = {}
    for k, a in case.items():
        if k not in COORDINATES:
            out[k] = a
        elif isinstance(a, dict):
            out[k] = {n: translate(b, s) for n, b in a.items()}
        else:
            out[k] = translate(a, s)
    return out


def name_of(s):
    return "0" if s == 0 else "2^%d" % int(np.log2(s))


def scaled(x, theta, defect=None):
    """fl(fl(sqrt(w_k)) x_k): the coordinates the dense Gaussian path keeps (h->xs_w)"""
    x = np.asarray(x, dtype=np.float64)
    _v, _vt, w = dl.params(theta, x.shape[1], np.float64)
    sw = np.sqrt(w)
    if defect == "sqrt32":
        sw = sw.astype(np.float32).astype(np.float64)
    a = x * sw
    return a.astype(np.float32).astype(np.float64) if defect == "scaled32" else a


def restated_grad(xs, theta, Kinv, alpha, defect=None):
    """gpx_nll_grad's d + 2 values in NumPy float64 from the scaled coordinates of xs (the inputs as the device sees them, translated)"""
    xs = np.asarray(xs, dtype=np.float64)
    N, d = xs.shape
    v, _vt, _w = dl.params(theta, d, np.float64)
    a = scaled(xs, theta, defect)
    Ki, al = np.asarray(Kinv, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    S = np.zeros(d + 2)
    for i0 in range(0, N, dl.ROWS):
        i1 = min(N, i0 + dl.ROWS)
        D = np.empty((d, i1 - i0, N))
        for k in range(d):
            ai, aj = a[i0:i1, k][:, None], a[:, k][None, :]
            if defect == "expanded":
                D[k] = np.maximum(ai * ai + aj * aj - 2.0 * ai * aj, 0.0)
            else:
                D[k] = (ai - aj) ** 2
        MK = (Ki[i0:i1] - np.outer(al[i0:i1], al)) * (v * np.exp(-0.5 * D.sum(0)))
        S[0] += MK.sum()
        for k in range(d):
            S[1 + k] += (MK * D[k]).sum()
    S[d + 1] = np.diagonal(Ki).sum() - al.dot(al)
    return dl.grad_from_sums(S, np.zeros_like(S), theta)[0]


def pair_distances(x, theta, s, defect=None):
    """the restatement's Kf_ij, pair by pair, on inputs x + s against long double on x, in the rule's units with the per-pair allowance that
    _dense_ld.grad_loss sums up for S_0: the worst max(|dKf| - Kf rq, 0) / Kf"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, _vt, w = dl.params(theta, d, dl.LD)
    xl = xr.astype(dl.LD)
    D = np.array([w[k] * (xl[:, k][:, None] - xl[:, k][None, :]) ** 2 for k in range(d)])
    Kf = v * np.exp(-D.sum(0) / 2)
    rq = dl.prescale_loss(xr, theta, s, D)[0] if s != 0.0 else 0
    a = scaled(translate(xr, s), theta, defect)
    acc = np.zeros((N, N))
    for k in range(d):
        ai, aj = a[:, k][:, None], a[:, k][None, :]
        acc += np.maximum(ai * ai + aj * aj - 2.0 * ai * aj, 0.0) if defect == "expanded" else (ai - aj) ** 2
    got = float(v) * np.exp(-0.5 * acc)
    return float((np.maximum(np.abs(got.astype(dl.LD) - Kf) - Kf * rq, 0) / Kf).max())


def rows_c(xs, theta, us, defect=None):
    """C_i = v exp(-q_i / 2) + vt iff x_i == u elementwise in float64 from the RAW differences of the translated inputs (gpx_cjh, the C row
    of gpx_rows_build); "eq_scaled" decides the equality on scaled(x) and scaled(u)"""
    xs, us = np.asarray(xs, dtype=np.float64), np.asarray(us, dtype=np.float64)
    v, vt, w = dl.params(theta, xs.shape[1], np.float64)
    delta = xs - us
    c = v * np.exp(-0.5 * (w * delta * delta).sum(1))
    if defect == "eq_scaled":
        same = (scaled(xs, theta) == scaled(us[None, :], theta)).all(1)
    else:
        same = (xs == us).all(1)
    return c + vt * same
