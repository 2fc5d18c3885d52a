"""CPU models of the numerical propagation (csrc/quadrature.hip, skgpuppy_amd.UncertaintyPropagationNumericalHG / MC).

  * the node builders (the rules and square roots the Python classes use, restated independently) and the device's node arithmetic -- ONE
    fma chain over e in increasing order that starts from U[i][k] -- bit for bit (exact rational arithmetic, rounded once per fma);
  * a long-double model of the five moments and of the density of a mixture  p(y) = sum_s wq_s N(y; mu_s, sigma^2_s);
  * a float64 restatement of the device's summation order (1024-node segments, four nodes a thread, butterfly over 64 lanes, the fixed
    sums of the wave slots and of the segments); it rounds each product before the add where the device fuses them, so it is a model of
    the ORDER, one rounding per term looser than the device;
  * the error units of each quantity, and the first-order bound of the moments and the density under an error of the predictor.

Units (u = 2^-53).  Every quantity is a sum of terms; its unit is u * sum |term| (a density term exp(-x) / ...: u |term| (1 + x), plus the
granularity of the normal range).  The central moments are taken about the float64 mean m,
whose own rounding error is a few units of m, u * sum |wq mu|.  c2 = sum wq (mu - m)^2 is stationary in m (sum wq (mu - m) = 0: the error is
second order), but d m3 / d m = -3 var and d m4 / d m = -4 m3, so the units of m3 and m4 carry 3 var and 4 |m3| units of m on top of their
own terms.  (mu_s - m is exact in float64 whenever |mu_s - m| <= |m| / 2: a large common offset costs the central moments nothing else.)
"""
import math
from fractions import Fraction
from itertools import product

import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
SEG = 1024
DENORMAL_FLOOR = LD(2.0 ** -1022)      # a density below the normal range is held to that range's granularity, not to its own size


# ---- rules and roots ---------------------------------------------------------------------------------------------------------------
def hg_rule(order, d):
    """(z [order^d, d], wq) in itertools.product order, wq = prod w / pi^(d/2)  (Utilities.py:159-167), sqrt(pi) taken as the sum of the
    one-dimensional weights (its value in exact arithmetic)"""
    x, w = np.polynomial.hermite.hermgauss(order)
    w = w / math.fsum(w)
    z = np.array(list(product(x, repeat=d)), dtype=float).reshape(-1, d)
    ws = np.array(list(product(w, repeat=d)), dtype=float).reshape(-1, d)
    return z, ws.prod(axis=1)


def hg_root(Sigma, full_sigma=False):
    Sigma = np.asarray(Sigma, dtype=float)
    if full_sigma:
        return np.sqrt(2.0) * np.linalg.cholesky(Sigma)
    return np.diag(np.sqrt(np.diag(Sigma)) * np.sqrt(2.0))      # the reference reads the diagonal alone (Utilities.py:157)


def mc_rule(n, d, seed):
    return np.random.RandomState(seed).standard_normal((n, d)), np.full(n, 1.0 / n)


def mc_root(Sigma):
    return np.linalg.cholesky(np.asarray(Sigma, dtype=float))


def _fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))      # exact, then ONE rounding to nearest even


def nodes_fma(U, A, z):
    """X [B, S, d] as the device builds it: acc = U[i][k]; for e = 0 .. d-1: acc = fma(A_i[k][e], z[s][e], acc).  A [d, d] or [B, d, d]."""
    U, A, z = np.asarray(U, float), np.asarray(A, float), np.asarray(z, float)
    B, d = U.shape
    X = np.empty((B, len(z), d))
    for i in range(B):
        Ai = A if A.ndim == 2 else A[i]
        for s in range(len(z)):
            for k in range(d):
                acc = U[i, k]
                for e in range(d):
                    acc = _fma(Ai[k, e], z[s, e], acc)
                X[i, s, k] = acc
    return X


def nodes_plain(U, A, z):
    """the same nodes in NumPy's arithmetic, [B, S, d] (for models that do not need the device's bits)"""
    U, A, z = np.asarray(U, float), np.asarray(A, float), np.asarray(z, float)
    if A.ndim == 2:
        return U[:, None, :] + z.dot(A.T)[None]
    return U[:, None, :] + np.einsum("ike,se->isk", A, z)


# ---- the mixture in long double ----------------------------------------------------------------------------------------------------
def _terms(mu, var, wq, m):
    dm = mu - m
    d2 = dm * dm
    return wq * d2, wq * (dm * d2 + 3 * dm * var), wq * (d2 * d2 + 6 * d2 * var + 3 * var * var)


def mixture_ld(mu, var, wq, y=None, shift=0.0):
    """one input: (mom [5] = m | var | Ev | m3 | m4, units [5], dens [ny] or None, dens units) in long double"""
    mu, var, wq = np.asarray(mu, LD), np.asarray(var, LD), np.asarray(wq, LD)
    m, am = (wq * mu).sum(), np.abs(wq * mu).sum()
    ev = (wq * var).sum()
    t2, t3, t4 = _terms(mu, var, wq, m)
    c2, m3, m4 = t2.sum(), t3.sum(), t4.sum()
    mom = np.array([m, ev + c2, ev, m3, m4], dtype=LD)
    units = LD(U64) * np.array([am, np.abs(wq * var).sum() + c2, np.abs(wq * var).sum(),
                                np.abs(t3).sum() + 3 * abs(ev + c2) * am, np.abs(t4).sum() + 4 * abs(m3) * am], dtype=LD)
    if y is None:
        return mom, units, None, None
    ys = np.asarray(y, LD) - LD(shift)
    with np.errstate(all="ignore"):
        x = (ys[:, None] - mu[None, :]) ** 2 / (2 * var[None, :])
        terms = wq[None, :] * np.exp(-x) / np.sqrt(2 * LD(np.pi) * var[None, :])
        dens = terms.sum(axis=1)
        # exp(-x) turns a relative error e of its argument into x e: a term's unit carries the factor 1 + x (as the Gram units of _periodic_ld)
        du = LD(U64) * np.nansum(np.abs(terms) * (1 + np.where(np.isfinite(x), x, 0)), axis=1) + DENORMAL_FLOOR
    return mom, units, dens, du


# ---- the device's summation order in float64 ---------------------------------------------------------------------------------------
def _butterfly(v):
    """xor-butterfly over the last axis (64 lanes): what lane 0 holds"""
    n = v.shape[-1]
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def _block_sum(v):
    """v [..., 256] thread values -> (p0 + p1) + (p2 + p3) of the four wave sums"""
    p = _butterfly(v.reshape(v.shape[:-1] + (4, 64)))
    return (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])


def _device_sum(w, term):
    """sum_s w_s term_s in the order of mixture_mean_kernel / mixture_central_kernel + mixture_finish_kernel"""
    S = len(w)
    nseg = (S + SEG - 1) // SEG
    t = np.zeros(nseg * SEG)
    t[:S] = w * term
    t = t.reshape(nseg, 4, 256)
    acc = np.zeros((nseg, 256))
    for j in range(4):
        acc = acc + t[:, j, :]
    part = _block_sum(acc)                                     # [nseg]
    rows = (nseg + 255) // 256
    p = np.zeros(rows * 256)
    p[:nseg] = part
    p = p.reshape(rows, 256)
    acc = np.zeros(256)
    for r in range(rows):
        acc = acc + p[r]
    return _block_sum(acc)


def mixture_f64(mu, var, wq, y=None, shift=0.0):
    """one input in float64, the device's order: (mom [5], dens [ny] or None)"""
    mu, var, wq = np.asarray(mu, float), np.asarray(var, float), np.asarray(wq, float)
    m = _device_sum(wq, mu)
    ev = _device_sum(wq, var)
    dm = mu - m
    d2 = dm * dm
    c2 = _device_sum(wq, d2)
    m3 = _device_sum(wq, dm * (3.0 * var + d2))
    m4 = _device_sum(wq, d2 * d2 + (6.0 * d2 * var + 3.0 * (var * var)))
    mom = np.array([m, ev + c2, ev, m3, m4])
    if y is None:
        return mom, None
    S = len(wq)
    nseg = (S + SEG - 1) // SEG
    nm, nh, nc = np.zeros(nseg * SEG), np.zeros(nseg * SEG), np.zeros(nseg * SEG)
    with np.errstate(all="ignore"):
        nm[:S], nh[:S], nc[:S] = mu, 0.5 / var, wq / np.sqrt(6.283185307179586477 * var)
        ys = np.asarray(y, float) - shift
        dy = ys[:, None] - nm[None, :]
        terms = nc[None, :] * np.exp(np.maximum(-(dy * dy) * nh[None, :], -750.0))      # [ny, nseg * 1024]; node l of a segment: thread l % 16
        terms = terms.reshape(len(ys), nseg, SEG // 16, 16)
        acc = np.zeros((len(ys), nseg, 16))
        for r in range(SEG // 16):
            acc = acc + terms[:, :, r, :]
        col = acc[:, :, 0]
        for q in range(1, 16):
            col = col + acc[:, :, q]
        dens = col[:, 0]
        for g in range(1, nseg):
            dens = dens + col[:, g]
    return mom, dens


def rho(cases):
    """worst distance of the float64 restatement from the long-double model over cases [(mu, var, wq, y or None, shift)], in units,
    per kind: (moments, density).  Non-finite model values (a sigma^2 = 0 node's densities) are left out of the density figure."""
    rm, rd = 0.0, 0.0
    for mu, var, wq, y, shift in cases:
        mom, units, dens, du = mixture_ld(mu, var, wq, y, shift)
        fm, fd = mixture_f64(mu, var, wq, y, shift)
        rm = max(rm, float(np.max(np.abs(LD(1) * fm - mom) / units)))
        if y is not None:
            ok = np.isfinite(dens) & (du > 0)
            if ok.any():
                rd = max(rd, float(np.max(np.abs(LD(1) * fd[ok] - dens[ok]) / du[ok])))
    return rm, rd


def reduce_bound_units(r):
    """the device bound of gpx_mixture_reduce in units: 8 max(rho, 4)  (tests/test_gauss_gram_model.py's rule, measured on the model)"""
    return 8.0 * max(r, 4.0)


# ---- first-order bounds under an error of the predictor ----------------------------------------------------------------------------
def first_order_bounds(mu, var, wq, y, shift, emu, evar):
    """Every predicted row is within emu (mean) and evar (variance) of the oracle's.  With wq > 0, sum wq = 1:
         |dm| <= emu,   |dvar| <= evar + 2 sqrt(c2) * 2 emu  (the cross term of (mu - m)^2, Cauchy-Schwarz, mu and m each off by emu)
       and for m3, m4 and the density TWICE the first-order bound  sum wq (|d/dmu| emu + |d/dsigma^2| evar) + 64 u |value|,
       (twice: the central-moment terms move with m as well as with mu_s, each by at most emu).  Returns (bm, bvar, bm3, bm4, bdens [ny])."""
    mu, var, wq = np.asarray(mu, LD), np.asarray(var, LD), np.asarray(wq, LD)
    emu, evar = LD(emu), LD(evar)
    mom, _u, dens, _du = mixture_ld(mu, var, wq, y, shift)
    m = mom[0]
    dm = mu - m
    c2 = (wq * dm * dm).sum()
    bm = emu
    bvar = evar + 4 * emu * np.sqrt(c2) + LD(1e-16)
    d3_mu = np.abs(3 * dm * dm + 3 * var) * emu
    d3_v = np.abs(3 * dm) * evar
    bm3 = 2 * (wq * (d3_mu + d3_v)).sum() + 64 * LD(U64) * abs(mom[3])
    d4_mu = np.abs(4 * dm ** 3 + 12 * dm * var) * emu
    d4_v = np.abs(6 * dm * dm + 6 * var) * evar
    bm4 = 2 * (wq * (d4_mu + d4_v)).sum() + 64 * LD(U64) * abs(mom[4])
    bd = None
    if y is not None:
        ys = np.asarray(y, LD) - LD(shift)
        r = ys[:, None] - mu[None, :]
        g = np.exp(-r * r / (2 * var[None, :])) / np.sqrt(2 * LD(np.pi) * var[None, :])
        dg_mu = np.abs(g * r / var[None, :]) * emu
        dg_v = np.abs(g * (r * r / (2 * var[None, :] ** 2) - 1 / (2 * var[None, :]))) * evar
        bd = 2 * (wq[None, :] * (dg_mu + dg_v)).sum(axis=1) + 64 * LD(U64) * np.abs(dens)
    return bm, bvar, bm3, bm4, bd


# ---- shared cases ------------------------------------------------------------------------------------------------------------------

REDUCE_S = [1, 2, 63, 64, 65, 255, 256, 257, 4097, 65536]
REDUCE_B = [1, 3, 130]
REDUCE_NY = [0, 1, 9, 65]


def reduce_shapes():
    """(S, b, ny, y_shared) of the gpx_mixture_reduce cases: every S with every b and ny = 0, and with every ny > 0 whose b S ny stays below
    3e6 terms (the long-double model evaluates every one of them); the y form alternates."""
    out = []
    for S in REDUCE_S:
        for b in REDUCE_B:
            for k, ny in enumerate(REDUCE_NY):
                if b * S * ny <= 3_000_000:
                    out.append((S, b, ny, (k + b + S) % 2))
    return out


def reduce_case(S, b, ny, y_shared):
    """adversarial data: odd inputs carry a 1e6 offset in mu (c2 must survive), sigma^2 spans 1e-6 .. 1e3, the last y of every row lies 40
    of the LARGEST sigma beyond every node (every term underflows: 0, not NaN), and -- with b >= 3 -- node 0 of the last input has
    sigma^2 = 0 (its densities are non-finite, its moments finite).  Returns mu, var [b, S], wq [S], y ([ny] or [b, ny]) or None."""
    rng = np.random.RandomState(1000003 * ny + 1009 * b + S)
    mu = rng.randn(b, S)
    mu[1::2] += 1e6
    var = 10.0 ** rng.uniform(-6, 3, (b, S))
    if b >= 3:
        var[-1, 0] = 0.0
    wq = rng.uniform(0.1, 1.0, S)
    wq /= wq.sum()
    if ny == 0:
        return mu, var, wq, None
    if y_shared:
        y = np.linspace(-3.0, 3.0, ny) * np.sqrt(var.max()) * (1 if b == 1 else 1e-3) + (1e6 if b == 2 else 0.0)
        y[-1] = 1e6 + 5.0 + 40.0 * np.sqrt(var.max())
    else:
        c = mu.mean(axis=1)
        y = c[:, None] + np.linspace(-3.0, 3.0, ny)[None, :] * np.sqrt(var.mean(axis=1))[:, None]
        y[:, -1] = c + 5.0 + 40.0 * np.sqrt(var.max())
    # y on the 2^-20 grid: y - shift is then exact for the shift the tests use (0.25), and what is measured is the reduction's arithmetic,
    # not the conditioning of a difference the caller asked for
    return mu, var, wq, np.round(y * 2.0 ** 20) / 2.0 ** 20


def reduce_rho():
    """rho over a subset of the shapes that covers every path of the restatement (one and many segments, one and many rows of segments)"""
    cases = []
    for S, b, ny, ysh in reduce_shapes():
        if b * S * max(ny, 1) > 600_000:
            continue
        mu, var, wq, y = reduce_case(S, b, ny, ysh)
        for i in range(b):
            if var[i].min() > 0:
                cases.append((mu[i], var[i], wq, None if y is None else (y if ysh else y[i]), 0.25))
    return rho(cases)


def periodic_estimate_many(x, t, theta, xs):
    """estimate_many of the reference's GP with PeriodicCovariance in NumPy (float64 kernel of _periodic_ld, Cholesky solves): mean WITH meant"""
    import _periodic_ld as pl
    t = np.asarray(t, float)
    meant = t.mean()
    K = pl.kernel_parts(x, x, theta, dt=np.float64)["K"]
    kv = pl.kernel_parts(xs, x, theta, dt=np.float64)["K"]
    L = np.linalg.cholesky(K)
    import scipy.linalg as sl
    zy = sl.solve_triangular(L, t - meant, lower=True)
    Z = sl.solve_triangular(L, kv.T, lower=True)
    v, vt = np.exp(theta[0]), np.exp(theta[1])
    return Z.T.dot(zy) + meant, (v + vt) - (Z * Z).sum(axis=0)
