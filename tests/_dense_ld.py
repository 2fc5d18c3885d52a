"""A long-double model of the N^2 reduction sums of the dense GP (scikit-gpuppy_amd/csrc/propagate.hip, fit.hip), the seeded inputs of
tests/test_dense_bounds.py and the rule those tests compare by.  Host only.

Every sum is a function of the training data and of K^-1 and alpha = K^-1 t, and the device hands both back (gpx_kinv, gpx_alpha): the
model evaluates the SAME sum in np.longdouble (x87, eps 1.08e-19) from the K^-1 and alpha it is given, so that the condition of K never
enters the comparison (the move of tests/_accuracy.py, which judges the solves on the device's own factor).  What is restated:
  gradient   S_0 = sum_ij M_ij Kf_ij, S_{1+k} = sum_ij M_ij Kf_ij w_k (x_ik - x_jk)^2, T = tr(Kinv) - alpha.alpha, M = Kinv - alpha alpha^T,
             Kf_ij = v exp(-1/2 sum_k w_k (x_ik - x_jk)^2) from DIRECT differences of the raw inputs (the device scales by sqrt(w) first);
             g_0 = S_0 / 2, g_1 = vt T / 2, g_{2+k} = -S_{1+k} / 4                                   (gpx_nll_grad)
             1/2 sum_ij Kinv_ij dK_ij - 1/2 alpha^T dK alpha for a supplied dK                          (gpx_nll_grad_matrix)
  C, J, H    c_i = v exp(-q_i / 2), q_i = sum_k w_k (x_ik - u_k)^2, C_i = c_i + vt iff x_i == u elementwise, J_ik = -w_k delta_k c_i,
             H_iab = (w_a delta_a w_b delta_b - [a == b] w_a) c_i                                         (gpx_cjh)
  Approx     the 4 + 2 d sums of gpx_propagate_approx_rows in its order -- beta.C, beta.tr, C.KinvC, KinvC.tr, then J_k.KinvJ_k and
             beta.J_k for every k, tr_i = c_i ((w delta)^T Sigma (w delta) - sum_k w_k Sigma_kk), full Sigma --, restricted to a row
             range of K^-1; mean, sigma2, rest and variance as skgpuppy_amd.distributed.combine_approx_partials combines them; and
             dvh_k = -(J_k.KinvJ_k - (beta.J_k)^2) - KinvC.H_kk                                           (gpx_propagate_dvh)
  Exact      Girard's constants as exact_constants of propagate_api.hip states them -- Delta^-1 = diag(w_k - w_k / (1 + w_k S_kk)),
             nc1 = prod (1 + w_k S_kk)^-1/2, nc2 = prod (1 + 2 w_k S_kk)^-1/2, Ls = the symmetric part of 2 W - (Sigma + W^-1 / 2)^-1 --,
             l_i = C_i nc1 exp(a_i^T Delta^-1 a_i / 2), a_i = u - x_i, and
             [sum_i beta_i l_i,  sum_{j <= i} wgt_ij (Ksym_ij - beta_i beta_j) C_i C_j exp(z^T Ls z / 2),  nc2],  z = (a_i + a_j) / 2,
             wgt 2 below the diagonal and 1 on it, Ksym the mean of both triangles; mean = p0, var = cuu - nc2 p1 - p0^2.

Every function takes `dt`: np.longdouble is the model, np.float64 the plain numpy evaluation of the same case that rho_ref is measured on.
Each returns (values, absolute scales): a sum's scale is the sum of the absolute values of its terms, with the differences that cancel
taken apart -- M_ij as |Kinv_ij| + |alpha_i| |alpha_j|, tr_i as c_i (|w delta|^T |Sigma| |w delta| + sum w_k |Sigma_kk|), a combined value
(mean, sigma2, rest, var, dvh) as the same combination of its parts' scales.  Row blocks of ROWS rows keep every temporary within
ROWS N d entries.

The rule is the one of tests/_spgp_ld.py, with its constants: distance = |got - model| / scale, and the device passes when every distance is
within MARGIN * max(rho_ref, FLOOR), rho_ref the largest distance of the float64 evaluation of the same sums.  Nothing here is fitted
to a device result.  What the device's arithmetic has and the float64 evaluation has not: q from sqrt(w)-prescaled inputs in the gradient,
x~_k = fl(sqrt(w_k) x_k): the difference of two prescaled coordinates is off by at most 2 u max_k(sqrt(w_k) |x_k|), hence
|dq| <= 4 max_k(sqrt(w_k) |x_k|) sqrt(d q) u + d q u and a term's relative error is half of it: 1.3e-14 at d = 64, q = 14 (the largest q of
a term above 1e-3 v), sqrt(w) |x| <= 0.5 -- under FLOOR, so the rule needs no extra term for it.  Away from the origin it is not: for
inputs translated by `shift` (tests/test_shifted_inputs.py: 2^10, 2^17) grad_loss() sums this quantity pair by pair (prescale_loss) and the
tests admit exactly it, as an absolute allowance outside the margin.

`defect=` plants one of the seeded defects of tests/test_dense_ld_model.py in an evaluation (meant for dt = np.float64)."""
import os

import numpy as np

from _spgp_ld import FLOOR, LD, MARGIN, _grid, bound  # noqa: F401  (the project's one rule: imported, not copied)

ROWS = 64
D_ALL = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
SMALL_N, SMALL_D = (128, 129, 200), (1, 3, 8)
CASES = [(700, d) for d in D_ALL] + [(N, d) for N in SMALL_N for d in SMALL_D]      # every (N, d) the GPU tests fit
QUIRK_ROW = 5
SHARP_CASE = (700, 3)      # the explicit Exact path's case with positive exponents
FAR_Q = 600.0       # smallest q_i of the far input: C_i <= v e^-300 = 1e-130, the quadratic forms 1e-260 and below


# ------------------------------------------------------------------------------------------------
# seeded inputs
# ------------------------------------------------------------------------------------------------
def make_case(N, d, seed, sharp=False):
    """(x, t centred, theta): x on the 2^-20 grid in [0, 10]^d, v = 2, vt = 0.01, w_k = 0.04 (3 / d) (1 +- 20 %), or [2, 8] (3 / d) if sharp"""
    rng = np.random.RandomState(seed)
    x = _grid(rng.uniform(0, 10, (N, d)))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    t = t - t.mean()
    w = (rng.uniform(2.0, 8.0, d) if sharp else 0.04 * (1 + 0.2 * rng.uniform(-1, 1, d))) * 3.0 / d
    return x, t, np.log(np.concatenate([[2.0, 0.01], w]))


def seed_of(N, d):
    return 1000 * d + N


def params(theta, d, dt=LD):
    """(v, vt, w): exp(theta) in float64 -- the parameters the device holds -- then widened"""
    th = np.asarray(theta, dtype=np.float64)
    return dt(np.exp(th[0])), dt(np.exp(th[1])), np.exp(th[2:2 + d]).astype(dt)


def live_pairs(x, theta):
    """the number of ordered pairs (i, j) with Kf_ij > 1e-3 v"""
    N, d = x.shape
    _v, _vt, w = params(theta, d, np.float64)
    cnt = 0
    for i0 in range(0, N, ROWS):
        q = np.zeros((min(N, i0 + ROWS) - i0, N))
        for k in range(d):
            q += w[k] * (x[i0:i0 + ROWS, k][:, None] - x[:, k][None, :]) ** 2
        cnt += int((np.exp(-0.5 * q) > 1e-3).sum())
    return cnt


def inputs_u(x, theta, seed):
    """the three inputs of a case: between the training points, bit-equal to training point QUIRK_ROW, far outside the data"""
    N, d = x.shape
    rng = np.random.RandomState(seed + 7)
    return {"between": _grid(rng.uniform(2, 8, d)), "equal": x[QUIRK_ROW].copy(), "far": far_u(x, theta)}


def far_u(x, theta, target=FAR_Q):
    """u = c (1, .., 1) on the grid, c > 10 the smallest with min_i q_i >= target"""
    N, d = x.shape
    _v, _vt, w = params(theta, d, np.float64)
    lo, hi = 10.0, 1e4
    for _ in range(60):
        c = 0.5 * (lo + hi)
        if ((w * (c - x) ** 2).sum(1)).min() >= target:
            hi = c
        else:
            lo = c
    return np.full(d, np.ceil(hi * 2.0 ** 20) / 2.0 ** 20)


def sigmas(d, seed):
    """a diagonal Sigma and, from d = 2 on, a full SPD one with off-diagonal entries"""
    rng = np.random.RandomState(seed + 11)
    out = {"diag": np.diag(rng.uniform(0.05, 0.5, d))}
    if d >= 2:
        A = rng.uniform(-0.3, 0.3, (d, d))
        out["full"] = A.dot(A.T) + 0.05 * np.eye(d)
    return out


def sharp_inputs(x, theta):
    """(u, Sigma, C_ux, w, cuu) of the sharp case: u at the corner 0 of the cube, Sigma = 0.01 I, C_ux from the kernel in float64.  The
    exponent z^T Ls z / 2 of a pair grows with its distance from the corner (Ls_kk = 4 w_k^2 S / (1 + 2 w_k S)), C_i C_j falls faster."""
    d = x.shape[1]
    v, vt, w = params(theta, d, np.float64)
    u = np.zeros(d)
    C = v * np.exp(-0.5 * (w * (x - u) ** 2).sum(1))
    return u, 0.01 * np.eye(d), C, w, float(v + vt)


# ------------------------------------------------------------------------------------------------
# the gradient
# ------------------------------------------------------------------------------------------------
def _pair_of(x, w):
    """the seeded defect's pair: row N // 2 and its nearest other row"""
    i = len(x) // 2
    q = (np.asarray(w, float) * (x - x[i]) ** 2).sum(1)
    q[i] = np.inf
    return i, int(np.argmin(q))


def _weights(defect, N, i0, i1, pair):
    """the seeded defects that drop or double terms, as a weight per (row of the block, column)"""
    W = np.ones((i1 - i0, N))
    if defect == "pair":
        for a, b in (pair, pair[::-1]):
            if i0 <= a < i1:
                W[a - i0, b] = 0.0
    elif defect == "diag2":
        W[np.arange(i1 - i0), np.arange(i0, i1)] = 2.0
    elif defect == "tail":
        W[:, (N * 512) // 700:] = 0.0          # 700 -> the last 700 - 512 columns
    elif defect == "quarter":
        W[:, 3::4] = 0.0
    return W


def prescale_loss(x, theta, shift, D, dt=LD):
    """What the device's prescaling costs the terms of a block of pairs when the inputs it sees are x + shift, as bounds per pair:
    (rq [rows, N], rk [d, rows, N]) for D [d, rows, N] = w_k (x_ik - x_jk)^2.  With m_k = sqrt(w_k) max_i |x_ik + shift|, m = max_k m_k, u = 2^-53 and e_k the exact scaled
    difference (e_k^2 = D[k] = w_k (x_ik - x_jk)^2), the difference of two prescaled coordinates is off by at most 2 u m_k (module
    docstring), so
      |d(e_k^2)| <= 4 u m_k |e_k| + u e_k^2                                                            =: rk[k]   (the factor of S_{1+k})
      |dq| <= 4 u m sum_k |e_k| + u q <= 4 m sqrt(d q) u + d q u,  a term's relative error half of it  =: rq      (the factor Kf of every sum)
    rq is the quantity the module docstring derives; rk is the same bound before Cauchy-Schwarz, for the one coordinate."""
    xr = np.asarray(x, dtype=np.float64)
    d = xr.shape[1]
    _v, _vt, w = params(theta, d, dt)
    u = dt(2.0 ** -53)
    mk = np.sqrt(w) * np.abs(xr + shift).max(0).astype(dt)
    q = D.sum(0)
    rq = (4 * mk.max() * np.sqrt(d * q) * u + d * q * u) / 2
    rk = np.array([4 * u * mk[k] * np.sqrt(D[k]) + u * D[k] for k in range(d)])
    return rq, rk


def _grad_sums(x, theta, Kinv, alpha, dt, defect, shift):
    """(sums, scales, loss): loss [d + 2] = sum over the pairs of |term| times its prescale_loss for a device that saw x + shift (0 at shift 0)"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, _vt, w = params(theta, d, dt)
    x = xr.astype(dt)
    Ki, al = np.asarray(Kinv).astype(dt), np.asarray(alpha).astype(dt)
    S, A, E = np.zeros(d + 2, dt), np.zeros(d + 2, dt), np.zeros(d + 2, dt)
    pair = _pair_of(xr, w) if defect == "pair" else None
    for i0 in range(0, N, ROWS):
        i1 = min(N, i0 + ROWS)
        D = np.empty((d, i1 - i0, N), dt)
        for k in range(d):
            D[k] = w[k] * (x[i0:i1, k][:, None] - x[:, k][None, :]) ** 2
        e = -(D[:d - 1].sum(0) if defect == "coord" else D.sum(0)) / 2
        Kf = v * (np.exp(e.astype(np.float32)).astype(dt) if defect == "exp32" else np.exp(e))
        if defect in ("pair", "diag2", "tail", "quarter"):
            Kf = Kf * _weights(defect, N, i0, i1, pair).astype(dt)
        MK = (Ki[i0:i1] - np.outer(al[i0:i1], al)) * Kf
        AK = (np.abs(Ki[i0:i1]) + np.outer(np.abs(al[i0:i1]), np.abs(al))) * Kf
        S[0] += MK.sum()
        A[0] += AK.sum()
        for k in range(d):
            S[1 + k] += (MK * D[k]).sum()
            A[1 + k] += (AK * D[k]).sum()
        if shift != 0.0:
            rq, rk = prescale_loss(xr, theta, shift, D, dt)
            E[0] += (AK * rq).sum()
            for k in range(d):
                E[1 + k] += (AK * (D[k] * rq + rk[k])).sum()
    dg = np.diagonal(Ki)
    S[d + 1] = dg.sum() - al.dot(al)
    A[d + 1] = np.abs(dg).sum() + al.dot(al)
    return S, A, E


def grad_sums(x, theta, Kinv, alpha, dt=LD, defect=None):
    """([S_0, S_1 .. S_d, T], their scales)"""
    return _grad_sums(x, theta, Kinv, alpha, dt, defect, 0.0)[:2]


def grad_loss(x, theta, Kinv, alpha, shift):
    """[d + 2], long double: what the prescaling may cost each entry of gpx_nll_grad when the device saw x + shift (x: the case as seeded) --
    the sum over the pairs of |term| prescale_loss, combined as grad_from_sums combines the sums.  An ABSOLUTE allowance: the tests take it
    off |got - model| before the rule (distances(loss=)), outside the margin, so exactly this quantity is admitted and nothing else."""
    _S, _A, E = _grad_sums(x, theta, Kinv, alpha, LD, None, shift)
    return grad_from_sums(E, E, theta)[1]


def grad_from_sums(S, A, theta):
    """(gradient, scales) as gpx_nll_grad combines the sums"""
    d = len(S) - 2
    vt = S.dtype.type(np.exp(np.float64(theta[1])))
    g, s = np.empty_like(S), np.empty_like(A)
    g[0], s[0] = S[0] / 2, A[0] / 2
    g[1], s[1] = vt * S[d + 1] / 2, vt * A[d + 1] / 2
    g[2:], s[2:] = -S[1:d + 1] / 4, A[1:d + 1] / 4
    return g, s


def grad(x, theta, Kinv, alpha, dt=LD, defect=None):
    return grad_from_sums(*grad_sums(x, theta, Kinv, alpha, dt, defect), theta=theta)


def grad_matrix(Kinv, alpha, dK, dt=LD):
    """1/2 sum_ij Kinv_ij dK_ij - 1/2 alpha^T dK alpha, as (value [1], scale [1])"""
    N = len(alpha)
    al = np.asarray(alpha).astype(dt)
    s, a = dt(0), dt(0)
    for i0 in range(0, N, ROWS):
        Kb, Db = np.asarray(Kinv[i0:i0 + ROWS]).astype(dt), np.asarray(dK[i0:i0 + ROWS]).astype(dt)
        s += (Kb * Db).sum() - al[i0:i0 + ROWS].dot(Db.dot(al))
        a += (np.abs(Kb) * np.abs(Db)).sum() + np.abs(al[i0:i0 + ROWS]).dot(np.abs(Db).dot(np.abs(al)))
    return np.array([s / 2], dt), np.array([a / 2], dt)


# ------------------------------------------------------------------------------------------------
# C, J, H and the Approx sums
# ------------------------------------------------------------------------------------------------
def _rows_of(x, theta, u, dt, defect=None):
    xr, ur = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    d = xr.shape[1]
    v, vt, w = params(theta, d, dt)
    delta = xr.astype(dt) - ur.astype(dt)
    wd = w * delta
    q = (wd[:, :d - 1] * delta[:, :d - 1]).sum(1) if defect == "coord" else (wd * delta).sum(1)
    c = v * np.exp(-q / 2)
    same = (xr == ur).all(1) & (defect != "quirk")
    return v, vt, w, wd, q, c, c + vt * same.astype(dt)


def cjh(x, theta, u, dt=LD):
    """(C [N], J [N, d], H [N, d, d], q [N], Habs [N, d, d]): Habs the entries of H with their difference taken apart"""
    d = np.shape(x)[1]
    _v, _vt, w, wd, q, c, C = _rows_of(x, theta, u, dt)
    J = -wd * c[:, None]
    outer = wd[:, :, None] * wd[:, None, :]
    eye = np.eye(d, dtype=dt) * w
    return C, J, (outer - eye) * c[:, None, None], q, (np.abs(outer) + eye) * c[:, None, None]


def approx_partials(x, theta, Kinv, alpha, u, Sigma, rows=None, dt=LD, defect=None):
    """{"partials": the 4 + 2 d sums over the rows [r0, r1) of K^-1, "mean", "var", "sigma2", "rest", "dvh" [d]}, each (values, scales);
    the combined values mean the sums of THESE rows combined (the whole model for rows = None)"""
    N, d = np.shape(x)
    r0, r1 = (0, N) if rows is None else rows
    v, vt, w, wd, _q, c, C = _rows_of(x, theta, u, dt, defect)
    S = np.asarray(Sigma).astype(dt)
    al, aal = np.asarray(alpha).astype(dt)[r0:r1], np.abs(np.asarray(alpha).astype(dt)[r0:r1])
    wdiag = (w * np.diagonal(S)).sum()
    awd = np.abs(wd)
    tr = c * ((wd.dot(S) * wd).sum(1) - wdiag)
    atr = c * ((awd.dot(np.abs(S)) * awd).sum(1) + (w * np.abs(np.diagonal(S))).sum())
    V = np.concatenate([C[:, None], -wd * c[:, None]], axis=1)                       # [N, d + 1]: C, J_1 .. J_d
    Ki = np.asarray(Kinv[r0:r1]).astype(dt)
    KV, aKV = Ki.dot(V), np.abs(Ki).dot(np.abs(V))                                   # [rows, d + 1]
    Vr, aVr = V[r0:r1], np.abs(V[r0:r1])
    o, A = np.empty(4 + 2 * d, dt), np.empty(4 + 2 * d, dt)
    o[0], A[0] = al.dot(Vr[:, 0]), aal.dot(aVr[:, 0])
    o[1], A[1] = al.dot(tr[r0:r1]), aal.dot(atr[r0:r1])
    o[2], A[2] = Vr[:, 0].dot(KV[:, 0]), aVr[:, 0].dot(aKV[:, 0])
    o[3], A[3] = KV[:, 0].dot(tr[r0:r1]), aKV[:, 0].dot(atr[r0:r1])
    o[4::2], A[4::2] = (Vr[:, 1:] * KV[:, 1:]).sum(0), (aVr[:, 1:] * aKV[:, 1:]).sum(0)
    o[5::2], A[5::2] = al.dot(Vr[:, 1:]), aal.dot(aVr[:, 1:])
    sd, asd = np.diagonal(S), np.abs(np.diagonal(S))
    mean, amean = o[0] + o[1] / 2, A[0] + A[1] / 2
    s2, as2 = (v + vt) - o[2], (v + vt) + A[2]
    rest, arest = -(sd * (o[4::2] - o[5::2] ** 2)).sum() - o[3], (asd * (A[4::2] + A[5::2] ** 2)).sum() + A[3]
    hkk, ahkk = (wd ** 2 - w) * c[:, None], (wd ** 2 + w) * c[:, None]
    dvh = -(o[4::2] - o[5::2] ** 2) - KV[:, 0].dot(hkk[r0:r1])
    advh = A[4::2] + A[5::2] ** 2 + aKV[:, 0].dot(ahkk[r0:r1])
    one = lambda a, b: (np.array([a], dt), np.array([b], dt))  # noqa: E731
    return {"partials": (o, A), "mean": one(mean, amean), "var": one(s2 + rest, as2 + arest), "sigma2": one(s2, as2),
            "rest": one(rest, arest), "dvh": (dvh, advh)}


# ------------------------------------------------------------------------------------------------
# Exact
# ------------------------------------------------------------------------------------------------
def small_inverse(A):
    """Gauss-Jordan with partial pivoting in A's own precision"""
    d = len(A)
    M = np.concatenate([np.array(A), np.eye(d, dtype=A.dtype)], axis=1)
    for c in range(d):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(d):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, d:]


def exact_constants(w, Sigma, dt=LD):
    """(Ls [d, d], Delta^-1 diagonal [d], nc1, nc2)"""
    w, S = np.asarray(w).astype(dt), np.asarray(Sigma).astype(dt)
    sk = np.diagonal(S)
    dd = w - w / (1 + w * sk)
    nc1 = 1 / np.sqrt(np.prod(1 + w * sk))
    nc2 = 1 / np.sqrt(np.prod(2 * w * sk + 1))
    Lam = np.diag(2 * w) - small_inverse(S + np.diag(1 / (2 * w)))
    return (Lam + Lam.T) / 2, dd, nc1, nc2


def exact_parts(x, w, Kinv, beta, C, u, Sigma, cuu, rows=None, dt=LD, defect=None):
    """{"parts": [sum_i beta_i l_i, the j <= i double sum without nc2, nc2] over the rows [r0, r1), "mean", "var", "emax": the largest
    exponent z^T Ls z / 2 of a visited pair}; parts / mean / var as (values, scales)"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    r0, r1 = (0, N) if rows is None else rows
    Ls, dd, nc1, nc2 = exact_constants(w, Sigma, dt)
    a = np.asarray(u, dtype=np.float64).astype(dt) - xr.astype(dt)
    C, be = np.asarray(C).astype(dt), np.asarray(beta).astype(dt)
    lm = C * nc1 * np.exp((a * a * dd).sum(1) / 2)
    p0, a0 = be[r0:r1].dot(lm[r0:r1]), np.abs(be[r0:r1]).dot(np.abs(lm[r0:r1]))
    aL = a.dot(Ls)
    ql = (aL * a).sum(1)
    p1, a1, emax = dt(0), dt(0), -np.inf
    cols = np.arange(N)
    for i0 in range(r0, r1, ROWS):
        i1 = min(r1, i0 + ROWS)
        Kl, Ku = np.asarray(Kinv[i0:i1]).astype(dt), np.asarray(Kinv[:, i0:i1]).astype(dt).T
        Ks = Kl if defect == "unsym" else (Kl + Ku) / 2
        E = (ql[i0:i1][:, None] + ql[None, :]) / 8 + aL[i0:i1].dot(a.T) / 4
        ii = np.arange(i0, i1)[:, None]
        wgt = np.where(cols[None, :] < ii, 2.0, np.where(cols[None, :] == ii, 2.0 if defect == "diag2" else 1.0, 0.0)).astype(dt)
        emax = max(emax, float(np.where(wgt > 0, E, -np.inf).max()))
        Lij = np.outer(C[i0:i1], C) * np.exp(E) * wgt
        p1 += ((Ks - np.outer(be[i0:i1], be)) * Lij).sum()
        a1 += ((np.abs(Ks) + np.outer(np.abs(be[i0:i1]), np.abs(be))) * np.abs(Lij)).sum()
    cuu = dt(cuu)
    one = lambda p, q: (np.array([p], dt), np.array([q], dt))  # noqa: E731
    return {"parts": (np.array([p0, p1, nc2], dt), np.array([a0, a1, nc2], dt)), "mean": one(p0, a0),
            "var": one(cuu - nc2 * p1 - p0 * p0, np.abs(cuu) + nc2 * a1 + a0 * a0), "emax": emax}


def exact_builtin(x, theta, Kinv, alpha, u, Sigma, rows=None, dt=LD, defect=None):
    """exact_parts for the built-in kernel: C from the model's own kernel (the quirk included), cuu = v + vt"""
    d = np.shape(x)[1]
    v, vt, w, _wd, _q, _c, C = _rows_of(x, theta, u, dt, defect if defect == "quirk" else None)
    return exact_parts(x, w, Kinv, alpha, C, u, Sigma, v + vt, rows, dt, defect)


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def distances(got, want, scale, loss=0):
    """|got - want| / scale entry by entry in long double; 0 where both the difference and the scale are 0.  loss: an absolute allowance
    per entry, taken off the difference first (grad_loss)"""
    g, w, s = (np.atleast_1d(np.asarray(a)).astype(LD) for a in (got, want, scale))
    if g.shape != w.shape:
        raise ValueError("shape %r against %r" % (g.shape, w.shape))
    diff = np.maximum(np.abs(g - w) - loss, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = diff / s
    return np.where((diff == 0) & (s == 0), LD(0), r).astype(np.float64)


def rho_of(groups_ref):
    """rho_ref of a case: the largest distance of its float64 evaluation over {group: distances}"""
    return max(float(np.max(r)) for r in groups_ref.values())


def assert_within(dist, rho, what=""):
    """every distance of {group: distances} finite and within MARGIN * max(rho, FLOOR)"""
    lim = bound(rho)
    bad = ["%s[%d] %.3e" % (k, int(np.argmax(~(r <= lim))), float(np.max(np.where(np.isnan(r), np.inf, r))))
           for k, r in dist.items() if not np.all(r <= lim)]
    assert not bad, "%s: beyond %g * max(rho_ref = %.3e, %.3e) = %.3e: %s" % (what, MARGIN, rho, FLOOR, lim, ", ".join(bad))
    return dist


def record(title, name, rho, dist, ref_dist):
    """print, and with GPX_DENSE_BOUNDS_RECORD=<file> append, rho_ref, the bound and each group's worst ratio to both"""
    lim = bound(rho)
    lines = ["%s | %s | rho_ref %.3e  bound %.3e (margin %g)" % (title, name, rho, lim, MARGIN)]
    for k, r in dist.items():
        worst = float(np.max(np.where(np.isnan(r), np.inf, r)))
        ref = float(np.max(ref_dist[k])) if k in ref_dist else float("nan")
        lines.append("    %-22s ref %.3e   device %.3e = %10.3f rho_ref = %8.6f bound" % (k, ref, worst, worst / max(rho, 1e-300), worst / lim))
    print("\n".join(lines))
    path = os.environ.get("GPX_DENSE_BOUNDS_RECORD")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
