"""A long-double model of the SPGP algebra (scikit-gpuppy_amd/csrc/spgp.hip), the seeded inputs of tests/test_spgp_bounds.py and the rule
those tests compare by.

numpy's longdouble is the x87 80-bit format here (eps 1.08e-19) and has no BLAS / LAPACK behind it: the column Cholesky and the two
substitutions below are the model's own.  What is restated:
  predictor   L_M = chol(K_M + 1e-5 I), Z = L_M^-1 K_MN, lambda_n = v + vt - |Z_n|^2, B~ = K_M + 1e-5 I + K_MN Lambda^-1 K_NM,
              beta = B~^-1 K_MN Lambda^-1 t;  mean* - mean(t) = K_*M beta,  var* = v + vt - |K_*M L_M^-T|^2 + |K_*M L_B^-T|^2
  likelihood  Snelson's, jitter 1e-6, as oracle.spgp_nll
  gradient    the analytic one of oracle.spgp_nll_grad, with every Gram entry from DIRECT differences sum_k w_k (a_k - b_k)^2 and the
              last contractions direct as well: -w_k/2 sum (E o dE^2 + F o dF^2) and -w_k sum E o dE - 2 w_k sum F o dF.  Neither the
              oracle (expanded squares in its Gram and its moments) nor the device (expanded moments) forms them this way.

The rule (`distances`, `bound`, `assert_within`) is measured, not chosen: a case's rho_ref is the largest scaled distance, over groups, of
the float64 CPU evaluation (oracle.spgp_nll / spgp_nll_grad, `woodbury_predict`) from the long-double values, and the device passes when
every group is within MARGIN * max(rho_ref, FLOOR) of them.  Groups and their scales: nll, log v, log vt and each log w_k by their own
absolute value; the pseudo-input block and the predicted means (less mean(t)) by their own max-norm; the variances by v + vt; any matrix
(the dense forms) by its max-norm.  MARGIN = 32 allows for the explicit inverses inv(L) and A^-1 and the device's summation orders; FLOOR
keeps a case where float64 is luckily exact from demanding the impossible."""
import hashlib

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import oracle as orc

LD = np.longdouble
MARGIN = 32.0
FLOOR = 1000.0 * 2.0 ** -53
NQ = 77                      # queries per case
SHIFT = float(2 ** 17)       # exact on the 2^-20 grid the inputs live on


# ------------------------------------------------------------------------------------------------
# seeded inputs
# ------------------------------------------------------------------------------------------------
def _grid(a):
    return np.round(a * 2.0 ** 20) / 2.0 ** 20


def make_case(N, d, m, wlo, whi, jit, shift=0.0):
    """(x, t centred, theta, xs): x, the pseudo-inputs and the queries on the 2^-20 grid, seed N + m; `shift` is added to every coordinate
    of all three (exactly: the problem is mathematically the same one)."""
    rng = np.random.RandomState(N + m)
    x = _grid(rng.uniform(0, 10, (N, d)))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    t = t - t.mean()
    xb = _grid(x[rng.randint(N, size=m)] + jit * rng.randn(m, d))
    logw = np.log(rng.uniform(wlo, whi, d))
    xs = _grid(rng.uniform(0, 10, (NQ, d)))
    theta = np.concatenate([np.log([1.7, 0.02]), logw, (xb + shift).ravel()])
    return x + shift, t, theta, xs + shift


def input_hash(x, t, theta, xs):
    h = hashlib.sha256()
    for a in (x, t, theta, xs):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------
# long-double linear algebra
# ------------------------------------------------------------------------------------------------
def chol(A):
    """lower Cholesky factor by columns (right-looking rank-1 updates)"""
    A = np.array(A, dtype=LD)
    n = len(A)
    for j in range(n):
        if not A[j, j] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A)


def fwd(L, B):
    """L X = B"""
    X = np.array(B, dtype=LD)
    for i in range(len(L)):
        if i:
            X[i] -= L[i, :i] @ X[:i]
        X[i] /= L[i, i]
    return X


def bwd(L, B):
    """L^T X = B"""
    X = np.array(B, dtype=LD)
    n = len(L)
    for i in range(n - 1, -1, -1):
        if i < n - 1:
            X[i] -= L[i + 1:, i] @ X[i + 1:]
        X[i] /= L[i, i]
    return X


def gram(a, b, v, w):
    """v exp(-sum_k w_k (a_k - b_k)^2 / 2) from direct differences"""
    D = np.zeros((len(a), len(b)), LD)
    for k in range(a.shape[1]):
        D += w[k] * (a[:, k][:, None] - b[:, k][None, :]) ** 2
    return v * np.exp(-D / 2)


def unpack(theta, d, m):
    th = np.asarray(theta).astype(LD)
    return np.exp(th[0]), np.exp(th[1]), np.exp(th[2:2 + d]), th[2 + d:].reshape(m, d)


def _eye(m):
    return np.eye(m, dtype=LD)


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
class Predictor(object):
    """the fitted low-rank model in long double: predict, and the dense forms gpx_spgp_dense / gpx_spgp_cross return"""

    def __init__(self, x, t, theta, m):
        self.x = np.asarray(x).astype(LD)
        self.N, self.d = self.x.shape
        self.m = m
        self.v, self.vt, self.w, self.xm = unpack(theta, self.d, m)
        y = np.asarray(t).astype(LD)
        Km = gram(self.xm, self.xm, self.v, self.w) + LD(1e-5) * _eye(m)
        self.Kmn = gram(self.xm, self.x, self.v, self.w)
        self.LM = chol(Km)
        self.Z = fwd(self.LM, self.Kmn)
        self.lam = self.v + self.vt - (self.Z ** 2).sum(0)
        Kl = self.Kmn / self.lam
        self.LB = chol(Km + Kl @ self.Kmn.T)
        self.beta = bwd(self.LB, fwd(self.LB, Kl @ y))

    def predict(self, xs):
        """(mean* - mean(t), var*)"""
        Ks = gram(self.xm, np.asarray(xs).astype(LD), self.v, self.w)      # [m, q]
        mean = self.beta @ Ks
        var = self.v + self.vt - (fwd(self.LM, Ks) ** 2).sum(0) + (fwd(self.LB, Ks) ** 2).sum(0)
        return mean, var

    def cov(self):
        """Q_N + diag(K_N - Q_N) + vt I"""
        return self.Z.T @ self.Z + np.diag(self.lam)

    def inv(self):
        """Lambda^-1 - Lambda^-1 K_NM B~^-1 K_MN Lambda^-1"""
        Y = fwd(self.LB, self.Kmn) / self.lam
        return np.diag(1 / self.lam) - Y.T @ Y

    def cross(self, xi, xj):
        """K_iM (K_M + 1e-5 I)^-1 K_Mj"""
        Zi = fwd(self.LM, gram(self.xm, np.asarray(xi).astype(LD), self.v, self.w))
        Zj = fwd(self.LM, gram(self.xm, np.asarray(xj).astype(LD), self.v, self.w))
        return Zi.T @ Zj


def nll(x, t, theta, m):
    """Snelson's likelihood, jitter 1e-6"""
    x = np.asarray(x).astype(LD)
    N, d = x.shape
    y = np.asarray(t).astype(LD)
    v, vt, w, xm = unpack(theta, d, m)
    L = chol(gram(xm, xm, v, w) + LD(1e-6) * _eye(m))
    V = fwd(L, gram(xm, x, v, w))
    return _nll_from_v(V, y, v, vt, N, m)


def _nll_from_v(V, y, v, vt, N, m):
    ep = 1 + (v - (V ** 2).sum(0)) / vt
    Vs = V / np.sqrt(ep)
    ys = y / np.sqrt(ep)
    Lm = chol(vt * _eye(m) + Vs @ Vs.T)
    bet = fwd(Lm, Vs @ ys)
    pi = 4 * np.arctan(LD(1))
    return (np.log(np.diag(Lm)).sum() + LD(N - m) / 2 * np.log(vt) + (ys @ ys - bet @ bet) / 2 / vt + np.log(ep).sum() / 2
            + LD(N) / 2 * np.log(2 * pi))


def nll_grad(x, t, theta, m):
    """(nll, d nll / d theta), theta = (log v, log vt, log w_1..d, pseudo-inputs row-major)"""
    x = np.asarray(x).astype(LD)
    N, d = x.shape
    y = np.asarray(t).astype(LD)
    v, vt, w, xm = unpack(theta, d, m)
    Qk = gram(xm, xm, v, w)
    K = gram(xm, x, v, w)
    L = chol(Qk + LD(1e-6) * _eye(m))
    V = fwd(L, K)
    gamma = vt + v - (V ** 2).sum(0)
    VD = V * (vt / gamma)
    LA = chol(vt * _eye(m) + VD @ V.T)
    Ainv = bwd(LA, fwd(LA, _eye(m)))
    T1 = Ainv @ VD
    betaA = T1 @ y
    alpha = (y - V.T @ betaA) / gamma
    s_n = (T1 * V).sum(0)
    g = ((1 - s_n) / gamma - alpha ** 2) / 2
    Vbar = T1 - np.outer(betaA, alpha) - 2 * V * g
    Kbar = bwd(L, Vbar)
    Qb = -(_eye(m) - vt * Ainv - np.outer(betaA, betaA)) / 2 + (V * g) @ V.T
    Qbar = bwd(L, bwd(L, Qb).T)
    Qbar = (Qbar + Qbar.T) / 2
    E = Kbar * K
    F = Qbar * Qk
    grad = np.empty(2 + d + m * d, LD)
    grad[0] = E.sum() + F.sum() + v * g.sum()
    grad[1] = vt * g.sum()
    dxb = np.empty((m, d), LD)
    for k in range(d):
        dE = xm[:, k][:, None] - x[:, k][None, :]
        dF = xm[:, k][:, None] - xm[:, k][None, :]
        grad[2 + k] = -w[k] / 2 * ((E * dE ** 2).sum() + (F * dF ** 2).sum())
        dxb[:, k] = -w[k] * (E * dE).sum(1) - 2 * w[k] * (F * dF).sum(1)
    grad[2 + d:] = dxb.ravel()
    return _nll_from_v(V, y, v, vt, N, m), grad


def evaluate(x, t, theta, m, xs):
    """every long-double value a case is compared with"""
    f, g = nll_grad(x, t, theta, m)
    mean, var = Predictor(x, t, theta, m).predict(xs)
    return {"nll": f, "grad": g, "mean": mean, "var": var}


# ------------------------------------------------------------------------------------------------
# the float64 CPU evaluation rho_ref is measured on
# ------------------------------------------------------------------------------------------------
def woodbury_predict(x, tc, theta, m, xs):
    """(mean* - mean(t), var*) by a numpy / LAPACK transcription of the Woodbury algebra: no N x N matrix"""
    x = np.asarray(x, dtype=float)
    d = x.shape[1]
    th_gc, xb = orc.spgp_split(theta, d, m)
    v, vt = np.exp(th_gc[0]), np.exp(th_gc[1])
    Knm, Km = orc.gram_ij(x, xb, th_gc), orc.gram_ij(xb, xb, th_gc)
    Lm = cholesky(Km + 1e-5 * np.eye(m), lower=True)
    lam = v + vt - (solve_triangular(Lm, Knm.T, lower=True) ** 2).sum(0)
    B = Km + 1e-5 * np.eye(m) + (Knm.T / lam).dot(Knm)
    Lb = cholesky(B, lower=True)
    beta = np.linalg.solve(B, (Knm.T / lam).dot(tc))
    Ks = orc.gram_ij(xs, xb, th_gc)
    mean = Ks.dot(beta)
    var = v + vt - (solve_triangular(Lm, Ks.T, lower=True) ** 2).sum(0) + (solve_triangular(Lb, Ks.T, lower=True) ** 2).sum(0)
    return mean, var


def evaluate_f64(x, t, theta, m, xs=None):
    out = {"nll": orc.spgp_nll(x, t, theta, m), "grad": orc.spgp_nll_grad(x, t, theta, m)}
    if xs is not None:
        out["mean"], out["var"] = woodbury_predict(x, t, theta, m, xs)
    return out


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def distances(got, want, d, vvt):
    """{group: scaled distance of got from want} over the keys of `got` (each must be in `want`): "nll", "grad", "mean", "var", and any
    other key as a matrix scaled by its max-norm.  vvt = v + vt."""
    out = {}
    for key in got:
        g, w = np.asarray(got[key]).astype(LD), np.asarray(want[key]).astype(LD)
        if g.shape != w.shape:
            raise ValueError("%s: shape %r against %r" % (key, g.shape, w.shape))
        diff = np.abs(g - w)
        if key == "nll":
            out["nll"] = diff / np.abs(w)
        elif key == "grad":
            out["log v"] = diff[0] / np.abs(w[0])
            out["log vt"] = diff[1] / np.abs(w[1])
            for k in range(d):
                out["log w_%d" % k] = diff[2 + k] / np.abs(w[2 + k])
            out["xb"] = diff[2 + d:].max() / np.abs(w[2 + d:]).max()
        elif key == "var":
            out["var"] = diff.max() / LD(vvt)
        else:
            out[key] = diff.max() / np.abs(w).max()
    return {k: float(r) for k, r in out.items()}


def rho_ref(ref, want, d, vvt):
    return max(distances(ref, want, d, vvt).values())


def bound(rho, margin=MARGIN):
    return margin * max(rho, FLOOR)


def assert_within(got, want, rho, d, vvt, margin=MARGIN, what=""):
    """every group of `got` within margin * max(rho, FLOOR) of `want`; returns the distances"""
    dist = distances(got, want, d, vvt)
    lim = bound(rho, margin)
    bad = ["%s %.3e" % (k, r) for k, r in dist.items() if not r <= lim]
    assert not bad, "%s: beyond %g * max(rho_ref = %.3e, %.3e) = %.3e: %s" % (what, margin, rho, FLOOR, lim, ", ".join(bad))
    return dist


def vvt_of(theta):
    return float(np.exp(theta[0]) + np.exp(theta[1]))
