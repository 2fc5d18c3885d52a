"""The SPGP model as a dense predictor over its pseudo-inputs: the seeded models and batches of tests/test_spgp_pseudo_model.py (host) and
tests/test_spgp_pseudo.py (device), the NumPy statement of (beta, P), a shim the oracle's propagation functions accept, and the Gauss-Hermite
mixture moments of the predictor.  Host only.

With k(x*) = K(x*, xbar) the plain ARD squared-exponential kernel against the m pseudo-inputs (no +vt anywhere: a pseudo-input is no
observation), SPGPCovariance's predictor (skgpuppy/Covariance.py:835-863 through GaussianProcess.py:68-80) is
    mean(x*) = k(x*)^T beta + mean(t),    var(x*) = v + vt - k(x*)^T P k(x*),
    Lambda = v + vt - diag(K_NM (K_M + 1e-5 I)^-1 K_MN),  B~ = K_M + 1e-5 I + K_MN Lambda^-1 K_NM,
    beta = B~^-1 K_MN Lambda^-1 t,   P = (K_M + 1e-5 I)^-1 - B~^-1.
P is positive semi-definite in exact arithmetic only; nothing here factors it.

The long-double models of the dense path (tests/_dense_ld.py, _predict_grad_model.py) read a model through (x, theta, Kinv, alpha): they take
(xbar, theta[:2 + d], P, beta) as they are.  The one difference is the reference's "+vt where u equals a training row": _dense_ld's functions
drop it with defect="quirk", _predict_grad_model's Gaussian rows never had it."""
import numpy as np

import _dense_ld as dl

# name: (N, d, m) -- A: two 128-tiles of pseudo-inputs, ragged; B: one tile; C: d > 8 (the other instantiation of every builder and
# reduction), m just over one tile; D: one tile at d = 8, the model of the chunk-seam test (a chunk of 32768 rows is cheap at npad = 128)
MODELS = {"A": (700, 3, 150), "B": (300, 2, 30), "C": (400, 9, 130), "D": (300, 8, 100)}
NQ = 77                     # queries / inputs of the large batch: 77 (d + 2) and 77 (d + 1) are no multiples of 128 for d = 2, 3, 9


def make_model(name):
    """(x, t, theta [2 + d + m d], theta_gc [2 + d], xbar [m, d]): the law of tests/test_gpu_parity.py's ragged SPGP case, seeded per model"""
    N, d, m = MODELS[name]
    rng = np.random.RandomState(9900 + N + d + m)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    th_gc = np.log(np.array([2.0, 0.01] + [0.04] * d))
    xb = rng.uniform(0, 10, (m, d))
    return x, t, np.concatenate([th_gc, xb.ravel()]), th_gc, xb


def se(xi, xj, th_gc):
    """the plain kernel matrix v exp(-1/2 sum_k w_k (xi_k - xj_k)^2) [len(xi), len(xj)], float64"""
    d = np.shape(xi)[1]
    v, w = np.exp(th_gc[0]), np.exp(th_gc[2:2 + d])
    q = np.zeros((len(xi), len(xj)))
    for k in range(d):
        q += w[k] * (np.asarray(xi)[:, k][:, None] - np.asarray(xj)[:, k][None, :]) ** 2
    return v * np.exp(-0.5 * q)


def beta_P(x, t, th_gc, xb):
    """(beta [m], P [m, m]) from the definition, float64 (t as given: it is centred here)"""
    v, vt = np.exp(th_gc[0]), np.exp(th_gc[1])
    tc = np.asarray(t, dtype=float) - np.mean(t)
    m = len(xb)
    Km = se(xb, xb, th_gc) + 1e-5 * np.eye(m)
    Knm = se(x, xb, th_gc)
    Kmi = np.linalg.inv(Km)
    lam = v + vt - np.einsum("ij,jk,ik->i", Knm, Kmi, Knm)
    Bt = Km + (Knm.T / lam).dot(Knm)
    Bi = np.linalg.inv(Bt)
    beta = Bi.dot(Knm.T.dot(tc / lam))
    P = Kmi - Bi
    return beta, 0.5 * (P + P.T)


def predictor(xs, th_gc, xb, beta, P, meant):
    """(mean with meant, var) of the pseudo-basis predictor at xs [M, d]"""
    k = se(xs, xb, th_gc)
    return k.dot(beta) + meant, np.exp(th_gc[0]) + np.exp(th_gc[1]) - np.einsum("ij,jk,ik->i", k, P, k)


class Shim(object):
    """what oracle.exact_propagate / approx_parts / cjh read of a GP, over the pseudo-inputs.  The oracle's scalar kernel keeps the
    reference's +vt on equal arguments: keep u off the pseudo-inputs."""

    def __init__(self, th_gc, xb, beta, P, meant):
        self.x = np.asarray(xb, dtype=float)
        self.n, self.d = self.x.shape
        self.theta_min = np.asarray(th_gc, dtype=float)
        self.Kinv = np.ascontiguousarray(P, dtype=float)
        self._beta = np.asarray(beta, dtype=float)
        self.meant = meant

    def beta(self):
        return self._beta


def full_sigma(d, seed):
    """a full SPD input covariance (diagonal at d = 1)"""
    rng = np.random.RandomState(seed)
    A = rng.uniform(-0.3, 0.3, (d, d))
    return A.dot(A.T) + 0.05 * np.eye(d)


def inputs(name, b):
    """U [b, d] on the 2^-20 grid inside the data (random: off every pseudo-input), the first rows of the model's NQ"""
    _N, d, _m = MODELS[name]
    rng = np.random.RandomState(4100 + d)
    return dl._grid(rng.uniform(1, 9, (NQ, d)))[:b].copy()


def sigma_runs(d, b, seed=0):
    """per-input Sigma [b, d, d]: runs of 7 bit-equal ones followed by 3 distinct ones, repeated -- gpx_propagate_exact_many takes its matrix
    path for a run of five or more and its pair path for the rest"""
    out = np.empty((b, d, d))
    for i in range(b):
        blk, r = divmod(i, 10)
        out[i] = full_sigma(d, 7000 + seed + (100 * blk if r < 7 else 100 * blk + r))
    return out


def gauss_hermite_moments(mu_var, u, Sigma, order=24):
    """(mean, variance) of the mixture sum_s wq_s N(mu(x_s), var(x_s)) over the tensor Gauss-Hermite rule x_s = u + sqrt(2) chol(Sigma) z_s:
    E[mu], E[var + mu^2] - E[mu]^2.  mu_var(X) -> (mu [S], var [S])."""
    d = len(u)
    z1, w1 = np.polynomial.hermite.hermgauss(order)
    w1 = w1 / w1.sum()
    z = np.stack(np.meshgrid(*([z1] * d), indexing="ij"), -1).reshape(-1, d)
    wq = np.stack(np.meshgrid(*([w1] * d), indexing="ij"), -1).reshape(-1, d).prod(axis=1)
    X = np.asarray(u)[None, :] + np.sqrt(2.0) * z.dot(np.linalg.cholesky(Sigma).T)
    mu, var = mu_var(X)
    mean = wq.dot(mu)
    return mean, wq.dot(var + (mu - mean) ** 2)
