"""A float64 numpy statement of the batched Exact propagation's matrix path (gpx_propagate_exact_many; scikit-gpuppy_amd/csrc/propagate.hip,
exact_weight_kernel / exact_many_build_kernel / exact_many_finish_kernel, and the host constants of propagate_api.hip).  Host only.

For the inputs u that share one Sigma the pair weight of Girard's exact variance factorises.  With a_i = u - x_i, A = Sigma + W^-1 / 2,
Ls = sym(2 W - A^-1) (tests/_dense_ld.exact_constants) and F_i = v, or v + vt iff x_i == u elementwise,

    L_ij / nc2 = F_i F_j exp(-1/2 a_i^T W a_i - 1/2 a_j^T W a_j + 1/8 (a_i + a_j)^T Ls (a_i + a_j))
               = h_i h_j E_ij,     h_i = F_i exp(-1/4 a_i^T A^-1 a_i),     E_ij = exp(-1/8 (x_i - x_j)^T Ls (x_i - x_j))

(2 a_i^T Ls a_j = a_i^T Ls a_i + a_j^T Ls a_j - (a_i - a_j)^T Ls (a_i - a_j); a_i - a_j = x_j - x_i; -W / 2 + Ls / 4 = -A^-1 / 4).  The four
stages, as the device runs them:
  1. each quadratic form on coordinates transformed by the eigenvectors of its matrix, M = V diag(lam) V^T -> T = diag(sqrt|lam|) V^T,
     s = sign(lam): z^T M z = sum_k s_k ((T z)_k)^2, formed from DIFFERENCES of the transformed coordinates of x - x_0 and u - x_0;
  2. Lo = the j <= i half of (Kinv - beta beta^T) o E, the diagonal halved, zero above it;
  3. H_ij = F_ij exp(-sum_k s_k (uh_ik - xh_jk)^2), and the mean sum_j beta_j C_ij nc1 exp(a^T Delta^-1 a / 2) as exact_build_kernel has it;
  4. Y = H Lo^T, S_i = 2 sum_j Y_ij H_ij, var_i = (v + vt) - nc2 S_i - mean_i^2.

`defect=` plants one seeded defect (tests/test_exact_many_model.py): "diag_full" the diagonal of Lo is not halved, "no_E" E = 1,
"abs_sign" every s_k is taken as +1, "no_quirk" F = v and C without vt on exact equality."""
import numpy as np

import _dense_ld as dl

ROWS = 64


def square_transform(M, scale):
    """(T [d, d], s [d]) of scale * sym(M)"""
    M = scale * (np.asarray(M, dtype=np.float64) + np.asarray(M, dtype=np.float64).T) / 2
    lam, V = np.linalg.eigh(M)
    return np.sqrt(np.abs(lam))[:, None] * V.T, np.sign(lam)


def weight_matrix(x, Kinv, beta, Ls, defect=None):
    """Lo [N, N]"""
    N = len(x)
    T, s = square_transform(Ls, 0.125)
    if defect == "abs_sign":
        s = np.abs(s)
    xt = (x - x[0]).dot(T.T)
    Lo = np.zeros((N, N))
    for i0 in range(0, N, ROWS):
        i1 = min(N, i0 + ROWS)
        D = xt[i0:i1, None, :] - xt[None, :, :]
        E = np.ones((i1 - i0, N)) if defect == "no_E" else np.exp(-(s * D * D).sum(-1))
        Lo[i0:i1] = (Kinv[i0:i1] - np.outer(beta[i0:i1], beta)) * E      # the device reads the j <= i half of its K^-1
    Lo = np.tril(Lo)
    if defect != "diag_full":
        Lo[np.arange(N), np.arange(N)] *= 0.5
    return Lo


def moments(x, theta, Kinv, alpha, U, Sigma, defect=None):
    """(mean [B] without meant, var [B]) of the inputs U [B, d] under one Sigma"""
    x, U = np.asarray(x, dtype=np.float64), np.atleast_2d(np.asarray(U, dtype=np.float64))
    N, d = x.shape
    v, vt, w = dl.params(theta, d, np.float64)
    S = np.asarray(Sigma, dtype=np.float64)
    Ls, dd, nc1, nc2 = dl.exact_constants(w, S, np.float64)
    Ainv = dl.small_inverse(S + np.diag(1 / (2 * w)))
    Kinv, beta = np.asarray(Kinv, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    Lo = weight_matrix(x, Kinv, beta, Ls, defect)
    T, s = square_transform(Ainv, 0.25)
    if defect == "abs_sign":
        s = np.abs(s)
    xh, uh = (x - x[0]).dot(T.T), (U - x[0]).dot(T.T)
    qa = (s * (uh[:, None, :] - xh[None, :, :]) ** 2).sum(-1)
    same = (x[None, :, :] == U[:, None, :]).all(-1) & (defect != "no_quirk")
    H = np.where(same, v + vt, v) * np.exp(-qa)
    a = U[:, None, :] - x[None, :, :]
    qw, qd = (w * a * a).sum(-1), (dd * a * a).sum(-1)
    C = v * np.exp(-0.5 * qw) + vt * same
    mean = (C * nc1 * np.exp(0.5 * qd)).dot(beta)
    Y = H.dot(Lo.T)
    Ssum = 2 * (Y * H).sum(1)
    return mean, (v + vt) - nc2 * Ssum - mean * mean
