"""Backward-error metrics for the factor, the triangular solves and K^-1, computed on the host in fp64 and in row blocks.

Backward error does not depend on the conditioning of K: for any Cholesky |L L^T - K|_ij <= gamma_{N+1} sqrt(K_ii K_jj), so a check of a
device factor against its own input -- and of the solves against the device's own L -- sits at rounding level at every size.  Each metric
is also evaluated on LAPACK's answer for the same input (numpy.linalg.cholesky, scipy.linalg.solve_triangular / cho_solve): that value is
the baseline a device result is judged against (bound: 16 x max(LAPACK, u), and for the factor also the rigorous ceiling N u).

Row blocks bound host memory: besides the inputs, no temporary is larger than ROWS x N doubles.  Host BLAS stays on at most 16 threads.
"""
import contextlib
import hashlib

import numpy as np
import scipy.linalg

U = 2.0 ** -53      # unit roundoff of fp64
ROWS = 512          # row block of every metric
FACTOR = 16.0       # a device metric may exceed LAPACK's (or u) by this factor


@contextlib.contextmanager
def blas_threads(n=16):
    """host BLAS on at most n threads (a GPU host allows 16; threadpoolctl when present, the environment otherwise).  Only ever lowers the
    count: OpenBLAS crashes when raised above the thread count it started with."""
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
    except ImportError:          # pragma: no cover
        yield
        return
    if all(i["num_threads"] <= n for i in threadpool_info() if i.get("user_api") == "blas"):
        yield
        return
    with threadpool_limits(limits=n, user_api="blas"):
        yield


def recipe(N, d, M=0):
    """the suite's GP recipe (tests/test_gpu_parity.py, _recipe): x uniform in [0, 10]^d, v = 2, vt = 0.01, w = 0.04"""
    rng = np.random.RandomState(20240 + N + d)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (M, d))
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    return x, t, xs, theta


def digest(a):
    """hash of an array's bytes: bit-identity of two results without keeping both"""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _check_lower(L, i0, i1):
    """the strict upper triangle of rows [i0, i1) is exactly zero (the metrics below read it as part of the products)"""
    blk = L[i0:i1]
    up = np.triu(blk[:, i0:i1], 1)
    if np.any(up) or np.any(blk[:, i1:]):
        raise AssertionError("factor has non-zero entries above the diagonal in rows [%d, %d)" % (i0, i1))


def chol_backward_error(L, K):
    """(max_{i>=j} |(L L^T - K)_ij| / sqrt(K_ii K_jj),  max_i |diag(L L^T)_i - K_ii| / K_ii).
    The first is N^3 / 3 flops over the lower triangle, the second O(N^2).  Only the lower triangle of K is read."""
    n = L.shape[0]
    assert L.shape == (n, n) and K.shape == (n, n)
    dK = np.ascontiguousarray(np.diag(K)).astype(np.float64)
    if not np.all(dK > 0):
        raise AssertionError("K has a non-positive diagonal entry")
    s = np.sqrt(dK)
    worst = 0.0
    with blas_threads():
        for i0 in range(0, n, ROWS):
            i1 = min(n, i0 + ROWS)
            _check_lower(L, i0, i1)
            R = L[i0:i1, :i1].dot(L[:i1, :i1].T)
            R -= K[i0:i1, :i1]
            np.abs(R, out=R)
            R /= s[i0:i1, None]
            R /= s[None, :i1]
            tail = R[:, i0:i1]
            tail[np.triu_indices(i1 - i0, 1)] = 0.0        # lower triangle only
            worst = max(worst, float(R.max()))
        dg = np.einsum("ij,ij->i", L, L)                    # diag(L L^T), row by row
    dworst = float(np.max(np.abs(dg - dK) / dK))
    return worst, dworst


def trsv_backward_error(L, Y, B, trans=False):
    """componentwise backward error of a triangular solve op(L) Y = B, op(L) = L (trans=False) or L^T:
    max_i |(op(L) Y - B)_i| / (|op(L)| |Y| + |B|)_i over every entry i of every column.  Y, B: (N,) or (N, k)."""
    n = L.shape[0]
    Y2 = Y.reshape(n, -1)
    B2 = B.reshape(n, -1)
    aY = np.abs(Y2)
    worst = 0.0
    with blas_threads():
        for i0 in range(0, n, ROWS):
            i1 = min(n, i0 + ROWS)
            _check_lower(L, i0, i1)
            if not trans:
                A = L[i0:i1, :i1]
                R = A.dot(Y2[:i1]) - B2[i0:i1]
                D = np.abs(A).dot(aY[:i1]) + np.abs(B2[i0:i1])
            else:
                A = L[i0:, i0:i1]                            # rows i0.. of column block i0:i1 = rows i0:i1 of L^T
                R = A.T.dot(Y2[i0:]) - B2[i0:i1]
                D = np.abs(A).T.dot(aY[i0:]) + np.abs(B2[i0:i1])
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.where(D > 0, np.abs(R) / np.where(D > 0, D, 1.0), np.where(R != 0, np.inf, 0.0))
            worst = max(worst, float(q.max()))
    return worst


def inverse_residual(K, X):
    """max |K X - I| / (||K||_inf ||X||_inf)"""
    n = K.shape[0]
    worst = 0.0
    with blas_threads():
        for i0 in range(0, n, ROWS):
            i1 = min(n, i0 + ROWS)
            R = K[i0:i1].dot(X)
            R[np.arange(i1 - i0), np.arange(i0, i1)] -= 1.0
            worst = max(worst, float(np.abs(R).max()))
        nk = float(np.abs(K).sum(1).max())
        nx = float(np.abs(X).sum(1).max())
    return worst / (nk * nx)


# ---- LAPACK's answers for the same inputs: the baselines --------------------------------------------------------------------------
def lapack_chol(K):
    with blas_threads():
        return np.linalg.cholesky(K)


def lapack_trsv(L, B, trans=False):
    with blas_threads():
        return scipy.linalg.solve_triangular(L, B, lower=True, trans=1 if trans else 0, check_finite=False)


def lapack_inverse(K):
    with blas_threads():
        return scipy.linalg.cho_solve(scipy.linalg.cho_factor(K, lower=True, check_finite=False), np.eye(K.shape[0]), check_finite=False)


def kappa2(K, L, iters=8, block=8):
    """2-norm condition number of SPD K (L: its LAPACK factor): lambda_max of K and of K^-1 = L^-T L^-1 by a few steps of subspace
    iteration on `block` vectors (Rayleigh quotients: lower bounds that converge fast for these spectra).  Two digits are plenty: it is
    reported, not asserted."""
    n = K.shape[0]
    with blas_threads():
        if n <= 1200:
            ev = np.linalg.eigvalsh(K)
            return float(ev[-1] / ev[0])

        def top(apply):
            V = np.linalg.qr(np.random.RandomState(0).randn(n, block))[0]
            for _ in range(iters):
                V = np.linalg.qr(apply(V))[0]
            return float(np.linalg.eigvalsh(V.T.dot(apply(V)))[-1])

        lmax = top(K.dot)
        imax = top(lambda V: lapack_trsv(L, lapack_trsv(L, V), trans=True))
    return lmax * imax


def bound(lapack_value):
    """the acceptance bound of a device factor / solve metric"""
    return FACTOR * max(lapack_value, U)
