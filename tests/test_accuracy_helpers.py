"""The backward-error metrics of tests/_accuracy.py can see the defects the GPU tests (tests/test_backward_error.py) are meant to catch.

Starting from LAPACK's own factor and solves of a recipe Gram matrix at N = 2300 (three 1024-column panels, the last one ragged), the clean
results pass the bounds the GPU tests apply, and each planted defect -- far below what the forward comparisons against the oracle can see
(alpha at 1e-6 max|beta|, K^-1 at 1e-7 max|K^-1|) -- fails them.  The defects are made the way a kernel would make them: a right-looking
blocked factorisation (128-column blocks) with one tile's update short of a rank-16 contribution, a blocked forward substitution with one
diagonal block's explicit inverse slightly wrong."""
import numpy as np
import pytest
import scipy.linalg

import _accuracy as acc
from oracle import oracle as orc

N, D = 2300, 3
NB = 128


@pytest.fixture(scope="module")
def problem():
    x, _t, _xs, theta = acc.recipe(N, D)
    K = orc.gram(x, theta)
    L = acc.lapack_chol(K)
    B = np.random.RandomState(3).randn(N, 4)
    return K, L, B


def _blocked_chol(K, skip=None):
    """right-looking Cholesky by 128-column blocks (LAPACK on the diagonal blocks, the panel by a triangular solve, the trailing update
    as one GEMM).  skip = (k0, r0, c0): the update of trailing tile (r0, c0) (and its mirror) misses L[:, k0:k0+16] L[:, k0:k0+16]^T."""
    A = np.array(K)
    n = A.shape[0]
    for b0 in range(0, n, NB):
        b1 = min(n, b0 + NB)
        A[b0:b1, b0:b1] = np.linalg.cholesky(A[b0:b1, b0:b1])
        if b1 == n:
            break
        P = scipy.linalg.solve_triangular(A[b0:b1, b0:b1], A[b1:, b0:b1].T, lower=True).T
        A[b1:, b0:b1] = P
        A[b1:, b1:] -= P.dot(P.T)
        if skip is not None and b0 <= skip[0] < b1:
            k0, r0, c0 = skip
            Pr = A[r0:r0 + NB, k0:k0 + 16]
            Pc = A[c0:c0 + NB, k0:k0 + 16]
            A[r0:r0 + NB, c0:c0 + NB] += Pr.dot(Pc.T)
            if r0 != c0:
                A[c0:c0 + NB, r0:r0 + NB] += Pc.dot(Pr.T)
    return np.tril(A)


def _blocked_trsv(L, B, bad_block=None, eps=1e-10):
    """forward substitution by 128-row blocks; block bad_block is solved with an explicit inverse of its diagonal block whose entries
    carry relative errors of eps"""
    Y = np.array(B, dtype=float)
    n = L.shape[0]
    for b0 in range(0, n, NB):
        b1 = min(n, b0 + NB)
        if b0:
            Y[b0:b1] -= L[b0:b1, :b0].dot(Y[:b0])
        if b0 // NB == bad_block:
            Dinv = scipy.linalg.solve_triangular(L[b0:b1, b0:b1], np.eye(b1 - b0), lower=True)
            Dinv *= 1.0 + eps * np.random.RandomState(1).uniform(-1, 1, Dinv.shape)
            Y[b0:b1] = Dinv.dot(Y[b0:b1])
        else:
            Y[b0:b1] = scipy.linalg.solve_triangular(L[b0:b1, b0:b1], Y[b0:b1], lower=True)
    return Y


def _factor_ok(L, K, base):
    off, dg = acc.chol_backward_error(L, K)
    return off <= acc.bound(base[0]) and dg <= acc.bound(base[1]) and off <= N * acc.U, (off, dg)


def test_clean_factors_pass(problem):
    K, L, _B = problem
    base = acc.chol_backward_error(L, K)
    assert base[0] < N * acc.U and base[1] < N * acc.U, base          # LAPACK's own factor, under the rigorous ceiling
    assert _factor_ok(L, K, base)[0]
    ok, got = _factor_ok(_blocked_chol(K), K, base)                      # a different, correct order of the same arithmetic
    assert ok, (got, base)


def test_one_entry_of_the_third_panel_off_by_1e_11_fails(problem):
    K, L, _B = problem
    base = acc.chol_backward_error(L, K)
    Lp = L.copy()
    c = 2048 + 37                                                        # the third panel's columns are 2048 ..
    i = c + int(np.argmax(np.abs(L[c:, c])))                             # its largest entry in that column
    Lp[i, c] *= 1.0 + 1e-11
    ok, got = _factor_ok(Lp, K, base)
    assert not ok, (got, base)


def test_tile_without_a_rank_16_contribution_fails(problem):
    """the update by the second panel's last block of the diagonal tile at rows 2048..2175 -- the first tile of the third panel -- misses
    columns 1920..1935"""
    K, L, _B = problem
    base = acc.chol_backward_error(L, K)
    Lm = _blocked_chol(K, skip=(1920, 2048, 2048))
    ok, got = _factor_ok(Lm, K, base)
    assert not ok, (got, base)


def test_clean_solves_pass(problem):
    _K, L, B = problem
    Y = acc.lapack_trsv(L, B)
    base = acc.trsv_backward_error(L, Y, B)
    assert base < N * acc.U, base
    assert acc.trsv_backward_error(L, _blocked_trsv(L, B), B) <= acc.bound(base)
    Z = acc.lapack_trsv(L, Y, trans=True)
    zb = acc.trsv_backward_error(L, Z, Y, trans=True)
    assert zb < N * acc.U, zb


def _most_visible(L, Y, B, trans):
    """the entry whose relative change moves the componentwise residual most: |L_ii Y_ij| / (|op(L)| |Y| + |B|)_ij largest"""
    A = np.abs(L.T if trans else L)
    share = np.abs(np.diag(L))[:, None] * np.abs(Y) / (A.dot(np.abs(Y)) + np.abs(B))
    return np.unravel_index(int(np.argmax(share)), Y.shape), float(share.max())


@pytest.mark.parametrize("trans", [False, True])
def test_one_entry_of_a_solve_off_by_1e_12_fails(problem, trans):
    """L^-1 B (the forward sweep) and L^-T (L^-1 B) (the backward sweep of K^-1 B): one entry off by 1e-12 relative"""
    _K, L, B = problem
    Y = acc.lapack_trsv(L, B)
    if trans:
        B, Y = Y, acc.lapack_trsv(L, Y, trans=True)
    base = acc.trsv_backward_error(L, Y, B, trans=trans)
    (i, j), share = _most_visible(L, Y, B, trans)
    assert share > 0.1
    Yp = Y.copy()
    Yp[i, j] *= 1.0 + 1e-12
    got = acc.trsv_backward_error(L, Yp, B, trans=trans)
    assert got > acc.bound(base), (got, base, (i, j))


def test_block_solved_with_a_perturbed_inverse_fails(problem):
    _K, L, B = problem
    base = acc.trsv_backward_error(L, acc.lapack_trsv(L, B), B)
    Yb = _blocked_trsv(L, B, bad_block=13)
    got = acc.trsv_backward_error(L, Yb, B)
    assert got > acc.bound(base), (got, base)


def test_inverse_residual_sees_a_perturbed_inverse():
    """inverse_residual on a small SPD matrix: LAPACK's inverse passes its own bound, an inverse with one entry off by 1e-10 does not"""
    rng = np.random.RandomState(4)
    A = rng.randn(300, 300)
    K = A.dot(A.T) / 300 + np.eye(300)
    X = acc.lapack_inverse(K)
    base = acc.inverse_residual(K, X)
    assert base < 300 * acc.U
    Xp = X.copy()
    Xp[17, 17] *= 1.0 + 1e-10
    assert acc.inverse_residual(K, Xp) > acc.bound(base)


def test_metric_rejects_a_factor_with_an_upper_triangle(problem):
    K, L, _B = problem
    Lu = L.copy()
    Lu[5, 900] = 1e-300
    with pytest.raises(AssertionError):
        acc.chol_backward_error(Lu, K)
