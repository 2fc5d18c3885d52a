"""Backward error of the device factor, solves and K^-1 on every schedule (-m gpu), against the device's own inputs.

The forward comparisons with the oracle elsewhere in the suite are as loose as the conditioning of K makes them (alpha at 1e-6 max|beta|,
K^-1 at 1e-7 max|K^-1|): a deterministic defect of relative size 1e-11 .. 1e-7 in one panel of the look-ahead schedule passes them.
Backward error does not depend on kappa(K): |L L^T - K|_ij <= gamma_{N+1} sqrt(K_ii K_jj) for any Cholesky.  So here

  A  the gpx_fit factor along a size ladder is checked against the device Gram it factors,
  B  every factorisation schedule (child processes: the knobs are read once per process) likewise at N = 12288 / 9000,
  C  designed SPD matrices (kappa up to 1e12, graded, a tiny Schur complement on a panel boundary) go through gpx_fit_matrix,
  D  L(4^k K) = 2^k L(K) is checked to a few ulp,
  E  gpx_spd_inverse (panel factor, small dataflow kernel, chol_rec; the launch chain) by its residual K X - I,
  F  the solves, estimate_many (more than one chunk of queries included) and K^-1 against the device's own L (which takes kappa(K)
     out of the comparison).

Bounds (tests/_accuracy.py): a factor / solve / inverse metric <= 16 x max(LAPACK's value for the same input, u), a factor metric also
<= N u.  The forward quantities of F have fixed tolerances, 10x the worst value measured on an unmodified build and at least 100x tighter
than the oracle-parity tolerance of the same quantity (measured worst values are quoted with each constant).  Fits are bit-reproducible,
so the margins hold on every box.  Each case prints one `ACC` line: what, device metric, LAPACK metric, bound, kappa_2(K), bit-identity.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from skgpuppy_amd.Covariance import _MatrixModel

import _accuracy as acc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "_backward_error_worker.py")
U = acc.U

# (N, d) of the ladder: one panel unpadded / padded, a look-ahead panel of a single 128-block, ragged last panels, square launches for the
# first panel and the tail, CU reservation and the trapezoid hand-off from C3 size on
LADDER = [(1000, 3), (1024, 4), (1025, 5), (2200, 3), (4224, 6), (8200, 6), (9000, 7), (12288, 8), (16384, 8)]
D_OF = dict(LADDER)

_BASE = {}      # (N, d) -> LAPACK metrics of the recipe problem and kappa_2(K)


def _report(section, what, dev, lap, bnd, kappa=float("nan"), same=""):
    print("ACC | %s | %s | %.3e | %.3e | %.3e | %.2e | %s" % (section, what, dev, lap, bnd, kappa, same))


def _dev_gram(x, theta):
    """gpx_gram(x, x, theta, add_diag = vt): the matrix gpx_fit factors.  Its own accuracy is held entry by entry to a long-double model
    within a derived bound by tests/test_gauss_gram.py (every d, both tile paths, the subnormal range, every launch mode of the device
    entry points); test_gram_golden adds six cases of the reference at rtol 1e-13."""
    return sk.GaussianCovariance().cov_matrix(x, theta)


def _chol_of(handle, n):
    out = np.empty((n, n))
    _gpx.check(_gpx.lib.gpx_chol(handle, _gpx.ptr(out)), "gpx_chol")
    return out


def _lapack_factor_metrics(K, with_kappa=True):
    L = acc.lapack_chol(K)
    m = acc.chol_backward_error(L, K)
    kappa = acc.kappa2(K, L) if with_kappa else float("nan")
    return m, kappa


def _baseline(N, d, K):
    if (N, d) not in _BASE:
        _BASE[(N, d)] = _lapack_factor_metrics(K)
    return _BASE[(N, d)]


def _assert_factor(what, got, base, N):
    off, dg = got
    assert off <= acc.bound(base[0]) and dg <= acc.bound(base[1]), (what, got, base)
    assert off <= N * U, (what, off, N * U)


# ------------------------------------------------------------------------------------------------
# A: the gpx_fit factor along a size ladder
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(2200, 3), (9000, 7)])
def test_fit_matrix_of_the_device_gram_is_the_fit(N, d):
    """gpx_fit_matrix on the device Gram gives gpx_fit's factor bit for bit (same padded copy, same schedule): measuring gpx_fit's factor
    against gpx_gram's matrix measures it against the matrix it factored."""
    x, t, _xs, theta = acc.recipe(N, d)
    K = _dev_gram(x, theta)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    L1 = gp._dev().chol()
    gp._dev().close()
    m = _MatrixModel(K, None)
    L2 = _chol_of(m.handle, N)
    m.close()
    assert np.array_equal(L1, L2), np.abs(L1 - L2).max()


@pytest.mark.parametrize("N,d", LADDER)
def test_fit_factor_backward_error(N, d):
    x, t, _xs, theta = acc.recipe(N, d)
    K = _dev_gram(x, theta)
    base, kappa = _baseline(N, d, K)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    assert gp._dev().jitter() == 0.0
    L = gp._dev().chol()
    gp._dev().close()
    _gpx.lib.gpx_pool_trim()
    got = acc.chol_backward_error(L, K)
    _report("A", "gpx_fit N=%d d=%d default" % (N, d), got[0], base[0], acc.bound(base[0]), kappa)
    _report("A", "gpx_fit N=%d d=%d default (diag)" % (N, d), got[1], base[1], acc.bound(base[1]), kappa)
    _assert_factor("N=%d" % N, got, base, N)


# ------------------------------------------------------------------------------------------------
# B: every factorisation schedule, each in a fresh process
# ------------------------------------------------------------------------------------------------
SCHEDULES = [
    ("default", {}, 12288),
    ("square launches nowhere", {"GPX_SQK_FROM": "-1"}, 12288),
    ("square launches everywhere, no CU reservation", {"GPX_SQK_FROM": "0", "GPX_RESERVE_CUS": "0"}, 12288),
    ("narrow and bulk as two launches", {"GPX_TRAP": "0"}, 12288),
    ("substitution after the factorisation", {"GPX_FIT_RIDE": "0"}, 12288),
    ("serialised streams", {"GPX_CONCURRENT_STREAMS": "0"}, 12288),
    ("one priority class", {"GPX_SIDE_PRIO": "0", "GPX_BLK_PRIO": "0"}, 12288),
    ("default", {}, 9000),
    ("whole matrix as one dataflow launch", {"GPX_DFLOW_MAX_BLOCKS": "1000"}, 9000),
]


def _child(args, extra, timeout=300):
    env = dict(os.environ)
    env.update(extra)
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args, extra, r.returncode, r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_every_factorisation_schedule():
    """The schedules differ in how the trailing updates are cut into launches and which stream runs what; each must factor K to rounding
    level.  Bit-identity with the default schedule is reported, not asserted."""
    res, default = [], {}
    for name, extra, N in SCHEDULES:
        d = D_OF[N]
        r = _child(["fit", N, d] + ([default[N]["hash"]] if N in default else []), extra)
        assert r["jitter"] == 0.0, (name, r)
        if name == "default":
            default[N] = r
        elif r["hash"] == default[N]["hash"]:
            r["offdiag"], r["diag"] = default[N]["offdiag"], default[N]["diag"]
        res.append((name, N, d, r))
    failures = []
    for name, N, d, r in res:
        x, _t, _xs, theta = acc.recipe(N, d)
        base, kappa = _baseline(N, d, _dev_gram(x, theta))
        same = "yes" if r["hash"] == default[N]["hash"] else "no"
        _report("B", "N=%d %s" % (N, name), r["offdiag"], base[0], acc.bound(base[0]), kappa, same)
        try:
            _assert_factor("%s N=%d" % (name, N), (r["offdiag"], r["diag"]), base, N)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------
# C: designed SPD matrices through gpx_fit_matrix (host-made: the input is exact)
# ------------------------------------------------------------------------------------------------
FAMILIES = ["spectral kappa=1e2", "spectral kappa=1e8", "spectral kappa=1e12", "graded D A D", "small Schur complement"]
_Q = {}


def _orthogonal(N):
    if N not in _Q:
        with acc.blas_threads():
            Q, R = np.linalg.qr(np.random.RandomState(N).randn(N, N))
        _Q[N] = Q * np.sign(np.diag(R))
    return _Q[N]


def _spectral(N, kappa):
    """Q diag(lambda) Q^T, lambda geometric from 1 to 1 / kappa, symmetrised"""
    lam = np.logspace(0.0, -np.log10(kappa), N)
    Q = _orthogonal(N)
    with acc.blas_threads():
        K = (Q * lam).dot(Q.T)
    K += K.T
    K *= 0.5
    return K


def _designed(family, N):
    if family.startswith("spectral"):
        return _spectral(N, float(family.split("=")[1]))
    if family == "graded D A D":
        s = 10.0 ** np.random.RandomState(N + 1).uniform(-3.0, 3.0, N)     # D log-uniform over [1e-3, 1e3]
        K = _spectral(N, 1e2)
        K *= s[:, None]
        K *= s[None, :]
        return K
    # small Schur complement: K = M M^T with M the factor of a well-conditioned matrix whose trailing part from column c on is scaled by
    # 1e-5 -- the Schur complement at column c (a panel boundary) is 1e-10 relative to K
    c = 1024 if N > 1024 else 512
    M = acc.lapack_chol(_spectral(N, 2.0))
    M[c:, c:] *= 1e-5
    with acc.blas_threads():
        K = M.dot(M.T)
    K += K.T
    K *= 0.5
    return K


# Measured finding (unmodified build): the device factor's backward error sits on the diagonal 128-tiles and grows with the number of
# trailing updates a tile has received -- at N = 9000 on the Q diag(lambda) Q^T family with kappa = 1e2, 12 u in the first block row, 50 .. 80 u
# from block row 16 on, median tile 1.9 u -- while LAPACK's stays at <= 6 u (median 0.1 u).  It is spread over every panel, schedule-
# independent (section B: all schedules bit-identical) and far under the rigorous ceiling N u (9000 u), so it is no single-tile defect but
# the accumulation of the device's trailing updates; against LAPACK it is largest where LAPACK's own error is smallest, on matrices with
# small off-diagonal entries: 14.2 x on spectral kappa = 1e2, 16.4 x on graded D A D (same A) at N = 9000.  The graded family is held to
# the measured ratio with a margin: GRADED_FACTOR x LAPACK; every other family keeps the 16 x bound.
GRADED_FACTOR = 24.0


@pytest.mark.parametrize("N", [1000, 1025, 3000, 9000])
@pytest.mark.parametrize("family", FAMILIES)
def test_designed_matrices_through_fit_matrix(family, N):
    """All are numerically SPD (LAPACK factors them): the device must factor them without jitter, to the bound (graded D A D: to
    GRADED_FACTOR x LAPACK, see above)."""
    K = _designed(family, N)
    L = acc.lapack_chol(K)                      # precondition: numerically SPD
    base = acc.chol_backward_error(L, K)
    if family.startswith("spectral"):
        kappa = float(family.split("=")[1])
    else:
        kappa = acc.kappa2(K, L) if N <= 3000 else float("nan")     # (reported only; at 9000 it costs more than the test)
    del L
    m = _MatrixModel(K, None)
    jit = m.jitter()
    Ld = _chol_of(m.handle, N)
    m.close()
    got = acc.chol_backward_error(Ld, K)
    factor = GRADED_FACTOR if family == "graded D A D" else acc.FACTOR
    _report("C", "N=%d %s" % (N, family), got[0], base[0], factor * max(base[0], U), kappa)
    assert jit == 0.0, (family, N, jit)
    assert got[0] <= factor * max(base[0], U) and got[1] <= factor * max(base[1], U), (family, N, got, base)
    assert got[0] <= N * U, (family, N, got[0])


# ------------------------------------------------------------------------------------------------
# D: exact scale equivariance
# ------------------------------------------------------------------------------------------------
def test_scale_equivariance_of_the_factor():
    """In exact arithmetic L(4^k K) = 2^k L(K), and every step of a Cholesky commutes with a power-of-two scaling except approximations
    whose error depends on the exponent (the leaf's v_rsq_f64 + Newton reciprocal square root, an absolute threshold).  N = 4224: the
    look-ahead schedule with a ragged last panel."""
    N, d = 4224, 6
    x, _t, _xs, theta = acc.recipe(N, d)
    K = _dev_gram(x, theta)
    m = _MatrixModel(K, None)
    L0 = _chol_of(m.handle, N)
    m.close()
    sp = np.spacing(np.abs(L0))
    worst = {}
    for k in (-100, -10, 10, 100):
        m = _MatrixModel(K * 4.0 ** k, None)
        Lk = _chol_of(m.handle, N) * 2.0 ** -k
        assert m.jitter() == 0.0
        m.close()
        ulps = float(np.max(np.abs(Lk - L0) / sp))
        worst[k] = ulps
        _report("D", "N=%d K x 4^%d" % (N, k), ulps * U, 0.0, 4 * U, float("nan"), "yes" if ulps == 0 else "no")
    print("scale equivariance, worst entry in ulp of L(K):", worst)
    assert max(worst.values()) <= 4.0, worst


# ------------------------------------------------------------------------------------------------
# E: the stream-less path, gpx_spd_inverse
# ------------------------------------------------------------------------------------------------
def _spd_inverse(K):
    n = K.shape[0]
    X = np.empty((n, n))
    ld = ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_spd_inverse(_gpx.ptr(K), n, _gpx.ptr(X), ctypes.byref(ld)), "gpx_spd_inverse")
    return X, ld.value


def _lapack_inverse_metrics(K):
    L = acc.lapack_chol(K)
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
    del L
    return acc.inverse_residual(K, acc.lapack_inverse(K)), logdet


LOGDET_RTOL = 1e-14     # measured worst 9.1e-16 (n = 1000); the suite's log det parity with the oracle is rel 1e-9 .. 1e-10


@pytest.mark.parametrize("n,d,extra", [(1000, 4, {}), (3000, 4, {}), (8300, 4, {}), (3000, 4, {"GPX_DFLOW_SMALL": "0"})])
def test_spd_inverse(n, d, extra):
    """n = 1000: one panel (chol_panel_factor); 3000: the small dataflow kernel (9 .. 64 block rows), or with GPX_DFLOW_SMALL=0 the launch
    chain (child process); 8300: chol_rec above 64 block rows."""
    x, _t, _xs, theta = acc.recipe(n, d)
    K = _dev_gram(x, theta)
    base, ld_ref = _lapack_inverse_metrics(K)
    if extra:
        r = _child(["spd_inverse", n, d], extra)
        res, sym, ld = r["residual"], r["symmetric"], r["logdet"]
    else:
        X, ld = _spd_inverse(K)
        res, sym = acc.inverse_residual(K, X), bool(np.array_equal(X, X.T))
    _report("E", "gpx_spd_inverse n=%d %s" % (n, extra or "default"), res, base, acc.bound(base))
    print("log det: device %.17g LAPACK %.17g rel %.3e" % (ld, ld_ref, abs(ld - ld_ref) / abs(ld_ref)))
    assert sym
    assert res <= acc.bound(base), (res, base)
    assert abs(ld - ld_ref) <= LOGDET_RTOL * abs(ld_ref), (ld, ld_ref)


# ------------------------------------------------------------------------------------------------
# F: solves, predictions and K^-1 against the device's own L
# ------------------------------------------------------------------------------------------------
# estimate_many against mean = meant + k* . beta_dev, var = v + vt - ||L_dev^-1 k*||^2, in units of v (the oracle-parity tolerance of the
# suite is rtol 1e-6 / atol 1e-9 v).  Measured worst over all N and M: mean 8.76e-13 v, var 1.28e-14 v (N = 16384, M >= 3071)
MEAN_ATOL_V = 9e-12
VAR_ATOL_V = 1.3e-13
# K^-1 (gpx_kinv, gpx_kinv_rows) against L_dev^-T L_dev^-1 built on the host, relative to max|K^-1| (oracle parity: 1e-7).  Measured
# worst 8.86e-15 (the whole inverse at N = 4224)
KINV_RTOL = 9e-14

SOLVE_N = (1025, 4224, 16384)
PREDICT_N = (2200, 16384)
KINV_N = 4224


@pytest.mark.parametrize("N", [1025, 2200, 4224, 16384])
def test_solves_and_predictions_against_the_device_factor(N):
    """gpx_solve (L^-1 B and K^-1 B for 1, 16, 17 and 33 right-hand sides: the fat-step solver with its inverted 1024-row squares),
    estimate_many (M = 1, 32, 33: the few-right-hand-side sweep; 3071, 3072, 4097: the many-query recursion and the fused row sums of
    gemm_nt_f64_reduce_kernel with full and ragged slabs) and K^-1 (whole and row panels) -- all against the device's own factor."""
    d = D_OF[N]
    x, t, xs, theta = acc.recipe(N, d, 4097)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    L = gp._dev().chol()
    v, vt = np.exp(theta[0]), np.exp(theta[1])
    if N in SOLVE_N:
        rng = np.random.RandomState(N)
        for nrhs in (1, 16, 17, 33):
            B = rng.randn(nrhs, N)
            kb, lb = gp._dev().solve(B, want_linv=True)
            Y, Z = lb.T, kb.T
            base1 = acc.trsv_backward_error(L, acc.lapack_trsv(L, B.T), B.T)
            got1 = acc.trsv_backward_error(L, Y, B.T)
            base2 = acc.trsv_backward_error(L, acc.lapack_trsv(L, Y, trans=True), Y, trans=True)
            got2 = acc.trsv_backward_error(L, Z, Y, trans=True)
            _report("F", "gpx_solve N=%d nrhs=%d L^-1 B" % (N, nrhs), got1, base1, acc.bound(base1))
            _report("F", "gpx_solve N=%d nrhs=%d L^-T (L^-1 B)" % (N, nrhs), got2, base2, acc.bound(base2))
            assert got1 <= acc.bound(base1), (nrhs, got1, base1)
            assert got2 <= acc.bound(base2), (nrhs, got2, base2)
    if N in PREDICT_N:
        beta = gp._get_beta()
        ks = sk.GaussianCovariance().cov_matrix_ij(xs, x, theta)          # gpx_gram, no noise term
        mean_ref = gp.meant + ks.dot(beta)
        W = acc.lapack_trsv(L, ks.T)
        var_ref = v + vt - np.einsum("ij,ij->j", W, W)
        del W
        for M in (1, 32, 33, 3071, 3072, 4097):
            mean, var = gp.estimate_many(xs[:M])
            em = float(np.abs(mean - mean_ref[:M]).max()) / v
            ev = float(np.abs(var - var_ref[:M]).max()) / v
            _report("F", "estimate_many N=%d M=%d mean (/v)" % (N, M), em, 0.0, MEAN_ATOL_V)
            _report("F", "estimate_many N=%d M=%d var (/v)" % (N, M), ev, 0.0, VAR_ATOL_V)
            assert em <= MEAN_ATOL_V and ev <= VAR_ATOL_V, (M, em, ev)
    if N == KINV_N:
        import scipy.linalg
        with acc.blas_threads():
            Li = scipy.linalg.solve_triangular(L, np.eye(N), lower=True)
            ref = Li.T.dot(Li)
        del Li
        scale = np.abs(ref).max()
        e = float(np.abs(gp.Kinv - ref).max()) / scale
        _report("F", "gpx_kinv N=%d (/max|K^-1|)" % N, e, 0.0, KINV_RTOL)
        assert e <= KINV_RTOL, e
        for r0, r1 in [(1152, 3200), (3072, 4224)]:
            g = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())     # a fresh handle: no whole K^-1 to fall back on
            rows = g._dev().kinv_rows(r0, r1)
            g._dev().close()
            e = float(np.abs(rows - ref[r0:r1]).max()) / scale
            _report("F", "gpx_kinv_rows N=%d [%d, %d) (/max|K^-1|)" % (N, r0, r1), e, 0.0, KINV_RTOL)
            assert e <= KINV_RTOL, (r0, r1, e)
    gp._dev().close()
    _gpx.lib.gpx_pool_trim()


SEAM_M = 32768 + 130      # predict_common's chunk is at most 32768 rows: one full chunk on the fused row sums, then a 130-row tail on the stand-alone reduction


@pytest.mark.parametrize("N,d", [(127, 3), (200, 8)])
def test_predictions_across_a_chunk_seam(N, d):
    """More than one chunk through gpx_predict (estimate_many) and gpx_predict_kv: the second chunk reads xs + m0 d, kv + m0 n and
    kdiag + m0 and writes mean_out + m0 and var_out + m0, and takes the other row reduction.  npad = 128 and 256.  Queries 32767 and 32768
    (the seam) and the last one are bit-equal to training rows, query 100 lies far outside the data (k* = 0: a zero row solves to a zero
    row, so it returns the prior exactly); kdiag of the kv call is v + vt plus a per-query offset that must reappear in the variance.
    Against mean = k* . beta_dev and var = kdiag - ||L_dev^-1 k*||^2 on the tolerances of this section; the tail and the seam queries called
    alone against the big call at the 1e-11 that test_estimate_many_fused_row_sums_ragged uses for path agreement."""
    M = SEAM_M
    x, t, _xs, theta = acc.recipe(N, d)
    rng = np.random.RandomState(N + d + 1)
    xs = rng.uniform(0, 10, (M, d))
    xs[32767], xs[32768], xs[M - 1], xs[100] = x[5], x[6], x[N - 1], 1.0e3
    v, vt = np.exp(theta[0]), np.exp(theta[1])
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    mm = _MatrixModel(_dev_gram(x, theta), gp.t)
    ks = sk.GaussianCovariance().cov_matrix_ij(xs, x, theta)              # gpx_gram, no noise term
    assert ks[32767, 5] == v and ks[32768, 6] == v and ks[M - 1, N - 1] == v and not ks[100].any()
    koff = 1e-3 * (np.arange(M) % 17)
    kdiag = v + vt + koff
    alone = [slice(32768, M), slice(32767, 32768), slice(32768, 32769)]

    def check(what, L, beta, predict, offset, shift):
        W = acc.lapack_trsv(L, ks.T)
        mean_ref = ks.dot(beta) + shift
        var_ref = v + vt + offset - np.einsum("ij,ij->j", W, W)
        mean, var = predict(slice(0, M))
        for name, lo, hi in (("first chunk", 0, 32768), ("tail", 32768, M)):
            em = float(np.abs(mean - mean_ref)[lo:hi].max()) / v
            ev = float(np.abs(var - var_ref)[lo:hi].max()) / v
            _report("F", "%s N=%d M=%d %s mean (/v)" % (what, N, M, name), em, 0.0, MEAN_ATOL_V)
            _report("F", "%s N=%d M=%d %s var (/v)" % (what, N, M, name), ev, 0.0, VAR_ATOL_V)
            assert em <= MEAN_ATOL_V and ev <= VAR_ATOL_V, (what, name, em, ev)
        assert mean[100] == shift and var[100] == v + vt + offset[100], (what, mean[100], var[100])
        for sl in alone:
            m1, v1 = predict(sl)
            np.testing.assert_allclose(m1, mean[sl], rtol=0, atol=1e-11, err_msg="%s %r" % (what, sl))
            np.testing.assert_allclose(v1, var[sl], rtol=0, atol=1e-11, err_msg="%s %r" % (what, sl))

    check("estimate_many", gp._dev().chol(), gp._get_beta(), lambda sl: gp.estimate_many(xs[sl]), np.zeros(M), gp.meant)
    check("gpx_predict_kv", _chol_of(mm.handle, N), mm.alpha(), lambda sl: mm.predict_kv(ks[sl], kdiag[sl]), koff, 0.0)
    gp._dev().close()
    mm.close()
    _gpx.lib.gpx_pool_trim()
