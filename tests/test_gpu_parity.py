"""GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against
  (1) golden vectors generated from the genuine reference (tests/golden, tools/gen_golden.py),
  (2) the CPU oracle on the same seeded inputs, and
  (3) size-independent properties at the BASELINE sizes.
Tolerances follow SURVEY.md 8a: Gram rel 1e-13; estimate_many rtol 1e-6 / atol 1e-9 v; propagated
means atol 1e-9, variances ABSOLUTE atol 1e-8 v (differences of O(v) terms); METIS (cond 1.6e7) 10x.
"""
import ctypes
import pickle

import numpy as np
import pytest

from conftest import GP_CASES, load_golden, torch

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------
# building blocks on device pointers
# ------------------------------------------------------------------------------------------------
def test_device_is_gfx950_and_library_loaded():
    assert _gpx.device_count() >= 1
    tf = ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_bench_mfma_f64(2000, ctypes.byref(tf)), "mfma bench")
    assert tf.value > 10.0          # fp64 MFMA is alive (vendor peak 78.6 TFLOP/s)


@pytest.mark.parametrize("M,N,K,lower", [(128, 128, 16, 0), (256, 128, 48, 0), (384, 256, 128, 0), (256, 256, 272, 1),
                                          (1024, 1024, 1024, 1)])   # the last one: <= 40 lower tiles with a long contraction -> the 32 x 32-tile variant
def test_gemm_nt_against_numpy(M, N, K, lower):
    rng = np.random.RandomState(M + N + K)
    A = rng.randn(M, K)
    B = rng.randn(N, K) + np.arange(N)[:, None] * 0.01      # asymmetric on purpose
    C0 = rng.randn(M, N)
    a, b, c = _dev(A), _dev(B), _dev(C0)
    st = _gpx.lib.gpx_dev_gemm_nt(_p(a), K, _p(b), K, _p(c), N, M, N, K, -0.75, 1.25, lower, None)
    _gpx.check(st, "gemm")
    torch.cuda.synchronize()
    got = c.cpu().numpy()
    want = -0.75 * A.dot(B.T) + 1.25 * C0
    if lower:   # contract: everything on/below the diagonal is updated, 128-tiles strictly above are untouched
        il = np.tril_indices(M)
        np.testing.assert_allclose(got[il], want[il], rtol=1e-13, atol=1e-12)
        for bi in range(M // 128):
            for bj in range(bi + 1, N // 128):
                blk = (slice(128 * bi, 128 * bi + 128), slice(128 * bj, 128 * bj + 128))
                np.testing.assert_array_equal(got[blk], C0[blk])
    else:
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-12)
    # beta = 0 must ignore (possibly NaN) C
    c2 = torch.full((M, N), float("nan"), dtype=torch.float64, device="cuda")
    _gpx.check(_gpx.lib.gpx_dev_gemm_nt(_p(a), K, _p(b), K, _p(c2), N, M, N, K, 1.0, 0.0, 0, None), "gemm")
    torch.cuda.synchronize()
    np.testing.assert_allclose(c2.cpu().numpy(), A.dot(B.T), rtol=1e-13, atol=1e-12)


def test_gemm_rejects_bad_shapes():
    a = torch.zeros(128, 16, dtype=torch.float64, device="cuda")
    assert _gpx.lib.gpx_dev_gemm_nt(_p(a), 16, _p(a), 16, _p(a), 128, 100, 128, 16, 1.0, 0.0, 0, None) == _gpx.GPX_ERR_BAD_ARG


@pytest.mark.parametrize("cond", [1e2, 1e8])
def test_potrf_leaf_and_inverse(cond):
    rng = np.random.RandomState(3)
    Q, _ = np.linalg.qr(rng.randn(128, 128))
    ev = np.logspace(0, np.log10(cond), 128)
    A = (Q * ev).dot(Q.T)
    A = 0.5 * (A + A.T)
    ld = 256
    buf = np.full((128, ld), np.nan)
    buf[:, :128] = A
    a = _dev(buf)
    dinv = torch.empty(128 * 128, dtype=torch.float64, device="cuda")
    diag = torch.empty(128, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    _gpx.check(_gpx.lib.gpx_dev_potrf_leaf(_p(a), ld, _p(dinv), _p(diag), _p(info), 0, None), "potrf leaf")
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    L = a.cpu().numpy()[:, :128]
    Lref = np.linalg.cholesky(A)
    assert np.all(np.triu(L, 1) == 0)
    np.testing.assert_allclose(L, Lref, rtol=0, atol=1e-13 * cond ** 0.5 * np.abs(Lref).max())
    np.testing.assert_allclose(diag.cpu().numpy(), np.diag(Lref), rtol=1e-12 * cond ** 0.5)
    X = dinv.cpu().numpy().reshape(128, 128)
    assert np.all(np.triu(X, 1) == 0)
    np.testing.assert_allclose(X.dot(L), np.eye(128), rtol=0, atol=1e-12 * cond ** 0.5)


def test_potrf_leaf_reports_non_pd():
    A = np.eye(128)
    A[40, 40] = -1.0
    a = _dev(A)
    dinv = torch.empty(128 * 128, dtype=torch.float64, device="cuda")
    diag = torch.empty(128, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    _gpx.check(_gpx.lib.gpx_dev_potrf_leaf(_p(a), 128, _p(dinv), _p(diag), _p(info), 1000, None), "potrf leaf")
    torch.cuda.synchronize()
    assert int(info.item()) == 1041


# ------------------------------------------------------------------------------------------------
# Gram (a1/a2)
# ------------------------------------------------------------------------------------------------
GRAM_CASES = ["grid_int", "n257_d5", "n64_d16", "rect_33x257_d5", "n257_d5_vt0", "n130_d1"]


@pytest.mark.parametrize("name", GRAM_CASES)
def test_gram_golden(name):
    g = load_golden("gram")
    xi, xj, th = g[name + "__xi"], g[name + "__xj"], g[name + "__theta"]
    cov = sk.GaussianCovariance()
    K = cov.cov_matrix_ij(xi, xj, th)
    np.testing.assert_allclose(K, g[name + "__K_ij"], rtol=1e-13, atol=1e-300)
    if name + "__K" in g:
        Kf = cov.cov_matrix(xi, th)
        np.testing.assert_allclose(Kf, g[name + "__K"], rtol=1e-13, atol=1e-300)
        # the reference's own identity test (skgpuppy/tests/tests.py:598-600): cov_matrix == cov_matrix_ij + vt I
        with np.errstate(divide="ignore"):
            vt = np.exp(th[1])
        assert np.abs(Kf - (K + vt * np.eye(len(xi)))).sum() <= 1e-10


def test_gram_empty_and_single():
    cov = sk.GaussianCovariance()
    th = np.zeros(5)
    assert cov.cov_matrix_ij(np.zeros((0, 3)), np.zeros((4, 3)), th).shape == (0, 4)
    K = cov.cov_matrix(np.ones((1, 3)), th)
    assert K.shape == (1, 1) and K[0, 0] == pytest.approx(2.0)


@pytest.mark.parametrize("n,d", [(128, 3), (384, 2), (1000, 5), (2176, 8)])
def test_gram_lower_only_triangular_grid(n, d):
    """the fit's lower-only Gram launch on its 1-D grid over the tiles that touch the lower triangle (64 x 128 tiles: row pairs (2m, 2m+1)
    hold m + 1 column tiles each): every entry on or below the diagonal equals the full launch's (incl. +vt on the diagonal and the
    identity padding), entries in tiles above the staircase are never written.  cov_matrix (Covariance.py:461-464) is the reference."""
    rng = np.random.RandomState(n + d)
    x = rng.uniform(0, 10, (n, d))
    theta = np.log(np.array([1.7, 0.03] + list(rng.uniform(0.02, 0.2, d))))
    npad = (n + 127) // 128 * 128
    xd = _dev(x)
    full = torch.full((npad, npad), -7.0, dtype=torch.float64, device=xd.device)
    low = torch.full((npad, npad), -7.0, dtype=torch.float64, device=xd.device)
    vt = float(np.exp(theta[1]))
    for out, lower in ((full, 0), (low, 1)):
        _gpx.check(_gpx.lib.gpx_dev_gram(_p(xd), n, _p(xd), n, d, _gpx.ptr(theta), vt, lower, 1, _p(out), npad, npad, npad, None), "gram")
    torch.cuda.synchronize()
    F, Lw = full.cpu().numpy(), low.cpu().numpy()
    il = np.tril_indices(npad)
    np.testing.assert_array_equal(Lw[il], F[il])
    np.testing.assert_allclose(F[:n, :n], orc.gram(x, theta), rtol=1e-9, atol=1e-12)   # (oracle: noise already on the diagonal; |a-b|^2 through a GEMM -> absolute accuracy for far pairs)
    np.testing.assert_array_equal(F[n:, n:], np.eye(npad - n))
    # a 64 x 128 tile strictly above the diagonal staircase stays untouched
    if npad >= 256:
        assert (Lw[0:64, 128:256] == -7.0).all()


# ------------------------------------------------------------------------------------------------
# GP cases against golden vectors of the reference
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=GP_CASES)
def case(request):
    g = load_golden(request.param)
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    return request.param, g, gp


def _loose(name):
    return 10.0 if name == "metis" else 1.0


def test_fit_golden(case):
    name, g, gp = case
    assert gp.meant == pytest.approx(float(g["meant"]), abs=1e-15)
    np.testing.assert_allclose(gp.t, g["t_centered"], rtol=0, atol=1e-15)
    beta = gp._get_beta()
    np.testing.assert_allclose(beta, g["beta"], rtol=0, atol=1e-6 * _loose(name) * np.abs(g["beta"]).max())
    assert gp._dev().logdet() == pytest.approx(float(g["logdet"]), rel=1e-9, abs=1e-7)
    assert gp._dev().jitter() == 0.0
    if "Kinv" in g:
        Kinv = gp.Kinv
        assert Kinv.shape == (gp.n, gp.n)
        np.testing.assert_allclose(Kinv, g["Kinv"], rtol=0, atol=1e-7 * np.abs(g["Kinv"]).max())
        np.testing.assert_allclose(Kinv, Kinv.T, rtol=0, atol=0)


def test_cholesky_reconstructs_K(case):
    name, g, gp = case
    L = gp._dev().chol()
    with np.errstate(divide="ignore"):
        K = orc.gram(g["x"], g["theta"])
    np.testing.assert_allclose(L.dot(L.T), K, rtol=0, atol=1e-12 * np.abs(K).max())


def test_estimate_many_golden(case):
    name, g, gp = case
    v = np.exp(g["theta"][0])
    mean, var = gp.estimate_many(g["xs"])
    k = _loose(name)
    np.testing.assert_allclose(mean, g["pred_mean"], rtol=1e-6 * k, atol=1e-9 * k)
    np.testing.assert_allclose(var, g["pred_var"], rtol=1e-6 * k, atol=1e-9 * v * k)
    m0, v0 = gp.estimate(g["xs"][0])
    assert m0 == pytest.approx(g["est0"][0], rel=1e-6 * k, abs=1e-9 * k)
    assert v0 == pytest.approx(g["est0"][1], rel=1e-6 * k, abs=1e-9 * v * k)
    m1, v1 = gp(g["xs"][0])
    assert (m1, v1) == (m0, v0)
    # list input, as the README passes it
    ml, vl = gp.estimate_many([list(r) for r in g["xs"][:3]])
    np.testing.assert_array_equal(ml, mean[:3])
    np.testing.assert_array_equal(vl, var[:3])


def test_propagation_golden(case):
    name, g, gp = case
    v = np.exp(g["theta"][0])
    k = _loose(name)
    for iu in range(int(g["nu"])):
        u = g["u%d" % iu]
        for iS in range(int(g["nS"])):
            S = g["Sigma%d" % iS]
            upa = sk.UncertaintyPropagationApprox(gp)
            ma, va = upa.propagate_GA(u, S)
            ref = g["approx_u%d_S%d" % (iu, iS)]
            assert ma == pytest.approx(ref[0], abs=1e-9 * k)
            assert va == pytest.approx(ref[1], abs=1e-8 * v * k)
            assert upa.propagate_mean(u, S) == pytest.approx(float(g["approx_mean_only_u%d_S%d" % (iu, iS)]), abs=1e-9 * k)
            f = upa._getFactor(u, S, float(g["v_out"]))
            assert f == pytest.approx(float(g["factor_u%d_S%d" % (iu, iS)]), rel=1e-5 * k)
            if iS == 0:
                np.testing.assert_allclose(upa.C_ux, g["C_ux_u%d" % iu], rtol=1e-13, atol=1e-300)
                np.testing.assert_allclose(upa.J_ux, g["J_ux_u%d" % iu], rtol=1e-12, atol=1e-300)
                # H = ((w d)(w d)^T - W) c cancels exactly where (w_k d_k)^2 == w_k: absolute floor
                Href = g["H_ux_u%d" % iu]
                np.testing.assert_allclose(upa.H_ux, Href, rtol=1e-12, atol=1e-15 * np.abs(Href).max())
                dv = np.array([upa._get_variance_dv_h(u, h) for h in range(gp.d)])
                np.testing.assert_allclose(dv, g["dvh_u%d" % iu], rtol=1e-6 * k, atol=1e-8 * v * k)
            key = "exact_u%d_S%d" % (iu, iS)
            if key in g:
                upe = sk.UncertaintyPropagationExact(gp)
                me, ve = upe.propagate_GA(u, S)
                assert me == pytest.approx(g[key][0], abs=1e-9 * k)
                assert ve == pytest.approx(g[key][1], abs=1e-8 * v * k)
                assert upe.propagate_mean(u, S) == pytest.approx(float(g["exact_mean_only_u%d_S%d" % (iu, iS)]), abs=1e-9 * k)
                # a caller-supplied C_ux is USED on the built-in route too (reference: UncertaintyPropagation.py:269-290)
                mc = upe.propagate_mean(u, S, g["C_alt_u%d" % iu])
                # (C_alt is not a covariance vector: sum_i beta_i C_alt_i does not cancel like beta . C, so the value is O(|beta|_1) --
                # 14 on METIS -- and carries the LU-vs-Cholesky difference of beta in RELATIVE terms: SURVEY 8a, 1e-9 .. 2e-7)
                assert mc == pytest.approx(float(g["exact_mean_C_alt_u%d_S%d" % (iu, iS)]), abs=1e-9 * k, rel=1e-8 * k)
                assert abs(float(g["exact_mean_C_alt_u%d_S%d" % (iu, iS)]) - float(g["exact_mean_only_u%d_S%d" % (iu, iS)])) > 1e-6 * k   # (the fixture tells the two apart)


def test_kat1_quirk_active():
    """u equal to a training row: the +vt-on-equality quirk of the scalar kernel must be reproduced."""
    g = load_golden("kat1_grid")
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    S = np.diag([0.01, 0.01])
    u = np.array([5.0, 5.0])
    assert sk.UncertaintyPropagationApprox(gp).propagate_GA(u, S) == pytest.approx(
        (0.18983893618073702, 0.0018348329974112298), abs=1e-9)
    assert sk.UncertaintyPropagationExact(gp).propagate_GA(u, S) == pytest.approx(
        (0.18981740098493302, 0.0018392233503982257), abs=1e-9)


def test_metis_reference_assertions():
    """The reference's own METIS test (skgpuppy/tests/tests.py:1381-1409) at the fixed theta of KAT2."""
    g = load_golden("metis")
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    u = np.array([15.05, 5.0, 0.025])
    S = np.diag([4.0, 1.0, 2.5e-5])
    meanG, varG = gp(u)
    code_u = varG - gp._get_vt()
    assert np.sqrt(code_u) < 0.0006
    for cls in (sk.UncertaintyPropagationExact, sk.UncertaintyPropagationApprox):
        m, var = cls(gp).propagate_GA(u, S)
        assert 0.0410788036621 < np.sqrt(var - code_u) < 0.0422334526251


# ------------------------------------------------------------------------------------------------
# oracle parity on fresh seeded inputs, ragged sizes and edge cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,M", [(1, 2, 3), (2, 1, 1), (127, 3, 5), (128, 3, 129), (129, 5, 1), (640, 6, 300), (1500, 8, 257)])
def test_against_oracle_ragged(N, d, M):
    rng = np.random.RandomState(100 + N + d)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (M, d))
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    og = orc.OracleGP(x, t, theta)
    mean, var = gp.estimate_many(xs)
    om, ov = og.estimate_many(xs)
    np.testing.assert_allclose(mean, om, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(var, ov, rtol=1e-6, atol=2e-9)
    np.testing.assert_allclose(gp._get_beta(), og.beta(), rtol=0, atol=1e-6 * np.abs(og.beta()).max())
    assert gp._dev().logdet() == pytest.approx(og.logdet(), rel=1e-9, abs=1e-7)
    if N >= 2:
        u = xs[0]
        S = np.diag(rng.uniform(0.005, 0.05, d))
        ma, va = sk.UncertaintyPropagationApprox(gp).propagate_GA(u, S)
        oma, ova = orc.approx_propagate(og, u, S)
        assert ma == pytest.approx(oma, abs=1e-9) and va == pytest.approx(ova, abs=2e-8)
        me, ve = sk.UncertaintyPropagationExact(gp).propagate_GA(u, S)
        ome, ove = orc.exact_propagate(og, u, S)
        assert me == pytest.approx(ome, abs=1e-9) and ve == pytest.approx(ove, abs=2e-8)


@pytest.mark.parametrize("N,d,M", [(2200, 3, 3100), (1153, 4, 3329), (3000, 2, 4097)])
def test_estimate_many_fused_row_sums_ragged(N, d, M):
    """estimate_many with M >= 3072 takes the row sums |z|^2 and z.y along in the epilogue of each slab's last product (gemm.hip,
    tile_row_reduce) instead of re-reading kv L^-T: full slabs through the fused 128 x 128-tile launch, a ragged last slab (N = 2200:
    2048 + 256 columns; N = 1153: 1024 + 256) through the small-tile product plus the slab's own reduction, M not a tile multiple.
    Against the oracle's dense formulas (GaussianProcess.py:75-78)."""
    rng = np.random.RandomState(7 + N + d)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (M, d))
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    mean, var = gp.estimate_many(xs)
    og = orc.OracleGP(x, t, theta)
    K = og.Kinv
    kv = orc.gram_ij(xs, x, theta)
    om = kv.dot(og.beta()) + og.meant
    ov = (np.exp(theta[0]) + np.exp(theta[1])) - np.einsum("ij,jk,ik->i", kv, K, kv)
    np.testing.assert_allclose(mean, om, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(var, ov, rtol=1e-6, atol=2e-9)
    # the same queries in two halves below the fused path's threshold: the other code path, the same numbers to rounding
    m2, v2 = gp.estimate_many(xs[:1500])
    np.testing.assert_allclose(mean[:1500], m2, rtol=0, atol=1e-11)
    np.testing.assert_allclose(var[:1500], v2, rtol=0, atol=1e-11)
    # ... and a handful of queries (estimate(x_star), plots): up to 32 go through the few-right-hand-side solver's forward sweep instead of
    # the many-query recursion (two groups of 16 right-hand sides; 33 is the recursion again) -- the third code path, the same numbers
    for k in (1, 16, 17, 32, 33):
        mk, vk = gp.estimate_many(xs[:k])
        np.testing.assert_allclose(mk, mean[:k], rtol=0, atol=1e-11)
        np.testing.assert_allclose(vk, var[:k], rtol=0, atol=1e-11)


def test_zero_queries():
    g = load_golden("kat1_grid")
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    mean, var = gp.estimate_many(np.zeros((0, 2)))
    assert mean.shape == (0,) and var.shape == (0,)


def test_pickle_roundtrip_bit_identical():
    """skgpuppy/tests/tests.py:626-659: protocol 0, estimate_many identical after reload."""
    g = load_golden("n203_d3")
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    m0, v0 = gp.estimate_many(g["xs"])
    gp2 = pickle.loads(pickle.dumps(gp, protocol=0))
    m1, v1 = gp2.estimate_many(g["xs"])
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(v0, v1)
    for attr in ("n", "d", "meant"):
        assert getattr(gp2, attr) == getattr(gp, attr)
    np.testing.assert_array_equal(gp2.theta_min, gp.theta_min)


def test_jitter_fallback_on_non_pd_K():
    """A tight cluster with vt = 0 makes K numerically indefinite (pivots ~ +-1e-16): the factorisation
    must fail and be repeated on K + 1e-5 I like the reference's fallback (skgpuppy/Covariance.py:180-185)."""
    rng = np.random.RandomState(5)
    x = rng.uniform(0, 1e-4, (200, 2))
    t = rng.randn(200)
    theta = np.array([0.0, -np.inf, 0.0, 0.0])
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta)
    assert gp._dev().jitter() == 1e-5
    with np.errstate(divide="ignore"):
        K = orc.gram(x, theta) + 1e-5 * np.eye(200)
    np.testing.assert_allclose(gp.Kinv.dot(K), np.eye(200), atol=1e-6)


def test_bad_arguments_raise():
    cov = sk.GaussianCovariance()
    with pytest.raises(ValueError):
        cov.cov_matrix_ij(np.zeros((3, 2)), np.zeros((3, 3)), np.zeros(4))
    with pytest.raises(ValueError):
        cov.cov_matrix_ij(np.zeros((3, 2)), np.zeros((3, 2)), np.zeros(5))
    x = np.random.RandomState(0).rand(10, 2)
    gp = sk.GaussianProcess(x, np.zeros(10), cov, np.zeros(4))
    with pytest.raises(ValueError):
        gp.estimate_many(np.zeros((3, 5)))
    with pytest.raises(ValueError):
        sk.UncertaintyPropagationApprox(gp).propagate_GA(np.zeros(3), np.eye(2))


# ------------------------------------------------------------------------------------------------
# BASELINE sizes: size-independent properties (C3/C4: the oracle needs minutes / cannot run them) and full-size oracle parity (C2)
# ------------------------------------------------------------------------------------------------
def _recipe(N, d, M):
    rng = np.random.RandomState(20240 + N + d)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (M, d))
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    return x, t, xs, theta


@pytest.mark.parametrize("N,d", [(4096, 4), (16384, 8)])
def test_full_size_properties(N, d):
    x, t, xs, theta = _recipe(N, d, 2048)
    cov = sk.GaussianCovariance()
    gp = sk.GaussianProcess(x, t, cov, theta.copy())
    v, vt = 2.0, 0.01
    # (1) K alpha = t : residual through an independent path (Gram rows from the Gram kernel, host GEMV)
    beta = gp._get_beta()
    rows = np.random.RandomState(1).choice(N, 512, replace=False)
    Krows = cov.cov_matrix_ij(x[rows], x, theta)
    Krows[np.arange(512), rows] += vt
    resid = Krows.dot(beta) - gp.t[rows]
    assert np.abs(resid).max() < 1e-8 * max(1.0, np.abs(beta).max())
    # (2) interpolation identity at training inputs: mean_i = t_i - vt alpha_i ; var_i = 2 vt - vt^2 Kinv_ii in [vt, 2 vt)
    mean, var = gp.estimate_many(x[rows])
    np.testing.assert_allclose(mean - gp.meant, gp.t[rows] - vt * beta[rows], rtol=0, atol=1e-8)
    assert np.all(var >= vt - 1e-9) and np.all(var < 2 * vt)
    # (3) far-away query: prior
    far = np.full((1, d), 1e3)
    mf, vf = gp.estimate_many(far)
    assert mf[0] == pytest.approx(gp.meant, abs=1e-12) and vf[0] == pytest.approx(v + vt, abs=1e-12)
    # (4) permutation equivariance + chunk independence of estimate_many
    m2, v2 = gp.estimate_many(xs[::-1])
    m1, v1 = gp.estimate_many(xs)
    np.testing.assert_array_equal(m1, m2[::-1])
    np.testing.assert_array_equal(v1, v2[::-1])
    # (5) propagation with vanishing input uncertainty reduces to the plain prediction
    u = xs[0]
    S0 = 1e-14 * np.eye(d)
    mu, va = sk.UncertaintyPropagationApprox(gp).propagate_GA(u, S0)
    me, ve = sk.UncertaintyPropagationExact(gp).propagate_GA(u, S0)
    assert mu == pytest.approx(m1[0], abs=1e-8) and me == pytest.approx(m1[0], abs=1e-8)
    assert va == pytest.approx(v1[0], abs=1e-7) and ve == pytest.approx(v1[0], abs=1e-7)
    # (6) Exact vs Approx agree to second order for small Sigma (reference tests.py:1200-1242 uses 1e-2)
    S = 0.01 * np.eye(d)
    mu, va = sk.UncertaintyPropagationApprox(gp).propagate_GA(np.full(d, 5.0), S)
    me, ve = sk.UncertaintyPropagationExact(gp).propagate_GA(np.full(d, 5.0), S)
    assert mu == pytest.approx(me, abs=1e-2) and va == pytest.approx(ve, abs=1e-2)


def test_c2_full_size_against_oracle():
    """BASELINE config 2 (N = M = 4096, d = 4) at FULL size against the oracle (LU inverse + GEMM estimate_many + serial
    double loops: ~5 s on the host), SURVEY 8a tolerances."""
    N, d = 4096, 4
    x, t, xs, theta = _recipe(N, d, N)
    v = 2.0
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    og = orc.OracleGP(x, t, theta)
    mean, var = gp.estimate_many(xs)
    om, ov = og.estimate_many(xs)
    np.testing.assert_allclose(mean, om, rtol=1e-6, atol=1e-9 * v)
    np.testing.assert_allclose(var, ov, rtol=1e-6, atol=1e-9 * v)
    beta, obeta = gp._get_beta(), og.beta()
    np.testing.assert_allclose(beta, obeta, rtol=0, atol=1e-6 * np.abs(obeta).max())
    assert gp._dev().logdet() == pytest.approx(og.logdet(), rel=1e-10)
    u, S = np.full(d, 5.0), 0.01 * np.eye(d)
    ma, va = sk.UncertaintyPropagationApprox(gp).propagate_GA(u, S)
    oma, ova = orc.approx_propagate(og, u, S)
    assert ma == pytest.approx(oma, abs=1e-8) and va == pytest.approx(ova, abs=1e-8 * v)
    me, ve = sk.UncertaintyPropagationExact(gp).propagate_GA(u, S)
    ome, ove = orc.exact_propagate(og, u, S)
    assert me == pytest.approx(ome, abs=1e-8) and ve == pytest.approx(ove, abs=1e-8 * v)
    np.testing.assert_allclose(gp.Kinv[::97, ::89], og.Kinv[::97, ::89], rtol=0, atol=1e-6 * np.abs(og.Kinv).max())


def test_c3_fit_and_propagation_against_oracle():
    """BASELINE config 3 (N = 16384, d = 8: fit + propagate_GA) at FULL size against the oracle: its LU inverse of K (seconds to a
    minute on the host's BLAS threads), then approx_propagate / exact_propagate in the serial loop order of
    UncertaintyPropagation2.pyx on that K^-1 (about 10 s and 60 s).  u = 5 1_d, Sigma = 0.01 I; SURVEY 8a tolerances.
    Both device paths of the Approx class are checked: the two-sweep solver right after the fit and the pass over K^-1."""
    N, d = 16384, 8
    x, t, xs, theta = _recipe(N, d, 64)
    v = 2.0
    u, S = np.full(d, 5.0), 0.01 * np.eye(d)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    ga_solve = sk.UncertaintyPropagationApprox(gp).propagate_GA(u, S)          # solver path: no K^-1 yet
    ge = sk.UncertaintyPropagationExact(gp).propagate_GA(u, S)                  # materialises K^-1
    ga_kinv = sk.UncertaintyPropagationApprox(gp).propagate_GA(u + 0.0, S)      # same u: cached; a new object, new-u path below
    ga_kinv2 = sk.UncertaintyPropagationApprox(gp).propagate_GA(u + 0.25, S)
    mean, var = gp.estimate_many(xs)
    beta = gp._get_beta()
    gp._dev().close()
    _gpx.lib.gpx_pool_trim()
    og = orc.OracleGP(x, t, theta)
    om, ov = og.estimate_many(xs)
    np.testing.assert_allclose(mean, om, rtol=1e-6, atol=1e-9 * v)
    np.testing.assert_allclose(var, ov, rtol=1e-6, atol=1e-9 * v)
    obeta = og.beta()
    np.testing.assert_allclose(beta, obeta, rtol=0, atol=1e-6 * np.abs(obeta).max())
    oa = orc.approx_propagate(og, u, S)
    for got in (ga_solve, ga_kinv):
        assert got[0] == pytest.approx(oa[0], abs=1e-9) and got[1] == pytest.approx(oa[1], abs=1e-8 * v)
    oa2 = orc.approx_propagate(og, u + 0.25, S)
    assert ga_kinv2[0] == pytest.approx(oa2[0], abs=1e-9) and ga_kinv2[1] == pytest.approx(oa2[1], abs=1e-8 * v)
    oe = orc.exact_propagate(og, u, S)
    assert ge[0] == pytest.approx(oe[0], abs=1e-9) and ge[1] == pytest.approx(oe[1], abs=1e-8 * v)


def test_c4_full_size_properties():
    """BASELINE config 4 (N = 65536, d = 16; K = 34 GB) on ONE GPU through the user-facing classes: the oracle cannot run
    this size (2 N^3 = 5.6e14 flop), so the checks are the size-independent ones of test_full_size_properties."""
    N, d = 65536, 16
    x, t, xs, theta = _recipe(N, d, 2048)
    v, vt = 2.0, 0.01
    cov = sk.GaussianCovariance()
    gp = sk.GaussianProcess(x, t, cov, theta.copy())
    beta = gp._get_beta()
    rows = np.random.RandomState(1).choice(N, 512, replace=False)
    Krows = cov.cov_matrix_ij(x[rows], x, theta)
    Krows[np.arange(512), rows] += vt
    assert np.abs(Krows.dot(beta) - gp.t[rows]).max() < 1e-8 * max(1.0, np.abs(beta).max())      # K alpha = t
    mean, var = gp.estimate_many(x[rows])                                                          # interpolation identity
    np.testing.assert_allclose(mean - gp.meant, gp.t[rows] - vt * beta[rows], rtol=0, atol=1e-8)
    assert np.all(var >= vt - 1e-9) and np.all(var < 2 * vt)
    mf, vf = gp.estimate_many(np.full((1, d), 1e3))                                                # prior far away
    assert mf[0] == pytest.approx(gp.meant, abs=1e-12) and vf[0] == pytest.approx(v + vt, abs=1e-12)
    m1, v1 = gp.estimate_many(xs)
    m2, v2 = gp.estimate_many(xs[::-1])
    np.testing.assert_array_equal(m1, m2[::-1])
    np.testing.assert_array_equal(v1, v2[::-1])
    ma, va = sk.UncertaintyPropagationApprox(gp).propagate_GA(xs[0], 1e-14 * np.eye(d))           # solve path, no K^-1
    assert ma == pytest.approx(m1[0], abs=1e-8) and va == pytest.approx(v1[0], abs=1e-7)
    # logdet through an independent route: sum of log pivots == slogdet of a leading 2048 block via numpy on the host
    Lrows = gp._dev().chol_rows(0, 2048)
    K0 = cov.cov_matrix(x[:2048], theta)
    np.testing.assert_allclose(Lrows[:, :2048], np.linalg.cholesky(K0), rtol=0, atol=1e-10)
    del gp
    _gpx.lib.gpx_pool_trim()


def test_chol_panel_split_is_the_joined_step_on_caller_streams():
    """gpx_dev_chol_panel_split -- the multi-GPU owner's panel step with the rows below the square cut into the next panel's square
    rows (stream_head) and the rest (stream_far) -- against numpy's factor and, bit for bit, against gpx_dev_chol_panel_next (one slice,
    joined): a middle panel with a previous panel to apply (launch-per-step chain), head = all / some / none of the rows below, and the
    first panel (square launch of the dataflow kernel, no previous panel); argument checks.  Multi-GPU form of Covariance.py:179."""
    nblk = 21
    n = 128 * nblk
    rng = np.random.RandomState(77)
    B = rng.randn(n, 64)
    A = B.dot(B.T) / 64.0 + np.diag(rng.uniform(1.0, 2.0, n))
    ref = np.linalg.cholesky(A)
    dev = torch.device("cuda")
    streams = [torch.cuda.Stream() for _ in range(3)]
    sp = lambda st: ctypes.c_void_p(st.cuda_stream)  # noqa: E731

    def step(b0, b1, hb, split):
        c0 = 128 * b0
        M = A.copy()
        M[:, :c0] = ref[:, :c0]
        if b0 >= 8:     # every panel but the one before [b0, b1) applied; that one is handed over as `prev`
            k0 = c0 - 1024
            M[c0:, c0:] = A[c0:, c0:] - ref[c0:, :k0].dot(ref[c0:, :k0].T)
            prev = torch.as_tensor(np.ascontiguousarray(ref[c0:, k0:c0])).to(dev)
        else:
            prev = None
        Ld = torch.as_tensor(M).to(dev).contiguous()
        dinv = torch.zeros((nblk, 128, 128), dtype=torch.float64, device=dev)
        diag = torch.zeros(n, dtype=torch.float64, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        if split:
            st = _gpx.lib.gpx_dev_chol_panel_split(_p(Ld), n, nblk, b0, b1, hb, _p(prev) if prev is not None else None, 1024, 1024,
                                                   _p(dinv), _p(diag), _p(info), sp(streams[0]), sp(streams[1]), sp(streams[2]))
        elif prev is not None:
            st = _gpx.lib.gpx_dev_chol_panel_next(_p(Ld), n, nblk, b0, b1, _p(prev), 1024, 1024, _p(dinv), _p(diag), _p(info), sp(streams[0]))
        else:
            st = _gpx.lib.gpx_dev_chol_panel(_p(Ld), n, nblk, b0, b1, _p(dinv), _p(diag), _p(info), sp(streams[0]))
        _gpx.check(st, "panel step")
        torch.cuda.synchronize()
        assert int(info.item()) == 0
        return Ld.cpu().numpy(), dinv.cpu().numpy(), diag.cpu().numpy()

    for b0, b1 in ((8, 16), (0, 8)):
        c0, c1 = 128 * b0, 128 * b1
        base = step(b0, b1, 0, False)
        np.testing.assert_allclose(np.tril(base[0][c0:c1, c0:c1]), ref[c0:c1, c0:c1], rtol=0, atol=1e-12 * np.abs(ref).max())
        np.testing.assert_allclose(base[0][c1:, c0:c1], ref[c1:, c0:c1], rtol=0, atol=1e-12 * np.abs(ref).max())
        for hb in (0, 2, 5, 8, 40):
            got = step(b0, b1, hb, True)
            np.testing.assert_array_equal(got[0][c0:, c0:c1], base[0][c0:, c0:c1])
            np.testing.assert_array_equal(got[1][b0:b1], base[1][b0:b1])
            np.testing.assert_array_equal(got[2][c0:c1], base[2][c0:c1])
            np.testing.assert_array_equal(got[0][c0:, c1:], base[0][c0:, c1:])          # nothing right of the panel is touched
    # last panel: no rows below at all
    last = step(16, 21, 8, True)
    np.testing.assert_allclose(np.tril(last[0][2048:, 2048:]), ref[2048:, 2048:], rtol=0, atol=1e-12 * np.abs(ref).max())
    # argument checks: the row streams must be two distinct non-null streams other than `stream`
    z = torch.zeros(16, dtype=torch.float64, device=dev)
    zi = torch.zeros(1, dtype=torch.int32, device=dev)
    for a_, b_, c_ in ((streams[0], streams[0], streams[2]), (streams[0], streams[1], streams[1])):
        assert _gpx.lib.gpx_dev_chol_panel_split(_p(z), 128, 1, 0, 1, 0, None, 0, 0, _p(z), _p(z), _p(zi), sp(a_), sp(b_), sp(c_)) == -1
    assert _gpx.lib.gpx_dev_chol_panel_split(_p(z), 128, 1, 0, 1, 0, None, 0, 0, _p(z), _p(z), _p(zi), sp(streams[0]), None, sp(streams[2])) == -1


# ------------------------------------------------------------------------------------------------
# N > 1 code path on the one GPU of the test box: 2 ranks share cuda:0, panels travel over gloo (host staged)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,message,transport", [(2500, 4, "split", "host"), (8200, 6, "split", "host"), (8200, 6, "whole", "host"),
                                                   (8200, 6, "split", "gloo-device"), (8200, 6, "whole", "gloo-device")])      # 8200 rows = 65 blocks = 9 outer panels
def test_sharded_fit_two_ranks_share_one_gpu(N, d, message, transport):
    """panel messages in two parts (head = the next panel's square rows, then the tail; the default for more than one rank) and as one
    message per panel; transport: staged through the host with every stream synchronised around each broadcast, or the product's TorchComm
    on a gloo group with device tensors (ordered against the posting stream by events only, like RCCL: the schedule's own event edges keep
    the ranks correct)"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2", GPX_PANEL_MESSAGE=message)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29733", os.path.join(ROOT, "tests", "_gpu_shard_worker.py"), str(N), str(d), "full", transport]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sharded vs single-GPU" in r.stdout
    assert ("panel message: head + tail" if message == "split" else "panel message: whole") + ", transport: " + transport in r.stdout


_MULTI_WORKER = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %(pkg)r); sys.path.insert(0, %(root)r)
import torch  # noqa: F401
import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
N, d, ndev, dup = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
rng = np.random.RandomState(20240 + N + d)
x = rng.uniform(0, 10, (N, d)); t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N); xs = rng.uniform(0, 10, (777, d))
theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
if dup:                                              # a cluster of numerically identical rows well inside the matrix + vt = 0: non-positive pivot
    x[N // 2:N // 2 + 150] = x[N // 2] + 1e-9 * rng.randn(150, d)
    theta[1] = -np.inf
tc = np.ascontiguousarray(t - t.mean())
devs = (ctypes.c_int * ndev)(*([0] * ndev))
h = ctypes.c_void_p()
st = _gpx.lib.gpx_multi_fit(_gpx.ptr(_gpx.f64(x)), _gpx.ptr(tc), N, d, _gpx.ptr(_gpx.f64(theta)), devs, ndev, ctypes.byref(h))
_gpx.check(st, "gpx_multi_fit")
nd, npan, jit = ctypes.c_int(), ctypes.c_int64(), ctypes.c_double()
_gpx.check(_gpx.lib.gpx_multi_info(h, ctypes.byref(nd), ctypes.byref(npan), ctypes.byref(jit)), "info")
beta = np.empty(N); mean = np.empty(len(xs)); var = np.empty(len(xs))
_gpx.check(_gpx.lib.gpx_multi_alpha(h, _gpx.ptr(beta)), "alpha")
_gpx.check(_gpx.lib.gpx_multi_predict(h, _gpx.ptr(_gpx.f64(xs)), len(xs), _gpx.ptr(mean), _gpx.ptr(var)), "predict")
u, S = np.full(d, 5.0), 0.01 * np.eye(d)
pm, pv, s2, rest = (ctypes.c_double() for _ in range(4))
_gpx.check(_gpx.lib.gpx_multi_propagate_approx(h, _gpx.ptr(u), _gpx.ptr(_gpx.f64(S)), ctypes.byref(pm), ctypes.byref(pv), ctypes.byref(s2), ctypes.byref(rest)), "propagate")
em, ev = ctypes.c_double(), ctypes.c_double()
_gpx.check(_gpx.lib.gpx_multi_propagate_exact(h, _gpx.ptr(u), _gpx.ptr(_gpx.f64(S)), ctypes.byref(em), ctypes.byref(ev)), "propagate exact")
# the single-GPU path on the same inputs
with np.errstate(divide="ignore"):
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    m1, v1 = gp.estimate_many(xs)
    b1 = gp._get_beta()
    a1 = sk.UncertaintyPropagationApprox(gp).propagate_GA(u, S)
    e1 = sk.UncertaintyPropagationExact(gp).propagate_GA(u, S)
scale = np.abs(b1).max()
print("MULTI ndev %%d panels %%d jitter %%g single-gpu jitter %%g" %% (nd.value, npan.value, jit.value, gp._dev().jitter()))
print("DBETA %%.3e" %% (np.abs(beta - b1).max() / scale))
print("DMEAN %%.3e" %% np.abs(mean + gp.meant - m1).max())
print("DVAR %%.3e" %% np.abs(var - v1).max())
print("DPROP %%.3e %%.3e" %% (abs(pm.value + gp.meant - a1[0]), abs(pv.value - a1[1])))
print("DEXACT %%.3e %%.3e" %% (abs(em.value + gp.meant - e1[0]), abs(ev.value - e1[1])))
_gpx.lib.gpx_multi_free(h)
"""


@pytest.mark.parametrize("N,d,ndev,dup,message", [(2500, 3, 1, 0, ""), (2500, 3, 3, 0, ""), (8200, 6, 2, 0, ""), (8200, 6, 3, 0, ""), (5000, 4, 2, 1, ""),
                                                  (900, 2, 3, 0, ""),            # (900 rows: ONE panel, two ranks own nothing)
                                                  (8200, 6, 3, 0, "split"), (8200, 6, 2, 0, "split"), (8200, 6, 1, 0, "split")])   # head + tail messages (the default only for ranks on different devices)
def test_multi_device_abi_on_one_gpu(N, d, ndev, dup, message):
    """e1-e4 behind the C-ABI (gpx_multi_*, csrc/multi.hip): one host process, `ndev` logical ranks -- all on the one GPU of
    the test box (device ordinals may repeat), so every rank has its own factor copy, streams and staging slots and panels travel by
    hipMemcpyPeerAsync on the receivers' copy streams, ordered by events only.  Against the single-GPU path on the same inputs: alpha,
    estimate_many (query-sharded), propagate_GA Approx (right-hand-side-sharded) and Exact (row panels of equal triangle area).  8200 rows = 9 outer panels: every staging slot is reused;
    dup = 1: a non-positive pivot in the middle of the matrix must be answered by ONE collective retry on K + 1e-5 I (Covariance.py:180-185)."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = _MULTI_WORKER % {"root": ROOT, "pkg": os.path.join(ROOT, "scikit-gpuppy_amd")}
    env = dict(os.environ)
    if message:
        env["GPX_PANEL_MESSAGE"] = message     # default: head (the next panel's square rows) + tail for ranks on different devices, else one message
    r = subprocess.run([sys.executable, "-c", code, str(N), str(d), str(ndev), str(dup)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    val = {l.split()[0]: [float(z) for z in l.split()[1:]] for l in r.stdout.splitlines() if l.startswith("D")}
    head = [l for l in r.stdout.splitlines() if l.startswith("MULTI")][0].split()
    print("multi-device ABI:", " ".join(head), val)
    assert int(head[2]) == ndev and int(head[4]) == (N + 1023) // 1024
    assert float(head[6]) == float(head[9]) == (1e-5 if dup else 0.0)          # both paths took (or did not take) the jitter retry
    tol = 1e-6 if dup else 1e-9        # (vt = 0 with a near-singular cluster: cond(K + 1e-5 I) ~ 1e6, summation order shows)
    assert val["DBETA"][0] < tol, val
    assert val["DMEAN"][0] < tol and val["DVAR"][0] < tol, val
    assert val["DPROP"][0] < tol and val["DPROP"][1] < 10 * tol, val
    # (Exact: row panels of K^-1 built per rank and summed in another order than the single-GPU pass over the whole matrix)
    assert val["DEXACT"][0] < 10 * tol and val["DEXACT"][1] < 100 * tol, val


def test_multi_device_abi_from_plain_c(tmp_path):
    """the sharded path reached from a plain C program (tests/native/multi_abi_from_c.c: gcc against include/gpx.h, three logical ranks
    on the GPU): fit, estimate_many and propagate_GA agree with gpx_fit / gpx_predict / gpx_propagate_approx called from the same program."""
    import subprocess
    from test_abi import _build_c_caller
    exe = _build_c_caller(tmp_path)
    r = subprocess.run([exe, "3000", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])
    assert "3 ranks" in r.stdout and "3 panels" in r.stdout


def test_multi_device_abi_rejects_bad_arguments():
    """gpx_multi_fit: a device ordinal that does not exist, a non-finite hyper-parameter, no devices -> GPX_ERR_BAD_ARG and no handle;
    gpx_kinv_model_create / gpx_propagate_exact_model: null pointers -> GPX_ERR_BAD_ARG."""
    import ctypes
    from skgpuppy_amd import _gpx
    rng = np.random.RandomState(3)
    x, t, th = _gpx.f64(rng.rand(300, 2)), _gpx.f64(rng.rand(300)), _gpx.f64(np.log([2.0, 0.01, 0.04, 0.04]))
    h = ctypes.c_void_p()
    bad = (ctypes.c_int * 2)(0, 99)
    assert _gpx.lib.gpx_multi_fit(_gpx.ptr(x), _gpx.ptr(t), 300, 2, _gpx.ptr(th), bad, 2, ctypes.byref(h)) == _gpx.GPX_ERR_BAD_ARG and not h
    assert b"99" in _gpx.lib.gpx_last_error()
    ok = (ctypes.c_int * 1)(0)
    assert _gpx.lib.gpx_multi_fit(_gpx.ptr(x), _gpx.ptr(t), 300, 2, _gpx.ptr(th), ok, 0, ctypes.byref(h)) == _gpx.GPX_ERR_BAD_ARG and not h
    thn = th.copy()
    thn[2] = np.nan
    assert _gpx.lib.gpx_multi_fit(_gpx.ptr(x), _gpx.ptr(t), 300, 2, _gpx.ptr(thn), ok, 1, ctypes.byref(h)) == _gpx.GPX_ERR_BAD_ARG and not h
    assert _gpx.lib.gpx_multi_predict(None, _gpx.ptr(x), 300, _gpx.ptr(t), _gpx.ptr(t)) == _gpx.GPX_ERR_BAD_ARG
    m = ctypes.c_void_p()
    assert _gpx.lib.gpx_kinv_model_create(None, _gpx.ptr(t), 300, ctypes.byref(m)) == _gpx.GPX_ERR_BAD_ARG and not m
    mean = ctypes.c_double()
    assert _gpx.lib.gpx_propagate_exact_model(None, _gpx.ptr(x), 2, _gpx.ptr(th), _gpx.ptr(t), _gpx.ptr(th), _gpx.ptr(th), 1.0, ctypes.byref(mean), None) == _gpx.GPX_ERR_BAD_ARG
    # and a good call still works afterwards (the caller's device choice was put back)
    assert _gpx.lib.gpx_multi_fit(_gpx.ptr(x), _gpx.ptr(_gpx.f64(t - t.mean())), 300, 2, _gpx.ptr(th), ok, 1, ctypes.byref(h)) == 0 and h
    _gpx.lib.gpx_multi_free(h)


@pytest.mark.parametrize("transport", ["host", "gloo-device", "gloo-device-chaos"])
def test_sharded_fit_four_ranks_share_one_gpu_c3_size(transport):
    """The panel-sharded path with FOUR ranks on the one GPU at the C3 size (N = 16384: 16 outer panels, every rank owns four, the three
    staging slots are reused five times; host-staged transport, and TorchComm on gloo with device tensors: 8 MB heads and larger tails as
    scatter + all-gather) against the single-GPU path: estimate_many, call-sharded and row-sharded propagation (Approx and Exact)."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    if transport.endswith("-chaos"):     # random busy-waits on random streams of every rank: late streams must not change the factor
        env["GPX_SHARD_CHAOS"] = "7"
        transport = "gloo-device"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", "29737", os.path.join(ROOT, "tests", "_gpu_shard_worker.py"), "16384", "8", "light", transport]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sharded vs single-GPU" in r.stdout and "4 ranks, 16 panels" in r.stdout and "panel message: head + tail" in r.stdout


def test_sharded_fit_c4_size_on_rccl_world_size_one():
    """BASELINE config 4 (N = 65536, d = 16) through the SHARDED code path on a real RCCL group of one rank (all this box offers):
    64 outer panels through the two staging slots, RCCL-resident collectives, against the single-GPU path and the
    size-independent checks of test_c4_full_size_properties."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "scikit-gpuppy_amd"))
import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from skgpuppy_amd.distributed import ShardedGaussianProcess
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29743", RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
N, d = 65536, 16
rng = np.random.RandomState(20240 + N + d)
x = rng.uniform(0, 10, (N, d)); t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N); xs = rng.uniform(0, 10, (1024, d))
theta = np.log(np.array([2.0, 0.01] + [0.04] * d)); v, vt = 2.0, 0.01
gp = ShardedGaussianProcess(x, t, theta, device=torch.device("cuda", 0))
assert gp.layout.npanels == 64 and gp.jitter == 0.0
rows = np.random.RandomState(1).choice(N, 512, replace=False)
mean, var = gp.estimate_many(x[rows])                               # interpolation identity: var in [vt, 2 vt)
assert np.all(var >= vt - 1e-9) and np.all(var < 2 * vt)
mf, vf = gp.estimate_many(np.full((1, d), 1e3))                      # prior far away
assert abs(mf[0] - gp.meant) < 1e-12 and abs(vf[0] - (v + vt)) < 1e-12
ms, vs = gp.estimate_many(xs)
pa = gp.propagate_GA(xs[0], 1e-14 * np.eye(d))                        # Sigma -> 0: the plain prediction
assert abs(pa[0] - ms[0]) < 1e-8 and abs(pa[1] - vs[0]) < 1e-7
gp.close(); _gpx.lib.gpx_pool_trim()
ref = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
m1, v1 = ref.estimate_many(xs)
beta = ref._get_beta()
e = max(np.abs(ms - m1).max(), np.abs(vs - v1).max())
assert e < 1e-9, e
np.testing.assert_allclose(mean - ref.meant, ref.t[rows] - vt * beta[rows], rtol=0, atol=1e-8)
dist.destroy_process_group(); print("sharded C4 on RCCL world size 1 ok, max dev vs single-GPU %%.2e" %% e)
''' % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "sharded C4 on RCCL world size 1 ok" in r.stdout


def test_panel_transport_on_rccl_multi_gpu():
    """TorchComm.broadcast (scatter + in-place all-gather, and the plain broadcast) between REAL GPUs: every rank receives what
    the source sent, slot reuse included.  Needs at least two devices; the 1-GPU boxes skip it (the gloo tests cover the logic,
    the world-size-1 test below the RCCL argument checks)."""
    import os
    import subprocess
    import sys
    import torch
    from conftest import ROOT
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("needs >= 2 GPUs")
    world = min(ndev, 4)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", "29745", os.path.join(ROOT, "tests", "_nccl_bcast_worker.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "panel transport over RCCL ok" in r.stdout


def test_sharded_collectives_on_rccl_world_size_one():
    """The public collectives of ShardedGaussianProcess on a real RCCL (nccl) group -- RCCL has no host path, so every
    operand of all_gather / all_reduce must live on the device (one rank is all this box offers; the two-rank run above
    goes through gloo).  Also: a K that needs the reference's +1e-5 jitter gets it collectively on the sharded path."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "scikit-gpuppy_amd"))
import skgpuppy_amd as sk
from skgpuppy_amd.distributed import ShardedGaussianProcess
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29741", RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
rng = np.random.RandomState(3)
N, d = 1500, 3
x = rng.uniform(0, 10, (N, d)); t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N); xs = rng.uniform(0, 10, (77, d))
theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
gp = ShardedGaussianProcess(x, t, theta, device=torch.device("cuda", 0))
ref = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
m, v = gp.estimate_many(xs); m1, v1 = ref.estimate_many(xs)
assert np.abs(m - m1).max() < 1e-10 and np.abs(v - v1).max() < 1e-10
us = np.array([[5.0] * d, x[7]]); Ss = [0.01 * np.eye(d)] * 2
pm, pv = gp.propagate_many(us, Ss)
up = sk.UncertaintyPropagationApprox(ref)
for i in range(2):
    want = up.propagate_GA(us[i], Ss[i])
    got = gp.propagate_GA_sharded(us[i], Ss[i])
    assert abs(pm[i] - want[0]) < 1e-9 and abs(pv[i] - want[1]) < 1e-9 and abs(got[0] - want[0]) < 1e-9 and abs(got[1] - want[1]) < 1e-9
    got = gp.propagate_GA_sharded(us[i], Ss[i], via="kinv")
    assert abs(got[0] - want[0]) < 1e-9 and abs(got[1] - want[1]) < 1e-9
    ew = sk.UncertaintyPropagationExact(ref).propagate_GA(us[i], Ss[i])
    eg = gp.propagate_exact_sharded(us[i], Ss[i])
    assert abs(eg[0] - ew[0]) < 1e-9 and abs(eg[1] - ew[1]) < 1e-9
gp.close()
# the panel transport's collectives (scatter + all_gather_into_tensor, and the plain broadcast) accepted by RCCL: a group of one
# rank normally skips them
from skgpuppy_amd.distributed import TorchComm
# ... for the message in two parts (head, tail: the default above one rank) and in one
for comm in (TorchComm(split_bytes=1, exercise_single_rank=True), TorchComm(split_bytes=1 << 60, exercise_single_rank=True)):
    for split in (True, False):
        g2 = ShardedGaussianProcess(x, t, theta, device=torch.device("cuda", 0), comm=comm, split=split)
        assert g2.layout.parts(0) == (("head", "tail") if split else ("tail",))
        m2, v2 = g2.estimate_many(xs)
        assert np.abs(m2 - m1).max() < 1e-10 and np.abs(v2 - v1).max() < 1e-10 and comm._split_ok
        g2.close()
# a tight cluster with vt = 0: K is numerically indefinite -> the single-GPU fit takes the +1e-5 jitter, and so must the sharded one
xd = rng.uniform(0, 1e-4, (600, d)); td = rng.randn(600); xs = rng.uniform(0, 1e-4, (77, d))
th2 = np.array([0.0, -np.inf] + [0.0] * d)
one = sk.GaussianProcess(xd, td, sk.GaussianCovariance(), th2.copy())
assert one._dev().jitter() == 1e-5
sh = ShardedGaussianProcess(xd, td, th2, device=torch.device("cuda", 0))
assert sh.jitter == 1e-5
ms, vs = sh.estimate_many(xs); mo, vo = one.estimate_many(xs)
assert np.allclose(ms, mo, rtol=0, atol=1e-8) and np.allclose(vs, vo, rtol=0, atol=1e-8)
sh.close(); dist.destroy_process_group(); print("RCCL world-size-1 collectives ok")
''' % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "collectives ok" in r.stdout


# ------------------------------------------------------------------------------------------------
# "next" row f1: hyper-parameter likelihood, gradient and ML estimate
# ------------------------------------------------------------------------------------------------
def test_nll_and_gradient_golden(case):
    name, g, gp = case
    cov = sk.GaussianCovariance()
    k = _loose(name)
    for tag in ("", "_p"):
        th = g["theta" + tag + "_used"]
        ref, refg = float(g["nll" + tag]), g["nll_grad" + tag]
        assert cov._negativeloglikelihood(g["x"], gp.t, th) == pytest.approx(ref, rel=1e-8 * k, abs=1e-6 * k)
        got = cov._d_nll_d_theta(g["x"], gp.t, th)
        np.testing.assert_allclose(got, refg, rtol=1e-6 * k, atol=1e-6 * k * max(1.0, np.abs(refg).max()))


def test_nll_and_gradient_against_oracle_at_4096():
    """f1 beyond the golden sizes (the largest fixture has N = 1000): one likelihood + gradient evaluation at N = 4096, d = 8 -- four
    outer panels of the look-ahead factorisation, K^-1 by the structured recursion, the fused gradient pass -- against the oracle's
    LU / 2 + d derivative Grams (skgpuppy/Covariance.py:197-282)."""
    N, d = 4096, 8
    x, t, _xs, theta = _recipe(N, d, 8)
    tc = t - t.mean()
    cov = sk.GaussianCovariance()
    th = theta + 0.05 * np.arange(d + 2)                 # away from the recipe's generating parameters
    ref, refg = orc.nll(x, tc, th), orc.nll_grad(x, tc, th)
    assert cov._negativeloglikelihood(x, tc, th) == pytest.approx(ref, rel=1e-8, abs=1e-6)
    np.testing.assert_allclose(cov._d_nll_d_theta(x, tc, th), refg, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(refg).max()))


def test_gradient_matches_finite_differences():
    """the reference's own check (skgpuppy/tests/tests.py:611-624, tolerance 5e-1 there)."""
    g = load_golden("n203_d3")
    cov = sk.GaussianCovariance()
    t = g["t_centered"]
    th = g["theta"].copy()
    grad = cov._d_nll_d_theta(g["x"], t, th)
    eps = 1e-5
    for j in range(len(th)):
        e = np.zeros(len(th))
        e[j] = eps
        num = (cov._negativeloglikelihood(g["x"], t, th + e) - cov._negativeloglikelihood(g["x"], t, th - e)) / (2 * eps)
        assert grad[j] == pytest.approx(num, rel=1e-4, abs=1e-4)


def test_ml_estimate_readme_example():
    """GaussianProcess(x, t, cov) without theta = the README usage (README.rst:112-116): L-BFGS-B from get_theta."""
    g = load_golden("kat1_grid")
    x, t = g["x"], g["ml_t_raw"]
    cov = sk.GaussianCovariance()
    np.testing.assert_allclose(cov.get_theta(x, t - t.mean()), g["ml_theta_start"], rtol=1e-14)
    gp = sk.GaussianProcess(x, t, cov)
    nll_here = cov._negativeloglikelihood(x, gp.t, gp.theta_min)
    assert nll_here <= float(g["ml_nll"]) + 1e-4           # at least as good an optimum as the reference found
    assert nll_here < float(g["ml_nll_start"]) - 10
    np.testing.assert_allclose(gp.theta_min, g["ml_theta"], atol=2e-2)
    mean, var = gp.estimate_many(g["xs"])
    np.testing.assert_allclose(mean, g["ml_pred_mean"], atol=5e-3)
    np.testing.assert_allclose(var, g["ml_pred_var"], atol=5e-3)


# ------------------------------------------------------------------------------------------------
# "next" row f2: inverse uncertainty propagation (callers of propagate_GA / _get_variance_dv_h / _getFactor)
# ------------------------------------------------------------------------------------------------
def test_inverse_uncertainty_propagation_golden():
    g = load_golden("kat1_grid")
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    u = np.array([5.25, 4.75])
    c = np.array([4.0, 1.0])
    sol_a = sk.InverseUncertaintyPropagationApprox(0.02, gp, u, c, 1 / c).get_best_solution()
    np.testing.assert_allclose(sol_a, g["iup_approx"], rtol=1e-6)
    sol_n = sk.InverseUncertaintyPropagationNumerical(0.02, gp, u, c, 1 / c,
                                                      upga_class=sk.UncertaintyPropagationApprox).get_best_solution()
    np.testing.assert_allclose(sol_n, g["iup_numerical"], rtol=2e-3)
    # the reference's own assertion (skgpuppy/tests/tests.py:399-400): analytic ~ numerical
    assert sol_n[0] == pytest.approx(sol_a[0], abs=1e-2) and sol_n[1] == pytest.approx(sol_a[1], abs=1e-3)
    sol_c = sk.InverseUncertaintyPropagationApprox(0.02, gp, u, c, np.array([0.25, 2.0]), coestimated=[[0, 1]]).get_best_solution()
    np.testing.assert_allclose(sol_c, g["iup_approx_coest"], rtol=1e-6)
    # the solution really produces the requested output variance under the approximate propagation
    assert sk.UncertaintyPropagationApprox(gp).propagate_GA(u, np.diag(sol_a))[1] == pytest.approx(0.02, abs=1e-9)


def test_inv_cov_matrix_with_supplied_matrix():
    """Covariance.inv_cov_matrix(x, theta, cov_matrix=K) = inv(K)  (skgpuppy/Covariance.py:186-187)."""
    g = load_golden("n256_d8")
    cov = sk.GaussianCovariance()
    K = cov.cov_matrix(g["x"], g["theta"])
    Kinv = cov.inv_cov_matrix(g["x"], g["theta"], cov_matrix=K)
    np.testing.assert_allclose(Kinv, g["Kinv"], rtol=0, atol=1e-7 * np.abs(g["Kinv"]).max())
    Kinv2 = cov.inv_cov_matrix(g["x"], g["theta"])
    np.testing.assert_allclose(Kinv2, g["Kinv"], rtol=0, atol=1e-7 * np.abs(g["Kinv"]).max())
    with pytest.raises(np.linalg.LinAlgError):
        cov.inv_cov_matrix(g["x"], g["theta"], cov_matrix=-np.eye(5))


def test_kinv_identity_at_scale():
    """K^-1 from the structured trtri + strip SYRK: K Kinv = I on sampled rows at N = 4096."""
    x, t, xs, theta = _recipe(4096, 4, 8)
    cov = sk.GaussianCovariance()
    gp = sk.GaussianProcess(x, t, cov, theta.copy())
    Kinv = gp.Kinv
    rows = np.random.RandomState(2).choice(4096, 64, replace=False)
    Krows = cov.cov_matrix_ij(x[rows], x, theta)
    Krows[np.arange(64), rows] += 0.01
    P = Krows.dot(Kinv)
    E = np.zeros_like(P)
    E[np.arange(64), rows] = 1.0
    assert np.abs(P - E).max() < 1e-8
    np.testing.assert_array_equal(Kinv, Kinv.T)


# ------------------------------------------------------------------------------------------------
# "next" row f3: SPGP low-rank path vs the reference's golden vectors and the oracle
# ------------------------------------------------------------------------------------------------
def _spgp_case(name):
    g = load_golden("spgp")
    pre = name + "__"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", ["grid_m10", "n300_d3_m37", "n700_d4_m150"])
def test_spgp_golden(name):
    g = _spgp_case(name)
    x, t, th, m, xs = g["x"], g["t_raw"], g["theta"], int(g["m"]), g["xs"]
    cov = sk.SPGPCovariance(m)
    v = np.exp(th[0])
    if "cov" in g:
        np.testing.assert_allclose(cov.cov_matrix(x, th), g["cov"], rtol=0, atol=1e-10 * v)
        # the inverse amplifies by 1/vt; the reference's own bar is sum|diff| <= 1e-5 (tests.py:529)
        inv = cov.inv_cov_matrix(x, th)
        np.testing.assert_allclose(inv, g["inv"], rtol=0, atol=1e-7 * np.abs(g["inv"]).max())
        assert np.abs(inv - np.linalg.inv(g["cov"])).sum() <= 1e-5 * max(1.0, np.abs(g["inv"]).sum())
    np.testing.assert_allclose(cov.cov_matrix_ij(xs[:16], x, th), g["cross"], rtol=0, atol=1e-10 * v)
    assert cov(x[0], x[1], th) == pytest.approx(float(g["scalar_01"]), abs=1e-10 * v)
    assert cov(x[0], x[0], th) == pytest.approx(float(g["scalar_00"]), abs=1e-12)
    tc = t - t.mean()
    assert cov._negativeloglikelihood(x, tc, th) == pytest.approx(float(g["nll_snelson"]), rel=1e-8, abs=1e-6)
    gp = sk.GaussianProcess(x, t, cov, th.copy())
    mu, var = gp.estimate_many(xs)
    np.testing.assert_allclose(mu, g["pred_mean"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(var, g["pred_var"], rtol=0, atol=1e-6 * v)
    m0, v0 = gp.estimate(xs[0])
    assert (m0, v0) == pytest.approx(tuple(g["est0"]), abs=5e-6)
    if "inv" in g:
        np.testing.assert_allclose(gp.Kinv, g["inv"], rtol=0, atol=1e-7 * np.abs(g["inv"]).max())
    gp2 = pickle.loads(pickle.dumps(gp))
    np.testing.assert_allclose(gp2.estimate_many(xs[:5])[0], mu[:5], rtol=0, atol=1e-12)
    if "exact" in g:
        # UncertaintyPropagationExact on the SPGP model: the reference's class reads the dense K^-1, beta, theta[2:2+d] and the SPGP scalar
        # kernel (UncertaintyPropagation.py:269-290, :323-379); here the double sum runs on the device over that dense inverse
        upe = sk.UncertaintyPropagationExact(gp)
        me, ve = upe.propagate_GA(g["exact_u"], g["exact_Sigma"])
        np.testing.assert_allclose([me, ve], np.ravel(g["exact"]), rtol=0, atol=1e-6 * v)
        np.testing.assert_allclose(upe.propagate_mean(g["exact_u"], g["exact_Sigma"]), float(g["exact_mean_only"]), rtol=0, atol=1e-6)
        # the dense K^-1 / beta stay on the device across calls (gpx_kinv_model_*: uploaded once per Kinv array), and the resident form
        # gives the one-shot form's numbers to the bit (gpx_propagate_exact_matrix with h == NULL: upload, use, free)
        model = upe._kinv_model[1].handle.value
        me2, ve2 = upe.propagate_GA(g["exact_u"], g["exact_Sigma"])
        assert upe._kinv_model[1].handle.value == model and (me2, ve2) == (me, ve)
        import ctypes
        from skgpuppy_amd import _gpx
        xg, n, d = _gpx.f64(gp.x), gp.n, gp.d
        C = _gpx.f64(np.array([gp._covariance(g["exact_u"], gp.x[i]) for i in range(n)]))
        w, uu, S = _gpx.f64(np.diag(gp._get_W_inv())), _gpx.f64(g["exact_u"]), _gpx.f64(g["exact_Sigma"])
        Kinv, beta = _gpx.f64(gp._inv_cov_matrix()), _gpx.f64(gp._get_beta())
        m1, v1 = ctypes.c_double(), ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_propagate_exact_matrix(None, _gpx.ptr(Kinv), _gpx.ptr(beta), _gpx.ptr(xg), n, d, _gpx.ptr(w), _gpx.ptr(C), _gpx.ptr(uu),
                                                       _gpx.ptr(S), float(gp._covariance(g["exact_u"], g["exact_u"])), ctypes.byref(m1), ctypes.byref(v1)),
                   "gpx_propagate_exact_matrix")
        assert m1.value + gp._get_mean_t() == me and v1.value == ve


def test_spgp_vs_oracle_ragged_and_large_m():
    """seeded inputs the reference never saw: N, m not tile multiples, m spanning three 128-blocks."""
    rng = np.random.RandomState(99)
    N, d, m = 1500, 5, 300
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (77, d))
    th_gc = np.log(np.array([2.0, 0.01] + [0.04] * d))
    xb = rng.uniform(0, 10, (m, d))
    th = np.concatenate([th_gc, xb.ravel()])
    cov = sk.SPGPCovariance(m)
    gp = sk.GaussianProcess(x, t, cov, th.copy())
    ogp = orc.OracleSPGP(x, t, th, m)
    mu, var = gp.estimate_many(xs)
    omu, ovar = ogp.estimate_many(xs)
    np.testing.assert_allclose(mu, omu, rtol=0, atol=2e-5)
    np.testing.assert_allclose(var, ovar, rtol=0, atol=2e-6)
    tc = t - t.mean()
    assert cov._negativeloglikelihood(x, tc, th) == pytest.approx(orc.spgp_nll(x, tc, th, m), rel=1e-7)
    # Snelson's O(N m^2) likelihood agrees with the dense one as in the reference's test (tests.py:803)
    assert cov._negativeloglikelihood(x, tc, th) == pytest.approx(orc.spgp_generic_nll(x, tc, th, m), abs=2e-1 * max(1.0, m / 10.0))


def test_spgp_gradient_and_bad_arguments():
    g = _spgp_case("grid_m10")
    x, t, th, m = g["x"], g["t_raw"], g["theta"], int(g["m"])
    cov = sk.SPGPCovariance(m)
    tc = t - t.mean()
    gr = cov._d_nll_d_theta(x, tc, th)
    assert gr.shape == th.shape and np.all(np.isfinite(gr))
    # the analytic O(N m^2) gradient (gpx_spgp_nll_grad) against the oracle's (pinned to central differences of the
    # likelihood in tests/test_oracle_golden.py; the reference's own gradient does not run on Python 3: parity unpinned)
    og = orc.spgp_nll_grad(x, tc, th, m)
    np.testing.assert_allclose(gr, og, rtol=0, atol=1e-7 * np.abs(og).max())
    e = np.zeros(len(th)); e[0] = 1e-4
    fd = (orc.spgp_nll(x, tc, th + e, m) - orc.spgp_nll(x, tc, th - e, m)) / 2e-4
    assert gr[0] == pytest.approx(fd, rel=1e-5, abs=1e-5)
    with pytest.raises(ValueError):
        cov.cov_matrix(x, th[:-1])
    start = cov.get_theta(x, tc)
    assert start.shape == th.shape
    assert np.isfinite(cov._negativeloglikelihood(x, tc, start))


@pytest.mark.parametrize("N,d,m", [(300, 2, 7), (1500, 3, 130), (5000, 10, 257), (20000, 4, 300), (20480, 4, 300)])
def test_spgp_analytic_gradient_against_oracle(N, d, m):
    """gpx_spgp_nll_grad on ragged shapes: m below / across / above a 128-tile, d above one 8-coordinate chunk of the
    E-pass, N beyond the split-K threshold of the rank-N products -- where 20000 still runs unsplit (npad / 128 = 157 is prime)
    and 20480 splits."""
    rng = np.random.RandomState(N + m)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    t = t - t.mean()
    xb = x[rng.choice(N, m, replace=False)] + 0.05 * rng.randn(m, d)
    th = np.concatenate([np.log([1.7, 0.02]), np.log(rng.uniform(0.02, 0.08, d)), xb.ravel()])
    cov = sk.SPGPCovariance(m)
    gr = cov._d_nll_d_theta(x, t, th)
    nll = cov._negativeloglikelihood(x, t, th)
    assert nll == pytest.approx(orc.spgp_nll(x, t, th, m), rel=1e-9)
    og = orc.spgp_nll_grad(x, t, th, m)
    np.testing.assert_allclose(gr, og, rtol=0, atol=2e-7 * np.abs(og).max())
    # likelihood and gradient share their N m^2 part (spgp_snelson_prepare): a gradient right behind a likelihood on the same device model
    # (an L-BFGS step) finds it done, any other call in between clears it -- the same bits either way
    dev = cov._fit_model(x, t, th)
    assert (dev.split() >= 2) == (N == 20480)
    np.testing.assert_array_equal(cov._d_nll_d_theta(x, t, th), gr)            # behind the likelihood above
    assert dev.nll() == nll and dev.nll() == nll                                 # behind a gradient (reuses the factor of A), then behind a likelihood
    np.testing.assert_array_equal(dev.nll_grad(), gr)                            # behind likelihoods that followed a gradient (Z was overwritten: rebuilt)
    dev.predict(x[:5])                                                           # overwrites Z and the vector scratch
    np.testing.assert_array_equal(dev.nll_grad(), gr)
    np.testing.assert_array_equal(dev.nll_grad(), gr)                            # behind a gradient


def test_spgp_full_size_properties():
    """BASELINE config 5 shape (d = 8, m = 2048) at a reduced N: with the pseudo-inputs equal to a subset of the
    training inputs the SPGP predictor at those inputs reproduces the dense GP's there up to the jitter; variance stays
    within [0, v + vt]."""
    rng = np.random.RandomState(5)
    N, d, m = 8192, 8, 2048
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    th_gc = np.log(np.array([2.0, 0.01] + [0.04] * d))
    xb = x[:m].copy()
    th = np.concatenate([th_gc, xb.ravel()])
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), th)
    xs = rng.uniform(0, 10, (4096, d))
    mu, var = gp.estimate_many(xs)
    assert np.all(np.isfinite(mu)) and np.all(var > 0) and np.all(var <= 2.01 * (1 + 1e-9))
    # two query batches == one batch (chunking / padding independence)
    mu2, var2 = gp.estimate_many(xs[:1000])
    np.testing.assert_allclose(mu2, mu[:1000], rtol=0, atol=1e-10)
    np.testing.assert_allclose(var2, var[:1000], rtol=0, atol=1e-10)
    # with m = N (all inputs are pseudo-inputs) Q_N = K_N (K_N + 1e-5 I)^-1 K_N ~ K_N: the SPGP posterior collapses onto the dense one
    Ns = 1024
    xs_s = xs[:64]
    th_full = np.concatenate([th_gc, x[:Ns].ravel()])
    sp = sk.GaussianProcess(x[:Ns], t[:Ns], sk.SPGPCovariance(Ns), th_full)
    de = sk.GaussianProcess(x[:Ns], t[:Ns], sk.GaussianCovariance(), th_gc)
    ms, vs = sp.estimate_many(xs_s)
    md, vd = de.estimate_many(xs_s)
    np.testing.assert_allclose(ms, md, rtol=0, atol=5e-3)
    np.testing.assert_allclose(vs, vd, rtol=0, atol=5e-3)


@pytest.mark.parametrize("N", [20000, 20480])
def test_spgp_split_k_path(N):
    """From N = 16384 on the rank-N products (K_MN Lambda^-1 K_NM, A) may run split over K: one launch over equal chunks of whole
    128-tiles into partial buffers and a summation pass, the chunk count a divisor of npad / 128 (spgp_pick_split).  N = 20000 has
    npad / 128 = 157, a prime: no divisor, one plain launch; N = 20480 has 160 and splits (the rule gives 10 chunks).  Which of the
    two ran is asserted through gpx_spgp_split.  Snelson's likelihood against the oracle's O(N m^2) restatement, predictions against
    a numpy transcription of the Woodbury algebra (tests/_spgp_ld.py: woodbury_predict; no N x N matrix on either side)."""
    from _spgp_ld import woodbury_predict
    rng = np.random.RandomState(31)
    d, m = 4, 300
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    th_gc = np.log(np.array([2.0, 0.01] + [0.04] * d))
    xb = rng.uniform(0, 10, (m, d))
    th = np.concatenate([th_gc, xb.ravel()])
    xs = rng.uniform(0, 10, (50, d))
    cov = sk.SPGPCovariance(m)
    tc = t - t.mean()
    assert cov._negativeloglikelihood(x, tc, th) == pytest.approx(orc.spgp_nll(x, tc, th, m), rel=1e-8)
    gp = sk.GaussianProcess(x, t, cov, th.copy())
    mu, var = gp.estimate_many(xs)
    for dev in (cov._fit_model(x, tc, th), gp._dev()):
        chunks = dev.split()
        assert chunks == 0 if N == 20000 else chunks >= 2, chunks
    want_mu, want_var = woodbury_predict(x, tc, th, m, xs)
    want_mu = want_mu + t.mean()
    np.testing.assert_allclose(mu, want_mu, rtol=0, atol=2e-5)
    np.testing.assert_allclose(var, want_var, rtol=0, atol=2e-6)


def test_c5_spgp_full_size_against_oracle():
    """BASELINE config 5 at FULL size (N = 262144, M = 2048 pseudo-inputs, d = 8) on one GPU: Snelson's likelihood against
    the oracle (chunked over N: O(N M^2) = 2.2e12 flop on the host) and the predictor against a numpy transcription of the
    Woodbury algebra (Covariance.py:835-863 folded into GaussianProcess.estimate_many), both chunked so that no N x M
    temporary of more than 0.5 GB lives on the host."""
    from scipy.linalg import cholesky, solve_triangular
    N, d, m = 262144, 8, 2048
    rng = np.random.RandomState(20240 + N + d)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (256, d))
    th_gc = np.log(np.array([2.0, 0.01] + [0.04] * d))
    xb = x[rng.choice(N, m, replace=False)].copy()
    th = np.concatenate([th_gc, xb.ravel()])
    cov = sk.SPGPCovariance(m)
    tc = t - t.mean()
    assert cov._negativeloglikelihood(x, tc, th) == pytest.approx(orc.spgp_nll_chunked(x, tc, th, m), rel=1e-8)
    gp = sk.GaussianProcess(x, t, cov, th.copy())
    mu, var = gp.estimate_many(xs)
    Km = orc.gram_ij(xb, xb, th_gc) + 1e-5 * np.eye(m)
    Lm = cholesky(Km, lower=True)
    B = Km.copy()
    rhs = np.zeros(m)
    for c0 in range(0, N, 32768):
        Kc = orc.gram_ij(xb, x[c0:c0 + 32768], th_gc)                          # K_MN chunk
        lam = 2.0 + 0.01 - (solve_triangular(Lm, Kc, lower=True) ** 2).sum(0)
        B += (Kc / lam).dot(Kc.T)
        rhs += (Kc / lam).dot(tc[c0:c0 + 32768])
    Lb = cholesky(B, lower=True)
    beta = solve_triangular(Lb, solve_triangular(Lb, rhs, lower=True), lower=True, trans=1)
    Ks = orc.gram_ij(xs, xb, th_gc)
    want_mu = Ks.dot(beta) + t.mean()
    want_var = 2.01 - (solve_triangular(Lm, Ks.T, lower=True) ** 2).sum(0) + (solve_triangular(Lb, Ks.T, lower=True) ** 2).sum(0)
    np.testing.assert_allclose(mu, want_mu, rtol=0, atol=5e-5)
    np.testing.assert_allclose(var, want_var, rtol=0, atol=5e-6)
    del gp
    _gpx.lib.gpx_pool_trim()


def test_approx_propagation_solve_path_equals_kinv_path():
    """The first new-u propagations after a fit are served by two triangular solves on the right-hand-side block
    (no K^-1); once K^-1 exists the one-pass kernel takes over.  Both must give the reference's numbers."""
    g = load_golden("n256_d8")
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    up = sk.UncertaintyPropagationApprox(gp)
    u0, S0 = g["u0"], g["Sigma0"]
    u1 = u0 + 0.37
    a0 = up.propagate_GA(u0, S0)                 # triangular-solve path
    a1 = up.propagate_GA(u1, S0)
    d0 = [up._get_variance_dv_h(u0, h) for h in range(len(u0))]
    _ = gp.Kinv                                  # materialises K^-1 on the device
    b1 = up.propagate_GA(u1, S0)                 # K^-1 pass
    b0 = up.propagate_GA(u0, S0)
    e0 = [up._get_variance_dv_h(u0, h) for h in range(len(u0))]
    v = np.exp(g["theta"][0])
    assert a0 == pytest.approx(b0, abs=1e-10 * v) and a1 == pytest.approx(b1, abs=1e-10 * v)
    assert d0 == pytest.approx(e0, abs=1e-9 * v)
    assert a0[0] == pytest.approx(float(g["approx_u0_S0"][0]), abs=1e-9)
    assert a0[1] == pytest.approx(float(g["approx_u0_S0"][1]), abs=1e-8 * v)


@pytest.mark.parametrize("N,d,nrhs", [(100, 2, 1), (1024, 3, 9), (1100, 4, 17), (2500, 5, 40), (3072, 2, 16), (4224, 3, 20)])
def test_solve_few_right_hand_sides_against_oracle(N, d, nrhs):
    """gpx_solve = the fat-step triangular solver behind alpha and the post-fit propagation: one, exactly eight, nine and
    more 128-blocks (whole and partial 1024-row steps), one and two groups of 16 right-hand sides, more than 32."""
    import scipy.linalg
    rng = np.random.RandomState(7 + N + nrhs)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    og = orc.OracleGP(x, t, theta)
    B = rng.randn(nrhs, N)
    kb, lb = gp._dev().solve(B, want_linv=True)
    K = orc.gram(x, theta)
    Lo = np.linalg.cholesky(K)
    lo = scipy.linalg.solve_triangular(Lo, B.T, lower=True).T
    np.testing.assert_allclose(lb, lo, rtol=0, atol=1e-9 * np.abs(lo).max())
    ko = og.Kinv.dot(B.T).T
    np.testing.assert_allclose(kb, ko, rtol=0, atol=1e-7 * np.abs(ko).max())
    # residual of the solve itself: K (K^-1 b) = b
    np.testing.assert_allclose(K.dot(kb.T).T, B, rtol=0, atol=1e-8 * np.abs(kb).max())


@pytest.mark.parametrize("N", [1100, 2500, 4224, 5000])
def test_kinv_with_inverted_squares_as_leaves(N):
    """K^-1 = L^-T L^-1 through the recursion whose leaves are the few-vector solver's inverted 1024 x 1024 squares (tsolve.hip,
    build_kinv_from_solver): two to five column slabs, whole and partial last squares, against the oracle's inverse entry by entry
    and as K K^-1 = I."""
    d = 3
    rng = np.random.RandomState(11 + N)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    Kinv = gp.Kinv
    K = orc.gram(x, theta)
    ref = np.linalg.inv(K)
    np.testing.assert_allclose(Kinv, ref, rtol=0, atol=1e-7 * np.abs(ref).max())
    np.testing.assert_allclose(Kinv, Kinv.T, rtol=0, atol=0)
    np.testing.assert_allclose(K.dot(Kinv), np.eye(N), rtol=0, atol=1e-7)


@pytest.mark.parametrize("N,ranges", [(2500, [(0, 1024), (1024, 2048), (128, 2432), (2432, 2500)]), (4224, [(1152, 3200), (3072, 4224)])])
def test_kinv_row_panel_equals_rows_of_the_whole_inverse(N, ranges):
    """gpx_kinv_rows (TriSolver::kinv_rows): a row panel of K^-1 built alone -- E^T L^-T by the many-right-hand-side solve, then the
    mirror-image sweep through transposed panels of L -- against numpy's inverse of the oracle Gram: panels that start / end inside a
    1024 square, cover several squares, and reach into the padding of the last one; then the row-sharded propagations that read it."""
    d = 3
    rng = np.random.RandomState(5 + N)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    ref = np.linalg.inv(orc.gram(x, theta))
    scale = np.abs(ref).max()
    for r0, r1 in ranges:
        gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())     # a fresh handle: no whole K^-1 to fall back on
        rows = gp._dev().kinv_rows(r0, r1)
        np.testing.assert_allclose(rows, ref[r0:r1], rtol=0, atol=1e-7 * scale)
        gp._dev().close()
    # the partial sums of the row-sharded propagation from panels alone add up to the single-call result
    u, S = np.full(d, 5.0), 0.01 * np.eye(d)
    cuts = [0] + [r1 for _r0, r1 in ranges if r1 < N][:1] + [N]
    cuts = sorted(set(c - c % 128 if c < N else c for c in cuts))
    def approx_rows(g, a, b):
        part = np.zeros(4 + 2 * d)
        _gpx.check(_gpx.lib.gpx_propagate_approx_rows(g._dev().handle, _gpx.ptr(u), _gpx.ptr(S), a, b, _gpx.ptr(part)), "approx_rows")
        return part

    def exact_rows(g, a, b):
        part = np.zeros(3)
        _gpx.check(_gpx.lib.gpx_propagate_exact_rows(g._dev().handle, _gpx.ptr(u), _gpx.ptr(S), a, b, _gpx.ptr(part)), "exact_rows")
        return part

    parts_a, parts_e = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):     # one handle per "rank": each builds its own panel, Approx first, then Exact on the same rows
        g = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
        parts_a.append(approx_rows(g, a, b))
        parts_e.append(exact_rows(g, a, b))
        g._dev().close()
    whole = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    wa = approx_rows(whole, 0, N)
    we = exact_rows(whole, 0, N)
    np.testing.assert_allclose(np.sum(parts_a, axis=0), wa, rtol=1e-9, atol=1e-9 * np.abs(wa).max())
    np.testing.assert_allclose(np.sum(parts_e, axis=0)[:2], np.asarray(we)[:2], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("N,d,k", [(64, 2, 3), (1300, 3, 33)])
def test_get_realisation_is_L_times_z(N, d, k):
    """f4 (GaussianProcess.py:44-57): the draw is t = L z with K = cov_matrix(x, theta) assembled and factored on the GPU
    and z from numpy's global generator -- given the same z it must equal cholesky(oracle Gram) z."""
    rng = np.random.RandomState(3 + N)
    x = rng.uniform(0, 10, (N, d))
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    Lo = np.linalg.cholesky(orc.gram(x, theta))
    np.random.seed(1234)
    draws = sk.GaussianProcess.get_realisation(x, sk.GaussianCovariance(), theta, size=k)
    np.random.seed(1234)
    z = np.random.standard_normal((k, N))
    assert draws.shape == (k, N)
    np.testing.assert_allclose(draws, z.dot(Lo.T), rtol=0, atol=1e-10 * np.abs(draws).max())
    np.random.seed(99)
    one = sk.GaussianProcess.get_realisation(x, sk.GaussianCovariance(), theta)     # the reference's signature
    np.random.seed(99)
    np.testing.assert_allclose(one, Lo.dot(np.random.standard_normal(N)), rtol=0, atol=1e-10 * np.abs(one).max())


def test_get_realisation_distribution():
    """Sample covariance of 4000 draws at N = 64 against K (the only parity the reference's SVD-based sampler allows:
    its random stream cannot be reproduced).  Entry-wise standard error of a sample covariance is
    sqrt((K_ii K_jj + K_ij^2) / n) <= 2.01 sqrt(2 / 4000) = 0.045; 5 sigma."""
    rng = np.random.RandomState(11)
    x = rng.uniform(0, 10, (64, 2))
    theta = np.log(np.array([2.0, 0.01, 0.04, 0.04]))
    K = orc.gram(x, theta)
    np.random.seed(2024)
    T = sk.GaussianProcess.get_realisation(x, sk.GaussianCovariance(), theta, size=4000)
    assert abs(T.mean(0)).max() < 5 * np.sqrt(2.01 / 4000)
    S = T.T.dot(T) / 4000
    assert abs(S - K).max() < 5 * 2.01 * np.sqrt(2.0 / 4000)


@pytest.mark.parametrize("M,N,K", [(256, 384, 48), (384, 1408, 64), (2048, 3072, 32), (512, 1024, 640)])   # (the last: 32 x 32 tiles with full columns on the left)
def test_gemm_nt_trapezoid(M, N, K):
    """lower_only with N > M: the first N - M columns are full, the remaining square is lower-triangular by 128-tiles
    (the Cholesky's merged trailing update); tiles above that staircase must stay untouched."""
    rng = np.random.RandomState(M + N + K)
    A, B, C0 = rng.randn(M, K), rng.randn(N, K), rng.randn(M, N)
    a, b, c = _dev(A), _dev(B), _dev(C0)
    _gpx.check(_gpx.lib.gpx_dev_gemm_nt(_p(a), K, _p(b), K, _p(c), N, M, N, K, -1.0, 1.0, 1, None), "gemm")
    torch.cuda.synchronize()
    got = c.cpu().numpy()
    want = C0 - A.dot(B.T)
    off = N - M
    for bi in range(M // 128):
        r = slice(128 * bi, 128 * bi + 128)
        for bj in range(N // 128):
            cs = slice(128 * bj, 128 * bj + 128)
            if 128 * bj < off + 128 * bi:          # strictly inside the trapezoid
                np.testing.assert_allclose(got[r, cs], want[r, cs], rtol=1e-13, atol=1e-12)
            elif 128 * bj > off + 128 * bi:        # above the staircase: untouched
                np.testing.assert_array_equal(got[r, cs], C0[r, cs])
            else:                                    # staircase tile: at least its lower triangle is updated
                il = np.tril_indices(128)
                np.testing.assert_allclose(got[r, cs][il], want[r, cs][il], rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize("N,d,M,seed", [(2500, 32, 100, 1), (3000, 1, 257, 2), (5000, 16, 300, 3), (1153, 64, 64, 4), (2049, 2, 1025, 5)])
def test_against_oracle_sweep_random_theta(N, d, M, seed):
    """fresh seeded inputs with random hyper-parameters, input dimensions up to GPX_MAX_D = 64, sizes that cross the
    look-ahead factorisation's panel boundaries (N > 1024) and are not tile multiples."""
    rng = np.random.RandomState(7000 + seed)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (M, d))
    theta = np.concatenate([[rng.uniform(-0.5, 1.0), rng.uniform(-5.0, -3.0)], rng.uniform(-4.5, -2.5, d) - np.log(d) / 2])
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    og = orc.OracleGP(x, t, theta)
    mean, var = gp.estimate_many(xs)
    om, ov = og.estimate_many(xs)
    v = np.exp(theta[0])
    np.testing.assert_allclose(mean, om, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(var, ov, rtol=1e-6, atol=1e-8 * v)
    assert gp._dev().logdet() == pytest.approx(og.logdet(), rel=1e-9, abs=1e-6)
    u = xs[1 % M]
    S = np.diag(rng.uniform(0.005, 0.05, d))
    ma, va = sk.UncertaintyPropagationApprox(gp).propagate_GA(u, S)
    oma, ova = orc.approx_propagate(og, u, S)
    assert ma == pytest.approx(oma, abs=1e-8) and va == pytest.approx(ova, abs=1e-7 * v)
    me, ve = sk.UncertaintyPropagationExact(gp).propagate_GA(u, S)
    ome, ove = orc.exact_propagate(og, u, S)
    assert me == pytest.approx(ome, abs=1e-8) and ve == pytest.approx(ove, abs=1e-7 * v)


def test_pool_trim_releases_cached_buffers():
    """gpx_free parks device buffers in the library's cache; gpx_pool_trim hands them back to the driver (it is also the
    out-of-memory retry path of every allocation) and the library keeps working afterwards."""
    g = load_golden("n256_d8")
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    m0, _ = gp.estimate_many(g["xs"][:5])
    _ = gp.Kinv                                                          # a few MB more in the cache
    gp._dev().close()
    cached = torch.cuda.mem_get_info()[0]
    assert _gpx.lib.gpx_pool_trim() == 0
    assert torch.cuda.mem_get_info()[0] >= cached + (1 << 20)            # the parked factor / K^-1 / workspaces went back
    assert _gpx.lib.gpx_pool_trim() == 0                                 # idempotent on an empty cache
    gp2 = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    np.testing.assert_array_equal(gp2.estimate_many(g["xs"][:5])[0], m0)


def test_spgp_ml_fit_like_reference_test_gp_2d():
    """the reference's test_gp_2D with SPGPCovariance(10) (skgpuppy/tests/tests.py:708-747; it errors on Python 3 inside the
    reference's analytic SPGP gradient): the default constructor runs the ML fit and the predictor stays within a few
    sigma of the generating surface."""
    g = load_golden("kat1_grid")
    x, t = g["x"], g["ml_t_raw"]
    np.random.seed(3)
    cov = sk.SPGPCovariance(10)
    start = cov.get_theta(x, t - t.mean())
    nll0 = cov._negativeloglikelihood(x, t - t.mean(), start)
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(10))          # L-BFGS-B on Snelson's likelihood
    nll1 = gp.cov._negativeloglikelihood(x, gp.t, gp.theta_min)
    assert np.isfinite(nll1) and nll1 <= nll0 + 1e-6
    mu, var = gp.estimate_many(x)
    assert np.all(var > 0)
    resid = np.abs(mu - t)
    assert np.mean(resid < 5 * np.sqrt(var)) > 0.9


def test_two_threads_two_handles():
    """SURVEY.md 8b threading contract: a handle is single-owner, distinct handles may be driven from distinct threads
    (ctypes releases the GIL; the allocator and stream caches are shared)."""
    import threading
    g = load_golden("n1000_d4")
    ref = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy()).estimate_many(g["xs"])
    errs = []

    def work(seed):
        try:
            for _ in range(6):
                gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
                m, v = gp.estimate_many(g["xs"])
                np.testing.assert_array_equal(m, ref[0])
                np.testing.assert_array_equal(v, ref[1])
                up = sk.UncertaintyPropagationApprox(gp).propagate_GA(g["u0"], g["Sigma0"])
                assert up[0] == pytest.approx(float(g["approx_u0_S0"][0]), abs=1e-9)
                gp._dev().close()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs


_CONCURRENT_FITS_WORKER = r"""
import sys, time, threading, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(pkg)r)
import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
theta = np.log(np.array([2.0, 0.01] + [0.04] * 8))
def data(N, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 10, (N, 8))
    return x, np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
jobs = {0: [(12288, 1), (12288, 2), (12288, 3), (16384, 4)], 1: [(12288, 5), (12288, 6), (12288, 7), (16384, 8)]}
def fit(N, seed):
    x, t = data(N, seed)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    beta, jit = gp._get_beta(), gp._dev().jitter()
    gp._dev().close()
    assert jit == 0.0
    return beta
fit(12288, 99); fit(16384, 98)                 # allocator, stream probes
t0 = time.perf_counter()
serial = {k: [fit(N, sd) for N, sd in v] for k, v in jobs.items()}
t_serial = time.perf_counter() - t0
out, errs = {}, []
def work(k):
    try:
        _gpx.check(_gpx.lib.gpx_set_device(0), "gpx_set_device")
        out[k] = [fit(N, sd) for N, sd in jobs[k]]
    except Exception as e:
        errs.append(repr(e))
ths = [threading.Thread(target=work, args=(k,)) for k in jobs]
t0 = time.perf_counter()
[t.start() for t in ths]; [t.join() for t in ths]
t_conc = time.perf_counter() - t0
assert not errs, errs
worst = 0.0
for k in jobs:
    for a, b in zip(serial[k], out[k]):
        worst = max(worst, float(np.abs(a - b).max()) / float(np.abs(a).max()))
print("SERIAL_SECONDS %%.4f" %% t_serial)
print("CONCURRENT_SECONDS %%.4f" %% t_conc)
print("WORST_REL_DIFF %%.3e" %% worst)
"""


def test_two_threads_large_fits_do_not_stall():
    """SURVEY.md 8b threading row at sizes that take the whole look-ahead machinery (CU blockers, square launches that hold whole CUs,
    kernels that wait for kernels of other streams): two host threads, each three fits at N = 12288 and one at 16384 on handles of
    its own, at the same time.  No in-kernel hand-off may stall (GPX_DEBUG would say so: a stall costs 5 s and a refit), alpha must
    be the serial run's (bit for bit when no fit took a fall-back schedule), and running side by side must not cost more than 1.55x the
    serial sum.  The reference's objects are plain Python and freely concurrent (GaussianProcess.py:19-41)."""
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CONCURRENT_FITS_WORKER % {"root": ROOT, "pkg": os.path.join(ROOT, "scikit-gpuppy_amd")}
    env = dict(os.environ)
    env["GPX_DEBUG"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "hand-off stalled" not in r.stderr, r.stderr[-3000:]
    val = {l.split()[0]: float(l.split()[1]) for l in r.stdout.splitlines() if l.split() and l.split()[0].endswith(("SECONDS", "DIFF"))}
    print("two threads, large fits:", val)
    assert val["WORST_REL_DIFF"] <= 1e-10, val       # (a thread whose stream pair was probed under load may take the serialised schedule: same factor to rounding)
    # measured (profiles/r06_concurrent_fits_ratio.txt): 1.08-1.28 x the serial sum since only one look-ahead fit runs per device at a
    # time; the bound is the worst measured ratio + 20 % (it was 2.5 x, and the schedule before that fix ran at 3.3 x)
    assert val["CONCURRENT_SECONDS"] <= 1.55 * val["SERIAL_SECONDS"] + 0.05, val


def test_jitter_fallback_on_the_lookahead_path():
    """same fallback at a size that takes the multi-stream look-ahead factorisation with pipelined panel solves
    (N > 1024): a cluster of near-duplicates in the THIRD panel makes a pivot non-positive well into the factorisation;
    the first attempt must report it (not hang, not return garbage) and the retry on K + 1e-5 I must succeed; non-finite
    hyper-parameters are refused."""
    rng = np.random.RandomState(11)
    N, d = 3000, 3
    x = rng.uniform(0, 10, (N, d))
    x[2300:2420] = x[2300] + 1e-9 * rng.randn(120, d)          # 120 numerically identical rows
    t = np.sin(x.sum(1))
    theta = np.array([0.5, -np.inf, -1.0, -1.0, -1.0])          # vt = 0
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta)
    assert gp._dev().jitter() == 1e-5
    mean, var = gp.estimate_many(x[:50])
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    with np.errstate(divide="ignore"):
        og_K = orc.gram(x, theta) + 1e-5 * np.eye(N)
    alpha = np.linalg.solve(og_K, t - t.mean())
    np.testing.assert_allclose(gp._get_beta(), alpha, rtol=0, atol=1e-5 * np.abs(alpha).max())
    xx = x.copy()
    xx[:, :] = xx[0]                                             # all inputs identical: K = v 11^T, rank one
    gp2 = sk.GaussianProcess(xx, t, sk.GaussianCovariance(), theta)
    assert gp2._dev().jitter() == 1e-5
    with pytest.raises(ValueError):      # scipy.linalg.inv's check_finite raises ValueError in the reference as well
        sk.GaussianProcess(x, t, sk.GaussianCovariance(), np.array([np.nan, -1.0, -1.0, -1.0, -1.0]))


# ------------------------------------------------------------------------------------------------
# operator surface: derivative Grams, log det, quadratic-form helpers
# ------------------------------------------------------------------------------------------------
def test_derivative_grams_and_logdet_golden():
    """GaussianCovariance._d_cov_matrix_d_theta(_ij), _d_cov_d_theta, _log_det_cov_matrix against the reference's own outputs
    (skgpuppy/Covariance.py:485-512, :605-657, :189-195; fixtures from tools/gen_golden.py)."""
    g = load_golden("gram")
    cov = sk.GaussianCovariance()
    for name, sq in (("n257_d5", True), ("rect_33x257_d5", False), ("n130_d1", True)):
        xi, xj, th = g[name + "__xi"], g[name + "__xj"], g[name + "__theta"]
        if name == "n257_d5":
            xi = xj = xi[:130]
        for j in range(len(th)):
            want = g["%s__dKij_%d" % (name, j)]
            got = cov._d_cov_matrix_d_theta_ij(xi, xj, th, j)
            np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13 * np.abs(want).max() + 1e-300, err_msg="%s j=%d" % (name, j))
            if sq and ("%s__dK_%d" % (name, j)) in g:
                np.testing.assert_allclose(cov._d_cov_matrix_d_theta(xi, th, j), g["%s__dK_%d" % (name, j)], rtol=1e-11, atol=1e-13)
        if sq:
            assert abs(cov._log_det_cov_matrix(xi, th) - float(g[name + "__logdet"])) < 1e-8 * max(1.0, abs(float(g[name + "__logdet"])))
            # the base-class route (Cholesky of the operator's own matrix on the GPU) agrees
            assert abs(sk.Covariance._log_det_cov_matrix(cov, xi, th) - float(g[name + "__logdet"])) < 1e-8 * max(1.0, abs(float(g[name + "__logdet"])))
    th = g["scalar__theta"]
    for (a, b), want in zip(g["scalar__pairs"], g["scalar__dcov"]):
        for j in range(len(th)):
            assert abs(cov._d_cov_d_theta(a, b, th, j) - want[j]) <= 1e-13 * max(1.0, abs(want[j]))


def test_gaussian_cov_derivative_mirrors_reference_test():
    """skgpuppy/tests/tests.py:485-503: the closed-form scalar derivative against the base class's central difference, delta 1e-3"""
    x = np.atleast_2d(np.linspace(0, 10, 50)).T
    theta = np.log(np.array([2.0, 0.01, 0.02]))
    cov = sk.GaussianCovariance()
    for xi in x[::7]:
        for xj in x[::5]:
            for j in range(3):
                assert abs(sk.Covariance._d_cov_d_theta(cov, xi, xj, theta, j) - cov._d_cov_d_theta(xi, xj, theta, j)) < 1e-3
    # and the generic matrix form built from it agrees with the closed-form derivative Gram
    xs = x[::10]
    for j in (0, 2):
        np.testing.assert_allclose(sk.Covariance._d_cov_matrix_d_theta_ij(cov, xs, xs, theta, j), cov._d_cov_matrix_d_theta_ij(xs, xs, theta, j),
                                   atol=1e-6)


def test_approx_helper_methods_golden(case):
    """_get_sigma2 / _get_variance_rest / _get_sigma2_and_variance_rest (UncertaintyPropagation.py:412-488) against the oracle's
    parts, and the Exact class's scalar correction factors against the oracle's l_i / L_ij building blocks."""
    name, g, gp = case
    og = orc.OracleGP(g["x"], g["t_raw"], g["theta"])
    k = _loose(name)
    up = sk.UncertaintyPropagationApprox(gp)
    d = gp.d
    for iu in range(int(g["nu"])):
        u = g["u%d" % iu]
        for iS in range(int(g["nS"])):
            S = g["Sigma%d" % iS]
            _m, o_s2, o_rest = orc.approx_parts(og, u, S)
            s2, rest = up._get_sigma2_and_variance_rest(u, S, gp.Kinv, gp.x, gp._get_beta())
            tol = 1e-8 * gp._get_v() * k
            assert abs(s2 - o_s2) < tol and abs(rest - o_rest) < tol
            assert abs(up._get_sigma2(u, gp.Kinv, gp.x, up.C_ux, up.J_ux, up.H_ux) - o_s2) < tol
            assert abs(up._get_variance_rest(u, S, gp.Kinv, gp.x, gp._get_beta(), up.C_ux, up.J_ux, up.H_ux) - o_rest) < tol
            # the reference's own number that is made of exactly these two: _getFactor = (v_out - sigma2) / rest
            assert (float(g["v_out"]) - s2) / rest == pytest.approx(float(g["factor_u%d_S%d" % (iu, iS)]), rel=1e-5 * k)
    ue = sk.UncertaintyPropagationExact(gp)
    u, S = g["u0"], g["Sigma0"]
    ue.propagate_GA(u, S)
    w = np.exp(g["theta"][2:2 + d])
    a = u - np.asarray(g["x"], dtype=float)[3]
    Delta_inv = np.diag(w) - np.diag(w / (1 + w * np.diag(S)))
    want1 = np.exp(0.5 * a @ Delta_inv @ a) / np.sqrt(np.linalg.det(np.eye(d) + np.diag(w) * S))
    Lam_inv = 2 * np.diag(w) - np.linalg.inv(0.5 * np.diag(1 / w) + S)
    want2 = np.exp(0.5 * a @ Lam_inv @ a) / np.sqrt(np.linalg.det(2 * np.diag(w) * S + np.eye(d)))
    assert abs(ue._get_C_corr(u, g["x"][3]) - want1) <= 1e-12 * abs(want1)
    assert abs(ue._get_C_corr2(u, g["x"][3]) - want2) <= 1e-12 * abs(want2)


# ------------------------------------------------------------------------------------------------
# the stream schedule of the factorisation has no race: identical inputs give bit-identical factors
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(16384, 8200, 16384, 12000, 16384, 12000, 8200), (65536, 65536, 65536)])
def test_fit_is_bit_reproducible(sizes):
    """No atomics in the arithmetic and fixed reduction orders: K^-1 t and the predictions of repeated fits of the same problem must
    agree to the last bit, whatever ran before (other sizes, propagation, K^-1, pool trims).  A difference means a race between the
    streams of the look-ahead factorisation (chain, column solves, trapezoid update with its in-kernel hand-off, CU reservation) or
    between the waves of a kernel -- a missing barrier in the leaf (one wrong factor in ~50 fits) was caught exactly this way."""
    first = {}
    d = 8
    for r, N in enumerate(sizes):
        x, t, xs, theta = _recipe(N, d, 64)
        gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
        if r % 3 == 1:
            sk.UncertaintyPropagationApprox(gp).propagate_GA(np.full(d, 5.0), 0.01 * np.eye(d))
        mean, var = gp.estimate_many(xs)
        beta = gp._get_beta()
        gp._dev().close()
        if r % 4 == 3:
            _gpx.lib.gpx_pool_trim()
        if N not in first:
            first[N] = (beta, mean, var)
        else:
            np.testing.assert_array_equal(beta, first[N][0])
            np.testing.assert_array_equal(mean, first[N][1])
            np.testing.assert_array_equal(var, first[N][2])
    _gpx.lib.gpx_pool_trim()


# ------------------------------------------------------------------------------------------------
# the factorisation's fall-back schedules: same numbers, no stall
# ------------------------------------------------------------------------------------------------
_SCHEDULE_WORKER = r"""
import sys, time, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(pkg)r)
import skgpuppy_amd as sk
rng = np.random.RandomState(5)
N, d = 12288, 8
x = rng.uniform(0, 10, (N, d)); t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
best = 1e9
for rep in range(3):
    a = time.perf_counter()
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    best = min(best, time.perf_counter() - a)
    beta = gp._get_beta()
    jit = gp._dev().jitter()
    gp._dev().close()
np.save(sys.argv[1], beta)
print("FIT_SECONDS %%.4f" %% best)
print("JITTER %%g" %% jit)
"""


@pytest.mark.gpu
def test_fallback_schedules_agree_and_do_not_stall(tmp_path):
    """The look-ahead factorisation has kernels that wait for kernels of other streams (CU blockers, the trapezoid launch's counters).
    When the streams cannot run side by side -- a profiler that serialises kernels, or a process whose streams share a hardware queue
    (forced here by putting all of the fit's streams into one priority class) -- the library must detect it and fall back, not sit out
    its time limits (measured before the per-pair probes: 371 ms per fit instead of 28).  Every schedule must give the same alpha."""
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variants = {"default": {}, "one_priority_class": {"GPX_SIDE_PRIO": "0", "GPX_BLK_PRIO": "0"}, "serialised": {"GPX_CONCURRENT_STREAMS": "0"},
                "alpha_after_the_factorisation": {"GPX_FIT_RIDE": "0"},
                # the diagonal chain as one square launch of the dataflow kernel per panel: nowhere / everywhere (default: first panel + tail)
                "launch_per_step_chains": {"GPX_SQK_FROM": "-1"}, "square_kernel_everywhere": {"GPX_SQK_FROM": "0", "GPX_RESERVE_CUS": "0"}}
    code = _SCHEDULE_WORKER % {"root": ROOT, "pkg": os.path.join(ROOT, "scikit-gpuppy_amd")}
    betas, secs = {}, {}
    for name, extra in variants.items():
        env = dict(os.environ)
        env.update(extra)
        out = tmp_path / (name + ".npy")
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        secs[name] = float([l for l in r.stdout.splitlines() if l.startswith("FIT_SECONDS")][-1].split()[1])
        betas[name] = np.load(out)
    print("fit seconds by schedule:", secs)
    for name in variants:
        # (the schedules differ in how the trailing update is cut into launches, not in any tile's arithmetic: alpha agrees to rounding)
        np.testing.assert_allclose(betas[name], betas["default"], rtol=0, atol=1e-9 * np.abs(betas["default"]).max())
        assert secs[name] < 5 * secs["default"] + 0.02, (name, secs)


@pytest.mark.gpu
def test_stalled_handoff_is_answered_by_a_plain_refit_not_by_jitter(tmp_path):
    """An in-kernel wait of the look-ahead schedule that expires (GPX_TEST_FORCE_STALL: the first wait of the process asks for a count
    that never comes and gives up after 10 us) sets the factorisation's STALL word, not the potrf status: the fit must discard that
    factor and repeat it on the plain schedule -- same alpha as an undisturbed fit, NO jitter (round 3 mapped the timeout onto the
    'not positive definite' code and silently refitted K + 1e-5 I)."""
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _SCHEDULE_WORKER % {"root": ROOT, "pkg": os.path.join(ROOT, "scikit-gpuppy_amd")}
    betas = {}
    for name, extra in {"default": {}, "forced_stall": {"GPX_TEST_FORCE_STALL": "1", "GPX_DEBUG": "1"}}.items():
        env = dict(os.environ)
        env.update(extra)
        out = tmp_path / (name + ".npy")
        r = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        assert [l for l in r.stdout.splitlines() if l.startswith("JITTER")][-1].split()[1] == "0", r.stdout
        if name == "forced_stall":
            assert "hand-off stalled: refit on the plain schedule" in r.stderr, r.stderr[-2000:]
        betas[name] = np.load(out)
    np.testing.assert_allclose(betas["forced_stall"], betas["default"], rtol=0, atol=1e-9 * np.abs(betas["default"]).max())
