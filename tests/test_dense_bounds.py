"""The N^2 reduction kernels of the dense GP (scikit-gpuppy_amd/csrc/propagate.hip, fit.hip) against a long-double model of the same sums,
each sum on the scale of its own absolute terms, under the bound measured on the float64 numpy evaluation of the same case
(tests/_dense_ld.py: the model, the inputs, the rule; tests/test_dense_ld_model.py: the model is right and the rule sees seeded defects).

Every sum is judged on the device's OWN K^-1 and alpha (gpx_kinv, gpx_alpha), so the condition of K does not enter and a term-level defect
of 1e-9 does not hide behind it.  kinv() is called before the row-sharded entry points: they then read that whole K^-1.

Which case reaches which instantiation (launch_nll_grad / launch_exact_sum dispatch on d, launch_kinv_pass on the vector count):
  nll_grad_kernel<2|4|8|16|32|64>   test_gradient at d = 1, 2 | 3, 4 | 5, 8 | 9, 16 | 17, 32 | 33, 64
  exact_sum_kernel<2|..|64>         test_exact at the same d; <2> and <4> also by test_exact_explicit_* (d = 1, 3)
  kinv_pass_kernel<9,8>             test_approx at d <= 8 (d + 1 vectors), test_symv at nrhs = 1, 9
  kinv_pass_kernel<17,4>            test_approx at d = 9, 16, test_symv at nrhs = 10, 17
  kinv_pass_kernel<33,2>            test_approx at d = 17, 32, test_symv at nrhs = 18, 33
  kinv_pass_kernel<65,1>            test_approx at d = 33, 64, test_symv at nrhs = 34, 64
Shapes: N = 700 (npad 768: 68 padded rows, more than one stride of 256 and of 512), 200 (a single partial stride), 128 (no padding),
129 (127 padded rows); every d of D_ALL at N = 700, d = 1, 3, 8 at the others.

With GPX_DENSE_BOUNDS_RECORD=<file> every comparison appends its rho_ref, the bound and each group's worst ratio to both
(profiles/r10_dense_bounds.txt is such a record)."""
import contextlib
import ctypes

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

from skgpuppy_amd import _gpx
from skgpuppy_amd.GaussianProcess import _DeviceModel
from oracle import oracle as orc

import _dense_ld as dl

pytestmark = pytest.mark.gpu

IDS = ["n%d_d%d" % c for c in dl.CASES]
U64 = 2.0 ** -53


class Fit(object):
    """one _DeviceModel per case, with the K^-1 and alpha the device hands back"""

    def __init__(self, N, d, sharp=False):
        self.N, self.d = N, d
        self.seed = dl.seed_of(N, d)
        self.x, self.t, self.theta = dl.make_case(N, d, self.seed, sharp)
        self.name = "N=%d d=%d%s" % (N, d, " sharp" if sharp else "")
        self.model = _DeviceModel(_gpx.f64(self.x), _gpx.f64(self.t), _gpx.f64(self.theta))
        self.Kinv = self.model.kinv()
        self.alpha = self.model.alpha()
        self.h = self.model.handle
        self.args = (self.x, self.theta, self.Kinv, self.alpha)


@contextlib.contextmanager
def fit(N, d, sharp=False):
    f = None
    try:
        f = Fit(N, d, sharp)
        yield f
    finally:
        if f is not None and getattr(f, "model", None) is not None:
            f.model.close()
        _gpx.lib.gpx_pool_trim()


def check(title, name, got, want, ref):
    """got {group: values} against want {group: (values, scales)} under the bound of ref, the float64 evaluation of the same sums"""
    ref_dist = {k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in got}
    rho = dl.rho_of(ref_dist)
    for k, g in got.items():
        assert np.all(np.isfinite(g)), (title, name, k, g)
    dist = {k: dl.distances(g, want[k][0], want[k][1]) for k, g in got.items()}
    dl.record(title, name, rho, dist, ref_dist)
    return dl.assert_within(dist, rho, what=title + " " + name)


def both(fn, *args, **kw):
    return fn(*args, **kw), fn(*args, dt=np.float64, **kw)


def _dbl(n=1):
    return [ctypes.c_double() for _ in range(n)]


# ------------------------------------------------------------------------------------------------
# a. / b. the gradient
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", dl.CASES, ids=IDS)
def test_gradient(N, d):
    with fit(N, d) as f:
        g = np.empty(d + 2)
        _gpx.check(_gpx.lib.gpx_nll_grad(f.h, _gpx.ptr(g)), "gpx_nll_grad")
        want, ref = both(dl.grad, *f.args)
        check("a gradient", f.name, {"grad": g}, {"grad": want}, {"grad": ref})


@pytest.mark.parametrize("N", [129, 700])
def test_gradient_matrix(N):
    """gpx_nll_grad_matrix (trace_quad_rows_kernel, sum_pairs_kernel) with a dense non-symmetric dK, the identity and the built-in
    dK / d theta_2; the same float64 matrix goes to the device and to the model"""
    with fit(N, 3) as f:
        rng = np.random.RandomState(N)
        for what, dK in (("dense", rng.randn(N, N)), ("identity", np.eye(N)), ("d theta_2", orc.d_gram_d_theta(f.x, f.theta, 2))):
            dK = _gpx.f64(dK)
            out = ctypes.c_double()
            _gpx.check(_gpx.lib.gpx_nll_grad_matrix(f.h, _gpx.ptr(dK), ctypes.byref(out)), "gpx_nll_grad_matrix")
            want, ref = both(dl.grad_matrix, f.Kinv, f.alpha, dK)
            check("b gradient from dK (%s)" % what, f.name, {"grad": np.array([out.value])}, {"grad": want}, {"grad": ref})


# ------------------------------------------------------------------------------------------------
# c. Approx
# ------------------------------------------------------------------------------------------------
def approx_rows(f, u, S, r0, r1):
    out = np.empty(4 + 2 * f.d)
    _gpx.check(_gpx.lib.gpx_propagate_approx_rows(f.h, _gpx.ptr(u), _gpx.ptr(S), r0, r1, _gpx.ptr(out)), "gpx_propagate_approx_rows")
    return out


@pytest.mark.parametrize("N,d", dl.CASES, ids=IDS)
def test_approx(N, d):
    """the 4 + 2 d sums of gpx_propagate_approx_rows over all rows, gpx_propagate_approx's mean / var / sigma2 / rest and gpx_propagate_dvh
    on the scale of the sums they are differences of: u between the training points, bit-equal to training point 5, far outside the data
    (C_i <= 1e-130: the sums sit at 1e-260 and some products of two C below the normal range); Sigma diagonal and full"""
    with fit(N, d) as f:
        for un, u in dl.inputs_u(f.x, f.theta, f.seed).items():
            u = _gpx.f64(u)
            for sn, S in dl.sigmas(d, f.seed).items():
                S = _gpx.f64(S)
                want, ref = both(dl.approx_partials, *f.args, u, S)
                got = {"partials": approx_rows(f, u, S, 0, N)}
                o = _dbl(4)
                _gpx.check(_gpx.lib.gpx_propagate_approx(f.h, _gpx.ptr(u), _gpx.ptr(S), *[ctypes.byref(a) for a in o]), "gpx_propagate_approx")
                for k, a in zip(("mean", "var", "sigma2", "rest"), o):
                    got[k] = np.array([a.value])
                dv = np.empty(d)
                _gpx.check(_gpx.lib.gpx_propagate_dvh(f.h, _gpx.ptr(u), _gpx.ptr(dv)), "gpx_propagate_dvh")
                got["dvh"] = dv
                check("c approx u %s, Sigma %s" % (un, sn), f.name, got, want, ref)


@pytest.mark.parametrize("d", dl.D_ALL)
def test_approx_row_ranges(d):
    """rows [0, 128) and [128, N) at N = 700, each against the model restricted to those rows; u = training point 5 (in the first range)"""
    N = 700
    with fit(N, d) as f:
        u = _gpx.f64(dl.inputs_u(f.x, f.theta, f.seed)["equal"])
        S = _gpx.f64(list(dl.sigmas(d, f.seed).values())[-1])
        for rows in ((0, 128), (128, N)):
            want, ref = both(dl.approx_partials, *f.args, u, S, rows=rows)
            check("c approx rows [%d, %d)" % rows, f.name, {"partials": approx_rows(f, u, S, *rows)}, want, ref)


@pytest.mark.parametrize("d", [1, 3, 9])
def test_cjh(d):
    """gpx_cjh entry by entry: within 16 u (1 + q_i) of the entry -- of C_i, J_ik and the off-diagonal H_iab themselves, and of the two terms
    of a diagonal H_iaa = ((w_a delta_a)^2 - w_a) c_i (the difference cancels: at w_a delta_a^2 = 1 the entry is 0 and its rounding error
    is not); the +vt of the quirk exactly"""
    N = 700
    with fit(N, d) as f:
        v, vt, _w = dl.params(f.theta, d, np.float64)
        for un, u in dl.inputs_u(f.x, f.theta, f.seed).items():
            u = _gpx.f64(u)
            C, J, H = np.empty(N), np.empty((N, d)), np.empty((N, d, d))
            _gpx.check(_gpx.lib.gpx_cjh(f.h, _gpx.ptr(u), _gpx.ptr(C), _gpx.ptr(J), _gpx.ptr(H)), "gpx_cjh")
            mC, mJ, mH, q, mHabs = dl.cjh(f.x, f.theta, u)
            lim = 16 * U64 * (1 + q)
            offdiag = ~np.eye(d, dtype=bool)
            ratios = [np.abs(C - mC) / (lim * np.abs(mC)), (np.abs(J - mJ) / (lim[:, None] * np.abs(mJ) + 1e-320)),
                      (np.abs(H - mH) / (lim[:, None, None] * np.where(offdiag, np.abs(mH), mHabs) + 1e-320))]
            print("cjh N=%d d=%d u %s: worst C %.3f J %.3f H %.3f of 16 u (1 + q)" % ((N, d, un) + tuple(float(r.max()) for r in ratios)))
            assert np.isfinite(C).all() and np.isfinite(J).all() and np.isfinite(H).all()
            for r in ratios:
                assert float(r.max()) <= 1.0
            near = lambda z: (np.nextafter(z, 0.0), z, np.nextafter(z, np.inf))  # noqa: E731  (the C library's exp(theta) may be numpy's neighbour)
            if un == "equal":
                # c_i = v exp(0) = v exactly, then one addition
                assert C[dl.QUIRK_ROW] in [a + b for a in near(v) for b in near(vt)]
                assert (np.delete(C, dl.QUIRK_ROW) <= near(v)[2]).all()
            else:
                assert (C <= near(v)[2]).all()


# ------------------------------------------------------------------------------------------------
# d. Exact, built-in path
# ------------------------------------------------------------------------------------------------
def exact_rows(f, u, S, r0, r1):
    out = np.empty(3)
    _gpx.check(_gpx.lib.gpx_propagate_exact_rows(f.h, _gpx.ptr(u), _gpx.ptr(S), r0, r1, _gpx.ptr(out)), "gpx_propagate_exact_rows")
    return out


@pytest.mark.parametrize("N,d", dl.CASES, ids=IDS)
def test_exact(N, d):
    """[sum beta_i l_i, the j <= i double sum, nc2] of gpx_propagate_exact_rows over all rows, gpx_propagate_exact's mean and variance and
    gpx_exact_mean; the three u of test_approx"""
    with fit(N, d) as f:
        for un, u in dl.inputs_u(f.x, f.theta, f.seed).items():
            u = _gpx.f64(u)
            for sn, S in dl.sigmas(d, f.seed).items():
                S = _gpx.f64(S)
                want, ref = both(dl.exact_builtin, *f.args, u, S)
                got = {"parts": exact_rows(f, u, S, 0, N)}
                m, var, m1 = _dbl(3)
                _gpx.check(_gpx.lib.gpx_propagate_exact(f.h, _gpx.ptr(u), _gpx.ptr(S), ctypes.byref(m), ctypes.byref(var)), "gpx_propagate_exact")
                _gpx.check(_gpx.lib.gpx_exact_mean(f.h, _gpx.ptr(u), _gpx.ptr(S), ctypes.byref(m1)), "gpx_exact_mean")
                got["mean"], got["var"] = np.array([m.value]), np.array([var.value])
                check("d exact u %s, Sigma %s" % (un, sn), f.name, got, want, ref)
                check("d exact mean only u %s, Sigma %s" % (un, sn), f.name, {"mean": np.array([m1.value])}, want, ref)


@pytest.mark.parametrize("d", dl.D_ALL)
def test_exact_row_ranges(d):
    N = 700
    with fit(N, d) as f:
        u = _gpx.f64(dl.inputs_u(f.x, f.theta, f.seed)["equal"])
        S = _gpx.f64(list(dl.sigmas(d, f.seed).values())[-1])
        for rows in ((0, 128), (128, N)):
            want, ref = both(dl.exact_builtin, *f.args, u, S, rows=rows)
            check("d exact rows [%d, %d)" % rows, f.name, {"parts": exact_rows(f, u, S, *rows)}, want, ref)


# ------------------------------------------------------------------------------------------------
# e. Exact, explicit K^-1 and beta
# ------------------------------------------------------------------------------------------------
def exact_explicit(Kinv, beta, x, w, C, u, S, cuu):
    """(mean, var) of gpx_propagate_exact_matrix(NULL, ..) and of gpx_kinv_model_create + gpx_propagate_exact_model"""
    n, d = x.shape
    Kinv, beta, x, w, C, u, S = (_gpx.f64(a) for a in (Kinv, beta, x, w, C, u, S))
    m, var = _dbl(2)
    _gpx.check(_gpx.lib.gpx_propagate_exact_matrix(None, _gpx.ptr(Kinv), _gpx.ptr(beta), _gpx.ptr(x), n, d, _gpx.ptr(w), _gpx.ptr(C), _gpx.ptr(u),
                                                   _gpx.ptr(S), cuu, ctypes.byref(m), ctypes.byref(var)), "gpx_propagate_exact_matrix")
    km = ctypes.c_void_p()
    _gpx.check(_gpx.lib.gpx_kinv_model_create(_gpx.ptr(Kinv), _gpx.ptr(beta), n, ctypes.byref(km)), "gpx_kinv_model_create")
    try:
        m2, var2 = _dbl(2)
        _gpx.check(_gpx.lib.gpx_propagate_exact_model(km, _gpx.ptr(x), d, _gpx.ptr(w), _gpx.ptr(C), _gpx.ptr(u), _gpx.ptr(S), cuu, ctypes.byref(m2),
                                                      ctypes.byref(var2)), "gpx_propagate_exact_model")
    finally:
        _gpx.lib.gpx_kinv_model_free(km)
    return (m.value, var.value), (m2.value, var2.value)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("N", [129, 700])
def test_exact_explicit_designed_inputs(N, d):
    """integer K^-1 (symmetric, [-8, 8]), beta and C, every x_i = u, Sigma = 0, w a power of two: a_i = 0, Ls = 0 and Delta^-1 = 0 exactly
    (the inverse of diag(1 / 2 w) is diag(2 w) in any arithmetic), every exponent is 0, exp gives 1 and nc1 = nc2 = 1.  Every device term
    is then an integer below 2^53: the mean is sum beta_i C_i, and with cuu = 0 the variance is -(double sum) - mean^2, bit for bit."""
    rng = np.random.RandomState(N + d)
    K = rng.randint(-8, 9, (N, N))
    K = np.tril(K) + np.tril(K, -1).T
    beta, C = rng.randint(-4, 5, N), rng.randint(-3, 4, N)
    u = np.round(rng.uniform(0, 10, d) * 2.0 ** 20) / 2.0 ** 20
    x, w, S = np.tile(u, (N, 1)), np.array([0.25, 2.0, 0.5][:d]), np.zeros((d, d))
    mean = int(beta.dot(C))
    total = int(C.dot((K - np.outer(beta, beta)).dot(C)))                     # int64, every term below 2^12
    assert abs(total) + mean * mean < 2 ** 53
    try:
        a, b = exact_explicit(K, beta, x, w, C, u, S, 0.0)
    finally:
        _gpx.lib.gpx_pool_trim()
    print("explicit designed N=%d d=%d: mean %r of %d, var %r of %d" % (N, d, a[0], mean, a[1], -total - mean * mean))
    assert a == b
    assert a[0] == float(mean) and a[1] == float(-total - mean * mean)


def test_exact_explicit_positive_exponents():
    """exact_build_generic_kernel hands exact_sum_kernel the exponents e_i + e_j + b_i.a_j = z^T Ls z / 2 >= 0 -- outside the "non-positive"
    of exp_nonpos's name.  Sharp length scales at d = 3, u at the corner 0 of the cube, Sigma = 0.01 I: the largest exponent of a visited
    pair is 210 (asserted >= 50); C_ux from the kernel in float64, the same to the device and to the model.  Both explicit entry points bit
    for bit, the handle form (its own K^-1, not symmetrised again) within the bound.  Then the same inputs with C_ux = 1 (below)."""
    N, d = dl.SHARP_CASE
    with fit(N, d, sharp=True) as f:
        u, S, C, w, cuu = dl.sharp_inputs(f.x, f.theta)
        want, ref = both(dl.exact_parts, f.x, w, f.Kinv, f.alpha, C, u, S, cuu)
        print("largest exponent %.2f" % want["emax"])
        assert 50 <= want["emax"] < 700
        a, b = exact_explicit(f.Kinv, f.alpha, f.x, w, C, u, S, cuu)
        assert a == b
        check("e explicit, positive exponents", f.name, {"mean": np.array([a[0]]), "var": np.array([a[1]])}, want, ref)
        m, var = _dbl(2)
        arrs = [_gpx.f64(v_) for v_ in (f.x, w, C, u, S)]
        _gpx.check(_gpx.lib.gpx_propagate_exact_matrix(f.h, None, None, _gpx.ptr(arrs[0]), N, d, *[_gpx.ptr(v_) for v_ in arrs[1:]], cuu,
                                                       ctypes.byref(m), ctypes.byref(var)), "gpx_propagate_exact_matrix (handle)")
        check("e explicit, handle form", f.name, {"mean": np.array([m.value]), "var": np.array([var.value])}, want, ref)
        # With the kernel's own C_ux the pairs with an exponent above 5 carry 1.6e-13 of the sum (C_i C_j falls faster than exp grows):
        # that part shows that +210 neither overflows nor poisons the sum, not how accurate exp is there.  Under a flat operator,
        # C_ux = 1 and cuu = 1, the pairs with the largest exponents ARE the sum (8e90).  A term's relative error is then the absolute
        # error of its exponent, at most (2 d + 6) u E = 2.8e-13 at E = 210 for the kernel's d fmas and three additions on e_i, e_j
        # that are themselves rounded products, plus exp's 2 ulp: inside the bound with nothing measured on the device.
        flat = np.ones(N)
        want, ref = both(dl.exact_parts, f.x, w, f.Kinv, f.alpha, flat, u, S, 1.0)
        a, b = exact_explicit(f.Kinv, f.alpha, f.x, w, flat, u, S, 1.0)
        assert a == b
        check("e explicit, flat operator: positive exponents carry the sum", f.name, {"mean": np.array([a[0]]), "var": np.array([a[1]])}, want, ref)


# ------------------------------------------------------------------------------------------------
# f. gpx_symv, exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [1, 9, 10, 17, 18, 33, 34, 64])
@pytest.mark.parametrize("n", [129, 200, 700])
def test_symv_exact_on_integers(n, nrhs):
    """M symmetric and V integer in [-512, 512]: every sum stays below 700 * 2^18 < 2^30, so any order of summation is exact"""
    rng = np.random.RandomState(1000 * nrhs + n)
    M = rng.randint(-512, 513, (n, n))
    M = np.tril(M) + np.tril(M, -1).T
    V = rng.randint(-512, 513, (nrhs, n))
    want = V.dot(M)                                                           # int64; out[r] = M V[r]
    assert np.abs(want).max() < 2 ** 30
    Mf, Vf, out = _gpx.f64(M), _gpx.f64(V), np.full((nrhs, n), np.nan)
    try:
        _gpx.check(_gpx.lib.gpx_symv(_gpx.ptr(Mf), n, _gpx.ptr(Vf), nrhs, _gpx.ptr(out)), "gpx_symv")
    finally:
        _gpx.lib.gpx_pool_trim()
    np.testing.assert_array_equal(out, want.astype(np.float64))


def test_symv_refuses_bad_arguments():
    M, V, out = np.eye(4), np.ones((65, 4)), np.full((65, 4), 7.25)
    assert _gpx.lib.gpx_symv(_gpx.ptr(M), 4, _gpx.ptr(V), 65, _gpx.ptr(out)) == _gpx.GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_symv(_gpx.ptr(M), 0, _gpx.ptr(V), 1, _gpx.ptr(out)) == _gpx.GPX_ERR_BAD_ARG
    np.testing.assert_array_equal(out, np.full((65, 4), 7.25))
