"""CPU-only: the long-double model of MaternCovariance (tests/_matern_ld.py) against the general-nu Bessel expression, the float64
restatement's own error rho_K / rho_ref that the device bounds of tests/test_matern.py are built on, the seeded defects those bounds must
catch, the host scalar methods of the class, the C-ABI's presence and the registers of csrc/matern.hip.

Measured here (x86-64, numpy float64 against np.longdouble), printed by the tests with -s:
  rho_K   = 2.74 units of u K (1 + s) over (130, 257) x D_ALL x both nu: under GRAM_FLOOR, so the Gram bound is 8 * 4 = 32 units;
  rho_ref < FLOOR over the gradient cases below (the 1000 u floor of the rule governs)."""
import ctypes
import functools
import pickle

import numpy as np
import pytest

from conftest import have_gpu

import _matern_ld as ml

import skgpuppy_amd
from skgpuppy_amd import _gpx

V, VT = 2.0, 0.01
NAMES = ("gpx_matern_gram", "gpx_matern_fit", "gpx_matern_predict", "gpx_matern_nll_grad", "gpx_matern_propagate_approx_many",
         "gpx_matern_propagate_dvh_many")


def _cov(nu2):
    return skgpuppy_amd.MaternCovariance(nu2 / 2.0)


@pytest.mark.parametrize("nu2", ml.NU2_ALL)
def test_model_against_the_bessel_expression(nu2):
    """Kf = v 2^(1 - nu) / Gamma(nu) s^nu K_nu(s), s = sqrt(2 nu q): 1e-13 relative wherever s > 0, exactly v at s = 0"""
    from scipy.special import gamma, kv
    nu = nu2 / 2.0
    for d in (1, 3, 9):
        xi, xj, theta = ml.make_gram_case(130, 257, d)
        pr = ml.kernel_parts(xi, xj, theta, nu2)
        s = pr["s"].astype(np.float64)
        pos = s > 0
        assert pos.any() and (~pos).any()
        want = V * 2.0 ** (1 - nu) / gamma(nu) * s[pos] ** nu * kv(nu, s[pos])
        np.testing.assert_allclose(pr["Kf"].astype(np.float64)[pos], want, rtol=1e-13, atol=0)
        v, vt, _w = ml.params(theta, d)
        assert (pr["Kf"][~pos] == v).all() and (pr["K"][~pos] == v + vt).all()
        assert np.array_equal(~pos, pr["eq"])


@functools.lru_cache(maxsize=None)
def rho_K():
    """the float64 restatement's worst error against the model in units of u K (1 + s), over (130, 257) x D_ALL x both nu"""
    worst = 0.0
    for nu2 in ml.NU2_ALL:
        for d in ml.D_ALL:
            xi, xj, theta = ml.make_gram_case(130, 257, d)
            ld = ml.kernel_parts(xi, xj, theta, nu2)
            worst = max(worst, float(ml.gram_units(ml.kernel_parts(xi, xj, theta, nu2, np.float64)["K"], ld).max()))
    return worst


def test_rho_K_of_the_float64_restatement():
    r = rho_K()
    print("rho_K = %.3e  -> Gram bound %.3e units of u K (1 + s)" % (r, ml.gram_bound(r)))
    assert 0 < r <= ml.GRAM_FLOOR
    assert ml.gram_bound(r) == 32.0


@pytest.mark.parametrize("nu2", ml.NU2_ALL)
@pytest.mark.parametrize("N,d", ml.FIT_CASES)
def test_conditions_on_the_inputs(N, d, nu2):
    """cond K <= 5.6e4 for every fit case; the off-diagonal arithmetic is exercised: most entries are far from 0 and from v"""
    x, _t, theta = ml.make_case(N, d)
    pr = ml.kernel_parts(x, x, theta, nu2, np.float64)
    off = pr["Kf"][~np.eye(N, dtype=bool)]
    assert (off > 0.05 * V).mean() >= 0.8
    assert np.linalg.cond(pr["K"]) <= 5.6e4


GRAD_MODEL_CASES = [(130, d) for d in ml.D_ALL] + [(257, 3)]


@functools.lru_cache(maxsize=None)
def _grad_case(N, d, nu2):
    x, t, theta = ml.make_case(N, d)
    K = ml.kernel_parts(x, x, theta, nu2, np.float64)["K"]
    Kinv = np.linalg.inv(K)
    Kinv = (Kinv + Kinv.T) / 2
    alpha = Kinv.dot(t)
    want, scale = ml.grad(x, theta, nu2, Kinv, alpha)
    return x, theta, Kinv, alpha, want, scale


@pytest.mark.parametrize("nu2", ml.NU2_ALL)
@pytest.mark.parametrize("N,d", GRAD_MODEL_CASES)
def test_rho_ref_of_the_gradient_sums(N, d, nu2):
    x, theta, Kinv, alpha, want, scale = _grad_case(N, d, nu2)
    ref, _ = ml.grad(x, theta, nu2, Kinv, alpha, np.float64)
    rho = float(ml.distances(ref, want, scale).max())
    print("(%d, %d, nu2 = %d): rho_ref = %.3e  bound %.3e" % (N, d, nu2, rho, ml.bound(rho)))
    assert rho < ml.FLOOR            # a float64 sum of N^2 terms on the scale of its absolute terms: far below 1000 u


@pytest.mark.parametrize("defect", ["poly32", "nos2", "novt", "diagvt", "exp32"])
def test_seeded_defects_fall_outside_the_gram_bound(defect):
    lim = ml.gram_bound(rho_K())
    for d in (1, 3, 9):
        xi, xj, theta = ml.make_gram_case(130, 257, d)
        ld = ml.kernel_parts(xi, xj, theta, 5)
        bad = ml.gram_units(ml.kernel_parts(xi, xj, theta, 5, np.float64, defect)["K"], ld)
        assert bad.max() > 10 * lim, (defect, d, bad.max(), lim)


def test_seeded_sign_defect_falls_outside_the_derivative_and_gradient_bounds():
    lim = ml.gram_bound(rho_K())
    xi, xj, theta = ml.make_gram_case(64, 129, 3)
    for nu2 in ml.NU2_ALL:
        ld = ml.kernel_parts(xi, xj, theta, nu2, keep=True)
        f64 = ml.kernel_parts(xi, xj, theta, nu2, np.float64, keep=True)
        for j in range(len(theta)):
            good = ml.deriv_units(ml.deriv(f64, theta, j, np.float64)[0], ld, theta, j)
            assert good.max() <= lim, (nu2, j, good.max())
        for j in range(2, 5):
            bad = ml.deriv_units(ml.deriv(f64, theta, j, np.float64, "sign")[0], ld, theta, j)
            assert bad.max() > 10 * lim
        x, theta_g, Kinv, alpha, want, scale = _grad_case(130, 3, nu2)
        defects = [df for df in ml.DEFECTS if df not in ("novt", "diagvt")]      # (the gradient never adds vt: T counts the equal pairs)
        if nu2 == 3:
            defects = [df for df in defects if df not in ("poly32", "nos2")]     # (defects of the 5/2 polynomial)
        for defect in defects:
            got, _ = ml.grad(x, theta_g, nu2, Kinv, alpha, np.float64, defect)
            dist = ml.distances(got, want, scale)
            assert dist.max() > 10 * ml.bound(0.0), (nu2, defect, dist.max())


@pytest.mark.parametrize("nu2", ml.NU2_ALL)
def test_host_scalars_against_the_model(nu2):
    cov = _cov(nu2)
    x, t, theta = ml.make_case(203, 3)
    pr = ml.kernel_parts(x[:40], x[:40], theta, nu2, keep=True)
    dK = [ml.deriv(pr, theta, j)[0].astype(np.float64) for j in range(len(theta))]
    K = pr["K"].astype(np.float64)
    rng = np.random.RandomState(3)
    for i, j in [(0, 0), (5, 5)] + [tuple(rng.randint(0, 40, 2)) for _ in range(40)]:
        assert cov(x[i], x[j], theta) == pytest.approx(K[i, j], rel=1e-14)
        for k in range(len(theta)):
            assert cov._d_cov_d_theta(x[i], x[j], theta, k) == pytest.approx(dK[k][i, j], rel=1e-13, abs=1e-300)
    assert cov(x[0], x[0].copy(), theta) == np.exp(theta[0]) + np.exp(theta[1])      # exactly v + vt at delta = 0
    np.testing.assert_array_equal(cov.get_theta(x, t), skgpuppy_amd.GaussianCovariance().get_theta(x, t))
    # central differences of the scalar kernel in theta
    for k in range(len(theta)):
        fd = skgpuppy_amd.Covariance._d_cov_d_theta(cov, x[1], x[2], theta, k)
        assert cov._d_cov_d_theta(x[1], x[2], theta, k) == pytest.approx(fd, rel=1e-7, abs=1e-10)


def test_jacobian_hessian_match_the_model_and_finite_differences():
    cov = _cov(5)
    x, _t, theta = ml.make_case(203, 3)
    u = np.array([4.25, 5.5, 3.125])
    J, H = ml.jacobian_hessian(u, x[:30], theta)
    for i in range(30):
        Ji, Hi = cov.get_Jacobian(u, x[i], theta), cov.get_Hessian(u, x[i], theta)
        assert Ji.shape == (3, 1) and Hi.shape == (3, 3)
        np.testing.assert_allclose(Ji[:, 0], J[i].astype(np.float64), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(Hi, H[i].astype(np.float64), rtol=1e-12, atol=1e-16)
    # the convention of GaussianCovariance.get_Jacobian / get_Hessian: derivatives of k(u, xi) in xi
    xi, eps = x[7], 1e-5
    Jn, Hn = np.empty(3), np.empty((3, 3))
    for a in range(3):
        ea = np.eye(3)[a] * eps
        Jn[a] = (cov(u, xi + ea, theta) - cov(u, xi - ea, theta)) / (2 * eps)
        for b in range(3):
            eb = np.eye(3)[b] * eps
            Hn[a, b] = (cov(u, xi + ea + eb, theta) - cov(u, xi + ea - eb, theta) - cov(u, xi - ea + eb, theta) + cov(u, xi - ea - eb, theta)) / (4 * eps * eps)
    np.testing.assert_allclose(cov.get_Jacobian(u, xi, theta)[:, 0], Jn, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(cov.get_Hessian(u, xi, theta), Hn, rtol=1e-4, atol=1e-6)
    # at the origin: J = 0 and H = -(5/3) v diag(w), no 0 * inf
    np.testing.assert_array_equal(cov.get_Jacobian(u, u, theta)[:, 0], np.zeros(3))
    np.testing.assert_allclose(cov.get_Hessian(u, u, theta), -(5.0 / 3.0) * V * np.diag(np.exp(theta[2:])), rtol=1e-15)


def test_nu_three_halves_keeps_the_base_class_derivatives():
    cov = _cov(3)
    x, _t, theta = ml.make_case(130, 1)
    with pytest.raises(NotImplementedError):
        cov.get_Jacobian(x[0], x[1], theta)
    with pytest.raises(NotImplementedError):
        cov.get_Hessian(x[0], x[1], theta)


def test_class_surface():
    cov = skgpuppy_amd.MaternCovariance()
    assert isinstance(cov, skgpuppy_amd.Covariance) and cov._fused() and cov.nu == 2.5
    assert skgpuppy_amd.MaternCovariance(1.5).nu == 1.5

    class Own(skgpuppy_amd.MaternCovariance):
        def cov_matrix_ij(self, xi, xj, theta):
            return skgpuppy_amd.Covariance.cov_matrix_ij(self, xi, xj, theta)

    assert not Own()._fused()
    cov._ml_cache = ("key", None)
    back = pickle.loads(pickle.dumps(cov))
    assert not hasattr(back, "_ml_cache") and back.nu == 2.5
    with pytest.raises(ValueError):
        cov.cov_matrix_ij(np.zeros((2, 2)), np.zeros((2, 2)), np.zeros(7))
    with pytest.raises(ValueError):
        skgpuppy_amd.MaternCovariance(nu=2.0)


@pytest.mark.parametrize("base", [skgpuppy_amd.PeriodicCovariance, skgpuppy_amd.MaternCovariance])
def test_fused_is_decided_per_subclass_on_the_common_base(base):
    """both raw-input kinds take _fused() from one base: a subclass that overrides no matrix method stays fused (its own scalar
    accessors do not count), one that overrides cov_matrix_ij takes the generic route"""
    class Plain(base):
        def get_theta(self, x, t):
            return base.get_theta(self, x, t)

    class Own(base):
        def cov_matrix_ij(self, xi, xj, theta):
            return skgpuppy_amd.Covariance.cov_matrix_ij(self, xi, xj, theta)

    assert Plain()._fused() is True and Own()._fused() is False


def test_abi_has_the_matern_entry_points():
    for name in NAMES:
        assert hasattr(_gpx.lib, name) and name in _gpx.SIGNATURES


@pytest.mark.skipif(have_gpu(), reason="checks the no-device behaviour")
def test_no_device_is_an_error_not_a_fallback():
    x = np.random.RandomState(0).rand(5, 2)
    th = np.zeros(4)
    out, h = np.empty((5, 5)), ctypes.c_void_p()
    assert _gpx.lib.gpx_matern_gram(_gpx.ptr(x), 5, _gpx.ptr(x), 5, 2, _gpx.ptr(th), 5, -1, _gpx.ptr(out)) == _gpx.GPX_ERR_NO_DEVICE
    assert _gpx.lib.gpx_matern_fit(_gpx.ptr(x), _gpx.ptr(np.zeros(5)), 5, 2, _gpx.ptr(th), 5, None, ctypes.byref(h)) == _gpx.GPX_ERR_NO_DEVICE
    assert not h
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        skgpuppy_amd.MaternCovariance().cov_matrix_ij(x, x, th)
    with pytest.raises(RuntimeError):
        skgpuppy_amd.GaussianProcess(x, np.zeros(5), skgpuppy_amd.MaternCovariance(), th)


def test_no_matern_kernel_uses_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage on csrc/matern.hip: every kernel keeps its accumulators in registers (DESIGN.md 5.5 quotes
    the figures)"""
    import os
    import re
    import shutil
    import subprocess
    from conftest import PKG_PARENT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(PKG_PARENT, "csrc", "matern.hip"),
                          "-o", str(tmp_path / "matern.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    vgprs = [int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", out.stderr)]
    assert len(names) == len(scratch) == len(vgprs)
    kernels = {n: (s, v) for n, s, v in zip(names, scratch, vgprs)}
    assert sum("matern_gram_kernel" in n for n in kernels) == 4 and sum("matern_nll_grad_kernel" in n for n in kernels) == 2
    assert sum("matern52_build_many_kernel" in n for n in kernels) == 4
    for n, (s, v) in kernels.items():
        assert s == 0 and v <= 256, (n, s, v)
