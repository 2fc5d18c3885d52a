"""CPU-only: the long-double model of PeriodicCovariance (tests/_periodic_ld.py) against the golden file written from the genuine
reference (tools/gen_periodic_golden.py), the float64 restatement's own error rho_K / rho_ref that the device bounds of
tests/test_periodic.py are built on, the seeded defects those bounds must catch, the host scalar methods of the class and the C-ABI's
presence.

Measured here (x86-64, numpy float64 against np.longdouble), printed by the tests with -s:
  rho_K   = 5.4 units of u K (1 + q) over the 40 Gram cases (the reference's pi / p * diff rounds the argument of the sine);
  rho_ref <= 1.2e-16 over the gradient cases below (the 1000 u floor of the rule governs)."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import have_gpu, load_golden

import _periodic_ld as pl

import skgpuppy_amd
from skgpuppy_amd import _gpx

V = 2.0


@functools.lru_cache(maxsize=None)
def _golden():
    return load_golden("periodic")


def _case(N, d):
    g = _golden()
    return {k[len("c%d_%d_" % (N, d)):]: v for k, v in g.items() if k.startswith("c%d_%d_" % (N, d))}


@pytest.mark.parametrize("N,d", pl.GOLDEN_CASES)
def test_golden_inputs_are_the_seeded_case(N, d):
    c = _case(N, d)
    x, t, theta = pl.make_case(N, d)
    assert np.array_equal(c["x"], x) and np.array_equal(c["t"], t) and np.array_equal(c["theta"], theta)
    assert np.array_equal(c["xs"], pl.make_queries(x, 64, pl.seed_of(N, d) + 1))
    assert np.array_equal(c["xs"][3], x[5])


@pytest.mark.parametrize("N,d", pl.GOLDEN_CASES)
def test_model_against_golden(N, d):
    """K and every dK entry-wise (the reference's float64 is good to a few hundred u: 1e-12), then -- SURVEY 8a's bounds of the generic
    route -- beta and the predictions at rtol 1e-6 / atol 1e-9 v, nll at 1e-9 relative, the gradient at rtol 1e-6 / atol 1e-7, all
    computed with numpy from the MODEL's K."""
    c = _case(N, d)
    x, t, theta, xs = c["x"], c["t"], c["theta"], c["xs"]
    pr = pl.kernel_parts(x, x, theta)
    K = pr["K"].astype(np.float64)
    np.testing.assert_allclose(K, c["K"], rtol=1e-12, atol=0)
    sub = pl.kernel_parts(x[:40], x[:40], theta, keep=True)
    for j in range(len(theta)):
        np.testing.assert_allclose(pl.deriv(sub, theta, j)[0].astype(np.float64), c["dK"][j], rtol=1e-11, atol=1e-15, err_msg="j=%d" % j)
    Kinv = np.linalg.inv(K)
    beta = Kinv.dot(t)
    np.testing.assert_allclose(beta, c["beta"], rtol=1e-6, atol=1e-9 * V)
    kv = pl.kernel_parts(xs, x, theta)["K"].astype(np.float64)
    assert kv[3, 5] == pytest.approx(V + 0.01, rel=1e-15)            # the query that equals a training row carries +vt
    np.testing.assert_allclose(kv.dot(beta), c["mean"], rtol=1e-6, atol=1e-9 * V)      # (t is centred: meant = 0 up to rounding)
    np.testing.assert_allclose((V + 0.01) - np.einsum("ij,jk,ik->i", kv, Kinv, kv), c["var"], rtol=1e-6, atol=1e-9 * V)
    assert pl.nll(K, t) == pytest.approx(float(c["nll"]), rel=1e-9)
    g, _s = pl.grad(x, theta, Kinv, beta)
    np.testing.assert_allclose(g.astype(np.float64), c["grad"], rtol=1e-6, atol=1e-7)


@functools.lru_cache(maxsize=None)
def rho_K():
    """the float64 restatement's worst error against the model in units of u K (1 + q), over all Gram cases of tests/test_periodic.py"""
    worst = 0.0
    for n1, n2 in pl.GRAM_SHAPES:
        for d in pl.D_ALL:
            xi, xj, theta = pl.make_gram_case(n1, n2, d)
            ld = pl.kernel_parts(xi, xj, theta)
            worst = max(worst, float(pl.gram_units(pl.kernel_parts(xi, xj, theta, np.float64)["K"], ld).max()))
    return worst


def test_rho_K_of_the_float64_restatement():
    r = rho_K()
    print("rho_K = %.3e  -> Gram bound %.3e units of u K (1 + q)" % (r, pl.gram_bound(r)))
    assert np.isfinite(r) and 0 < r < 200       # 1.35 u of the argument pi delta / p at |delta / p| <= 6.7, times w2 / 2 <= 1.5: some tens of units


@pytest.mark.parametrize("N,d", pl.FIT_CASES)
def test_conditions_on_the_inputs(N, d):
    """the kernel's off-diagonal arithmetic is what the results hang on: at least 80 % of the off-diagonal entries exceed 0.05 v,
    cond K <= 2.5e4"""
    x, _t, theta = pl.make_case(N, d)
    pr = pl.kernel_parts(x, x, theta, np.float64)
    off = pr["Kf"][~np.eye(N, dtype=bool)]
    assert (off > 0.05 * V).mean() >= 0.8
    assert pr["q"].max() <= 10.0
    assert np.linalg.cond(pr["K"]) <= 2.5e4


GRAD_MODEL_CASES = [(130, d) for d in pl.D_ALL] + [(257, 3)]


@functools.lru_cache(maxsize=None)
def _grad_case(N, d):
    x, t, theta = pl.make_case(N, d)
    K = pl.kernel_parts(x, x, theta, np.float64)["K"]
    Kinv = np.linalg.inv(K)
    Kinv = (Kinv + Kinv.T) / 2
    alpha = Kinv.dot(t)
    want, scale = pl.grad(x, theta, Kinv, alpha)
    return x, theta, Kinv, alpha, want, scale


@pytest.mark.parametrize("N,d", GRAD_MODEL_CASES)
def test_rho_ref_of_the_gradient_sums(N, d):
    x, theta, Kinv, alpha, want, scale = _grad_case(N, d)
    ref, _ = pl.grad(x, theta, Kinv, alpha, np.float64)
    rho = float(pl.distances(ref, want, scale).max())
    print("(%d, %d): rho_ref = %.3e  bound %.3e" % (N, d, rho, pl.bound(rho)))
    assert rho < pl.FLOOR            # a float64 sum of N^2 terms on the scale of its absolute terms: far below 1000 u


@pytest.mark.parametrize("defect", ["sin32", "novt", "swap", "unreduced"])
def test_seeded_defects_fall_outside_the_gram_bound(defect):
    lim = pl.gram_bound(rho_K())
    for d in (1, 3, 9):
        xi, xj, theta = pl.make_gram_case(130, 257, d)
        ld = pl.kernel_parts(xi, xj, theta)
        bad = pl.gram_units(pl.kernel_parts(xi, xj, theta, np.float64, defect)["K"], ld)
        assert bad.max() > 10 * lim, (defect, d, bad.max(), lim)
    if defect == "unreduced":        # the case the defect is named for: |delta / p| about 6
        theta = np.log(np.array([2.0, 0.01, 0.05, 1.5, 1.0]))
        xi, xj = np.array([[0.0]]), np.array([[9.0 + 2.0 ** -3]])
        ld = pl.kernel_parts(xi, xj, theta)
        assert abs(9.125 / 1.5 - 6) < 0.1
        assert pl.gram_units(pl.kernel_parts(xi, xj, theta, np.float64)["K"], ld).max() <= lim
        assert not pl.gram_units(pl.kernel_parts(xi, xj, theta, np.float64, defect)["K"], ld).max() <= lim


def test_seeded_sign_defect_falls_outside_the_derivative_and_gradient_bounds():
    lim = pl.gram_bound(rho_K())
    xi, xj, theta = pl.make_gram_case(64, 129, 3)
    ld = pl.kernel_parts(xi, xj, theta, keep=True)
    f64 = pl.kernel_parts(xi, xj, theta, np.float64, keep=True)
    for j in range(len(theta)):
        good = pl.deriv_units(pl.deriv(f64, theta, j, np.float64)[0], ld, theta, j)
        assert good.max() <= lim, (j, good.max())
    for j in range(2 + 3, 2 + 6):
        bad = pl.deriv_units(pl.deriv(f64, theta, j, np.float64, "sign")[0], ld, theta, j)
        assert bad.max() > 10 * lim
    x, theta, Kinv, alpha, want, scale = _grad_case(130, 3)
    for defect in pl.DEFECTS:
        if defect == "novt":
            continue                 # (the gradient never adds vt: T counts the equal pairs, which the defect leaves alone)
        got, _ = pl.grad(x, theta, Kinv, alpha, np.float64, defect)
        dist = pl.distances(got, want, scale)
        assert dist.max() > 10 * pl.bound(0.0), (defect, dist.max())


@pytest.mark.parametrize("N,d", pl.GOLDEN_CASES)
def test_host_scalar_methods_against_golden(N, d):
    c = _case(N, d)
    cov = skgpuppy_amd.PeriodicCovariance()
    x, theta = c["x"], c["theta"]
    rng = np.random.RandomState(3)
    for i, j in [(0, 0), (5, 5)] + [tuple(rng.randint(0, 40, 2)) for _ in range(40)]:
        assert cov(x[i], x[j], theta) == pytest.approx(c["K"][i, j], rel=1e-14)
        for k in range(len(theta)):
            assert cov._d_cov_d_theta(x[i], x[j], theta, k) == pytest.approx(c["dK"][k][i, j], rel=1e-13, abs=1e-300)
    np.testing.assert_array_equal(cov.get_theta(x, c["t"]), c["theta0"])
    th0 = cov.get_theta(x, None)
    assert th0[0] == 1 and th0[1] == 1 and len(th0) == 2 + 3 * d
    assert cov(x[0], x[0].copy(), theta) == pytest.approx(V + 0.01, rel=1e-15)


def test_class_surface():
    cov = skgpuppy_amd.PeriodicCovariance()
    assert isinstance(cov, skgpuppy_amd.Covariance) and cov._fused()

    class Own(skgpuppy_amd.PeriodicCovariance):
        def cov_matrix_ij(self, xi, xj, theta):
            return skgpuppy_amd.Covariance.cov_matrix_ij(self, xi, xj, theta)

    assert not Own()._fused()
    import pickle
    cov._ml_cache = ("key", None)
    assert not hasattr(pickle.loads(pickle.dumps(cov)), "_ml_cache")
    with pytest.raises(ValueError):
        cov.cov_matrix_ij(np.zeros((2, 2)), np.zeros((2, 2)), np.zeros(7))


def test_abi_has_the_periodic_entry_points():
    for name in ("gpx_periodic_gram", "gpx_periodic_fit", "gpx_periodic_predict", "gpx_periodic_nll_grad"):
        assert hasattr(_gpx.lib, name) and name in _gpx.SIGNATURES


@pytest.mark.skipif(have_gpu(), reason="checks the no-device behaviour")
def test_no_device_is_an_error_not_a_fallback():
    x = np.random.RandomState(0).rand(5, 2)
    th = np.zeros(8)
    out, h = np.empty((5, 5)), ctypes.c_void_p()
    assert _gpx.lib.gpx_periodic_gram(_gpx.ptr(x), 5, _gpx.ptr(x), 5, 2, _gpx.ptr(th), -1, _gpx.ptr(out)) == _gpx.GPX_ERR_NO_DEVICE
    assert _gpx.lib.gpx_periodic_fit(_gpx.ptr(x), _gpx.ptr(np.zeros(5)), 5, 2, _gpx.ptr(th), None, ctypes.byref(h)) == _gpx.GPX_ERR_NO_DEVICE
    assert not h
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP device"):
        skgpuppy_amd.PeriodicCovariance().cov_matrix_ij(x, x, th)
    with pytest.raises(RuntimeError):
        skgpuppy_amd.GaussianProcess(x, np.zeros(5), skgpuppy_amd.PeriodicCovariance(), th)


def test_no_periodic_kernel_uses_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage on csrc/periodic.hip: the Gram, its derivative variant and the gradient pass keep their
    accumulators in registers (DESIGN.md 5.4 quotes the figures)"""
    import os
    import re
    import shutil
    import subprocess
    from conftest import PKG_PARENT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(PKG_PARENT, "csrc", "periodic.hip"),
                          "-o", str(tmp_path / "periodic.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    vgprs = [int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", out.stderr)]
    assert len(names) == len(scratch) == len(vgprs)
    kernels = {n: (s, v) for n, s, v in zip(names, scratch, vgprs)}
    assert sum("periodic_gram_kernel" in n for n in kernels) == 2 and sum("periodic_nll_grad_kernel" in n for n in kernels) == 1
    for n, (s, v) in kernels.items():
        assert s == 0 and v <= 256, (n, s, v)
