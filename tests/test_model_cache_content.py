"""The likelihood of a covariance object is that of the arrays' CONTENT at the call, end to end on the device: after x is overwritten in
place, and for temporaries that NumPy places at one recycled address, `_negativeloglikelihood` and `_d_nll_d_theta` give the bits of a new
object on a new array (fits are bit-reproducible: no tolerance), and those sit within the family's existing bound of its long-double
reference.  tests/test_model_cache_keys.py holds the cache keys themselves, without a device.

N = 130, d = 3: one row past a 128-tile, the smallest shape of the Python-level tests."""
import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import _dense_ld as dl
import _gauss_ld as gl
import _matern_ld as ml
import _periodic_ld as pl

import skgpuppy_amd as sk
from skgpuppy_amd.Covariance import _MaternModel, _MatrixModel, _PeriodicModel
from skgpuppy_amd.GaussianProcess import _DeviceModel

pytestmark = pytest.mark.gpu
N, D = 130, 3


class OwnCrossCovariance(sk.GaussianCovariance):
    """a user subclass with its own cov_matrix_ij: `_fused()` is false, the generic route of `Covariance` serves it"""

    def cov_matrix_ij(self, xi, xj, theta):
        return sk.GaussianCovariance.cov_matrix_ij(self, xi, xj, theta)


class Family(object):
    """a kernel family: how to make its covariance object and seeded case, its long-double K, and its gradient held to the family's bound"""

    def __init__(self, name, make, case, K_ld, model, grad):
        self.name, self.make, self.case, self.K_ld, self.model, self.grad = name, make, case, K_ld, model, grad


def _gauss_K(x, theta):
    return gl.kernel_parts(x, x, theta, add_diag=float(np.exp(theta[1])))["Kd"].astype(np.float64)


def _fused_gradient(mod, grad_fn):
    """(want, ref): grad_fn(x, theta, Kinv, alpha, dt) in long double and in float64, on the K^-1 and alpha the device hands back"""
    def check(x, t, theta, g, what, new_model):
        model = new_model(x, t, theta)
        try:
            Kinv, alpha = model.kinv(), model.alpha()
        finally:
            model.close()
        want, scale = grad_fn(x, theta, Kinv, alpha, mod.LD)
        ref, _ = grad_fn(x, theta, Kinv, alpha, np.float64)
        rho = float(mod.distances(ref, want, scale).max())
        mod.assert_within({"grad": mod.distances(g, want, scale)}, rho, what)
    return check


def _generic_gradient(x, t, theta, g, what, new_model):
    """entry j against dl.grad_matrix on the operator's own dK_j, as test_dense_bounds.test_gradient_matrix holds gpx_nll_grad_matrix"""
    cov = OwnCrossCovariance()
    model = new_model(x, t, theta)
    try:
        Kinv, alpha = model.kinv(), model.alpha()
    finally:
        model.close()
    for j in range(len(theta)):
        dK = np.ascontiguousarray(cov._d_cov_matrix_d_theta(x, theta, j), dtype=np.float64)
        want, scale = dl.grad_matrix(Kinv, alpha, dK)
        ref, _ = dl.grad_matrix(Kinv, alpha, dK, dt=np.float64)
        rho = float(dl.distances(ref, want, scale).max())
        dl.assert_within({"grad[%d]" % j: dl.distances(np.array([g[j]]), want, scale)}, rho, what)


def _matern(nu2):
    return Family("matern_nu2_%d" % nu2, lambda: sk.MaternCovariance(nu2 / 2.0), lambda seed: ml.make_case(N, D, seed),
                  lambda x, th: ml.kernel_parts(x, x, th, nu2)["K"].astype(np.float64), lambda x, t, th: _MaternModel(x, t, th, nu2),
                  _fused_gradient(ml, lambda x, th, Ki, al, dt: ml.grad(x, th, nu2, Ki, al, dt)))


FAMILIES = [
    Family("gaussian", sk.GaussianCovariance, lambda seed: dl.make_case(N, D, seed), _gauss_K, _DeviceModel,
           _fused_gradient(dl, lambda x, th, Ki, al, dt: dl.grad(x, th, Ki, al, dt))),
    _matern(3), _matern(5),                                  # every nu MaternCovariance accepts (ml.NU2_ALL)
    Family("periodic", sk.PeriodicCovariance, lambda seed: pl.make_case(N, D, seed),
           lambda x, th: pl.kernel_parts(x, x, th)["K"].astype(np.float64), _PeriodicModel,
           _fused_gradient(pl, lambda x, th, Ki, al, dt: pl.grad(x, th, Ki, al, dt))),
    Family("generic_subclass", OwnCrossCovariance, lambda seed: dl.make_case(N, D, seed), _gauss_K,
           lambda x, t, th: _MatrixModel(OwnCrossCovariance().cov_matrix(x, th), t), _generic_gradient),
]
assert tuple(ml.NU2_ALL) == (3, 5)


def _both(cov, x, t, theta):
    return cov._negativeloglikelihood(x, t, theta), np.array(cov._d_nll_d_theta(x, t, theta))


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_x_overwritten_in_place_is_refitted(fam):
    x, t, theta = fam.case(4101)
    x2 = fam.case(4102)[0]
    assert x2.shape == x.shape and not np.array_equal(x, x2)
    cov = fam.make()
    assert cov._fused() == (fam.name != "generic_subclass")
    nll1, g1 = _both(cov, x, t, theta)
    x[:] = x2
    nll, g = _both(cov, x, t, theta)
    fresh_nll, fresh_g = _both(fam.make(), x2.copy(), t.copy(), theta.copy())
    print("%s: nll at x1 %.17g, at x2 %.17g, new object at x2 %.17g" % (fam.name, nll1, nll, fresh_nll))
    assert nll == fresh_nll and g.tobytes() == fresh_g.tobytes(), "a model fitted to the old content of x was served"
    assert nll != nll1
    np.testing.assert_allclose(nll, ml.nll(fam.K_ld(x2, theta), t), rtol=dl.NLL_RTOL)
    fam.grad(x2, t, theta, g, "%s after an in-place edit" % fam.name, fam.model)


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_scaled_temporaries_each_get_their_own_fit(fam):
    """a profile likelihood over an input scaling: for s in (1, 1.5, 2): f(x * s, t, theta)"""
    x, t, theta = fam.case(4101)
    cov = fam.make()
    scales = (1.0, 1.5, 2.0)
    got = []
    for s in scales:
        got.append(cov._negativeloglikelihood(x * s, t, theta))
    held = [x * s for s in scales]
    want = [fam.make()._negativeloglikelihood(xs, t, theta) for xs in held]
    print("%s: %r" % (fam.name, got))
    assert got == want, "a temporary was served the model of another"
    assert len(set(got)) == 3
