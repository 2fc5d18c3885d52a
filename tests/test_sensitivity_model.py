"""The long-double model of tests/_sensitivity_model.py is the variance decomposition it claims to be, the comparison rule sees the defects
it is meant to catch, and SensitivityAnalysis._variances_of parses every accepted form of Sigma_x.  CPU only.

  * at (N, d) = (12, 1), (12, 2), (12, 3) -- d = 3 with w = (0.3, 0.08, 0.5), s = (0.7, 1.5, 0.2) -- mean, V and every first_k / total_k of
    the model equal the 60-node tensor Gauss-Hermite evaluation of the DEFINITIONS (E mu, Var mu, Var_{x_k} E[mu | x_k],
    E Var_{x_k}(mu | x_~k)) within 1e-12 max(V, 1e-300): three orders above the 6e-16 the two agree to, far below any error of a formula;
    doubling the order to 120 moves the quadrature by less than that;
  * three seeded defects in the float64 evaluation -- a dropped pair, weight 1 instead of 2 below the diagonal, products over all l instead
    of l != k -- land outside the bound, on cases whose own float64 evaluation stays inside it;
  * _variances_of: the vector, the diagonal matrix, [b, d], [b, d, d], and its ValueErrors."""
import numpy as np
import pytest

import _dense_ld as dl
import _sensitivity_model as sm

W3, S3 = (0.3, 0.08, 0.5), (0.7, 1.5, 0.2)


def small_case(d):
    rng = np.random.RandomState(40 + d)
    x = dl._grid(rng.uniform(0, 10, (12, d)))
    beta = rng.randn(12)
    theta = np.log(np.concatenate([[2.0, 0.01], W3[:d]]))
    u = dl._grid(rng.uniform(3, 7, d))
    return x, theta, beta, u, np.array(S3[:d])


@pytest.mark.parametrize("d", [1, 2, 3])
def test_model_is_the_definitions(d):
    x, theta, beta, u, s = small_case(d)
    model = sm.sums(x, theta, beta, u, s)
    mean, V, first, total = sm.quadrature(x, theta, beta, u, s, 60)
    mean2, V2, first2, total2 = sm.quadrature(x, theta, beta, u, s, 120)
    tol = 1e-12 * max(float(V), 1e-300)
    worst = 0.0
    for name, got, q60, q120 in (("mean", model["mean"][0][0], mean, mean2), ("V", model["V"][0][0], V, V2)):
        worst = max(worst, float(abs(got - q60)))
        assert abs(got - q60) <= tol, (name, float(got), float(q60))
        assert abs(q60 - q120) <= tol, (name, "order", float(q60 - q120))
    for name, got, q60, q120 in (("first", model["first"][0], first, first2), ("total", model["total"][0], total, total2)):
        worst = max(worst, float(np.abs(got - q60).max()))
        assert np.all(np.abs(got - q60) <= tol), (name, got, q60)
        assert np.all(np.abs(q60 - q120) <= tol), (name, "order")
    print("d=%d: V %.6g, worst |model - quadrature| %.3e (tolerance %.3e)" % (d, float(V), worst, tol))
    F, T = model["first"][0], model["total"][0]
    assert float(V) > 0 and np.all(F > 0)
    assert F.sum() <= model["V"][0][0] * (1 + 1e-15) and model["V"][0][0] <= T.sum() * (1 + 1e-15)
    if d == 1:
        assert abs(F[0] - model["V"][0][0]) <= tol and abs(T[0] - model["V"][0][0]) <= tol


def test_zero_variance_coordinates_vanish():
    x, theta, beta, u, s = small_case(3)
    s = s.copy()
    s[1] = 0.0
    model = sm.sums(x, theta, beta, u, s)
    for key in ("first", "total"):
        val, scale = model[key]
        assert abs(val[1]) <= 1e-17 * scale[1] and val[0] > 0 and val[2] > 0
    none = sm.sums(x, theta, beta, u, np.zeros(3))
    assert abs(none["V"][0][0]) <= 1e-17 * none["V"][1][0]
    v, w = np.exp(theta[0]), np.exp(theta[2:])
    plain = (beta * v * np.exp(-0.5 * (w * (u - x) ** 2).sum(1))).sum()
    assert float(none["mean"][0][0]) == pytest.approx(plain, rel=1e-14)


@pytest.mark.parametrize("N,d", [(200, 3), (129, 8)])
def test_rule_sees_seeded_defects(N, d):
    seed = dl.seed_of(N, d)
    x, t, theta = dl.make_case(N, d, seed)
    rng = np.random.RandomState(seed)
    beta = rng.randn(N)
    u = dl.inputs_u(x, theta, seed)["between"]
    s = sm.variances(d, seed)["drawn"]
    want, ref = sm.both(x, theta, beta, u, s)
    rho = dl.rho_of(sm.ref_distances(want, ref))
    assert rho <= sm.FLOOR, rho                     # the float64 evaluation leaves the whole margin to the device
    lim = sm.bound(rho)
    for defect, keys in (("pair", ("V", "first", "total")), ("offdiag1", ("V", "first", "total")), ("allprod", ("first", "total"))):
        bad = sm.sums(x, theta, beta, u, s, dt=np.float64, defect=defect)
        dist = {k: dl.distances(bad[k][0], want[k][0], want[k][1]) for k in keys}
        print("N=%d d=%d %-8s " % (N, d, defect) + "  ".join("%s %.3e" % (k, float(r.max())) for k, r in dist.items()) + "  bound %.3e" % lim)
        for k, r in dist.items():
            assert float(r.max()) > lim, (defect, k, float(r.max()), lim)


# ------------------------------------------------------------------------------------------------
# Sigma_x parsing (needs no device)
# ------------------------------------------------------------------------------------------------
def test_variances_of_accepted_forms():
    from skgpuppy_amd import SensitivityAnalysis
    vo = SensitivityAnalysis._variances_of
    s = np.array([0.5, 0.0, 2.0])
    np.testing.assert_array_equal(vo(s, 3), s)
    np.testing.assert_array_equal(vo([0.5, 0.0, 2.0], 3), s)
    np.testing.assert_array_equal(vo(np.diag(s), 3), s)
    np.testing.assert_array_equal(vo(s, 3, b=5), s)                       # one set for all inputs
    np.testing.assert_array_equal(vo(np.diag(s), 3, b=5), s)
    many = np.arange(10.0).reshape(5, 2)
    np.testing.assert_array_equal(vo(many, 2, b=5), many)
    np.testing.assert_array_equal(vo(np.stack([np.diag(r) for r in many]), 2, b=5), many)
    out = vo(np.stack([np.diag(r) for r in many]), 2, b=5)
    assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and out.shape == (5, 2)
    assert vo(np.array([[0.25]]), 1).shape == (1,)
    assert vo(np.zeros((0, 2, 2)), 2, b=0).shape == (0, 2)


def test_variances_of_refusals():
    from skgpuppy_amd import SensitivityAnalysis
    vo = SensitivityAnalysis._variances_of
    full = np.array([[1.0, 0.1], [0.1, 1.0]])
    with pytest.raises(ValueError, match="independent"):
        vo(full, 2)
    with pytest.raises(ValueError, match="independent"):
        vo(np.stack([np.eye(2), full, np.eye(2)]), 2, b=3)
    with pytest.raises(ValueError, match="independent"):
        vo(np.array([[1.0, np.nan], [0.0, 1.0]]), 2)
    for bad in (np.array([1.0, -0.5]), np.array([1.0, np.inf]), np.array([np.nan, 1.0])):
        with pytest.raises(ValueError, match="finite"):
            vo(bad, 2)
    for shape, b in (((3,), None), ((2, 3), None), ((4, 2), 5), ((5, 2, 3), 5), ((5, 2), None), ((2, 2, 2, 2), 2)):
        with pytest.raises(ValueError, match="expected"):
            vo(np.ones(shape), 2, b=b)
    with pytest.raises(ValueError, match="b == d"):
        vo(np.eye(2), 2, b=2)
    np.testing.assert_array_equal(vo(np.ones((2, 2, 2)) * np.eye(2), 2, b=2), np.ones((2, 2)))
