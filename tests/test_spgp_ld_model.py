"""The long-double SPGP model of tests/_spgp_ld.py is the operation the GPU tests (tests/test_spgp_bounds.py) think it is, and their
comparison rule can see the defects they are meant to catch.

The model agrees with the float64 oracle on the inputs the older gradient tests use (cond(K_M) about 1e8 there: to what that leaves of
float64); its gradient is the derivative of its own likelihood (central differences in long double, Richardson-extrapolated); the committed
fixture belongs to the inputs the tests rebuild; and a change of 1e-9 of a group's maximum in one pseudo-input entry, one log w entry or
one prediction fails the rule."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as orc

import _spgp_ld as ld

LD = ld.LD


def _old_recipe(N, d, m):
    """the inputs of test_spgp_analytic_gradient_against_oracle (tests/test_gpu_parity.py)"""
    rng = np.random.RandomState(N + m)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    t = t - t.mean()
    xb = x[rng.choice(N, m, replace=False)] + 0.05 * rng.randn(m, d)
    th = np.concatenate([np.log([1.7, 0.02]), np.log(rng.uniform(0.02, 0.08, d)), xb.ravel()])
    xs = rng.uniform(0, 10, (ld.NQ, d))
    return x, t, th, xs


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps < 2.0 ** -60


def test_linear_algebra_against_lapack():
    rng = np.random.RandomState(4)
    G = rng.randn(40, 60)
    A = G.dot(G.T) + 40 * np.eye(40)
    B = rng.randn(40, 3)
    L = ld.chol(A)
    assert L.dtype == LD and np.abs(L @ L.T - A.astype(LD)).max() < 1e-16 * np.abs(A).max()
    np.testing.assert_allclose(L.astype(float), np.linalg.cholesky(A), rtol=0, atol=1e-13)
    assert np.abs(L @ ld.fwd(L, B) - B).max() < 1e-17 * 40 and np.abs(L.T @ ld.bwd(L, B) - B).max() < 1e-17 * 40


@pytest.mark.parametrize("N,d,m", [(300, 2, 7), (1500, 3, 130)])
def test_model_agrees_with_oracle_on_existing_inputs(N, d, m):
    """These length scales make K_M ill conditioned -- cond(K_M + 1e-6 I) reaches 1e8 at m = 130 -- and float64 keeps eps * cond of a
    group's scale, taken with a factor m for the sums: 130 * 1e8 * 2^-53 = 1.4e-6 for both cases.  (A transcription error moves a group
    by parts in ten, not in a million.)"""
    x, t, th, xs = _old_recipe(N, d, m)
    want = ld.evaluate(x, t, th, m, xs)
    ref = ld.evaluate_f64(x, t, th, m, xs)
    xb = th[2 + d:].reshape(m, d)
    cond = np.linalg.cond(orc.gram_ij(xb, xb, th[:2 + d]) + 1e-6 * np.eye(m))
    tol = 130 * 1e8 * 2.0 ** -53
    dist = ld.distances(ref, want, d, ld.vvt_of(th))
    print(N, d, m, "cond %.2e" % cond, {k: "%.1e" % r for k, r in dist.items()})
    assert cond < 1e8 and max(dist.values()) <= tol, dist
    # the generic dense route of the oracle (the reference's own formulas) gives the same predictor
    omu, ovar = orc.OracleSPGP(x, t, th, m).estimate_many(xs)
    dist = ld.distances({"mean": omu, "var": ovar}, want, d, ld.vvt_of(th))
    assert max(dist.values()) <= 10 * tol, dist


def _richardson(f, h):
    d1 = (f(h) - f(-h)) / (2 * h)
    d2 = (f(h / 2) - f(-h / 2)) / h
    return (4 * d2 - d1) / 3


@pytest.mark.parametrize("shape,recipe,entries", [((300, 2, 7), (0.5, 2.0, 0.05), None),
                                                  ((100, 3, 130), (2.0, 8.0, 0.3), [0, 1, 2, 3, 4, 5, 6, 200, 394])],
                         ids=["all_entries_m7", "n_below_m"])
def test_gradient_is_the_derivative_of_the_likelihood(shape, recipe, entries):
    """central differences at h and h / 2 in long double, extrapolated: the truncation error is O(h^4) = 3.6e-15 times a fifth-derivative
    ratio, the rounding error eps_ld |nll| / h = 1e-13; 1e-10 of each group's scale leaves both room and is far below any wrong term."""
    N, d, m = shape
    x, t, th, _xs = ld.make_case(N, d, m, *recipe)
    _f, g = ld.nll_grad(x, t, th, m)
    idx = list(range(len(th))) if entries is None else entries
    h = LD(2.0) ** -12
    thl = th.astype(LD)
    scale = np.abs(g).copy()
    scale[2 + d:] = np.abs(g[2 + d:]).max()
    for j in idx:
        def f(s):
            e = thl.copy()
            e[j] += s
            return ld.nll(x, t, e, m)
        fd = _richardson(f, h)
        assert abs(fd - g[j]) <= 1e-10 * scale[j], (j, float(fd), float(g[j]))


def test_fixture_belongs_to_the_inputs():
    """every fixture case: the hash of the rebuilt inputs, and the float64 oracle on them within 1e-6 of the stored long-double values.
    (Values of another problem differ in the first digit.  rho_ref is 1e-13 .. 1e-11 for the other cases; at d = 9 the sharp length
    scales leave a kernel that is nearly diagonal, log w and pseudo-input gradients of 1e-8 that are sums of cancelling terms, and the
    float64 evaluation keeps 1e-7 of them.)"""
    g = load_golden("spgp_ld")
    cases = {"n300_d3_m520": ((300, 3, 520), (2.0, 8.0, 0.3)), "n300_d9_m520": ((300, 9, 520), (2.0, 8.0, 0.3)),
             "n300_d9_m520_wide": ((300, 9, 520), (0.05, 0.2, 0.3)),
             "n200_d3_m1030": ((200, 3, 1030), (2.0, 8.0, 0.3)), "n16384_d3_m130": ((16384, 3, 130), (0.5, 2.0, 0.05))}
    assert sorted(k.split("__")[0] for k in g if k.endswith("__nll")) == sorted(cases)
    for name, ((N, d, m), recipe) in cases.items():
        x, t, th, xs = ld.make_case(N, d, m, *recipe)
        assert str(g[name + "__sha256"]) == ld.input_hash(x, t, th, xs)
        want = {k: g[name + "__" + k] for k in ("nll", "grad", "mean", "var")}
        assert want["grad"].shape == (2 + d + m * d,) and want["mean"].shape == want["var"].shape == (ld.NQ,)
        rho = ld.rho_ref(ld.evaluate_f64(x, t, th, m, xs), want, d, ld.vvt_of(th))
        print(name, "rho_ref %.3e" % rho)
        assert rho < 1e-6


def test_shift_is_exact_in_the_model():
    """the translated inputs are the same problem: the model's direct differences give the same long-double bits"""
    N, d, m = 300, 2, 7
    a = ld.evaluate(*_with_m(ld.make_case(N, d, m, 0.5, 2.0, 0.05), m))
    b = ld.evaluate(*_with_m(ld.make_case(N, d, m, 0.5, 2.0, 0.05, shift=ld.SHIFT), m))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def _with_m(c, m):
    x, t, th, xs = c
    return x, t, th, m, xs


@pytest.fixture(scope="module", params=[((300, 2, 7), (0.5, 2.0, 0.05)), ((256, 3, 128), (2.0, 8.0, 0.3))], ids=["m7", "m128"])
def clean(request):
    (N, d, m), recipe = request.param
    x, t, th, xs = ld.make_case(N, d, m, *recipe)
    want = ld.evaluate(x, t, th, m, xs)
    ref = ld.evaluate_f64(x, t, th, m, xs)
    vvt = ld.vvt_of(th)
    rho = ld.rho_ref(ref, want, d, vvt)
    return d, m, vvt, want, ref, rho


def test_rule_passes_the_float64_evaluation(clean):
    d, m, vvt, want, ref, rho = clean
    assert rho < 1e-11                                         # the recipe is well conditioned: the bound below means something
    ld.assert_within(ref, want, rho, d, vvt)
    ld.assert_within(ref, want, rho, d, vvt, margin=1.0)       # rho_ref is the largest ratio itself


@pytest.mark.parametrize("planted", ["pseudo-input", "log w", "mean", "var"])
def test_rule_fails_a_planted_error(clean, planted):
    """one entry moved by 1e-9 of its group's maximum, on top of the float64 evaluation's own error"""
    d, m, vvt, want, ref, rho = clean
    bad = {k: np.array(v, dtype=float) for k, v in ref.items()}
    if planted == "pseudo-input":
        bad["grad"][2 + d + (m * d) // 2] += 1e-9 * np.abs(ref["grad"][2 + d:]).max()
    elif planted == "log w":
        bad["grad"][2 + d - 1] *= 1 + 1e-9
    elif planted == "mean":
        bad["mean"][5] += 1e-9 * np.abs(ref["mean"]).max()
    else:
        bad["var"][ld.NQ - 1] += 1e-9 * vvt
    with pytest.raises(AssertionError) as info:
        ld.assert_within(bad, want, rho, d, vvt)
    group = {"pseudo-input": "xb", "log w": "log w_%d" % (d - 1), "mean": "mean", "var": "var"}[planted]
    assert group + " " in str(info.value)
    dist = ld.distances(bad, want, d, vvt)
    assert [k for k, r in dist.items() if r > ld.bound(rho)] == [group]      # and only that group
