"""The long-double model of tests/_dense_ld.py is the operation the GPU tests (tests/test_dense_bounds.py) think it is, the inputs of
those tests are what they are meant to be, and the comparison rule sees the defects it is meant to catch.  CPU only.

  * on the goldens n203_d3 and n256_d8, with K^-1 and alpha from the oracle, the model's gradient, Approx and Exact moments and C / J / H are
    the oracle's, to the tolerances tests/test_oracle_golden.py holds the oracle to;
  * every (N, d) the GPU tests fit: at least a quarter of the pairs have Kf_ij > 1e-3 v (sharp case: at least N pairs), and the float64
    numpy evaluation of every sum of the case is within FLOOR of the model -- the reference alone leaves the whole margin to the device;
  * eight seeded defects in the float64 evaluation at (N, d) = (700, 9) and (200, 2) each land outside the bound.
K^-1 here is numpy's inverse of the oracle's Gram matrix (symmetrised); on the device the tests use the device's own."""
import functools

import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as orc

import _dense_ld as dl

LD = dl.LD


@functools.lru_cache(maxsize=None)
def fitted(N, d, sharp=False):
    x, t, theta = dl.make_case(N, d, dl.seed_of(N, d), sharp)
    Kinv = np.linalg.inv(orc.gram(x, theta))
    Kinv = (Kinv + Kinv.T) / 2
    return x, t, theta, Kinv, Kinv.dot(t)


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps < 2.0 ** -60


def test_small_inverse_and_constants():
    rng = np.random.RandomState(3)
    A = rng.randn(9, 9)
    A = A.dot(A.T) + 9 * np.eye(9)
    Ai = dl.small_inverse(A.astype(LD))
    assert Ai.dtype == LD and np.abs(Ai.dot(A.astype(LD)) - np.eye(9)).max() < 1e-17
    w, S = rng.uniform(0.01, 0.1, 9), dl.sigmas(9, 1)["full"]
    Ls, dd, nc1, nc2 = dl.exact_constants(w, S, np.float64)
    Lam = 2 * np.diag(w) - np.linalg.inv(0.5 * np.diag(1 / w) + S)            # oracle.exact_propagate's Linv
    np.testing.assert_allclose(Ls, (Lam + Lam.T) / 2, rtol=0, atol=1e-15)
    np.testing.assert_allclose(dd, np.diagonal(np.diag(w) - np.diag(w / (1 + w * np.diag(S)))), rtol=1e-14)
    assert nc1 == pytest.approx(1 / np.sqrt(np.linalg.det(np.eye(9) + np.diag(w) * S)), rel=1e-14)
    assert nc2 == pytest.approx(1 / np.sqrt(np.linalg.det(2 * np.diag(w) * S + np.eye(9))), rel=1e-14)


# ------------------------------------------------------------------------------------------------
# the model is the oracle's operation
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["n203_d3", "n256_d8"])
def golden_case(request):
    g = load_golden(request.param)
    return g, orc.OracleGP(g["x"], g["t_raw"], g["theta"])


def test_gradient_is_the_oracles(golden_case):
    g, gp = golden_case
    got, _s = dl.grad(g["x"], g["theta"], gp.Kinv, gp.beta())
    ref = orc.nll_grad(g["x"], gp.t, g["theta"])
    np.testing.assert_allclose(got.astype(float), ref, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(ref).max()))
    # the generic entry's form on the oracle's derivative matrices
    for j in (0, 1, len(ref) - 1):
        one, _s = dl.grad_matrix(gp.Kinv, gp.beta(), orc.d_gram_d_theta(g["x"], g["theta"], j))
        np.testing.assert_allclose(float(one[0]), ref[j], rtol=1e-6, atol=1e-6 * max(1.0, np.abs(ref).max()))


def test_propagation_is_the_oracles(golden_case):
    g, gp = golden_case
    v = np.exp(g["theta"][0])
    tol = 1e-9 * v
    for iu in range(int(g["nu"])):
        u = g["u%d" % iu]
        C, J, H = orc.cjh(gp, u)
        # the same functions in float64 at the golden test's tolerances; in long double as well, except that a diagonal entry of H is a
        # difference ((w_a delta_a)^2 - w_a) c that float64 keeps to 1e-13 of its two terms, not of itself (1.7e-12 of one entry here)
        fC, fJ, fH, _q, _a = dl.cjh(g["x"], g["theta"], u, dt=np.float64)
        np.testing.assert_allclose(fC, C, rtol=1e-14, atol=0)
        np.testing.assert_allclose(fJ, J[:, :, 0], rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(fH, H, rtol=1e-13, atol=1e-300)
        mC, mJ, mH, _q, mHabs = dl.cjh(g["x"], g["theta"], u)
        np.testing.assert_allclose(mC.astype(float), C, rtol=1e-14, atol=0)
        np.testing.assert_allclose(mJ.astype(float), J[:, :, 0], rtol=1e-13, atol=1e-300)
        assert (np.abs(mH - H.astype(LD)) <= 1e-13 * mHabs + 1e-300).all()
        dv = np.array([orc.approx_dvh(gp, u, h, (C, J, H)) for h in range(gp.d)])
        for iS in range(int(g["nS"])):
            S = g["Sigma%d" % iS]
            m = dl.approx_partials(g["x"], g["theta"], gp.Kinv, gp.beta(), u, S)
            om, os2, orest = orc.approx_parts(gp, u, S, (C, J, H))
            assert float(m["mean"][0][0]) == pytest.approx(om, abs=1e-10)
            assert float(m["sigma2"][0][0]) == pytest.approx(os2, abs=tol) and float(m["rest"][0][0]) == pytest.approx(orest, abs=tol)
            assert float(m["var"][0][0]) == pytest.approx(orc.approx_propagate(gp, u, S, (C, J, H))[1], abs=tol)
            np.testing.assert_allclose(m["dvh"][0].astype(float), dv, rtol=1e-7, atol=tol * 10)
            # the partials are what distributed.combine_approx_partials combines
            from skgpuppy_amd.distributed import combine_approx_partials
            mu, var, s2, rest = combine_approx_partials(m["partials"][0].astype(float), S, v, np.exp(g["theta"][1]))
            assert (mu, var) == pytest.approx((om, os2 + orest), abs=tol)
            e = dl.exact_builtin(g["x"], g["theta"], gp.Kinv, gp.beta(), u, S)
            me, ve = orc.exact_propagate(gp, u, S)
            assert float(e["mean"][0][0]) + gp.meant == pytest.approx(me, abs=1e-10)
            assert float(e["var"][0][0]) == pytest.approx(ve, abs=tol)
    # and row ranges add up to the whole
    u, S = g["u0"], g["Sigma0"]
    whole = dl.approx_partials(g["x"], g["theta"], gp.Kinv, gp.beta(), u, S)["partials"][0]
    parts = [dl.approx_partials(g["x"], g["theta"], gp.Kinv, gp.beta(), u, S, rows=r)["partials"][0] for r in ((0, 128), (128, gp.n))]
    assert np.abs(parts[0] + parts[1] - whole).max() <= 1e-17 * np.abs(whole).max() + 1e-30
    whole = dl.exact_builtin(g["x"], g["theta"], gp.Kinv, gp.beta(), u, S)["parts"][0]
    parts = [dl.exact_builtin(g["x"], g["theta"], gp.Kinv, gp.beta(), u, S, rows=r)["parts"][0] for r in ((0, 128), (128, gp.n))]
    assert np.abs(parts[0][:2] + parts[1][:2] - whole[:2]).max() <= 1e-17 * np.abs(whole[:2]).max() and parts[0][2] == whole[2]


# ------------------------------------------------------------------------------------------------
# the GPU tests' cases
# ------------------------------------------------------------------------------------------------
def reference_distances(x, theta, Kinv, alpha):
    """{group: distances of the float64 evaluation from the model} over every sum tests/test_dense_bounds.py compares for one fit"""
    N, d = x.shape
    seed = dl.seed_of(N, d)
    want, ref = dl.grad(x, theta, Kinv, alpha), dl.grad(x, theta, Kinv, alpha, dt=np.float64)
    out = {"grad": dl.distances(ref[0], want[0], want[1])}
    for un, u in dl.inputs_u(x, theta, seed).items():
        for sn, S in dl.sigmas(d, seed).items():
            for name, fn, keys in (("approx", dl.approx_partials, ("partials", "mean", "var", "sigma2", "rest", "dvh")),
                                   ("exact", dl.exact_builtin, ("parts", "mean", "var"))):
                w, f = fn(x, theta, Kinv, alpha, u, S), fn(x, theta, Kinv, alpha, u, S, dt=np.float64)
                for k in keys:
                    out["%s %s %s %s" % (name, un, sn, k)] = dl.distances(f[k][0], w[k][0], w[k][1])
    return out


RHO = {}


@pytest.mark.parametrize("N,d", dl.CASES, ids=["n%d_d%d" % c for c in dl.CASES])
def test_case_inputs_and_reference(N, d):
    x, t, theta, Kinv, alpha = fitted(N, d)
    assert np.array_equal(x, np.round(x * 2.0 ** 20) / 2.0 ** 20) and x.min() >= 0 and x.max() <= 10 and abs(t.mean()) < 1e-15
    assert dl.live_pairs(x, theta) >= N * N / 4
    us = dl.inputs_u(x, theta, dl.seed_of(N, d))
    assert np.array_equal(us["equal"], x[dl.QUIRK_ROW]) and not (x == us["between"]).all(1).any()
    _v, _vt, w = dl.params(theta, d, np.float64)
    qfar = (w * (x - us["far"]) ** 2).sum(1)
    assert dl.FAR_Q <= qfar.min() < dl.FAR_Q + 1 and qfar.max() < 1400          # some C_i C_j below the normal range, no C_i itself
    dist = reference_distances(x, theta, Kinv, alpha)
    rho = dl.rho_of(dist)
    RHO[N, d] = rho
    print("N=%d d=%d rho_ref %.3e (%s)" % (N, d, rho, max(dist, key=lambda k: dist[k].max())))
    assert rho <= dl.FLOOR
    dl.assert_within(dist, rho, what="the float64 evaluation")


def test_sharp_case_inputs_and_reference():
    """the explicit Exact path's case: sharp length scales at d = 3, u at a corner of the cube, C_ux from the kernel in float64"""
    N, d = dl.SHARP_CASE
    x, t, theta, Kinv, alpha = fitted(N, d, True)
    assert dl.live_pairs(x, theta) >= N
    u, S, C, w, cuu = dl.sharp_inputs(x, theta)
    want = dl.exact_parts(x, w, Kinv, alpha, C, u, S, cuu)
    ref = dl.exact_parts(x, w, Kinv, alpha, C, u, S, cuu, dt=np.float64)
    assert 50 <= want["emax"] < 700                       # positive exponents, and exp of the largest is finite in float64
    rho = max(dl.distances(ref[k][0], want[k][0], want[k][1]).max() for k in ("parts", "mean", "var"))
    print("sharp: largest exponent %.1f, rho_ref %.3e" % (want["emax"], rho))
    assert rho <= dl.FLOOR
    # with the kernel's own C_ux the large exponents weigh nothing: the pairs above 5 carry less than 1e-12 of the absolute terms ...
    a = u - x
    Ls = dl.exact_constants(w, S, np.float64)[0]
    aL = a.dot(Ls)
    E = ((aL * a).sum(1)[:, None] + (aL * a).sum(1)[None, :]) / 8 + aL.dot(a.T) / 4
    terms = np.outer(C, C) * np.exp(E)
    assert terms[E >= 5].sum() < 1e-12 * terms.sum() and E.max() == pytest.approx(want["emax"], rel=1e-12)
    # ... so the GPU test runs the same inputs under a flat operator as well, C_ux = 1, where the largest exponents ARE the sum
    flat = np.ones(N)
    want, ref = dl.exact_parts(x, w, Kinv, alpha, flat, u, S, 1.0), dl.exact_parts(x, w, Kinv, alpha, flat, u, S, 1.0, dt=np.float64)
    rho = max(dl.distances(ref[k][0], want[k][0], want[k][1]).max() for k in ("parts", "mean", "var"))
    top = np.exp(E - E.max())
    print("flat: rho_ref %.3e, pairs within e^-5 of the largest term: %d" % (rho, (top > np.exp(-5.0)).sum()))
    assert rho <= dl.FLOOR and float(want["parts"][0][1]) > 1e80


# ------------------------------------------------------------------------------------------------
# the rule sees the seeded defects
# ------------------------------------------------------------------------------------------------
DEFECT_MOVED = {}


@pytest.mark.parametrize("defect", ["pair", "diag2", "coord", "tail", "quarter", "exp32", "quirk", "unsym"])
@pytest.mark.parametrize("N,d", [(700, 9), (200, 2)])
def test_rule_fails_a_seeded_defect(N, d, defect):
    """pair: one (i, j) (and (j, i)) dropped; diag2: the diagonal weighted 2; coord: coordinate d - 1 left out of q; tail: the last
    700 - 512 columns dropped (at N = 200 the same fraction); quarter: one of four interleaved column partials dropped; exp32: exp in
    float32; quirk: +vt ignored at u = a training point; unsym: the lower triangle of a non-symmetric K^-1 alone in the j <= i form"""
    x, t, theta, Kinv, alpha = fitted(N, d)
    seed = dl.seed_of(N, d)
    S = dl.sigmas(d, seed)["full"]
    us = dl.inputs_u(x, theta, seed)
    if defect == "quirk":
        args = (x, theta, Kinv, alpha, us["equal"], S)
        want, ref, bad = dl.approx_partials(*args), dl.approx_partials(*args, dt=np.float64), dl.approx_partials(*args, dt=np.float64, defect=defect)
        keys = ("partials", "mean", "var", "sigma2", "rest")
    elif defect == "unsym":
        rng = np.random.RandomState(5)
        Kn = Kinv * (1 + 1e-3 * rng.uniform(-1, 1, Kinv.shape))              # symmetric to three digits only
        args = (x, theta, Kn, alpha, us["between"], S)
        want, ref, bad = dl.exact_builtin(*args), dl.exact_builtin(*args, dt=np.float64), dl.exact_builtin(*args, dt=np.float64, defect=defect)
        keys = ("parts", "var")
    else:
        args = (x, theta, Kinv, alpha)
        want, ref, bad = ({"grad": dl.grad(*args, **kw)} for kw in ({}, {"dt": np.float64}, {"dt": np.float64, "defect": defect}))
        keys = ("grad",)
    rho = max(dl.distances(ref[k][0], want[k][0], want[k][1]).max() for k in keys)
    dist = {k: dl.distances(bad[k][0], want[k][0], want[k][1]) for k in keys}
    moved = max(r.max() for r in dist.values())
    DEFECT_MOVED[N, d, defect] = moved
    print("N=%d d=%d %-8s rho_ref %.3e  bound %.3e  moved %.3e" % (N, d, defect, rho, dl.bound(rho), moved))
    assert rho <= dl.FLOOR and moved > dl.bound(rho) == dl.MARGIN * dl.FLOOR
    with pytest.raises(AssertionError):
        dl.assert_within(dist, rho)
    dl.assert_within({k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in keys}, rho)      # and passes the clean evaluation


def test_rule_details():
    assert dl.distances([0.0, 1.0], [0.0, 1.0], [0.0, 2.0]).tolist() == [0.0, 0.0]       # 0 / 0: exactly 0 where the model is
    with pytest.raises(AssertionError):
        dl.assert_within({"g": dl.distances([1e-300], [0.0], [0.0])}, 0.0)                # anything against an exact 0 fails
    with pytest.raises(AssertionError):
        dl.assert_within({"g": dl.distances([np.nan], [1.0], [1.0])}, 0.0)
    with pytest.raises(AssertionError):
        dl.assert_within({"g": dl.distances([np.inf], [1.0], [1.0])}, 0.0)
    dl.assert_within({"g": dl.distances([1.0 + 2.0 ** -40], [1.0], [1.0])}, 2.0 ** -45)     # 32 rho_ref
    assert dl.bound(0.0) == dl.MARGIN * dl.FLOOR == 32 * 1000 * 2.0 ** -53
