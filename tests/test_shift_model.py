"""The host side of tests/test_shifted_inputs.py, without a device: the translations are exact, the long-double models do not move under
them, the float64 restatement of the prescaled gradient (tests/_shift.restated_grad) stays within the allowance of _dense_ld.grad_loss, and
seeded defects are seen by the comparison that holds the device.

K^-1 and alpha are NumPy's, from the float64 Gram of the case as seeded: the sums are judged on a GIVEN K^-1 and alpha, as on the device.

The bound is the rule's smallest, dl.bound(0) = MARGIN * FLOOR, on the plain scales of _dense_ld.grad.  The restatement alone must pass
against long double once _dense_ld.grad_loss is taken off (the reference meets the bound it sets), sum by sum and, since the allowance is
a sum of per-pair terms, pair by pair.  The seeded defects are judged where the device is judged (tests/_shift.py, "against the
restatement"): the defective arithmetic takes the device's place and its d + 2 values are compared with restated_grad's under the plain
rule.  What they show there, in all twelve cases:
  expanded   passes as seeded (sqrt(w) |x| <= 2: u |a|^2 is a few u), stays under the rule's floor at 2^10 (at most 8.5e-13 of the absolute
             terms: no assertion on the d + 2 sums has power there) and exceeds the bound at 2^17 by 150 to 3000 times: the device test
             asserts at 2^17 for this reason;
  scaled32   the scaled coordinate in float32: exceeds the bound at 2^10 and 2^17 and grows with the offset (1e4 times from 0 to 2^17);
             it does not pass as seeded either (float32 is too coarse for a 3.6e-12 rule at any offset);
  sqrt32     a float32 sqrt(w) is a relative 6e-8 in every w_k wherever the inputs are: the same distance at every shift, to 1 %, which is
             what the test asserts; the sums see it in eight of the twelve cases, with or without a translation (figures printed);
  eq_scaled  cannot be seen on these inputs, at any shift, and the test says why by asserting it: two grid points that differ are at
             least 2^-20 apart, 2^-37 relative at 2^17, and stay 2^15 ulps apart after one rounded multiplication by fl(sqrt(w_k)); two
             that are equal stay equal.  Equality on scaled coordinates and equality on raw ones are the same predicate here.  The
             device-side guard for the equality is the exact `+vt at every shift` comparison of tests/test_shifted_inputs.py."""
import numpy as np
import pytest

import _dense_ld as dl
import _exact_grad_model as eg
import _matern_ld as ml
import _periodic_ld as pl
import _predict_grad_model as pg
import _rows_ld as rl
import _sensitivity_model as sm
import _shift as sh

CASES = [(N, d) for N in (129, 200) for d in (1, 3, 8, 9, 17)] + [(700, 3), (700, 8)]      # tests/test_shifted_inputs.py's
IDS = ["n%d_d%d" % c for c in CASES]
SMALL = (129, 3)


def dense_case(N, d):
    seed = dl.seed_of(N, d)
    x, t, theta = dl.make_case(N, d, seed)
    return {"x": x, "t": t, "theta": theta, "u": dl.inputs_u(x, theta, seed)}


def host_fit(case):
    """(K^-1, alpha) in float64 from the Gram of the case as seeded"""
    x, theta = case["x"], case["theta"]
    v, vt, w = dl.params(theta, x.shape[1], np.float64)
    q = sum(w[k] * (x[:, k][:, None] - x[:, k][None, :]) ** 2 for k in range(x.shape[1]))
    Kinv = np.linalg.inv(v * np.exp(-0.5 * q) + vt * np.eye(len(x)))
    return Kinv, Kinv.dot(case["t"])


# ------------------------------------------------------------------------------------------------
# the translation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", sh.SHIFTS, ids=sh.name_of)
def test_the_translation_is_exact_for_every_family(s):
    N, d = 200, 9
    families = [dense_case(N, d)]
    for mod in (ml, pl):
        x, t, theta = mod.make_case(N, d)
        families.append({"x": x, "t": t, "theta": theta, "xs": mod.make_queries(x, 300, 41)})
    x, t, theta, Uin, Sig = rl.make_case(N, d)
    families.append({"x": x, "t": t, "theta": theta, "U": Uin, "Sigma": Sig})
    for case in families:
        moved = sh.shifted(case, s)                                      # (asserts (a + s) - s == a for every coordinate)
        for k, a in case.items():
            if k not in sh.COORDINATES:
                assert moved[k] is a, k                                  # t, theta, Sigma: untouched
        assert (moved["x"] >= s).all() and moved["x"].shape == case["x"].shape
    with pytest.raises(AssertionError):                                  # off the grid the check does fire
        sh.translate(np.array([0.1]), sh.SHIFT)
    assert sh.shifted({"x": np.zeros((2, 1)), "t": None}, 0.0)["x"].tolist() == [[0.0], [0.0]]


# ------------------------------------------------------------------------------------------------
# the models do not move
# ------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for p, q in zip(a, b):
            _same(p, q)
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("dt", [dl.LD, np.float64], ids=["ld", "f64"])
@pytest.mark.parametrize("s", sh.SHIFTS, ids=sh.name_of)
def test_the_models_return_identical_values_for_translated_input(s, dt):
    """every model that tests/test_shifted_inputs.py takes for the truth, on (x + s, u + s) against (x, u): assert_array_equal"""
    N, d = SMALL
    case = dense_case(N, d)
    moved = sh.shifted(case, s)
    Kinv, alpha = host_fit(case)
    x, X, theta = case["x"], moved["x"], case["theta"]
    S = dl.sigmas(d, 1)["full"]
    _same(dl.grad(X, theta, Kinv, alpha, dt), dl.grad(x, theta, Kinv, alpha, dt))
    for un in case["u"]:
        u, U = case["u"][un], moved["u"][un]
        _same(dl.cjh(X, theta, U, dt), dl.cjh(x, theta, u, dt))
        _same(dl.approx_partials(X, theta, Kinv, alpha, U, S, dt=dt), dl.approx_partials(x, theta, Kinv, alpha, u, S, dt=dt))
        _same(dl.exact_builtin(X, theta, Kinv, alpha, U, S, dt=dt), dl.exact_builtin(x, theta, Kinv, alpha, u, S, dt=dt))
        _same(eg.moments_grad(X, theta, Kinv, alpha, U, S, dt=dt), eg.moments_grad(x, theta, Kinv, alpha, u, S, dt=dt))
        _same(sm.sums(X, theta, alpha, U, np.full(d, 0.3), dt=dt), sm.sums(x, theta, alpha, u, np.full(d, 0.3), dt=dt))
    Q, Qs = np.array(list(case["u"].values())), np.array(list(moved["u"].values()))
    for nu2 in pg.KINDS:
        _same(pg.mean_grad(X, theta, alpha, Qs, nu2, dt=dt), pg.mean_grad(x, theta, alpha, Q, nu2, dt=dt))
        _same(pg.var_grad(X, theta, Kinv, Qs, nu2, dt=dt), pg.var_grad(x, theta, Kinv, Q, nu2, dt=dt))
    x, _t, theta, Uin, Sig = rl.make_case(N, d)
    X, Us = sh.translate(x, s), sh.translate(Uin, s)
    for kind in rl.KINDS:
        for layout in rl.LAYOUTS_OF[kind]:
            _same(rl.rows(X, theta, Us, Sig, kind, layout, dt=dt), rl.rows(x, theta, Uin, Sig, kind, layout, dt=dt))
    x, _t, theta = ml.make_case(N, d)
    xs = ml.make_queries(x, 33, 41)
    for nu2 in ml.NU2_ALL:
        _same(ml.kernel_parts(sh.translate(xs, s), sh.translate(x, s), theta, nu2, dt, keep=True), ml.kernel_parts(xs, x, theta, nu2, dt, keep=True))
    x, _t, theta = pl.make_case(N, d)
    xs = pl.make_queries(x, 33, 41)
    _same(pl.kernel_parts(sh.translate(xs, s), sh.translate(x, s), theta, dt, keep=True), pl.kernel_parts(xs, x, theta, dt, keep=True))


# ------------------------------------------------------------------------------------------------
# the prescaled restatement, the allowance, and the defects on the device's own yardstick
# ------------------------------------------------------------------------------------------------
ALL_SHIFTS = (0.0,) + sh.SHIFTS


def _to_long_double(case, Kinv, alpha, s, defect=None):
    """the restatement on x + s against the long-double model of the case as seeded, on the plain scales less grad_loss (0 at shift 0)"""
    want, scale = dl.grad(case["x"], case["theta"], Kinv, alpha)
    loss = dl.grad_loss(case["x"], case["theta"], Kinv, alpha, s)
    got = sh.restated_grad(sh.translate(case["x"], s), case["theta"], Kinv, alpha, defect)
    return dl.distances(got, want, scale, loss), dl.distances(got, want, scale)


def _to_restatement(case, Kinv, alpha, s, defect):
    """what tests/test_shifted_inputs.py asserts of gpx_nll_grad, with the defective arithmetic in the device's place: the d + 2 values
    against restated_grad on the plain scales, no allowance"""
    _want, scale = dl.grad(case["x"], case["theta"], Kinv, alpha)
    X = sh.translate(case["x"], s)
    return dl.distances(sh.restated_grad(X, case["theta"], Kinv, alpha, defect), sh.restated_grad(X, case["theta"], Kinv, alpha), scale)


@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_the_restatement_stays_within_the_allowance(N, d):
    """the reference alone meets the bound it sets: the plain rule at shift 0, the rule after grad_loss at 2^10 and 2^17"""
    case = dense_case(N, d)
    Kinv, alpha = host_fit(case)
    for s in ALL_SHIFTS:
        dist, plain = _to_long_double(case, Kinv, alpha, s)
        print("restated gradient N=%d d=%d shift %s: %.3e after the allowance, %.3e without, of %.3e" % (
            N, d, sh.name_of(s), dist.max(), plain.max(), dl.bound(0.0)))
        dl.assert_within({"grad": dist}, 0.0, "restated gradient N=%d d=%d shift %s" % (N, d, sh.name_of(s)))


@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_the_restatement_stays_within_the_allowance_pair_by_pair(N, d):
    """the allowance is a sum of per-pair terms: the restatement's Kf_ij within MARGIN * FLOOR of long double after its own pair's term,
    on every pair of every case -- the derivation of _dense_ld.prescale_loss holds where it is made"""
    case = dense_case(N, d)
    for s in ALL_SHIFTS:
        dK = sh.pair_distances(case["x"], case["theta"], s)
        print("pairs N=%d d=%d shift %s: Kf %.3e of %.3e" % (N, d, sh.name_of(s), dK, dl.bound(0.0)))
        assert dK <= dl.bound(0.0), (s, dK)


@pytest.mark.parametrize("defect", ["expanded", "sqrt32", "scaled32"])
@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_seeded_defects_on_the_yardstick_of_the_device_test(N, d, defect):
    """module docstring: each defect in the device's place, on the d + 2 sums, against the restatement under the plain rule"""
    case = dense_case(N, d)
    Kinv, alpha = host_fit(case)
    dist = {s: float(_to_restatement(case, Kinv, alpha, s, defect).max()) for s in ALL_SHIFTS}
    lim = dl.bound(0.0)
    print("%s N=%d d=%d (bound %.3e): " % (defect, N, d, lim) + "  ".join("shift %s %.3e" % (sh.name_of(s), dist[s]) for s in ALL_SHIFTS))
    if defect == "expanded":
        assert dist[0.0] <= lim < dist[sh.SHIFT], dist                   # passes as seeded, seen at 2^17 in every case
        assert dist[sh.SHIFT] > 100 * dist[sh.OFFSET]                    # (quadratic in the offset; at 2^10 still under the rule's floor)
    elif defect == "scaled32":
        assert dist[sh.OFFSET] > lim and dist[sh.SHIFT] > lim, dist      # seen at both shifts in every case
        assert dist[sh.SHIFT] > 100 * dist[0.0]                          # and made by the translation: it grows with the offset
    else:
        for s in sh.SHIFTS:                                              # sqrt32 does not know where the inputs are
            assert abs(dist[s] / dist[0.0] - 1) < 0.01, dist


@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_equality_on_scaled_coordinates_is_the_same_predicate_on_the_grid(N, d):
    """module docstring, eq_scaled: the C row with its +vt is the same bits either way at every shift, for every input of the case, and the
    scaled coordinates of two different training values never collide"""
    case = dense_case(N, d)
    for s in (0.0,) + sh.SHIFTS:
        moved = sh.shifted(case, s)
        for un, u in moved["u"].items():
            a, b = sh.rows_c(moved["x"], case["theta"], u), sh.rows_c(moved["x"], case["theta"], u, "eq_scaled")
            np.testing.assert_array_equal(a, b)
            v, vt = float(np.exp(case["theta"][0])), float(np.exp(case["theta"][1]))
            assert ((a - sh.rows_c(case["x"], case["theta"], case["u"][un])) == 0).all()          # and the row does not move either
            assert (a[dl.QUIRK_ROW] > v + 0.5 * vt) == (un == "equal")
        raw, sc = moved["x"], sh.scaled(moved["x"], case["theta"])
        for k in range(d):
            assert len(np.unique(sc[:, k])) == len(np.unique(raw[:, k]))
