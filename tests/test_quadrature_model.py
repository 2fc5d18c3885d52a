"""CPU: the model of the numerical propagation (tests/_quadrature_model.py) against the genuine reference's recorded values
(tests/golden/quadrature.npz, tools/gen_quadrature_golden.py), its own consistency, and planted defects.

The model is what the device is held to in tests/test_quadrature.py: the oracle's estimate_many on the node set, and long-double sums.
Tolerances against the reference: mean 1e-12, variance 1e-11 (the reference forms E[mu^2] - m^2, whose cancellation is the limit),
density 1e-10 of its peak.  Every planted defect must leave these bounds on a case the device tests also run.
"""
import math

import numpy as np
import pytest

from conftest import load_golden

from oracle import oracle as orc

import _periodic_ld as pl
import _quadrature_model as qm

LD = qm.LD
HG_MODELS = ["n203_d3", "grid_int", "n256_d8"]
MC_MODELS = ["n203_d3", "grid_int"]
Q = load_golden("quadrature")
_OG = {}


def _oracle(name):
    if name not in _OG:
        g = load_golden(name)
        _OG[name] = (orc.OracleGP(g["x"], g["t_raw"], g["theta"]), float(np.mean(g["t_raw"])))
    return _OG[name]


def _hg_model(estimate_many, key, i, j, shift=0.0, root=None, rule=None, var_map=None, naive_var=False):
    """(mean, var, dens [9]) of the model for pair (u_i, Sigma_j) of the golden group `key`; the keyword arguments plant defects"""
    u, Sigma, order = Q[key + "u"], Q[key + "Sigma"], int(Q[key + "order"])
    z, wq = (rule or qm.hg_rule)(order, u.shape[1])
    A = (root or qm.hg_root)(Sigma[j])
    mu, var = estimate_many(qm.nodes_plain(u[i:i + 1], A, z)[0])
    if var_map:
        var = var_map(var)
    mom, _units, dens, _du = qm.mixture_ld(mu, var, wq, Q[key + "y"][i, j], shift)
    v = mom[1]
    if naive_var:
        v = mom[2] + ((LD(1) * wq * mu * mu).sum() - mom[0] ** 2)
    return float(mom[0]), float(v), np.asarray(dens, dtype=float)


def _hg_errors(estimate_many, key, **defect):
    """worst (mean, variance, density / peak) distance of the model from the golden group over all its pairs"""
    e = [0.0, 0.0, 0.0]
    nu, nS = Q[key + "mean"].shape
    for i in range(nu):
        for j in range(nS):
            m, v, dens = _hg_model(estimate_many, key, i, j, **defect)
            ref = Q[key + "dens"][i, j]
            e = [max(e[0], abs(m - Q[key + "mean"][i, j]), abs(m - Q[key + "ga"][i, j, 0])), max(e[1], abs(v - Q[key + "ga"][i, j, 1])),
                 max(e[2], float(np.max(np.abs(dens - ref)) / ref.max()))]
    return e


@pytest.mark.parametrize("name", HG_MODELS)
def test_model_matches_the_reference_hg(name):
    og, _meant = _oracle(name)
    e = _hg_errors(og.estimate_many, "hg_%s_" % name)
    print("HG %s: dmean %.2e dvar %.2e ddens/peak %.2e" % ((name,) + tuple(e)))
    assert e[0] <= 1e-12 and e[1] <= 1e-11 and e[2] <= 1e-10


def _periodic_estimate():
    x, t, theta = pl.make_case(203, 3)
    return lambda xs: qm.periodic_estimate_many(x, t, theta, xs)


def test_model_matches_the_reference_periodic():
    e = _hg_errors(_periodic_estimate(), "hgper_")
    print("HG periodic: dmean %.2e dvar %.2e ddens/peak %.2e" % tuple(e))
    assert e[0] <= 1e-12 and e[1] <= 1e-11 and e[2] <= 1e-10


@pytest.mark.parametrize("name", MC_MODELS)
def test_model_replays_the_reference_mc(name):
    """the reference's three sample sets, replayed: its three expectations and what propagate_GA returned"""
    og, _meant = _oracle(name)
    key = "mc_%s_" % name
    smp, exp, ga = Q[key + "samples"], Q[key + "exp"], Q[key + "ga"]
    n = smp.shape[1]
    wq = np.full(n, 1.0 / n)
    e0 = float((LD(1) * wq * og.estimate_many(smp[0])[0]).sum())
    e1 = float((LD(1) * wq * og.estimate_many(smp[1])[1]).sum())
    e2 = float((LD(1) * wq * og.estimate_many(smp[2])[0] ** 2).sum())
    print("MC %s: %.2e %.2e %.2e" % (name, abs(e0 - exp[0]), abs(e1 - exp[1]), abs(e2 - exp[2])))
    assert abs(e0 - exp[0]) <= 1e-12 and abs(e1 - exp[1]) <= 1e-11 and abs(e2 - exp[2]) <= 1e-11
    assert abs(e0 - ga[0]) <= 1e-12 and abs(e1 + e2 - e0 * e0 - ga[1]) <= 1e-11
    # the samples are u + root z for the reference's own (SVD-based) root: their mean and covariance are the inputs' within sampling error
    assert np.all(np.abs(smp[0].mean(0) - Q[key + "u"]) <= 5 * np.sqrt(np.diag(Q[key + "Sigma"]) / n))


def test_weights_sum_to_one():
    import skgpuppy_amd as sk
    worst = 0.0
    for order in range(1, 9):
        for d in range(1, 5):
            z, wq = qm.hg_rule(order, d)
            hg = sk.UncertaintyPropagationNumericalHG.__new__(sk.UncertaintyPropagationNumericalHG)
            hg.order = order
            z2, wq2 = hg._rule(d)
            np.testing.assert_array_equal(z, z2)          # the class and the model build the same grid, in itertools.product order
            np.testing.assert_array_equal(wq, wq2)
            worst = max(worst, abs(math.fsum(wq) - 1.0) / qm.U64)
            assert abs(math.fsum(wq) - 1.0) <= 4 * qm.U64, (order, d)
            assert z.shape == (order ** d, d) and (wq > 0).all()
    print("worst |sum wq - 1| = %.1f u" % worst)


def test_rules_and_roots_of_the_classes():
    import skgpuppy_amd as sk
    S = Q["hg_n203_d3_Sigma"][1]
    hg = sk.UncertaintyPropagationNumericalHG.__new__(sk.UncertaintyPropagationNumericalHG)
    hg.order, hg.full_sigma = 4, False
    np.testing.assert_array_equal(hg._root(S), qm.hg_root(S))
    assert np.count_nonzero(hg._root(S) - np.diag(np.diag(hg._root(S)))) == 0       # the reference's quirk: the diagonal alone
    hg.full_sigma = True
    np.testing.assert_allclose(hg._root(S).dot(hg._root(S).T), 2 * S, rtol=1e-14)
    hg.order = 5
    with pytest.raises(ValueError):
        hg._rule(10)                                                               # 5^10 > 2^22 nodes
    mc = sk.UncertaintyPropagationMC.__new__(sk.UncertaintyPropagationMC)
    mc.n, mc.seed = 50, 3
    z, wq = mc._rule(3)
    np.testing.assert_array_equal(z, qm.mc_rule(50, 3, 3)[0])
    assert np.all(wq == 1.0 / 50)
    mc.seed = None
    np.random.seed(3)
    np.testing.assert_array_equal(mc._rule(3)[0], z)                               # the global state, as the reference
    np.testing.assert_allclose(mc._root(S).dot(mc._root(S).T), S, rtol=1e-14)
    sing = np.outer([1.0, 2.0, 0.5], [1.0, 2.0, 0.5])
    np.testing.assert_allclose(mc._root(sing).dot(mc._root(sing).T), sing, atol=1e-15)


def test_nodes_fma_chain_is_the_plain_sum_to_rounding():
    rng = np.random.RandomState(5)
    U, A, z = rng.randn(2, 3), rng.randn(2, 3, 3), rng.randn(7, 3)
    X = qm.nodes_fma(U, A, z)
    np.testing.assert_allclose(X, qm.nodes_plain(U, A, z), rtol=0, atol=8 * qm.U64 * (np.abs(U).max() + 3 * np.abs(A).max() * np.abs(z).max()))
    assert qm._fma(2.0 ** 27 + 1, 2.0 ** 27 + 1, -2.0 ** 54) == 2.0 ** 28 + 1   # one rounding: the product's low bit survives


def test_rho_of_the_float64_restatement():
    """rho: the restatement's worst distance from the long-double model, in units; the device bound of gpx_mixture_reduce is
    8 max(rho, 4) units (tests/test_quadrature.py takes it from the same function)"""
    rm, rd = qm.reduce_rho()
    print("rho: moments %.2f units, density %.2f units -> device bounds %.0f and %.0f units" % (rm, rd, qm.reduce_bound_units(rm), qm.reduce_bound_units(rd)))
    assert rm <= 16 and rd <= 16            # a restatement further off than this would not be a model of the device's arithmetic


# ---- planted defects: each leaves the bounds on a case the device tests run too ------------------------------------------------------
def _outside(e):
    return e[0] > 1e-12 or e[1] > 1e-11 or e[2] > 1e-10


def test_defect_density_without_meant():
    og, meant = _oracle("n203_d3")
    e = _hg_errors(og.estimate_many, "hg_n203_d3_", shift=meant)       # the oracle's means carry meant: shifting AGAIN is a dropped meant
    assert e[2] > 1e-10 and e[0] <= 1e-12


def test_defect_sigma_for_sigma_squared():
    og, _ = _oracle("grid_int")
    e = _hg_errors(og.estimate_many, "hg_grid_int_", var_map=np.sqrt)
    assert e[1] > 1e-11 and e[2] > 1e-10 and e[0] <= 1e-12


def test_defect_missing_pi_power():
    og, _ = _oracle("n203_d3")

    def rule(order, d):
        z, wq = qm.hg_rule(order, d)
        return z, wq * np.sqrt(np.pi) ** d
    assert _outside(_hg_errors(og.estimate_many, "hg_n203_d3_", rule=rule))


def test_defect_missing_sqrt2_in_the_nodes():
    og, _ = _oracle("n256_d8")
    assert _outside(_hg_errors(og.estimate_many, "hg_n256_d8_", root=lambda S: qm.hg_root(S) / np.sqrt(2.0)))


def test_defect_off_diagonal_used_without_full_sigma():
    og, _ = _oracle("n203_d3")
    key = "hg_n203_d3_"
    m, v, dens = _hg_model(og.estimate_many, key, 0, 1, root=lambda S: qm.hg_root(S, True))
    assert abs(m - Q[key + "mean"][0, 1]) > 1e-12 or abs(v - Q[key + "ga"][0, 1, 1]) > 1e-11
    m, v, dens = _hg_model(og.estimate_many, key, 0, 0, root=lambda S: qm.hg_root(S, True))      # a diagonal Sigma: both rules agree
    assert abs(m - Q[key + "mean"][0, 0]) <= 1e-12 and abs(v - Q[key + "ga"][0, 0, 1]) <= 1e-11


def test_defect_weights_out_of_step_with_the_nodes():
    """A tensor grid of ONE one-dimensional rule is symmetric: transposing the node order against the weight order permutes the grid onto
    itself with equal weights (asserted), so that swap is no defect.  The weights one node out of step is one."""
    og, _ = _oracle("grid_int")
    z, wq = qm.hg_rule(4, 2)
    order = np.arange(16).reshape(4, 4).T.ravel()
    np.testing.assert_array_equal(wq[order], wq)
    np.testing.assert_array_equal(z[order], z[:, ::-1])

    def rule(o, d):
        z, wq = qm.hg_rule(o, d)
        return z, np.roll(wq, 1)
    assert _outside(_hg_errors(og.estimate_many, "hg_grid_int_", rule=rule))


def test_defect_naive_second_moment_on_the_offset_case():
    """E[mu^2] - m^2 in float64 in place of the central c2, on an input with a 1e6 offset of the reduce cases: far outside the device bound"""
    mu, var, wq, _y = qm.reduce_case(257, 3, 0, 1)
    i = 1
    assert mu[i].mean() > 1e5
    mom, units, _d, _du = qm.mixture_ld(mu[i], var[i], wq)
    good, _ = qm.mixture_f64(mu[i], var[i], wq)
    bound = qm.reduce_bound_units(qm.reduce_rho()[0])
    assert abs(good[1] - mom[1]) <= bound * units[1]
    m = float(np.dot(wq, mu[i]))
    naive = float(np.dot(wq, var[i])) + (float(np.dot(wq, mu[i] * mu[i])) - m * m)
    assert abs(naive - mom[1]) > bound * units[1]
