"""The factored form of the Exact double sum (tests/_exact_many_model.py: what gpx_propagate_exact_many's matrix path computes) is Girard's
double sum, and the comparison rule sees the defects the factored form can have.  CPU only.

  * on plain and sharp cases the float64 model agrees with the long-double model of the unfactored sum (tests/_dense_ld.exact_builtin)
    under the rule of tests/_dense_ld.py: distance on the sum's absolute scale within MARGIN * max(rho_ref, FLOOR), rho_ref from the float64
    evaluation of the unfactored sum.  Inputs: dl.inputs_u and dl.sigmas; the far input on plain cases only (on a sharp case the float64
    evaluation of the UNFACTORED sum overflows there, exp(+E) C_i C_j: the reference's limit, not the path's);
  * each seeded defect lands outside the bound on the case that exposes it: no_E and diag_full on a sharp case (E far from 1, a heavy
    diagonal), no_quirk on the input that equals a training point, abs_sign on a sharp case with Sigma = diag(-0.1 / w_k), where
    Ls = -w / 2 is negative definite -- after the undefected model has passed that very case.
K^-1 here is numpy's inverse of the oracle's Gram matrix (symmetrised), as in tests/test_dense_ld_model.py; on the device the tests use the
device's own."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc

import _dense_ld as dl
import _exact_many_model as em

PLAIN = [(129, 1), (200, 3), (200, 8), (200, 17), (200, 64)]
SHARP = [(200, 3), (200, 8)]
NEG_FACTOR = 0.1       # Sigma = diag(-NEG_FACTOR / w_k): W/2 + Sigma stays invertible, Ls = sym(2 W - A^-1) turns negative definite


@functools.lru_cache(maxsize=None)
def fitted(N, d, sharp=False):
    x, t, theta = dl.make_case(N, d, dl.seed_of(N, d), sharp)
    Kinv = np.linalg.inv(orc.gram(x, theta))
    Kinv = (Kinv + Kinv.T) / 2
    return x, t, theta, Kinv, Kinv.dot(t)


def negative_sigma(theta, d):
    _v, _vt, w = dl.params(theta, d, np.float64)
    return np.diag(-NEG_FACTOR / w)


def distances_of(N, d, sharp, u, S, defect=None):
    """({group: distances of the float64 factored model}, rho_ref of the float64 unfactored evaluation)"""
    x, _t, theta, Kinv, alpha = fitted(N, d, sharp)
    want = dl.exact_builtin(x, theta, Kinv, alpha, u, S)
    ref = dl.exact_builtin(x, theta, Kinv, alpha, u, S, dt=np.float64)
    rho = dl.rho_of({k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in ("mean", "var")})
    mean, var = em.moments(x, theta, Kinv, alpha, u[None, :], S, defect=defect)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    return {"mean": dl.distances(mean, want["mean"][0], want["mean"][1]), "var": dl.distances(var, want["var"][0], want["var"][1])}, rho


def cases_of(N, d, sharp):
    x, _t, theta, _K, _a = fitted(N, d, sharp)
    seed = dl.seed_of(N, d)
    for un, u in dl.inputs_u(x, theta, seed).items():
        if sharp and un == "far":
            continue
        for sn, S in dl.sigmas(d, seed).items():
            yield un, u, sn, S


@pytest.mark.parametrize("N,d,sharp", [c + (False,) for c in PLAIN] + [c + (True,) for c in SHARP])
def test_factored_form_is_the_double_sum(N, d, sharp):
    for un, u, sn, S in cases_of(N, d, sharp):
        dist, rho = distances_of(N, d, sharp, u, S)
        print("N=%d d=%d%s u %s Sigma %s: rho_ref %.3e mean %.3e var %.3e" % (N, d, " sharp" if sharp else "", un, sn, rho,
                                                                             dist["mean"].max(), dist["var"].max()))
        dl.assert_within(dist, rho, what="factored model N=%d d=%d u %s Sigma %s" % (N, d, un, sn))


def test_eigen_transform_restates_the_quadratic_form():
    rng = np.random.RandomState(5)
    for d in (1, 3, 17):
        A = rng.uniform(-1, 1, (d, d))
        M = A + A.T                                   # indefinite
        T, s = em.square_transform(M, 0.125)
        z = rng.uniform(-3, 3, (40, d))
        np.testing.assert_allclose((s * z.dot(T.T) ** 2).sum(1), 0.125 * (z.dot(M) * z).sum(1), rtol=0, atol=1e-13 * d * np.abs(M).max() * 9)


def flagged(dist, rho):
    return any(not np.all(r <= dl.bound(rho)) for r in dist.values())


@pytest.mark.parametrize("N,d", SHARP)
@pytest.mark.parametrize("defect", ["no_E", "diag_full"])
def test_defects_of_the_weight_matrix_are_flagged(defect, N, d):
    for un, u, sn, S in cases_of(N, d, True):
        dist, rho = distances_of(N, d, True, u, S, defect)
        print("%s N=%d d=%d u %s Sigma %s: var %.3e against %.3e" % (defect, N, d, un, sn, dist["var"].max(), dl.bound(rho)))
        assert flagged({"var": dist["var"]}, rho)
        dl.assert_within({"mean": dist["mean"]}, rho)         # the mean does not read the weight matrix


@pytest.mark.parametrize("N,d,sharp", [(200, 3, False), (200, 8, False), (200, 3, True)])
def test_missing_quirk_is_flagged(N, d, sharp):
    for un, u, sn, S in cases_of(N, d, sharp):
        dist, rho = distances_of(N, d, sharp, u, S, "no_quirk")
        if un == "equal":
            assert flagged(dist, rho), (sn, dist)
        else:
            dl.assert_within(dist, rho)


@pytest.mark.parametrize("N,d", SHARP)
def test_dropped_sign_is_flagged_under_a_negative_sigma(N, d):
    x, _t, theta, _K, _a = fitted(N, d, True)
    S = negative_sigma(theta, d)
    _v, _vt, w = dl.params(theta, d, np.float64)
    Ls = dl.exact_constants(w, S, np.float64)[0]
    assert (np.linalg.eigvalsh(Ls) < 0).all()
    for un, u in dl.inputs_u(x, theta, dl.seed_of(N, d)).items():
        if un == "far":
            continue
        dist, rho = distances_of(N, d, True, u, S)
        print("negative Sigma N=%d d=%d u %s: rho_ref %.3e mean %.3e var %.3e" % (N, d, un, rho, dist["mean"].max(), dist["var"].max()))
        dl.assert_within(dist, rho, what="undefected model under a negative Sigma")
        if (N, d) == SHARP[0]:       # at d = 8 the sharp points stand alone: the off-diagonal pairs, where E acts, carry 1e-17 of the sum
            bad, rho = distances_of(N, d, True, u, S, "abs_sign")
            print("abs_sign N=%d d=%d u %s: var %.3e against %.3e" % (N, d, un, bad["var"].max(), dl.bound(rho)))
            assert flagged({"var": bad["var"]}, rho), bad
