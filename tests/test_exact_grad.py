"""The closed-form gradients of the Exact moments: gpx_propagate_exact_grad_many, UncertaintyPropagationExact.propagate_GA_gradient(_many)
and InverseUncertaintyPropagationNumerical.get_best_solution(method="slsqp").

The device is held to the long-double model of the UNFACTORED pair sums (tests/_exact_grad_model.moments_grad; tests/test_exact_grad_model.py
holds that model to differences of the exact moments) evaluated on the device's own K^-1 and alpha, under the rule of tests/_dense_ld.py:
distance on each output's absolute scale within MARGIN * max(rho_ref, FLOOR), rho_ref from the float64 evaluation of the same sums.  Shapes
are the smallest that cross each seam: N = 129 (127 padded columns), 200, 700 (npad 768: 12 column tiles, 68 padded); d = 1, 3, 8, 9, 17
(rows per input 3 .. 35, inputs per workgroup row 16) and 64 at N = 200 (129 rows: more than one 128-row tile per input, 64 KB of LDS);
b = 1, 5, 130; GPX_EXACT_MANY_SLAB=128 cuts a batch into several slabs of whole inputs and is itself smaller than one input at d = 64.
Where two device calls are compared (the new call's mean and var with gpx_propagate_exact_many's), each is held to the bound, so they may
differ by twice it: 2 * MARGIN * FLOOR on the float64 evaluation's scale (test_exact_many.TWO_PATHS)."""
import os

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _dense_ld as dl
import _exact_grad_model as eg
from test_dense_bounds import fit
from test_exact_many import FILL, GPX_K_EXACT, GPX_K_GEMM, GPX_K_GEMM_SMALL, TWO_PATHS, _launches, env, raw_many, seeded

HERE = os.path.dirname(os.path.abspath(__file__))
GRADS = eg.OUTPUTS[2:]
FAR_TINY = 1e-100          # the far input: C_i <= v e^-300 (dl.FAR_Q), every term of every gradient is below 1e-120 times a power of N


def raw_grad(h, U, S, want=eg.OUTPUTS, status=False):
    """gpx_propagate_exact_grad_many itself: {name: array} for the outputs in want (the others are passed as NULL); arrays enter holding FILL"""
    U, S = _gpx.f64(U), _gpx.f64(S)
    b, d = U.shape
    out = {k: np.full(b if k in ("mean", "var") else (b, d), FILL) for k in want}
    st = _gpx.lib.gpx_propagate_exact_grad_many(h, _gpx.ptr(U), _gpx.ptr(S), int(S.ndim == 2), b,
                                                *[_gpx.ptr(out[k]) if k in out else None for k in eg.OUTPUTS])
    if status:
        return st, out
    _gpx.check(st, "gpx_propagate_exact_grad_many")
    return out


def against_model(title, f, got, i, u, S, cache=None, key=None, quirk=True, args=None):
    """input i of the outputs in got against the model at (u, S) under the rule; each comparison is recorded"""
    args = f.args if args is None else args
    if cache is not None and key in cache:
        want, ref = cache[key]
    else:
        want, ref = (eg.moments_grad(*args, u, S, dt=dt, quirk=quirk) for dt in (dl.LD, np.float64))
        if cache is not None:
            cache[key] = (want, ref)
    ref_dist = eg.distances({k: ref[k][0] for k in got}, want)
    rho = dl.rho_of(ref_dist)
    mine = {k: np.ravel(g[i]) for k, g in got.items()}
    for k, g in mine.items():
        assert np.isfinite(g).all(), (title, k, g)
    dist = eg.distances(mine, want)
    name = f if isinstance(f, str) else f.name
    dl.record("%s input %d" % (title, i), name, rho, dist, ref_dist)
    dl.assert_within(dist, rho, what="%s input %d %s" % (title, i, name))


def test_symbol_methods_and_abi_version():
    assert "gpx_propagate_exact_grad_many" in _gpx.SIGNATURES and hasattr(_gpx.lib, "gpx_propagate_exact_grad_many")
    assert callable(getattr(sk.UncertaintyPropagationExact, "propagate_GA_gradient_many"))
    assert callable(getattr(sk.UncertaintyPropagationExact, "propagate_GA_gradient"))
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpx.h")).read()
    assert "int gpx_propagate_exact_grad_many(" in header and "InverseUncertaintyPropagation.py:103-104" in header
    assert _gpx.lib.gpx_abi_version() == 1      # additive
    U, S = np.zeros((3, 2)), np.eye(2)
    st, out = raw_grad(None, U, S, status=True)
    assert st == _gpx.GPX_ERR_BAD_ARG and "null handle" in _gpx.last_error()
    for o in out.values():
        assert (o == FILL).all()


CASES = [(N, d) for N in (129, 200, 700) for d in (1, 3, 8, 9, 17)] + [(200, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,d", CASES, ids=["n%d_d%d" % c for c in CASES])
def test_rule_against_the_long_double_model(N, d):
    """one shared Sigma (full; diagonal at d = 1), b = 5 = [between, equal, far, two seeded] and b = 1; under GPX_EXACT_MANY_SLAB=128 as well,
    which at d >= 9 holds fewer than five inputs (several slabs) and at d = 64 less than one (raised to one input per slab).  The far input:
    every output finite, every gradient tiny."""
    with fit(N, d) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        U = np.array([ins["between"], ins["equal"], ins["far"]] + seeded(f, 2, 23))
        sig = dl.sigmas(d, f.seed)
        S = sig["full" if d >= 2 else "diag"]
        cache = {}
        pick = (0, 1) if N == 700 and d >= 9 else (0, 1, 3)          # the model's cost grows as N^2 d
        many = raw_grad(f.h, U, S)
        with env(GPX_EXACT_MANY_SLAB=128):
            slabs = raw_grad(f.h, U, S)
        for title, got in (("grad b=5", many), ("grad b=5 slab 128", slabs)):
            for i in pick:
                against_model(title, f, got, i, U[i], S, cache, i)
            for k in eg.OUTPUTS:
                assert np.isfinite(got[k]).all(), (title, k)
            for k in GRADS:
                assert np.abs(got[k][2]).max() < FAR_TINY, (title, k, got[k][2])
        one = raw_grad(f.h, U[1:2], S)
        against_model("grad b=1", f, one, 0, U[1], S, cache, 1)
        # mean and var are the batched Exact call's
        mean, var = raw_many(f.h, U, S)
        for i in pick:
            scale = dl.exact_builtin(*f.args, U[i], S, dt=np.float64)
            assert dl.distances(many["mean"][i], mean[i], scale["mean"][1]).max() <= TWO_PATHS
            assert dl.distances(many["var"][i], var[i], scale["var"][1]).max() <= TWO_PATHS


@pytest.mark.gpu
def test_larger_batch_in_slabs_of_whole_inputs():
    """b = 130 at N = 700, d = 8 under GPX_EXACT_MANY_SLAB=128: 17 rows per input, 7 inputs per slab, 19 slabs, the last of 4 inputs.  The
    inputs either side of slab seams and the ends against the model; every input finite and, in mean and var, the batched Exact call's."""
    with fit(700, 8) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        U = np.array([ins["between"], ins["equal"], ins["far"]] + seeded(f, 127, 31))
        S = dl.sigmas(8, f.seed)["full"]
        _gpx.check(_gpx.lib.gpx_profile_enable(f.h, 2), "gpx_profile_enable")
        _gpx.check(_gpx.lib.gpx_profile_reset(f.h), "gpx_profile_reset")
        with env(GPX_EXACT_MANY_SLAB=128):
            got = raw_grad(f.h, U, S)
        assert _launches(f.h, GPX_K_EXACT) == 1 + 2 * 19             # the weight pass once, build and finish per slab
        _gpx.check(_gpx.lib.gpx_profile_enable(f.h, 0), "gpx_profile_enable")
        for k in eg.OUTPUTS:
            assert np.isfinite(got[k]).all(), k
        for i in (0, 6, 7, 129):
            against_model("grad b=130 slab 128", f, got, i, U[i], S)
        whole = raw_grad(f.h, U, S)                                     # the default slab: one product of 130 * 17 rows
        against_model("grad b=130", f, whole, 7, U[7], S)
        mean, var = raw_many(f.h, U, S)
        for i in (0, 1, 6, 7, 77, 129):
            scale = dl.exact_builtin(*f.args, U[i], S, dt=np.float64)
            for g in (got, whole):
                assert dl.distances(g["mean"][i], mean[i], scale["mean"][1]).max() <= TWO_PATHS
                assert dl.distances(g["var"][i], var[i], scale["var"][1]).max() <= TWO_PATHS


@pytest.mark.gpu
def test_per_input_sigma_in_runs_of_one_two_and_six():
    """per-input Sigma in runs [S0 x 1, S1 x 2, S2 x 6] at N = 200, d = 3: every run takes the matrix path; every input under the rule.  The
    same batch with one run's Sigma repeated for all gives the bits of the shared form."""
    with fit(200, 3) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        U = np.array([ins["between"], ins["equal"]] + seeded(f, 7, 43))
        sig = dl.sigmas(3, f.seed)
        Ss = [sig["diag"], sig["full"], 0.5 * sig["full"]]
        which = [0] + [1] * 2 + [2] * 6
        S = np.array([Ss[k] for k in which])
        got = raw_grad(f.h, U, S)
        for i in range(9):
            against_model("grad runs 1+2+6", f, got, i, U[i], S[i])
        shared = raw_grad(f.h, U, Ss[1])
        rep = raw_grad(f.h, U, np.repeat(Ss[1][None], 9, 0))
        rev = raw_grad(f.h, U[::-1], Ss[1])
        for k in eg.OUTPUTS:
            np.testing.assert_array_equal(shared[k], rep[k])
            np.testing.assert_array_equal(shared[k], rev[k][::-1])


@pytest.mark.gpu
def test_null_subsets_and_the_means_only_call_leaves_kinv_unbuilt():
    x, t, theta = dl.make_case(200, 3, 707)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    h = gp._dev().handle
    U = dl._grid(np.random.RandomState(3).uniform(2, 8, (5, 3)))
    S = dl.sigmas(3, 5)["full"]
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 2), "gpx_profile_enable")
    _gpx.check(_gpx.lib.gpx_profile_reset(h), "gpx_profile_reset")
    means = raw_grad(h, U, S, want=("mean", "dmean_du", "dmean_ds"))
    assert _launches(h, GPX_K_EXACT) == 0 and _launches(h, GPX_K_GEMM) == 0 and _launches(h, GPX_K_GEMM_SMALL) == 0
    assert gp._Kinv is None
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 0), "gpx_profile_enable")
    full = raw_grad(h, U, S)
    for k, g in means.items():
        np.testing.assert_array_equal(g, full[k])
    for want in (("dvar_ds",), ("dmean_du",), ("var", "dvar_du"), ("mean", "var", "dmean_ds", "dvar_ds"), GRADS):
        part = raw_grad(h, U, S, want=want)
        for k in want:
            np.testing.assert_array_equal(part[k], full[k], err_msg=str(want) + " " + k)
    # no gradient asked for, a null U or Sigma, a negative b: refused with nothing written; b = 0 is a no-op
    st, out = raw_grad(h, U, S, want=("mean", "var"), status=True)
    assert st == _gpx.GPX_ERR_BAD_ARG and (out["mean"] == FILL).all() and (out["var"] == FILL).all()
    o = np.full((5, 3), FILL)
    for args in ((None, _gpx.ptr(S), 1, 5), (_gpx.ptr(U), None, 1, 5), (_gpx.ptr(U), _gpx.ptr(S), 1, -1)):
        assert _gpx.lib.gpx_propagate_exact_grad_many(h, *args, None, None, _gpx.ptr(o), None, None, None) == _gpx.GPX_ERR_BAD_ARG
    assert (o == FILL).all()
    assert _gpx.lib.gpx_propagate_exact_grad_many(h, None, None, 1, 0, None, None, None, None, None, None) == 0
    st, out = raw_grad(h, U, np.full((3, 3), 1e300), status=True)
    assert st == _gpx.GPX_ERR_BAD_ARG and "singular" in _gpx.last_error() and all((a == FILL).all() for a in out.values())
    # the Python methods are the C call
    up = sk.UncertaintyPropagationExact(gp)
    py = up.propagate_GA_gradient_many(U, S)
    np.testing.assert_array_equal(py[0], full["mean"] + gp.meant)
    for a, k in zip(py[1:], eg.OUTPUTS[1:]):
        np.testing.assert_array_equal(a, full[k])
    single = up.propagate_GA_gradient(U[2], S)
    alone = raw_grad(h, U[2:3], S)
    assert single[0] == alone["mean"][0] + gp.meant and single[1] == alone["var"][0]
    for a, k in zip(single[2:], GRADS):
        assert a.shape == (3,)
        np.testing.assert_array_equal(a, alone[k][0])
    for name in ("Winv", "Sigma_x", "Deltainv", "LambdaInv", "normalize_C_corr", "normalize_C_corr2"):
        assert not hasattr(up, name), name
    with pytest.raises(ValueError):
        up.propagate_GA_gradient_many(np.zeros(3), S)


@pytest.mark.gpu
def test_pseudo_handle():
    """a pseudo-input model (GaussianProcess.pseudo_gp()): the same call on (xbar, beta, P), no vt on exact equality"""
    from test_spgp_pseudo import case
    c = case("A")
    U = c.U[:3]
    got = raw_grad(c.h, U, c.S)
    for i in range(3):
        against_model("grad pseudo", "model " + c.name, got, i, U[i], c.S, quirk=False, args=(c.xb, c.th_gc, c.P, c.beta))
    py = sk.UncertaintyPropagationExact(c.pgp).propagate_GA_gradient_many(U, c.S)
    np.testing.assert_array_equal(py[0], got["mean"] + c.pgp._get_mean_t())
    for a, k in zip(py[1:], eg.OUTPUTS[1:]):
        np.testing.assert_array_equal(a, got[k])


@pytest.mark.gpu
def test_difference_route_on_a_matern_gp():
    """an unfused route takes central differences through propagate_GA_many: the same differences taken by hand, to the last bit"""
    x, t, theta = dl.make_case(129, 2, 911)
    gp = sk.GaussianProcess(x, t, sk.MaternCovariance(2.5), theta.copy())
    assert gp._route() != "gaussian"
    up = sk.UncertaintyPropagationExact(gp)
    U = dl._grid(np.random.RandomState(9).uniform(3, 7, (2, 2)))
    S = np.array([np.diag([0.05, 0.1]), np.array([[0.2, 0.02], [0.02, 0.0]])])
    h = 2.0 ** -14
    mean, var, dmu, dvu, dmv, dvv = up.propagate_GA_gradient_many(U, S, h=h)
    for i in range(2):
        one = sk.UncertaintyPropagationExact(gp)
        m0, v0 = one.propagate_GA(U[i], S[i])
        assert (mean[i], var[i]) == (m0, v0)
        for k in range(2):
            e = h * np.eye(2)[k]
            (mp, vp), (mm, vm) = one.propagate_GA(U[i] + e, S[i]), one.propagate_GA(U[i] - e, S[i])
            assert dmu[i, k] == (mp - mm) / (2.0 * h) and dvu[i, k] == (vp - vm) / (2.0 * h)
            step = h * S[i][k, k] if S[i][k, k] != 0 else h
            Sp, Sm = S[i].copy(), S[i].copy()
            Sp[k, k] += step
            Sm[k, k] -= step
            (mp, vp), (mm, vm) = one.propagate_GA(U[i], Sp), one.propagate_GA(U[i], Sm)
            assert dmv[i, k] == (mp - mm) / (2.0 * step) and dvv[i, k] == (vp - vm) / (2.0 * step)
    assert not hasattr(up, "Winv") and not hasattr(up, "Sigma_x")
    s1 = up.propagate_GA_gradient(U[0], S[0], h=h)
    assert s1[0] == mean[0] and s1[1] == var[0] and (s1[5] == dvv[0]).all()


@pytest.mark.gpu
def test_slsqp_inverse_solver_against_cobyla():
    """N = 200, d = 3, both methods started at the log of InverseUncertaintyPropagationApprox's solution: SLSQP ends feasible within its acc
    (1e-8, slsqp_inverse's default) and at a cost no more than 1 + 1e-3 times COBYLA's (rhoend 1e-4 in log-variance, fmin_cobyla's default)."""
    x, t, theta = dl.make_case(200, 3, dl.seed_of(200, 3))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    u = dl.inputs_u(x, theta, dl.seed_of(200, 3))["between"]
    c, I = np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 1.5])
    up = sk.UncertaintyPropagationExact(gp)
    target = up.propagate_GA(u, np.diag([0.30, 0.20, 0.25]))[1]
    start = np.log(sk.InverseUncertaintyPropagationApprox(target, gp, u, c, I).get_best_solution())
    inv = sk.InverseUncertaintyPropagationNumerical(target, gp, u, c, I, upga_class=sk.UncertaintyPropagationExact)
    v_cob = inv.get_best_solution(start.copy())
    v_sl = inv.get_best_solution(start.copy(), method="slsqp")
    cost = lambda v: float(np.sum(c / v / I))      # noqa: E731
    var_sl = up.propagate_GA(u, np.diag(v_sl))[1]
    print("slsqp v %s cost %.9g var - target %.3e calls %d | cobyla v %s cost %.9g var - target %.3e"
          % (v_sl, cost(v_sl), var_sl - target, inv.slsqp_info["calls"], v_cob, cost(v_cob), up.propagate_GA(u, np.diag(v_cob))[1] - target))
    assert (v_sl > 0).all() and inv.slsqp_info["result"].success
    assert target - var_sl >= -1e-8
    assert cost(v_sl) <= (1 + 1e-3) * cost(v_cob)
    with pytest.raises(TypeError):
        sk.InverseUncertaintyPropagationNumerical(target, gp, u, c, I, upga_class=sk.UncertaintyPropagationApprox).get_best_solution(method="slsqp")
    with pytest.raises(ValueError):
        inv.get_best_solution(method="newton")
