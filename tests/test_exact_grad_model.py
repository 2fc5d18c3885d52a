"""The model of the Exact moments' gradients (tests/_exact_grad_model.py) is right, the device's route is that model's arithmetic, the rule
sees the defects the route can have, and the SLSQP driver of the inverse solver converges on it.  CPU only.

  * moments_grad in long double agrees with central differences of tests/_dense_ld.exact_builtin, itself in long double.  Step and agreement
    come from the difference's own error terms: D(h) = f' + h^2 f''' / 6 + O(h^4) and a rounding error of at most eps F / h per evaluated
    value (eps = 2^-63, F the absolute scale exact_builtin returns with the value; CANCEL such values enter a difference quotient and
    each carries a few rounded operations per term).  With |f'''| <~ F / l^3 the sum of both is smallest at h* = l (3 eps)^(1/3); l is
    the shortest length on which any factor of any term varies: in u (2 max_k w_k)^-1/2 (every exponent's curvature is at most 2 W:
    D <= W, A^-1 <= 2 W), in s_k = Sigma_kk min_k (1 / (2 w_k) + s_k) (the distance to the pole of A^-1, the nearest one).  h is the
    largest power of two below h*, so that u +- h and u +- 2 h are exact in float64 (exact_builtin rounds u to float64).  The truncation
    term is MEASURED, not assumed: D(2 h) - D(h) = h^2 f''' / 2 + O(h^4), hence |D(h) - f'| = |D(2 h) - D(h)| / 3 to leading order; the
    test allows twice that plus the rounding term, and asserts that this allowance is below 1e-9 of the derivative's absolute scale, so
    that the agreement means something.  Cases: d = 1, 3, 8, a diagonal and (d >= 2) a full Sigma.
  * route (float64, the device's 2 d + 1 rows, Lo and the G / Q formulas) agrees with the long-double model under the rule of
    tests/_dense_ld.py, rho_ref from the float64 evaluation of the model's own pair sums;
  * each seeded defect of route moves some output past that bound;
  * slsqp_inverse (skgpuppy_amd.InverseUncertaintyPropagation), fed route as its value_and_grad on N = 200, d = 3, ends feasible within
    its `acc` and at a point that satisfies the first-order condition grad cost + lambda grad var = 0, lambda > 0, free and with
    coestimated = [[0, 1]].  SLSQP stops when the cost changes by less than acc; near the optimum the cost exceeds its minimum by
    1/2 r^T H^-1 r for a stationarity residual r and the Hessian H of the Lagrangian (in the log-variances), so |r| <= sqrt(2 acc lmax(H));
    H is measured by differences of the model's gradients, and the test allows twice that."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc

import _dense_ld as dl
import _exact_grad_model as eg

LD = dl.LD
EPS_LD = float(np.finfo(LD).eps)
CANCEL = 8.0            # module docstring: rounding allowance of a difference quotient, in units of eps F / h
FD_CASES = [(129, 1), (129, 3), (129, 8)]
ROUTE_CASES = [(129, 1), (200, 3), (200, 8), (200, 17)]


@functools.lru_cache(maxsize=None)
def fitted(N, d):
    x, t, theta = dl.make_case(N, d, dl.seed_of(N, d))
    Kinv = np.linalg.inv(orc.gram(x, theta))
    Kinv = (Kinv + Kinv.T) / 2
    return x, t, theta, Kinv, Kinv.dot(t)


def pow2_below(h):
    return 2.0 ** np.floor(np.log2(h))


def central(f, h):
    """(D(h), D(2 h)) of f: step -> {name: (values, scales)}, and the scales of f at the largest step, per output"""
    p1, m1, p2, m2 = f(h), f(-h), f(2 * h), f(-2 * h)
    out = {}
    for k in ("mean", "var"):
        D1 = (p1[k][0][0] - m1[k][0][0]) / LD(2 * h)
        D2 = (p2[k][0][0] - m2[k][0][0]) / LD(4 * h)
        out[k] = (D1, D2, max(float(q[k][1][0]) for q in (p1, m1, p2, m2)))
    return out


@pytest.mark.parametrize("N,d", FD_CASES)
def test_model_is_the_derivative_of_the_exact_moments(N, d):
    x, _t, theta, Kinv, alpha = fitted(N, d)
    seed = dl.seed_of(N, d)
    _v, _vt, w = dl.params(theta, d, np.float64)
    u = dl.inputs_u(x, theta, seed)["between"]
    for sn, S in dl.sigmas(d, seed).items():
        S = S.astype(LD)
        model = eg.moments_grad(x, theta, Kinv, alpha, u, S)
        hu = pow2_below((2 * w.max()) ** -0.5 * (3 * EPS_LD) ** (1.0 / 3))
        hs = pow2_below(float((1 / (2 * w) + np.diagonal(S).astype(np.float64)).min()) * (3 * EPS_LD) ** (1.0 / 3))
        worst = 0.0
        for k in range(d):
            ek = np.eye(d)[k]

            def in_u(step):
                return dl.exact_builtin(x, theta, Kinv, alpha, u + step * ek, S)

            def in_s(step):
                Sk = S.copy()
                Sk[k, k] += LD(step)
                return dl.exact_builtin(x, theta, Kinv, alpha, u, Sk)

            for f, h, names in ((in_u, hu, ("dmean_du", "dvar_du")), (in_s, hs, ("dmean_ds", "dvar_ds"))):
                D = central(f, h)
                for name, key in zip(names, ("mean", "var")):
                    D1, D2, F = D[key]
                    allow = 2 * abs(float(D2 - D1)) / 3 + CANCEL * EPS_LD * F / h
                    scale = float(model[name][1][k])
                    err = abs(float(model[name][0][k] - D1))
                    worst = max(worst, err / scale)
                    assert allow <= 1e-9 * scale, (name, k, sn, allow, scale)
                    assert err <= allow, (name, k, sn, err, allow, float(D1), float(model[name][0][k]))
        print("N=%d d=%d Sigma %s: h_u %.3e h_s %.3e, worst |model - difference| / scale %.3e" % (N, d, sn, hu, hs, worst))


def route_distances(N, d, u, S, defect=None):
    x, _t, theta, Kinv, alpha = fitted(N, d)
    want = eg.moments_grad(x, theta, Kinv, alpha, u, S)
    ref = eg.moments_grad(x, theta, Kinv, alpha, u, S, dt=np.float64)
    rho = dl.rho_of(eg.distances({k: ref[k][0] for k in eg.OUTPUTS}, want))
    got = eg.route(x, theta, Kinv, alpha, u[None, :], S, defect=defect)
    for k in eg.OUTPUTS:
        assert np.isfinite(got[k]).all(), k
    return eg.distances(got, want), rho


def cases_of(N, d):
    x, _t, theta, _K, _a = fitted(N, d)
    seed = dl.seed_of(N, d)
    for un, u in dl.inputs_u(x, theta, seed).items():
        for sn, S in dl.sigmas(d, seed).items():
            yield un, u, sn, S


@pytest.mark.parametrize("N,d", ROUTE_CASES)
def test_device_route_is_the_model(N, d):
    for un, u, sn, S in cases_of(N, d):
        dist, rho = route_distances(N, d, u, S)
        print("N=%d d=%d u %s Sigma %s: rho_ref %.3e " % (N, d, un, sn, rho) + " ".join("%s %.2e" % (k, r.max()) for k, r in dist.items()))
        dl.assert_within(dist, rho, what="route N=%d d=%d u %s Sigma %s" % (N, d, un, sn))


def flagged(dist, rho):
    return any(not np.all(r <= dl.bound(rho)) for r in dist.values())


@pytest.mark.parametrize("defect", ["no_2m", "no_nc2", "q_half", "b_W", "diag_full"])
@pytest.mark.parametrize("N,d", [(200, 3), (200, 8)])
def test_seeded_defects_are_flagged(N, d, defect):
    for un, u, sn, S in cases_of(N, d):
        if un == "far":
            continue
        dist, rho = route_distances(N, d, u, S, defect)
        print("%s N=%d d=%d u %s Sigma %s: worst %.3e against %.3e" % (defect, N, d, un, sn, max(r.max() for r in dist.values()), dl.bound(rho)))
        assert flagged(dist, rho), (un, sn)
        dl.assert_within({k: dist[k] for k in ("mean", "dmean_du", "dmean_ds")}, rho)     # no defect touches the mean's sums


# ------------------------------------------------------------------------------------------------
# the SLSQP driver on the model
# ------------------------------------------------------------------------------------------------
ACC = 1e-8
V_REF = np.array([0.30, 0.20, 0.25])        # the target output variance is the model's at these input variances: feasible by construction
COST_C, COST_I = np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 1.5])


def inverse_problem():
    x, _t, theta, Kinv, alpha = fitted(200, 3)
    u = dl.inputs_u(x, theta, dl.seed_of(200, 3))["between"]

    def value_and_grad(v):
        out = eg.route(x, theta, Kinv, alpha, u[None, :], np.diag(v))
        return out["var"][0], out["dvar_ds"][0]

    return value_and_grad, value_and_grad(V_REF)[0]


@pytest.mark.parametrize("coestimated", [[], [[0, 1]]], ids=["free", "coestimated01"])
def test_slsqp_driver_converges_on_the_model(coestimated):
    from skgpuppy_amd.InverseUncertaintyPropagation import slsqp_inverse
    vg, target = inverse_problem()
    free = [0, 2] if coestimated else [0, 1, 2]
    start = np.log(0.5 * V_REF[free])
    v, info = slsqp_inverse(vg, target, COST_C, COST_I, coestimated, start, acc=ACC)
    assert info["result"].success, info["result"].message
    assert (v > 0).all() and info["calls"] < 100
    if coestimated:
        assert v[1] == v[0] * COST_I[0] / COST_I[1]

    def reduced(vfull):
        """(cost, grad cost, var, grad var) in the free log-variances, by hand"""
        var, dv = vg(vfull)
        gc = -COST_C / vfull / COST_I
        gv = dv * vfull
        if coestimated:           # the follower 1 moves with its lead 0, and is no term of the cost (the reference deletes it)
            return (COST_C[free] / vfull[free] / COST_I[free]).sum(), gc[free], var, np.array([gv[0] + gv[1], gv[2]])
        return (COST_C / vfull / COST_I).sum(), gc, var, gv

    cost, gc, var, gv = reduced(v)
    assert target - var >= -ACC, (target, var)
    lam = -gc.dot(gv) / gv.dot(gv)
    assert lam > 0                                                  # the constraint is active: the problem is well posed
    r = gc + lam * gv

    def lagrangian_grad(xlog):
        vf = np.zeros(3)
        vf[free] = np.exp(xlog)
        if coestimated:
            vf[1] = vf[0] * COST_I[0] / COST_I[1]
        _c, a, _v, b = reduced(vf)
        return a + lam * b

    x0, step = np.log(v[free]), 1e-4
    H = np.array([(lagrangian_grad(x0 + step * e) - lagrangian_grad(x0 - step * e)) / (2 * step) for e in np.eye(len(free))])
    lmax = float(np.abs(np.linalg.eigvalsh((H + H.T) / 2)).max())
    tol = 2 * np.sqrt(2 * ACC * lmax)
    print("slsqp %s: v %s cost %.9g var - target %.3e lambda %.4g |r| %.3e tol %.3e calls %d" % (coestimated, v, cost, var - target, lam,
                                                                                              np.linalg.norm(r), tol, info["calls"]))
    assert np.linalg.norm(r) <= tol, (np.linalg.norm(r), tol)
    if not coestimated:
        assert cost <= (COST_C / V_REF / COST_I).sum() + ACC            # no worse than the feasible point the target was built from
