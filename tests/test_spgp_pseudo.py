"""GaussianProcess.pseudo_gp() on the device: the pseudo-input model handle (gpx_spgp_pseudo_handle) and everything served on it.

Models and batches: tests/_spgp_pseudo.py (A: N = 700, d = 3, m = 150, two ragged 128-tiles; B: N = 300, d = 2, m = 30, one tile; C: N = 400,
d = 9, m = 130, the d > 8 instantiations, m just over one tile; b = 1 and b = 77; a shared full Sigma and per-input runs of 7 equal + 3 distinct).

1. contents     beta and P fetched by gpx_alpha / gpx_kinv, k built in NumPy: k.beta + meant and v + vt - k^T P k are the parent's estimate_many
                within 2e-5 / 2e-6 v (the bars of test_spgp_vs_oracle_ragged_and_large_m); P is symmetric to the bit.  The padding of P is not
                reachable through the interface (gpx_kinv copies n x n): it enters every product against zeros, so a non-finite entry there
                would show as a non-finite result in 2.; its being zero is stated in spgp_pseudo_p_kernel.
2. sums         every served call against the long-double models of tests/_dense_ld.py / _predict_grad_model.py evaluated on the DEVICE's
                own P and beta, quirk off, by the project's rule (distance on the scale of the absolute terms, bound MARGIN max(rho_ref, FLOOR),
                rho_ref from the float64 evaluation of the same case): Exact single / many, Approx single / many, gpx_predict_mean_grad,
                gpx_predict_grad, Linear through the class.
3. oracle       oracle.exact_propagate / approx_parts on a shim of the fetched P and beta within 1e-6 v (the bar of test_spgp_golden).
4. no quirk     u bit-equal to pseudo-input 0: gpx_cjh's C_0 is v, not v + vt, and Exact / Approx match the quirk-free model.
5. invariance   input i of the b = 77 batch is the b = 1 call bit for bit (approx_many, predict_grad in their K^-1 form); per-input and shared
                Sigma agree bit for bit when the per-input ones are all equal.
6. lifetime     the pseudo GP answers after cov.clear_cache() and after the parent's device model is closed; a pickle round trip works.
7. refusals     every other entry point returns GPX_ERR_STATE naming the pseudo-input model; pseudo_gp() needs the SPGP route; HG / MC refuse.
8. unchanged    UncertaintyPropagationExact(gp_spgp) gives the same bits before and after pseudo_gp(); estimate_many_gradient on the SPGP GP
                is still its central-difference definition.
9. seam         the K^-1 form of the batched calls' chunk loop across one chunk boundary (model D: m = 100, d = 8): the inputs on both sides
                of the seam, the first and the last are the b = 1 call bit for bit.

With GPX_DENSE_BOUNDS_RECORD=<file> every comparison of 2. appends its rho_ref, bound and worst ratios (profiles/r23_spgp_pseudo.txt)."""
import ctypes
import pickle

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from oracle import oracle as orc

import _dense_ld as dl
import _predict_grad_model as pg
import _spgp_pseudo as sp
from _periodic_ld import gram_bound

pytestmark = pytest.mark.gpu

GPX_ERR_STATE = -4
NAMES = ["A", "B", "C"]


class Case(object):
    def __init__(self, name):
        self.name = name
        self.N, self.d, self.m = sp.MODELS[name]
        self.x, self.t, self.th, self.th_gc, self.xb = sp.make_model(name)
        self.gp = sk.GaussianProcess(self.x, self.t, sk.SPGPCovariance(self.m), self.th.copy())
        self.pgp = self.gp.pseudo_gp()
        self.h = self.pgp._dev().handle
        self.P = self.pgp.Kinv
        self.beta = self.pgp._get_beta()
        self.v, self.vt = float(np.exp(self.th_gc[0])), float(np.exp(self.th_gc[1]))
        self.meant = float(self.gp.meant)
        self.S = sp.full_sigma(self.d, 20 + self.d)
        self.U = sp.inputs(name, sp.NQ)
        self.Sruns = sp.sigma_runs(self.d, sp.NQ)
        self._ld = {}

    def ld(self, key, fn):
        """(long double, float64) evaluations, computed once and shared"""
        if key not in self._ld:
            self._ld[key] = (fn(np.longdouble), fn(np.float64))
        return self._ld[key]

    def exact_ld(self, key, U, Sig):
        """{"mean": (values [b], scales), "var": ...} x (long double, float64); Sig (d, d) or (b, d, d)"""
        def run(dt):
            rows = [dl.exact_builtin(self.xb, self.th_gc, self.P, self.beta, U[i], Sig if Sig.ndim == 2 else Sig[i], dt=dt, defect="quirk")
                    for i in range(len(U))]
            return {k: tuple(np.concatenate([r[k][j] for r in rows]) for j in (0, 1)) for k in ("mean", "var")}
        return self.ld(key, run)

    def approx_ld(self, key, U, Sig):
        def run(dt):
            rows = [dl.approx_partials(self.xb, self.th_gc, self.P, self.beta, U[i], Sig if Sig.ndim == 2 else Sig[i], dt=dt, defect="quirk")
                    for i in range(len(U))]
            return {k: tuple(np.concatenate([r[k][j] for r in rows]) for j in (0, 1)) for k in ("mean", "var", "sigma2", "rest")}
        return self.ld(key, run)

    def grad_ld(self, key, U):
        def run(dt):
            out = dict(pg.mean_grad(self.xb, self.th_gc, self.beta, U, 0, dt=dt))
            out.update(pg.var_grad(self.xb, self.th_gc, self.P, U, 0, dt=dt))
            return out
        return self.ld(key, run)


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def check(title, name, got, models):
    """got {group: values} against the long-double model under the bound of the float64 evaluation of the same sums"""
    want, ref = models
    ref_dist = {k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in got}
    rho = dl.rho_of(ref_dist)
    for k, g in got.items():
        assert np.all(np.isfinite(g)), (title, name, k)
    dist = {k: dl.distances(g, want[k][0], want[k][1]) for k, g in got.items()}
    dl.record(title, "model " + name, rho, dist, ref_dist)
    return dl.assert_within(dist, rho, what=title + " model " + name)


def take(models, idx):
    """the rows idx of a pair of model evaluations"""
    return tuple({k: (v[0][idx], v[1][idx]) for k, v in m.items()} for m in models)


def approx_many(h, U, S):
    U, S = _gpx.f64(U), _gpx.f64(S)
    out = [np.empty(len(U)) for _ in range(4)]
    _gpx.check(_gpx.lib.gpx_propagate_approx_many(h, _gpx.ptr(U), _gpx.ptr(S), int(S.ndim == 2), len(U), *[_gpx.ptr(o) for o in out]),
               "gpx_propagate_approx_many")
    return dict(zip(("mean", "var", "sigma2", "rest"), out))


def exact_many(h, U, S):
    U, S = _gpx.f64(U), _gpx.f64(S)
    mean, var = np.empty(len(U)), np.empty(len(U))
    _gpx.check(_gpx.lib.gpx_propagate_exact_many(h, _gpx.ptr(U), _gpx.ptr(S), int(S.ndim == 2), len(U), _gpx.ptr(mean), _gpx.ptr(var)),
               "gpx_propagate_exact_many")
    return {"mean": mean, "var": var}


def predict_grad(h, U):
    U = _gpx.f64(U)
    m, d = U.shape
    mean, var, dm, dv = np.empty(m), np.empty(m), np.empty((m, d)), np.empty((m, d))
    _gpx.check(_gpx.lib.gpx_predict_grad(h, _gpx.ptr(U), m, _gpx.ptr(mean), _gpx.ptr(var), _gpx.ptr(dm), _gpx.ptr(dv)), "gpx_predict_grad")
    return {"mean": mean, "var": var, "dmean": dm, "dvar": dv}


# ------------------------------------------------------------------------------------------------
# 1. contents
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_contents(name):
    c = case(name)
    assert c.P.shape == (c.m, c.m) and c.beta.shape == (c.m,) and c.pgp.n == c.m and c.pgp.d == c.d
    assert np.array_equal(c.P, c.P.T), "P is not symmetric to the bit"
    assert np.all(np.isfinite(c.P)) and np.all(np.isfinite(c.beta))
    np.testing.assert_array_equal(c.pgp.x, c.xb)
    np.testing.assert_array_equal(c.pgp.theta_min, c.th_gc)
    xs = np.random.RandomState(31 + c.d).uniform(0, 10, (sp.NQ, c.d))
    mu, var = sp.predictor(xs, c.th_gc, c.xb, c.beta, c.P, c.meant)
    pmu, pvar = c.gp.estimate_many(xs)
    dm, dv = np.abs(mu - pmu).max(), np.abs(var - pvar).max()
    print("contents model %s: worst |mean - estimate_many| %.3e (bar 2e-5), worst |var - estimate_many| %.3e (bar %.1e), max|P| %.4g" %
          (name, dm, dv, 2e-6 * c.v, np.abs(c.P).max()))
    assert dm <= 2e-5 and dv <= 2e-6 * c.v
    # the same rows through the other accessor
    rows = c.pgp._dev().kinv_rows(0, c.m)
    np.testing.assert_array_equal(rows, c.P)
    # estimate / estimate_many / __call__ are the parent's, bit for bit
    np.testing.assert_array_equal(c.pgp.estimate_many(xs[:5])[0], pmu[:5])
    assert c.pgp(xs[0]) == c.gp(xs[0]) and c.pgp.estimate(xs[0]) == c.gp.estimate(xs[0])


# ------------------------------------------------------------------------------------------------
# 2. sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_exact_sums(name):
    c = case(name)
    shared = c.exact_ld("exact_shared", c.U, c.S)
    runs = c.exact_ld("exact_runs", c.U, c.Sruns)
    up = sk.UncertaintyPropagationExact(c.pgp)
    for i in range(3):                                   # single: the class on gpx_propagate_exact / gpx_exact_mean
        mean, var = up.propagate_GA(c.U[i], c.S)
        check("exact single %d" % i, name, {"mean": np.array([mean - c.meant]), "var": np.array([var])}, take(shared, [i]))
        check("exact mean single %d" % i, name, {"mean": np.array([up.propagate_mean(c.U[i], c.S)])}, take(shared, [i]))
    check("exact many b=1 shared", name, exact_many(c.h, c.U[:1], c.S), take(shared, [0]))
    check("exact many b=77 shared", name, exact_many(c.h, c.U, c.S), shared)
    check("exact many b=77 runs 7+3", name, exact_many(c.h, c.U, c.Sruns), runs)
    mean, var = up.propagate_GA_many(c.U, c.S)
    check("exact class many", name, {"mean": mean - c.meant, "var": var}, shared)


@pytest.mark.parametrize("name", NAMES)
def test_approx_sums(name):
    c = case(name)
    shared = c.approx_ld("approx_shared", c.U, c.S)
    runs = c.approx_ld("approx_runs", c.U, c.Sruns)
    up = sk.UncertaintyPropagationApprox(c.pgp)
    for i in range(3):                                   # single: gpx_propagate_approx (launch_kinv_pass on the resident P)
        mean, var, s2, rest = up._parts(c.U[i], c.S)
        check("approx single %d" % i, name, {"mean": np.array([mean]), "var": np.array([var]), "sigma2": np.array([s2]), "rest": np.array([rest])},
              take(shared, [i]))
    check("approx many b=1 shared", name, approx_many(c.h, c.U[:1], c.S), take(shared, [0]))
    check("approx many b=77 shared", name, approx_many(c.h, c.U, c.S), shared)
    check("approx many b=77 runs 7+3", name, approx_many(c.h, c.U, c.Sruns), runs)
    mean, var = up.propagate_GA_many(c.U, c.S)
    check("approx class many", name, {"mean": mean - c.meant, "var": var}, shared)


@pytest.mark.parametrize("name", NAMES)
def test_gradient_sums(name):
    c = case(name)
    models = c.grad_ld("grad", c.U)
    for b in (1, sp.NQ):
        U = _gpx.f64(c.U[:b])
        mean, g = np.empty(b), np.empty((b, c.d))
        _gpx.check(_gpx.lib.gpx_predict_mean_grad(c.h, _gpx.ptr(U), b, _gpx.ptr(mean), _gpx.ptr(g)), "gpx_predict_mean_grad")
        check("mean_grad b=%d" % b, name, {"mean": mean, "dmean": g}, take(models, slice(0, b)))
        check("predict_grad b=%d (K^-1 form)" % b, name, predict_grad(c.h, U), take(models, slice(0, b)))
    # the classes: estimate_many_gradient and Linear
    mean, var, dm, dv = c.pgp.estimate_many_gradient(c.U)
    check("estimate_many_gradient", name, {"mean": mean - c.meant, "var": var, "dmean": dm, "dvar": dv}, models)
    lin = sk.UncertaintyPropagationLinear(c.pgp)
    lm, lg = lin._mean_grad(c.U)
    check("linear mean / gradient", name, {"mean": lm, "dmean": lg}, models)
    gm, gv = lin.propagate_GA_many(c.U, c.S)
    want = np.zeros(len(c.U))
    for k in range(c.d):
        want = want + lg[:, k] ** 2 * c.S[k, k]
    np.testing.assert_array_equal(gm, lm + c.meant)
    np.testing.assert_array_equal(gv, want + c.vt)
    one = lin.propagate_GA(c.U[3], c.S)
    assert one[0] == gm[3] and one[1] == gv[3]


# ------------------------------------------------------------------------------------------------
# 3. parity with the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_parity(name):
    c = case(name)
    shim = sp.Shim(c.th_gc, c.xb, c.beta, c.P, c.meant)
    ex, ap = sk.UncertaintyPropagationExact(c.pgp), sk.UncertaintyPropagationApprox(c.pgp)
    bar = 1e-6 * c.v
    for i in range(3):
        u = c.U[i]
        om, ov = orc.exact_propagate(shim, u, c.S)
        gm, gv = ex.propagate_GA(u, c.S)
        am, as2, arest = orc.approx_parts(shim, u, c.S)
        pm, pv = ap.propagate_GA(u, c.S)
        print("oracle parity model %s input %d: exact %.3e %.3e approx %.3e %.3e (bar %.1e)" %
              (name, i, abs(gm - om), abs(gv - ov), abs(pm - am - c.meant), abs(pv - as2 - arest), bar))
        assert abs(gm - om) <= bar and abs(gv - ov) <= bar
        assert abs(pm - (am + c.meant)) <= bar and abs(pv - (as2 + arest)) <= bar


# ------------------------------------------------------------------------------------------------
# 4. no equality quirk
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_no_equality_quirk(name):
    c = case(name)
    u = c.xb[0].copy()
    C, J, H = np.empty(c.m), np.empty((c.m, c.d)), np.empty((c.m, c.d, c.d))
    _gpx.check(_gpx.lib.gpx_cjh(c.h, _gpx.ptr(u), _gpx.ptr(C), _gpx.ptr(J), _gpx.ptr(H)), "gpx_cjh")
    Cm, Jm, Hm, q, Habs = dl.cjh(c.xb, c.th_gc, u)
    assert q[0] == 0 and float(Cm[0]) == pytest.approx(c.v + c.vt)           # the dense model's row WITH the quirk
    assert abs(C[0] - c.v) <= 4 * 2.0 ** -53 * c.v                            # the device's: the plain kernel
    # every entry by the rule for rows of tests/_rows_ld.py: units of u c (1 + q), bound gram_bound(rho of the float64 evaluation)
    e0 = (np.arange(c.m) == 0)
    plain = Cm - np.longdouble(c.vt) * e0
    unit = np.longdouble(2.0 ** -53) * plain * (1 + q)
    rho = float(np.max(np.abs(dl.cjh(c.xb, c.th_gc, u, dt=np.float64)[0] - c.vt * e0 - plain) / unit))
    worst = float(np.max(np.abs(C - plain) / unit))
    print("cjh C at a pseudo-input, model %s: worst %.3f units, float64 %.3f, bound %.1f" % (name, worst, rho, gram_bound(rho)))
    assert worst <= gram_bound(rho)
    assert np.all(J[0] == 0)
    U = u[None, :]
    check("exact at a pseudo-input", name, exact_many(c.h, U, c.S), c.exact_ld("exact_eq", U, c.S))
    mean, var = sk.UncertaintyPropagationExact(c.pgp).propagate_GA(u, c.S)
    check("exact single at a pseudo-input", name, {"mean": np.array([mean - c.meant]), "var": np.array([var])}, c.exact_ld("exact_eq", U, c.S))
    check("approx many at a pseudo-input", name, approx_many(c.h, U, c.S), c.approx_ld("approx_eq", U, c.S))
    p = sk.UncertaintyPropagationApprox(c.pgp)._parts(u, c.S)
    check("approx single at a pseudo-input", name, dict(zip(("mean", "var", "sigma2", "rest"), [np.array([o]) for o in p])),
          c.approx_ld("approx_eq", U, c.S))
    check("predict_grad at a pseudo-input", name, predict_grad(c.h, U), c.grad_ld("grad_eq", U))
    # the model WITH the quirk is far outside the bound: the comparison above can tell
    quirk = dl.exact_builtin(c.xb, c.th_gc, c.P, c.beta, u, c.S)
    assert abs(float(quirk["mean"][0][0]) - (mean - c.meant)) > 1e-6 * abs(c.beta[0])


# ------------------------------------------------------------------------------------------------
# 5. batch invariance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_batch_invariance(name):
    c = case(name)
    am, gm = approx_many(c.h, c.U, c.S), predict_grad(c.h, c.U)
    for i in (0, 1, 38, sp.NQ - 1):
        a1, g1 = approx_many(c.h, c.U[i:i + 1], c.S), predict_grad(c.h, c.U[i:i + 1])
        for k in am:
            assert a1[k][0] == am[k][i], ("approx_many", k, i)
        for k in gm:
            np.testing.assert_array_equal(g1[k][0], gm[k][i], err_msg="predict_grad %s %d" % (k, i))
    same = np.broadcast_to(c.S, (sp.NQ, c.d, c.d)).copy()
    ap = approx_many(c.h, c.U, same)
    for k in am:
        np.testing.assert_array_equal(ap[k], am[k], err_msg="approx_many per-input Sigma " + k)
    es, ep = exact_many(c.h, c.U, c.S), exact_many(c.h, c.U, same)
    for k in es:
        np.testing.assert_array_equal(ep[k], es[k], err_msg="exact_many per-input Sigma " + k)


# ------------------------------------------------------------------------------------------------
# 6. lifetime, pickling, the inverse propagation
# ------------------------------------------------------------------------------------------------
def test_lifetime_and_pickle():
    x, t, th, th_gc, xb = sp.make_model("B")
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(sp.MODELS["B"][2]), th.copy())
    pgp = gp.pseudo_gp()
    assert pgp.parent is gp
    u, S = sp.inputs("B", 1)[0], sp.full_sigma(2, 3)
    ex = sk.UncertaintyPropagationExact(pgp)
    r0 = ex.propagate_GA(u, S)
    g0 = pgp.estimate_many_gradient(u[None, :])
    clone = pickle.loads(pickle.dumps(pgp))              # (before the parent's model goes: the clone's parent refits on first use)
    gp.cov.clear_cache()
    gp._dev().close()
    r1 = ex.propagate_GA(u, S)
    assert r1[0] == r0[0] and r1[1] == r0[1]
    g1 = pgp.estimate_many_gradient(u[None, :])
    for a, b in zip(g0, g1):
        np.testing.assert_array_equal(a, b)
    assert clone._model is None and clone.parent._model is None
    r2 = sk.UncertaintyPropagationExact(clone).propagate_GA(u, S)
    bar = 2e-6 * float(np.exp(th_gc[0]))                 # two fits of one model, each within the oracle parity bar 1e-6 v of 3.
    assert abs(r2[0] - r0[0]) <= bar and abs(r2[1] - r0[1]) <= bar
    pgp.close()
    clone.close()


def test_inverse_propagation():
    c = case("B")
    up = sk.UncertaintyPropagationApprox(c.pgp)
    U = c.U[:4]
    dvh, s2 = up._get_variance_dv_many(U)                # loops the single call on a pseudo GP
    for i in range(len(U)):
        one = sk.UncertaintyPropagationApprox(c.pgp)
        for h in range(c.d):
            assert one._get_variance_dv_h(U[i], h) == dvh[i, h]
        assert one._get_sigma2(U[i]) == s2[i]
    models = [dl.approx_partials(c.xb, c.th_gc, c.P, c.beta, U[i], np.zeros((c.d, c.d)), defect="quirk") for i in range(len(U))]
    ref = [dl.approx_partials(c.xb, c.th_gc, c.P, c.beta, U[i], np.zeros((c.d, c.d)), dt=np.float64, defect="quirk") for i in range(len(U))]
    stack = lambda rows: {"dvh": tuple(np.stack([r["dvh"][j] for r in rows]) for j in (0, 1))}  # noqa: E731
    check("dvh", "B", {"dvh": dvh}, (stack(models), stack(ref)))
    inv = sk.InverseUncertaintyPropagationApprox(s2[0] + 0.05, c.pgp, U[0], np.ones(c.d), np.ones(c.d))
    many = inv.get_best_solution_many(U, s2 + 0.05)
    assert many.shape == (len(U), c.d)
    want = inv._closed_form(dvh, s2, inv.c, inv.I, inv.coestimated, s2 + 0.05)
    np.testing.assert_array_equal(many, want)
    if np.all(np.isfinite(many[0])):
        np.testing.assert_allclose(inv.get_best_solution(), many[0], rtol=1e-9)


# ------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals():
    c = case("B")
    h, m, d = c.h, c.m, c.d
    buf = np.zeros(max(4 * m * m, 4096))
    p = _gpx.ptr(buf)
    dbl, status = ctypes.c_double(), ctypes.c_int()
    lib = _gpx.lib
    calls = {
        "gpx_predict": lambda: lib.gpx_predict(h, p, 1, p, p),
        "gpx_solve": lambda: lib.gpx_solve(h, p, 1, p, p),
        "gpx_chol": lambda: lib.gpx_chol(h, p),
        "gpx_chol_mul": lambda: lib.gpx_chol_mul(h, p, 1, p),
        "gpx_logdet": lambda: lib.gpx_logdet(h, ctypes.byref(dbl)),
        "gpx_nll": lambda: lib.gpx_nll(h, ctypes.byref(dbl)),
        "gpx_nll_grad": lambda: lib.gpx_nll_grad(h, p),
        "gpx_propagate_dvh_many": lambda: lib.gpx_propagate_dvh_many(h, p, 1, p, p),
        "gpx_propagate_quadrature_many": lambda: lib.gpx_propagate_quadrature_many(h, p, p, 1, 1, p, p, 1, None, 0, 1, 0.0, p, None),
        "gpx_emu_trsm_left": lambda: lib.gpx_emu_trsm_left(h, p, 128, 128, p, p, 0, ctypes.byref(status)),
        "gpx_predict_kv": lambda: lib.gpx_predict_kv(h, p, 1, p, p, p),
        "gpx_rows_build": lambda: lib.gpx_rows_build(h, 2, p, p, 1, 1, p),
        "gpx_propagate_approx_rows": lambda: lib.gpx_propagate_approx_rows(h, p, p, 0, m, p),
        "gpx_propagate_exact_matrix": lambda: lib.gpx_propagate_exact_matrix(h, None, None, p, m, d, p, p, p, p, 1.0, ctypes.byref(dbl), None),
    }
    for name, call in calls.items():
        st = call()
        msg = _gpx.last_error()
        assert st == GPX_ERR_STATE, (name, st, msg)
        assert "pseudo-input model" in msg and "gpx_spgp_pseudo_handle" in msg, (name, msg)
    # the handle still serves afterwards
    n, dd = ctypes.c_int64(), ctypes.c_int()
    assert lib.gpx_n(h, ctypes.byref(n), ctypes.byref(dd)) == 0 and (n.value, dd.value) == (m, d)
    np.testing.assert_array_equal(c.pgp._get_beta(), c.beta)
    # Python
    g = dl.make_case(128, 2, 5)
    dense = sk.GaussianProcess(g[0], g[1], sk.GaussianCovariance(), g[2].copy())
    with pytest.raises(TypeError):
        dense.pseudo_gp()
    with pytest.raises(TypeError, match="parent"):
        sk.UncertaintyPropagationNumericalHG(c.pgp)
    with pytest.raises(TypeError, match="parent"):
        sk.UncertaintyPropagationMC(c.pgp, n=10, seed=1)
    sk.UncertaintyPropagationNumericalHG(c.gp)           # the parent itself is served, as before


# ------------------------------------------------------------------------------------------------
# 8. unchanged behaviour
# ------------------------------------------------------------------------------------------------
def test_parent_routes_unchanged():
    x, t, th, th_gc, xb = sp.make_model("B")
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(sp.MODELS["B"][2]), th.copy())
    u, S = sp.inputs("B", 1)[0], sp.full_sigma(2, 3)
    before = sk.UncertaintyPropagationExact(gp).propagate_GA(u, S)
    pgp = gp.pseudo_gp()
    pgp._dev()
    sk.UncertaintyPropagationExact(pgp).propagate_GA(u, S)
    after = sk.UncertaintyPropagationExact(gp).propagate_GA(u, S)
    assert before[0] == after[0] and before[1] == after[1]
    # estimate_many_gradient on the SPGP GP: the central differences of its docstring, through ONE estimate_many call
    xs, h = sp.inputs("B", 6), 1e-5
    m, d = xs.shape
    mean, var, dm, dv = gp.estimate_many_gradient(xs, h=h)
    pts = np.concatenate([xs[None]] + [xs[None] + s * h * np.eye(d)[k] for k in range(d) for s in (-1.0, 1.0)]).reshape(-1, d)
    mu, vv = gp.estimate_many(pts)
    mu, vv = np.asarray(mu).reshape(2 * d + 1, m), np.asarray(vv).reshape(2 * d + 1, m)
    np.testing.assert_array_equal(mean, mu[0])
    np.testing.assert_array_equal(var, vv[0])
    np.testing.assert_array_equal(dm, ((mu[2::2] - mu[1::2]) / (2.0 * h)).T)
    np.testing.assert_array_equal(dv, ((vv[2::2] - vv[1::2]) / (2.0 * h)).T)
    pgp.close()


# ------------------------------------------------------------------------------------------------
# 9. the chunk seam of the K^-1 form
# ------------------------------------------------------------------------------------------------
CHUNK_ROWS = 32768                                       # row_solve_chunk_cap at npad = 128


def test_chunk_seam_of_the_pair_form():
    """npad = 128, d = 8: a chunk holds 32768 // 10 = 3276 inputs of d + 2 rows (approx_many; B = 3300 is 33000 rows) and 32768 // 9 = 3640
    queries of d + 1 rows (predict_grad; B = 3700).  Every output is finite, and the last input of the first chunk, the first of the second,
    the first and the last of the batch equal the call on that input alone bit for bit."""
    c = case("D")
    assert c.m <= 128 and c.d == 8
    U = dl._grid(np.random.RandomState(4100 + 97 * c.d).uniform(1, 9, (3700, c.d)))
    for title, B, nrow, call in (("approx_many", 3300, c.d + 2, lambda V: approx_many(c.h, V, c.S)),
                                 ("predict_grad", 3700, c.d + 1, lambda V: predict_grad(c.h, V))):
        first = CHUNK_ROWS // nrow                       # inputs in the first chunk
        assert first < B <= 2 * first and first == {"approx_many": 3276, "predict_grad": 3640}[title]
        full = call(U[:B])
        for k, g in full.items():
            assert np.all(np.isfinite(g)), (title, k)
        for i in (0, first - 1, first, B - 1):
            alone = call(U[i:i + 1])
            for k, g in full.items():
                np.testing.assert_array_equal(alone[k][0], g[i], err_msg="%s %s input %d" % (title, k, i))
