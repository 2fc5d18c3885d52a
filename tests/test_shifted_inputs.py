"""Every kernel family under an exact translation of its inputs (-m gpu).  The seeded inputs live on the 2^-20 grid, so x + 2^10 and
x + 2^17 are exact (tests/_shift.shifted asserts it) and the long-double models, which take direct differences, return for the translated
case the values of the case as seeded (tests/test_shift_model.py asserts that too).

1. Raw-input handles (Matern 3/2 and 5/2, Periodic): Gram and every derivative, the fit (factor, alpha, log det, NLL, gradient), the
   predictor at m = 33 and m = 300 and, for Matern, the batched propagation calls, gpx_predict_grad and gpx_rows_build -- the translated run
   reproduces the run as seeded BIT FOR BIT: these kernels form xi - xj first and see nothing else of the coordinates.
2. Gaussian handle, what does not depend on the fit: gpx_rows_build in every layout and gpx_cjh, bit for bit.
3. Gaussian handle, the sums over alpha and K^-1: the fit differs (the Gram comes from prescaled coordinates), so each sum is judged on the
   translated fit's own gpx_alpha / gpx_kinv against the long-double model of the case as seeded, by the unchanged rule
   MARGIN * max(rho_ref, FLOOR) of tests/_dense_ld.py, rho_ref from the float64 evaluation of the translated case, no extra term.
4. The consumers of the prescaled coordinates: gpx_nll_grad against its float64 restatement (tests/_shift.restated_grad) under the plain
   rule at BOTH shifts, and against long double less the derived allowance of _dense_ld.grad_loss with rho_ref from the restatement --
   asserted at 2^10, at 2^17 recorded, finite and of the model's signs; gpx_predict
   against a host triangular solve with the translated fit's own factor and rows from gpx_gram on the translated inputs, within
   MEAN_ATOL_V / VAR_ATOL_V of tests/test_backward_error.py; and no fit takes the jitter retry.

Shapes: N = 129 (127 padded columns) and 200 at d = 1, 3, 8, 9, 17 (one, two and three sweeps of the gradient passes, DR = 8 and 0 of the
row builds), N = 700 (npad 768) at d = 3 and 8.  One fit per (case, shift), closed and followed by gpx_pool_trim().

With GPX_DENSE_BOUNDS_RECORD=<file> every comparison appends a line (profiles/r27_shifted_inputs.txt is such a record)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from skgpuppy_amd.Covariance import _MaternModel, _PeriodicModel
from skgpuppy_amd.GaussianProcess import _DeviceModel

import _accuracy as acc
import _dense_ld as dl
import _exact_grad_model as eg
import _matern_ld as ml
import _periodic_ld as pl
import _predict_grad_model as pg
import _rows_ld as rl
import _sensitivity_model as sm
import _shift as sh
from test_backward_error import MEAN_ATOL_V, VAR_ATOL_V
from test_dense_bounds import approx_rows, check
from test_exact_grad import raw_grad
from test_exact_many import raw_many, seeded
from test_predict_grad import full_grad
from test_rows import build
from test_sensitivity import one as sens_one, sens

pytestmark = pytest.mark.gpu

CASES = [(N, d) for N in (129, 200) for d in (1, 3, 8, 9, 17)] + [(700, 3), (700, 8)]
IDS = ["n%d_d%d" % c for c in CASES]
SHIFT_IDS = [sh.name_of(s) for s in sh.SHIFTS]
RAW_KINDS = ("matern32", "matern52", "periodic")


def note(line):
    print(line)
    path = os.environ.get("GPX_DENSE_BOUNDS_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _dbl(n=1):
    return [ctypes.c_double() for _ in range(n)]


def _chol(h, n):
    out = np.empty((n, n))
    _gpx.check(_gpx.lib.gpx_chol(h, _gpx.ptr(out)), "gpx_chol")
    return out


def _sigma(d, seed):
    return dl.sigmas(d, seed)["full" if d >= 2 else "diag"]


# ------------------------------------------------------------------------------------------------
# 1. raw-input handles: the whole pipeline, bit for bit
# ------------------------------------------------------------------------------------------------
def raw_case(kind, N, d):
    mod = pl if kind == "periodic" else ml
    x, t, theta = mod.make_case(N, d)
    seed = mod.seed_of(N, d)
    sig = np.array([_sigma(d, seed + 100 * i) for i in range(8)])
    return {"x": x, "t": t, "theta": theta, "xs": mod.make_queries(x, 300, seed + 1), "U": mod.make_queries(x, 8, seed + 2), "Sigma": sig}


def raw_pipeline(kind, case):
    """{name: array} of everything section 1 lists, from one fit of the case"""
    x, t, theta, xs, U, Sig = (_gpx.f64(case[k]) for k in ("x", "t", "theta", "xs", "U", "Sigma"))
    N, d = x.shape
    out = {}
    if kind == "periodic":
        cov, model, nderiv = sk.PeriodicCovariance(), _PeriodicModel(x, t, theta), 2 + 3 * d
    else:
        nu2 = 3 if kind == "matern32" else 5
        cov, model, nderiv = sk.MaternCovariance(nu2 / 2.0), _MaternModel(x, t, theta, nu2), 2 + d
    try:
        h = model.handle
        out["gram"] = cov.cov_matrix(x, theta)
        out["cross"] = cov.cov_matrix_ij(xs[:33], x, theta)
        for j in range(nderiv):
            out["deriv %d" % j] = cov._d_cov_matrix_d_theta_ij(xs[:33], x, theta, j)
        assert model.jitter() == 0.0
        out["chol"], out["alpha"] = _chol(h, N), model.alpha()
        out["logdet"], out["nll"] = np.array([model.logdet()]), np.array([model.nll()])
        out["nll_grad"] = model.nll_grad()
        for m in (33, 300):                                              # the few-row and the many-row solver
            out["mean m=%d" % m], out["var m=%d" % m] = model.predict(np.ascontiguousarray(xs[:m]))
        if kind != "periodic":
            for k, a in zip(("mean", "var", "dmean", "dvar"), full_grad(h, U)):
                out["predict_grad " + k] = a
            out["rows grad"] = build(h, rl.GRAD, U, None, N, d)
        if kind == "matern52":
            for shared in (True, False):
                S = Sig[2] if shared else Sig
                o = [np.empty(len(U)) for _ in range(4)]
                _gpx.check(_gpx.lib.gpx_matern_propagate_approx_many(h, _gpx.ptr(U), _gpx.ptr(_gpx.f64(S)), int(shared), len(U), *[_gpx.ptr(a) for a in o]),
                           "gpx_matern_propagate_approx_many")
                for k, a in zip(("mean", "var", "sigma2", "rest"), o):
                    out["approx_many %s shared=%d" % (k, shared)] = a
                out["rows approx shared=%d" % shared] = build(h, rl.APPROX, U, S, N, d, shared=shared)
            dvh, s2 = np.empty((len(U), d)), np.empty(len(U))
            _gpx.check(_gpx.lib.gpx_matern_propagate_dvh_many(h, _gpx.ptr(U), len(U), _gpx.ptr(dvh), _gpx.ptr(s2)), "gpx_matern_propagate_dvh_many")
            out["dvh_many dvh"], out["dvh_many sigma2"] = dvh, s2
            out["rows dvh"] = build(h, rl.DVH, U, None, N, d)
    finally:
        model.close()
        _gpx.lib.gpx_pool_trim()
    return out


@pytest.mark.parametrize("kind", RAW_KINDS)
@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_raw_input_handles_reproduce_the_unshifted_run_bit_for_bit(N, d, kind):
    case = raw_case(kind, N, d)
    base = raw_pipeline(kind, case)
    v, vt = float(np.exp(case["theta"][0])), float(np.exp(case["theta"][1]))
    for a in base.values():
        assert np.isfinite(a).all()
    for s in sh.SHIFTS:
        got = raw_pipeline(kind, sh.shifted(case, s))
        assert got.keys() == base.keys()
        for k in base:
            np.testing.assert_array_equal(got[k], base[k], err_msg="%s N=%d d=%d shift %s: %s" % (kind, N, d, sh.name_of(s), k))
        # the equality quirk: query 3 is training row 5, at every shift: +vt there and nowhere else in the row
        row = got["cross"][3]
        assert row[5] > v + 0.5 * vt and (np.delete(row, 5) < v + 0.5 * vt).all(), (kind, s)
        note("1 raw %s N=%d d=%d shift %s: %d outputs, %d values, all bit-equal to the unshifted run" % (
            kind, N, d, sh.name_of(s), len(base), sum(a.size for a in base.values())))


# ------------------------------------------------------------------------------------------------
# the Gaussian handle
# ------------------------------------------------------------------------------------------------
class Fit(object):
    """one _DeviceModel of the dense case (N, d) translated by s; x, u, args: the case AS SEEDED (what the long-double model reads), X: what
    the device was given; Kinv and alpha: the device's own"""

    def __init__(self, N, d, s, kinv=True):
        self.N, self.d, self.s = N, d, s
        self.seed = dl.seed_of(N, d)
        self.x, self.t, self.theta = dl.make_case(N, d, self.seed)
        self.u = dl.inputs_u(self.x, self.theta, self.seed)
        moved = sh.shifted({"x": self.x, "u": self.u}, s)
        self.X, self.U = moved["x"], moved["u"]
        self.name = "N=%d d=%d shift %s" % (N, d, sh.name_of(s))
        self.model = _DeviceModel(_gpx.f64(self.X), _gpx.f64(self.t), _gpx.f64(self.theta))
        self.h = self.model.handle
        assert self.model.jitter() == 0.0, self.name                     # the translated fit does not take the +1e-5 I retry
        self.alpha = self.model.alpha()
        self.Kinv = self.model.kinv() if kinv else None
        self.args = (self.x, self.theta, self.Kinv, self.alpha)
        self.moved_args = (self.X, self.theta, self.Kinv, self.alpha)

    def both(self, fn, un, *rest, **kw):
        """(the long-double model on the case as seeded, the float64 evaluation of the TRANSLATED case)"""
        return fn(*self.args, self.u[un], *rest, **kw), fn(*self.moved_args, self.U[un], *rest, dt=np.float64, **kw)


@contextlib.contextmanager
def fit(N, d, s, kinv=True):
    f = None
    try:
        f = Fit(N, d, s, kinv)
        yield f
    finally:
        if f is not None and getattr(f, "model", None) is not None:
            f.model.close()
        _gpx.lib.gpx_pool_trim()


# ------------------------------------------------------------------------------------------------
# 2. outputs that do not depend on the fit: bit for bit
# ------------------------------------------------------------------------------------------------
def gauss_rows(N, d, s):
    with fit(N, d, s, kinv=False) as f:
        seed = f.seed
        U = np.array([f.U[k] for k in ("between", "equal", "far")])
        Sig = np.array([_sigma(d, seed + 100 * i) for i in range(3)])
        out = {"rows dvh": build(f.h, rl.DVH, U, None, N, d), "rows grad": build(f.h, rl.GRAD, U, None, N, d),
               "rows approx shared": build(f.h, rl.APPROX, U, Sig[1], N, d, shared=True), "rows approx per input": build(f.h, rl.APPROX, U, Sig, N, d)}
        for un, u in f.U.items():
            C, J, H = np.empty(N), np.empty((N, d)), np.empty((N, d, d))
            _gpx.check(_gpx.lib.gpx_cjh(f.h, _gpx.ptr(_gpx.f64(u)), _gpx.ptr(C), _gpx.ptr(J), _gpx.ptr(H)), "gpx_cjh")
            out["cjh C " + un], out["cjh J " + un], out["cjh H " + un] = C, J, H
        return out


@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_gaussian_rows_and_cjh_bit_for_bit(N, d):
    base = gauss_rows(N, d, 0.0)
    theta = dl.make_case(N, d, dl.seed_of(N, d))[2]
    v, vt = float(np.exp(theta[0])), float(np.exp(theta[1]))
    for s in sh.SHIFTS:
        got = gauss_rows(N, d, s)
        for k in base:
            assert np.isfinite(got[k]).all(), k
            np.testing.assert_array_equal(got[k], base[k], err_msg="gauss N=%d d=%d shift %s: %s" % (N, d, sh.name_of(s), k))
        C = got["cjh C equal"]
        assert C[dl.QUIRK_ROW] > v + 0.5 * vt and (np.delete(C, dl.QUIRK_ROW) < v + 0.5 * vt).all()
        assert (got["cjh C between"] < v + 0.5 * vt).all()
        note("2 gauss rows / cjh N=%d d=%d shift %s: %d outputs, %d values, all bit-equal to the unshifted run" % (
            N, d, sh.name_of(s), len(base), sum(a.size for a in base.values())))


# ------------------------------------------------------------------------------------------------
# 3. the sums over alpha and K^-1: the existing rule, no extra term
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", sh.SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_approx_dvh_exact_single_calls(N, d, s):
    """gpx_propagate_approx_rows (all rows), gpx_propagate_dvh, gpx_propagate_exact: the three inputs, Sigma diagonal and full"""
    with fit(N, d, s) as f:
        for un in f.u:
            u = _gpx.f64(f.U[un])
            for sn, S in dl.sigmas(d, f.seed).items():
                S = _gpx.f64(S)
                want, ref = f.both(dl.approx_partials, un, S)
                dv = np.empty(d)
                _gpx.check(_gpx.lib.gpx_propagate_dvh(f.h, _gpx.ptr(u), _gpx.ptr(dv)), "gpx_propagate_dvh")
                check("3 approx u %s, Sigma %s" % (un, sn), f.name, {"partials": approx_rows(f, u, S, 0, N), "dvh": dv}, want, ref)
                want, ref = f.both(dl.exact_builtin, un, S)
                m, var = _dbl(2)
                _gpx.check(_gpx.lib.gpx_propagate_exact(f.h, _gpx.ptr(u), _gpx.ptr(S), ctypes.byref(m), ctypes.byref(var)), "gpx_propagate_exact")
                check("3 exact u %s, Sigma %s" % (un, sn), f.name, {"mean": np.array([m.value]), "var": np.array([var.value])}, want, ref)


@pytest.mark.parametrize("s", sh.SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_exact_many_and_its_gradients(N, d, s):
    """gpx_propagate_exact_many and gpx_propagate_exact_grad_many, b = 5 = [between, equal, far, two seeded], one shared Sigma"""
    with fit(N, d, s) as f:
        extra = seeded(f, 2, 23)
        U0 = np.array([f.u["between"], f.u["equal"], f.u["far"]] + extra)
        U = sh.translate(U0, s)
        S = _sigma(d, f.seed)
        mean, var = raw_many(f.h, U, S)
        got = raw_grad(f.h, U, S)
        for i in ((0, 1) if N == 700 else (0, 1, 3)):                    # (the gradient model's cost grows as N^2 d)
            want = dl.exact_builtin(*f.args, U0[i], S)
            ref = dl.exact_builtin(*f.moved_args, U[i], S, dt=np.float64)
            check("3 exact_many input %d" % i, f.name, {"mean": mean[i:i + 1], "var": var[i:i + 1]}, want, ref)
            want = eg.moments_grad(*f.args, U0[i], S)
            ref = eg.moments_grad(*f.moved_args, U[i], S, dt=np.float64)
            ref_dist = eg.distances({k: ref[k][0] for k in got}, want)
            dist = eg.distances({k: np.ravel(g[i]) for k, g in got.items()}, want)
            dl.record("3 exact_grad_many input %d" % i, f.name, dl.rho_of(ref_dist), dist, ref_dist)
            dl.assert_within(dist, dl.rho_of(ref_dist), what="3 exact_grad_many input %d %s" % (i, f.name))
        assert np.isfinite(mean).all() and np.isfinite(var).all() and all(np.isfinite(g).all() for g in got.values())


@pytest.mark.parametrize("s", sh.SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_sensitivity(N, d, s):
    """gpx_sensitivity_many on tests/_sensitivity_model.combos: one batched call with per-input s"""
    with fit(N, d, s, kinv=False) as f:
        cs = sm.combos(f.x, f.theta, f.seed)
        out = sens(f.h, sh.translate(np.stack([u for _n, u, _s in cs]), s), np.stack([sg for _n, _u, sg in cs]))
        for i, (cn, u, sg) in enumerate(cs):
            want = sm.sums(f.x, f.theta, f.alpha, u, sg)
            ref = sm.sums(f.X, f.theta, f.alpha, sh.translate(u, s), sg, dt=np.float64)
            got = sens_one(out, i)
            check("3 sensitivity " + cn, f.name, got, want, ref)
            for key in ("first", "total"):
                assert np.all(got[key][sg == 0] == 0.0), (cn, key, got[key])


@pytest.mark.parametrize("s", sh.SHIFTS, ids=SHIFT_IDS)
@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_batched_solver_calls(N, d, s):
    """gpx_predict_grad, gpx_propagate_approx_many, gpx_propagate_dvh_many at the three inputs: d + 1, d + 2 and 2 d + 1 solved rows an input
    reduced on the device, each output against the same sum over the device's own K^-1 and alpha"""
    with fit(N, d, s) as f:
        names = list(f.u)
        U0, U = np.array([f.u[k] for k in names]), np.array([f.U[k] for k in names])
        S = _gpx.f64(_sigma(d, f.seed))
        mean, var, dm, dv = full_grad(f.h, U)
        ld_m, ld_v = pg.mean_grad(f.x, f.theta, f.alpha, U0, 0), pg.var_grad(f.x, f.theta, f.Kinv, U0, 0)
        rf_m, rf_v = pg.mean_grad(f.X, f.theta, f.alpha, U, 0, dt=np.float64), pg.var_grad(f.X, f.theta, f.Kinv, U, 0, dt=np.float64)
        check("3 predict_grad", f.name, {"mean": mean, "var": var, "dmean": dm, "dvar": dv}, dict(ld_m, **ld_v), dict(rf_m, **rf_v))
        o = [np.empty(len(U)) for _ in range(4)]
        _gpx.check(_gpx.lib.gpx_propagate_approx_many(f.h, _gpx.ptr(_gpx.f64(U)), _gpx.ptr(S), 1, len(U), *[_gpx.ptr(a) for a in o]), "gpx_propagate_approx_many")
        dvh, s2 = np.empty((len(U), d)), np.empty(len(U))
        _gpx.check(_gpx.lib.gpx_propagate_dvh_many(f.h, _gpx.ptr(_gpx.f64(U)), len(U), _gpx.ptr(dvh), _gpx.ptr(s2)), "gpx_propagate_dvh_many")
        for i, un in enumerate(names):
            want, ref = f.both(dl.approx_partials, un, S)
            got = {k: a[i:i + 1] for k, a in zip(("mean", "var", "sigma2", "rest"), o)}
            check("3 approx_many u %s" % un, f.name, got, want, ref)
            check("3 dvh_many u %s" % un, f.name, {"dvh": dvh[i], "sigma2": s2[i:i + 1]}, want, ref)


# ------------------------------------------------------------------------------------------------
# 4. the consumers of the prescaled coordinates
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_gradient_against_the_restatement_and_with_the_allowance(N, d):
    """gpx_nll_grad at both shifts, both yardsticks of tests/_shift.py on the plain scales of _dense_ld.grad:
    - against restated_grad (float64, differences of the scaled coordinates, the same K^-1 and alpha) under the plain rule with no
      allowance, ASSERTED AT 2^10 AND 2^17: an arithmetic that loses more than the differences of scaled coordinates do -- expanded
      squares sit 150 to 3000 bounds out at 2^17 (tests/test_shift_model.py) -- fails here;
    - against long double less _dense_ld.grad_loss, rho_ref from the restatement: asserted at 2^10; at 2^17 recorded, the gradient finite
      and of the model's sign wherever the model's value stands clear of its own bound.
    The distance to long double without the allowance is recorded at both shifts."""
    for s in sh.SHIFTS:
        with fit(N, d, s) as f:
            g = np.empty(d + 2)
            _gpx.check(_gpx.lib.gpx_nll_grad(f.h, _gpx.ptr(g)), "gpx_nll_grad")
            assert np.isfinite(g).all(), (f.name, g)
            want, scale = dl.grad(*f.args)
            ref = sh.restated_grad(f.X, f.theta, f.Kinv, f.alpha)
            twin = {"grad": dl.distances(g, ref, scale)}
            note("4 gradient against the float64 restatement, plain scales | %s | worst %.3e = %.6f of the bound %.3e" % (
                f.name, twin["grad"].max(), twin["grad"].max() / dl.bound(0.0), dl.bound(0.0)))
            dl.assert_within(twin, 0.0, what="gpx_nll_grad against its restatement " + f.name)
            loss = dl.grad_loss(f.x, f.theta, f.Kinv, f.alpha, s)
            ref_dist = {"grad": dl.distances(ref, want, scale, loss)}
            rho = dl.rho_of(ref_dist)
            dist = {"grad": dl.distances(g, want, scale, loss)}
            dl.record("4 gradient against long double less the prescale allowance", f.name, rho, dist, ref_dist)
            dl.record("4 gradient against long double, no allowance (recorded only)", f.name, rho, {"grad": dl.distances(g, want, scale)},
                      {"grad": dl.distances(ref, want, scale)})
            if s == sh.OFFSET:
                dl.assert_within(dist, rho, what="gpx_nll_grad " + f.name)
            else:
                clear = np.abs(want) > dl.bound(rho) * scale + loss
                assert (np.sign(g[clear]) == np.sign(want[clear].astype(np.float64))).all(), (f.name, g, want)


def _queries(x, m, seed):
    """m queries on the grid in [0, 10]^d, query 3 bit-equal to training row 5"""
    xs = dl._grid(np.random.RandomState(seed + 17).uniform(0, 10, (m, x.shape[1])))
    xs[3] = x[dl.QUIRK_ROW]
    return xs


@pytest.mark.parametrize("N,d", CASES, ids=IDS)
def test_predictor_rows_are_the_grams(N, d):
    """gpx_predict, m = 33 and m = 300, against mean = k* . alpha_dev and var = v + vt - |L_dev^-1 k*|^2 with k* from gpx_gram on the
    translated queries and training inputs (held to its model at this offset by tests/test_gauss_gram.py): the Gram's own loss is on both
    sides, so the tolerances are those of tests/test_backward_error.py, unchanged"""
    for s in sh.SHIFTS:
        with fit(N, d, s, kinv=False) as f:
            xs = sh.translate(_queries(f.x, 300, f.seed), s)
            v, vt = np.exp(f.theta[0]), np.exp(f.theta[1])
            L = f.model.chol()
            ks = sk.GaussianCovariance().cov_matrix_ij(xs, f.X, f.theta)
            assert ks[3, dl.QUIRK_ROW] == v                               # (gpx_gram carries no noise term)
            W = acc.lapack_trsv(L, ks.T)
            mean_ref, var_ref = ks.dot(f.alpha), v + vt - np.einsum("ij,ij->j", W, W)
            for m in (33, 300):
                mean, var = f.model.predict(np.ascontiguousarray(xs[:m]))
                em, ev = float(np.abs(mean - mean_ref[:m]).max()) / v, float(np.abs(var - var_ref[:m]).max()) / v
                note("4 predict %s m=%d: mean %.3e (<= %.1e) var %.3e (<= %.1e), in units of v" % (f.name, m, em, MEAN_ATOL_V, ev, VAR_ATOL_V))
                assert em <= MEAN_ATOL_V and ev <= VAR_ATOL_V, (f.name, m, em, ev)
