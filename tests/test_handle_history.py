"""A call's result depends on its arguments and the fitted model alone -- never on what the same gpx_handle was asked before.

A handle carries state between calls ("State a handle carries between calls"): the single-u cache of gpx_propagate_approx /
gpx_propagate_dvh (have_u, u, V, KV, AUX), the count of new-u calls served by solves, the lazily built K^-1 and K^-1 row panel, the
memoised log det, and the workspace every entry point shares (Z, small, the pinned staging block, the pooled scratch).  Here every entry
point runs after every other one on a NEW handle and must give the bits it gives alone.

Two baselines an entry point: `cold` on a new handle, `warm` on a new handle right after gpx_kinv.  Legitimate history is exactly this:
whether K^-1 is resident.  The single-u Approx calls take two triangular solves before it exists and the one-pass kernel after, and the row
calls take a K^-1 row panel before and rows of the whole matrix after.  Where the two differ in bits they agree to the tolerance
test_gpu_parity.py holds the solve path to against the K^-1 path; every comparison of a history with its baseline is bitwise, on the
bytes, so that a NaN cannot hide.  Which baseline a history must reproduce is decided from the table's `leaves_kinv` (read from csrc:
who calls ensure_kinv), never from a result."""
import ctypes
import os
import time
from collections import namedtuple

import numpy as np
import pytest

from skgpuppy_amd import _gpx
from test_gpu_parity import SOLVE_VS_KINV_ATOL_PER_V, SOLVE_VS_KINV_DVH_ATOL_PER_V

pytestmark = pytest.mark.gpu

L = _gpx.lib
N, D, M_QUERIES = 300, 3, 131
SOLVE_CALLS = 24                        # GPX_APPROX_SOLVE_CALLS' default (csrc/propagate_api.hip, approx_solve_limit): not set here, it is read once per process

# name; fn(handle) -> every output as one float64 vector, the status first; leaves_kinv: the call leaves the whole K^-1 resident
# (it reaches ensure_kinv at these arguments); keeps_u: it leaves the single-u cache as it found it (have_u, u, V, KV, AUX).
Entry = namedtuple("Entry", "name fn leaves_kinv keeps_u")


def _p(a):
    return _gpx.ptr(a)


def _out(status, *arrays):
    return np.concatenate([[float(status)]] + [np.ravel(a) for a in arrays])


def _scalars(k):
    return [ctypes.c_double(np.nan) for _ in range(k)]


def _vals(cs):
    return np.array([c.value for c in cs])


def _gauss_gram(a, b, theta):
    w = np.exp(theta[2:])
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2 * w).sum(-1)
    return np.exp(theta[0]) * np.exp(-0.5 * d2)


class Model(object):
    """one seeded model of a handle kind, the fixed arguments of every call on it, and the table of its entry points"""

    def __init__(self, kind, seed=0, n=N, scale=10.0, v=2.0):
        rng = np.random.RandomState(1234 + seed)
        self.kind, self.n, self.d, self.v = kind, n, D, v
        self.x = rng.uniform(0, scale, (n, D))
        t = np.sin(0.3 * self.x.sum(1)) + 0.1 * rng.randn(n)
        self.t = np.ascontiguousarray(t - t.mean())
        w = 0.04 * (10.0 / scale) ** 2
        self.theta = np.log(np.array([v, 0.01] + [w, 1.5 * w, 0.75 * w]))
        if kind == "periodic":
            self.theta = np.concatenate([self.theta, np.log([3.0, 4.0, 5.0]), np.log([0.5, 0.25, 0.125])])
        c = scale / 2
        self.u1 = np.array([c + 0.25, c - 0.25, c + 0.5])
        self.u2 = np.array([c - 1.9, c + 1.2, c - 0.6])
        self.S = np.array([[0.04, 0.01, 0.0], [0.01, 0.09, -0.02], [0.0, -0.02, 0.0625]]) * (scale / 10.0) ** 2
        self.xs = rng.uniform(0, scale, (M_QUERIES, D))
        self.U5 = rng.uniform(0.2 * scale, 0.8 * scale, (5, D))        # 25 rows of d + 2: one partly filled tile
        self.U40 = rng.uniform(0.2 * scale, 0.8 * scale, (40, D))      # 200 rows: crosses a tile
        self.U26 = rng.uniform(0.2 * scale, 0.8 * scale, (26, D))      # the solve-to-K^-1 switch
        self.B2 = rng.randn(2, n)
        self.A = np.linalg.cholesky(self.S)
        self.z = rng.randn(7, D)
        self.wq = np.full(7, 1.0 / 7)
        self.y = np.linspace(-1.0, 1.0, 4)
        self.svar = np.ascontiguousarray(np.diag(self.S))
        self.wvec = np.exp(self.theta[2:2 + D])
        self.Cux = np.ascontiguousarray(_gauss_gram(self.u1[None, :], self.x, self.theta[:2 + D])[0])
        self.K = _gauss_gram(self.x, self.x, self.theta[:2 + D]) + 0.01 * np.eye(n)
        self.dK = np.ascontiguousarray(self.K - 0.01 * np.eye(n))
        self.kv = np.ascontiguousarray(_gauss_gram(self.xs, self.x, self.theta[:2 + D]))
        self.kdiag = np.full(M_QUERIES, v + 0.01)
        if kind == "pseudo":
            self.xb = np.ascontiguousarray(self.x[rng.permutation(n)[:130]] + 0.01 * rng.randn(130, D))
        self.entries = self._entries()
        self.by_name = {e.name: e for e in self.entries}

    # ---- handles ----
    def fit(self):
        h = ctypes.c_void_p()
        x, t, th = _p(self.x), _p(self.t), _p(self.theta)
        if self.kind == "gauss":
            st = L.gpx_fit(x, t, self.n, D, th, None, ctypes.byref(h))
        elif self.kind == "matern":
            st = L.gpx_matern_fit(x, t, self.n, D, th, 5, None, ctypes.byref(h))
        elif self.kind == "periodic":
            st = L.gpx_periodic_fit(x, t, self.n, D, th, None, ctypes.byref(h))
        elif self.kind == "matrix":
            st = L.gpx_fit_matrix(_p(self.K), t, self.n, None, ctypes.byref(h))
        else:
            sp = ctypes.c_void_p()
            _gpx.check(L.gpx_spgp_fit(x, t, self.n, D, th, _p(self.xb), 130, ctypes.byref(sp)), "gpx_spgp_fit")
            st = L.gpx_spgp_pseudo_handle(sp, ctypes.byref(h))
            L.gpx_spgp_free(sp)                 # the pseudo-input handle owns its copies
        _gpx.check(st, "fit (%s)" % self.kind)
        if self.kind != "pseudo":
            j = ctypes.c_double(np.nan)
            _gpx.check(L.gpx_jitter_used(h, ctypes.byref(j)), "gpx_jitter_used")
            assert j.value == 0.0, "theta was chosen so that the fit takes no jitter"
        return h

    @property
    def rows(self):
        """the rows the model has: the pseudo-input model's are its m = 130 pseudo-inputs"""
        return 130 if self.kind == "pseudo" else self.n

    # ---- the table ----
    def _entries(self):
        m, n, d = self, self.rows, D
        npad = (n + 127) // 128 * 128
        r0, r1 = 128, n
        B2 = np.ascontiguousarray(m.B2[:, :n])      # (held here: a pointer into a temporary would dangle)
        E = []

        def add(name, leaves_kinv=False, keeps_u=True):
            def deco(fn):
                E.append(Entry(name, fn, leaves_kinv, keeps_u))
                return fn
            return deco

        def two(fname):
            def fn(h):
                a, b = np.full(M_QUERIES, np.nan), np.full(M_QUERIES, np.nan)
                return _out(getattr(L, fname)(h, _p(m.xs), M_QUERIES, _p(a), _p(b)), a, b)
            return fn

        def approx_many(fname, U):
            def fn(h):
                o = np.full((4, len(U)), np.nan)
                return _out(getattr(L, fname)(h, _p(U), _p(m.S), 1, len(U), _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3])), o)
            return fn

        def dvh_many(fname):
            def fn(h):
                o, s2 = np.full((40, d), np.nan), np.full(40, np.nan)
                return _out(getattr(L, fname)(h, _p(m.U40), 40, _p(o), _p(s2)), o, s2)
            return fn

        def solve(h):
            a, b = np.full((2, n), np.nan), np.full((2, n), np.nan)
            return _out(L.gpx_solve(h, _p(B2), 2, _p(a), _p(b)), a, b)

        def kinv(h):
            o = np.full((n, n), np.nan)
            return _out(L.gpx_kinv(h, _p(o)), o)

        def exact_matrix(h):
            c = _scalars(2)
            st = L.gpx_propagate_exact_matrix(h, None, None, _p(m.x), n, d, _p(m.wvec), _p(m.Cux), _p(m.u1), _p(m.S), m.v + 0.01,
                                              ctypes.byref(c[0]), ctypes.byref(c[1]))
            return _out(st, _vals(c))

        def nll_grad(fname, k):
            def fn(h):
                g = np.full(k, np.nan)
                return _out(getattr(L, fname)(h, _p(g)), g)
            return fn

        def approx_at(u):
            def fn(h):
                c = _scalars(4)
                return _out(L.gpx_propagate_approx(h, _p(u), _p(m.S), *[ctypes.byref(ci) for ci in c]), _vals(c))
            return fn

        if m.kind in ("matern", "periodic"):
            add("gpx_%s_predict" % m.kind)(two("gpx_%s_predict" % m.kind))
            add("gpx_%s_nll_grad" % m.kind, leaves_kinv=True)(nll_grad("gpx_%s_nll_grad" % m.kind, len(m.theta)))
            add("gpx_matern_propagate_approx_many")(approx_many("gpx_matern_propagate_approx_many", m.U40))
            add("gpx_matern_propagate_dvh_many")(dvh_many("gpx_matern_propagate_dvh_many"))
            add("gpx_propagate_exact_matrix", leaves_kinv=True)(exact_matrix)
            add("gpx_solve")(solve)
            add("gpx_kinv", leaves_kinv=True)(kinv)
            return E
        if m.kind == "matrix":
            @add("gpx_predict_kv")
            def predict_kv(h):
                a, b = np.full(M_QUERIES, np.nan), np.full(M_QUERIES, np.nan)
                return _out(L.gpx_predict_kv(h, _p(m.kv), M_QUERIES, _p(m.kdiag), _p(a), _p(b)), a, b)
            add("gpx_solve")(solve)

            @add("gpx_nll_grad_matrix", leaves_kinv=True)
            def nll_grad_matrix(h):
                c = _scalars(1)
                return _out(L.gpx_nll_grad_matrix(h, _p(m.dK), ctypes.byref(c[0])), _vals(c))
            add("gpx_propagate_exact_matrix", leaves_kinv=True)(exact_matrix)
            add("gpx_kinv", leaves_kinv=True)(kinv)
            return E

        # a Gaussian handle, or a pseudo-input handle (which holds K^-1 from the start: `warm` is its one baseline)
        add("gpx_predict")(two("gpx_predict"))

        @add("gpx_predict_grad")
        def predict_grad(h):
            a, b, c, e = np.full(M_QUERIES, np.nan), np.full(M_QUERIES, np.nan), np.full((M_QUERIES, d), np.nan), np.full((M_QUERIES, d), np.nan)
            return _out(L.gpx_predict_grad(h, _p(m.xs), M_QUERIES, _p(a), _p(b), _p(c), _p(e)), a, b, c, e)

        @add("gpx_predict_mean_grad")
        def predict_mean_grad(h):
            a, c = np.full(M_QUERIES, np.nan), np.full((M_QUERIES, d), np.nan)
            return _out(L.gpx_predict_mean_grad(h, _p(m.xs), M_QUERIES, _p(a), _p(c)), a, c)

        @add("gpx_alpha")
        def alpha(h):
            o = np.full(n, np.nan)
            return _out(L.gpx_alpha(h, _p(o)), o)
        add("gpx_solve")(solve)

        @add("gpx_chol_mul")
        def chol_mul(h):
            o = np.full((2, n), np.nan)
            return _out(L.gpx_chol_mul(h, _p(B2), 2, _p(o)), o)

        @add("gpx_logdet")
        def logdet(h):
            c = _scalars(1)
            return _out(L.gpx_logdet(h, ctypes.byref(c[0])), _vals(c))

        @add("gpx_nll")
        def nll(h):
            c = _scalars(1)
            return _out(L.gpx_nll(h, ctypes.byref(c[0])), _vals(c))
        add("gpx_nll_grad", leaves_kinv=True)(nll_grad("gpx_nll_grad", 2 + d))
        add("gpx_kinv", leaves_kinv=True)(kinv)

        @add("gpx_kinv_rows")                    # 4 (384 - 128) < 3 * 384: a row PANEL, not the matrix (ensure_kinv_rows)
        def kinv_rows(h):
            o = np.full((r1 - r0, n), np.nan)
            return _out(L.gpx_kinv_rows(h, r0, r1, _p(o)), o)

        @add("gpx_cjh")
        def cjh(h):
            c, j, hh = np.full(n, np.nan), np.full((n, d), np.nan), np.full((n, d, d), np.nan)
            return _out(L.gpx_cjh(h, _p(m.u1), _p(c), _p(j), _p(hh)), c, j, hh)
        add("gpx_propagate_approx(u1)")(approx_at(m.u1))
        add("gpx_propagate_approx(u2)", keeps_u=False)(approx_at(m.u2))     # (the cache then belongs to u2)

        @add("gpx_propagate_dvh(u1)")
        def dvh(h):
            o = np.full(d, np.nan)
            return _out(L.gpx_propagate_dvh(h, _p(m.u1), _p(o)), o)

        @add("gpx_propagate_approx_rows", keeps_u=False)
        def approx_rows(h):
            o = np.full(4 + 2 * d, np.nan)
            return _out(L.gpx_propagate_approx_rows(h, _p(m.u1), _p(m.S), r0, r1, _p(o)), o)

        @add("gpx_propagate_approx_rhs", keeps_u=False)
        def approx_rhs(h):
            o = np.full(4 + 2 * d, np.nan)
            return _out(L.gpx_propagate_approx_rhs(h, _p(m.u1), _p(m.S), 1, 3, _p(o)), o)
        add("gpx_propagate_approx_many(b=5)")(approx_many("gpx_propagate_approx_many", m.U5))
        add("gpx_propagate_approx_many(b=40)")(approx_many("gpx_propagate_approx_many", m.U40))
        add("gpx_propagate_dvh_many")(dvh_many("gpx_propagate_dvh_many"))

        @add("gpx_propagate_exact(u1)", leaves_kinv=True)
        def exact(h):
            c = _scalars(2)
            return _out(L.gpx_propagate_exact(h, _p(m.u1), _p(m.S), ctypes.byref(c[0]), ctypes.byref(c[1])), _vals(c))

        @add("gpx_exact_mean")
        def exact_mean(h):
            c = _scalars(1)
            return _out(L.gpx_exact_mean(h, _p(m.u1), _p(m.S), ctypes.byref(c[0])), _vals(c))

        @add("gpx_propagate_exact_many", leaves_kinv=True)
        def exact_many(h):
            a, b = np.full(40, np.nan), np.full(40, np.nan)
            return _out(L.gpx_propagate_exact_many(h, _p(m.U40), _p(m.S), 1, 40, _p(a), _p(b)), a, b)

        @add("gpx_propagate_exact_grad_many", leaves_kinv=True)
        def exact_grad_many(h):
            o = [np.full(5, np.nan), np.full(5, np.nan)] + [np.full((5, d), np.nan) for _ in range(4)]
            return _out(L.gpx_propagate_exact_grad_many(h, _p(m.U5), _p(m.S), 1, 5, *[_p(a) for a in o]), *o)

        @add("gpx_propagate_exact_rows")         # the same panel as gpx_kinv_rows
        def exact_rows(h):
            o = np.full(3, np.nan)
            return _out(L.gpx_propagate_exact_rows(h, _p(m.u1), _p(m.S), r0, r1, _p(o)), o)

        @add("gpx_propagate_quadrature_many")
        def quadrature(h):
            mom, dens = np.full((5, 5), np.nan), np.full((5, 4), np.nan)
            st = L.gpx_propagate_quadrature_many(h, _p(m.U5), _p(m.A), 1, 5, _p(m.z), _p(m.wq), 7, _p(m.y), 4, 1, 0.25, _p(mom), _p(dens))
            return _out(st, mom, dens)

        @add("gpx_sensitivity_many")
        def sensitivity(h):
            o = [np.full(5, np.nan), np.full(5, np.nan), np.full((5, d), np.nan), np.full((5, d), np.nan)]
            return _out(L.gpx_sensitivity_many(h, _p(m.U5), _p(m.svar), 1, 5, *[_p(a) for a in o]), *o)

        @add("gpx_rows_build")
        def rows_build(h):
            o = np.full((128, npad), np.nan)
            return _out(L.gpx_rows_build(h, _gpx.ROWS_APPROX, _p(m.U5), _p(m.S), 1, 5, _p(o)), o)
        return E

    # ---- baselines ----
    def run(self, names, warm_first=False):
        """the calls `names`, in order, on a NEW handle (after gpx_kinv when warm_first): their results"""
        h = self.fit()
        try:
            if warm_first:
                assert self.by_name["gpx_kinv"].fn(h)[0] == 0.0
            return [self.by_name[k].fn(h) for k in names]
        finally:
            L.gpx_free(h)

    def baselines(self):
        if not hasattr(self, "_base"):
            cold = {} if self.kind == "pseudo" else {e.name: self.run([e.name])[0] for e in self.entries}
            warm = {e.name: self.run([e.name], warm_first=True)[0] for e in self.entries}
            self._base = (cold, warm)
        return self._base

    def expected(self, name, kinv_resident):
        cold, warm = self.baselines()
        return warm[name] if kinv_resident or self.kind == "pseudo" else cold[name]


_MODELS = {}


def model(kind, seed=0, **kw):
    key = (kind, seed)
    if key not in _MODELS:
        _MODELS[key] = Model(kind, seed, **kw)
    return _MODELS[key]


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _log(line):
    """GPX_HANDLE_HISTORY_RECORD=<file>: the figures behind profiles/r28_handle_history.txt"""
    path = os.environ.get("GPX_HANDLE_HISTORY_RECORD")
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


GAUSS_NAMES = [e.name for e in model("gauss").entries]           # (host arrays and closures alone: no device call at import)
KIND_NAMES = {k: [e.name for e in model(k).entries] for k in ("pseudo", "matern", "periodic", "matrix")}
# what a kind of handle refuses with GPX_ERR_STATE (include/gpx.h): a pseudo-input handle (gpx_spgp_pseudo_handle) has no factor and no
# targets; a periodic handle has no gpx_matern_* entry point -- the two stay in its table to go on being refused after any call
REFUSED = {"pseudo": ["gpx_predict", "gpx_solve", "gpx_chol_mul", "gpx_logdet", "gpx_nll", "gpx_nll_grad", "gpx_propagate_approx_rows",
                      "gpx_propagate_approx_rhs", "gpx_propagate_dvh_many", "gpx_propagate_quadrature_many", "gpx_rows_build"],
           "periodic": ["gpx_matern_propagate_approx_many", "gpx_matern_propagate_dvh_many"]}


@pytest.mark.parametrize("kind", ["gauss", "pseudo", "matern", "periodic", "matrix"])
def test_baselines_cold_and_warm_agree(kind):
    """every entry point succeeds alone (or is refused with GPX_ERR_STATE where the header says so); where its cold and warm results
    differ in bits, the two arithmetic paths agree to the tolerance the solve path is held to against the K^-1 path"""
    m = model(kind)
    t0 = time.perf_counter()
    cold, warm = m.baselines()
    for e in m.entries:
        w = warm[e.name]
        refused = e.name in REFUSED.get(kind, ())
        assert w[0] == (float(_gpx.GPX_ERR_STATE) if refused else 0.0), "%s: status %r" % (e.name, w[0])
        assert refused or np.isfinite(w).all(), e.name
        if kind == "pseudo":
            continue
        c = cold[e.name]
        assert c[0] == w[0] and (refused or np.isfinite(c).all()), e.name
        equal = same_bits(c, w)
        worst = 0.0 if equal else float(np.abs(c - w).max())
        _log("baseline %-8s %-36s cold == warm in bits: %-5s max |cold - warm| = %.3e" % (kind, e.name, equal, worst))
        if not equal:
            per_v = SOLVE_VS_KINV_DVH_ATOL_PER_V if "dvh" in e.name else SOLVE_VS_KINV_ATOL_PER_V
            assert worst <= per_v * m.v, "%s: cold and warm differ by %.3e > %.1e v" % (e.name, worst, per_v)
    _log("time baselines[%s] %.2f s" % (kind, time.perf_counter() - t0))


def _pairs_after(m, a_name):
    """A on a new handle, then every B: the B whose bits moved"""
    a = m.by_name[a_name]
    moved = []
    for b in m.entries:
        ra, rb = m.run([a.name, b.name])
        if not same_bits(ra, m.expected(a.name, False)):
            moved.append("%s itself (first call on a new handle)" % a.name)
        if not same_bits(rb, m.expected(b.name, a.leaves_kinv)):
            moved.append(b.name)
    return moved


@pytest.mark.parametrize("a_name", GAUSS_NAMES)
def test_ordered_pairs_gaussian(a_name):
    """for every ordered pair (A, B): B after A on a new handle gives B's warm bits if A leaves K^-1 resident, else its cold bits"""
    m = model("gauss")
    m.baselines()
    t0 = time.perf_counter()
    moved = _pairs_after(m, a_name)
    _log("time pairs[gauss] after %-36s %d pairs %.2f s" % (a_name, len(m.entries), time.perf_counter() - t0))
    assert not moved, "after %s these moved: %s" % (a_name, moved)


@pytest.mark.parametrize("kind", ["pseudo", "matern", "periodic", "matrix"])
def test_ordered_pairs_other_kinds(kind):
    """the same on the entry points each other kind of handle accepts; what a pseudo-input handle refuses it goes on refusing after any A
    (the status is the first entry of every result)"""
    m = model(kind)
    m.baselines()
    t0 = time.perf_counter()
    moved = {a: _pairs_after(m, a) for a in KIND_NAMES[kind]}
    moved = {a: bs for a, bs in moved.items() if bs}
    _log("time pairs[%s] %d pairs %.2f s" % (kind, len(m.entries) ** 2, time.perf_counter() - t0))
    assert not moved, "moved, by the call before: %s" % moved


@pytest.mark.parametrize("x_name", GAUSS_NAMES)
def test_warm_u_cache_survives_an_intervening_call(x_name):
    """approx(u1), X, dvh(u1), approx(u1): the last two give the bits of the sequence without X.  prepare_u (csrc/propagate_api.hip) serves
    a u it holds from the cache whether or not K^-1 has appeared since: after an X that keeps the cache (`keeps_u`) the results are those of
    the handle that never saw X, K^-1 or not.  After an X that drops or replaces the cache, V and KV are rebuilt: by solves -- the same
    bits -- unless X left K^-1 resident, when the sequence on a warm handle is the baseline.  An X that scribbles on V, KV, AUX or `small`
    under a live have_u fails here."""
    m = model("gauss")
    seq = ["gpx_propagate_dvh(u1)", "gpx_propagate_approx(u1)"]
    if not hasattr(m, "_seq"):
        m._seq = (m.run(["gpx_propagate_approx(u1)"] + seq)[1:], m.run(["gpx_propagate_approx(u1)"] + seq, warm_first=True)[1:])
    x = m.by_name[x_name]
    want = m._seq[0] if x.keeps_u or not x.leaves_kinv else m._seq[1]
    got = m.run(["gpx_propagate_approx(u1)", x_name] + seq)
    assert same_bits(got[0], m.expected("gpx_propagate_approx(u1)", False))
    assert same_bits(got[1], m.expected(x_name, False)), "%s itself moved after gpx_propagate_approx(u1)" % x_name
    moved = [k for k, g, w in zip(seq, got[2:], want) if not same_bits(g, w)]
    assert not moved, "after approx(u1), %s: %s moved" % (x_name, moved)


def test_solve_to_kinv_switch_happens_once():
    """26 distinct inputs on one handle: call i is served by solves while fewer than 24 new-u calls were (i < 24: the cold bits), by the
    K^-1 pass from then on (the warm bits) -- decided here from the count and the limit; the switch never reverts"""
    assert "GPX_APPROX_SOLVE_CALLS" not in os.environ
    m = model("gauss")

    def approx(h, u):
        c = _scalars(4)
        _gpx.check(L.gpx_propagate_approx(h, _p(u), _p(m.S), *[ctypes.byref(ci) for ci in c]), "gpx_propagate_approx")
        return _vals(c)

    def alone(u, warm):
        h = m.fit()
        try:
            if warm:
                assert m.by_name["gpx_kinv"].fn(h)[0] == 0.0
            return approx(h, u)
        finally:
            L.gpx_free(h)

    us = [np.ascontiguousarray(u) for u in m.U26]
    h = m.fit()
    try:
        got = [approx(h, u) for u in us]
        again = [approx(h, us[0]), approx(h, us[1])]          # new to the cache again: the K^-1 pass, not the solves
    finally:
        L.gpx_free(h)
    wrong = [i for i, (u, g) in enumerate(zip(us, got)) if not same_bits(g, alone(u, warm=i >= SOLVE_CALLS))]
    assert not wrong, "calls %s are not on the side the count puts them" % wrong
    assert same_bits(again[0], alone(us[0], True)) and same_bits(again[1], alone(us[1], True)), "the switch reverted"


SHORT = ["gpx_predict", "gpx_propagate_approx(u1)", "gpx_propagate_exact_many", "gpx_kinv"]


@pytest.mark.parametrize("a_name", SHORT)
def test_two_handles_interleaved(a_name):
    """A on one handle alternating with B on another (different x, theta, scale), one host thread: the shared pool, the stream cache and the
    pinned staging blocks.  Each result is its own handle's single-handle baseline: cold at first, warm the second time if the call itself
    left K^-1 there"""
    m1, m2 = model("gauss"), model("gauss", seed=1, n=260, scale=4.0, v=1.25)
    a = m1.by_name[a_name]
    moved = []
    for b_name in SHORT:
        b = m2.by_name[b_name]
        h1, h2 = m1.fit(), m2.fit()
        try:
            got = [a.fn(h1), b.fn(h2), a.fn(h1), b.fn(h2)]
        finally:
            L.gpx_free(h1)
            L.gpx_free(h2)
        want = [m1.expected(a.name, False), m2.expected(b.name, False), m1.expected(a.name, a.leaves_kinv), m2.expected(b.name, b.leaves_kinv)]
        moved += ["%s / %s: result %d" % (a_name, b_name, i) for i, (g, w) in enumerate(zip(got, want)) if not same_bits(g, w)]
    assert not moved, moved
