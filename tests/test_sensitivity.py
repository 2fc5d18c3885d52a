"""gpx_sensitivity_many and SensitivityAnalysis on the device: the variance decomposition of the predictor mean under independent Gaussian
inputs against the long-double model of tests/_sensitivity_model.py, each sum on the scale of its own absolute terms, under the bound
measured on the float64 numpy evaluation of the same case (the project's one rule: tests/_spgp_ld.py through tests/_dense_ld.py;
tests/test_sensitivity_model.py: the model is the definitions and the rule sees seeded defects).

Every sum is judged on the device's OWN alpha (gpx_alpha).  Shapes: N = 700 (npad 768) at every d of _dense_ld.D_ALL -- 1 .. 8 one sweep of
8 slots, 9 and 16 two (one slot / a full one in the last), 17, 32, 33, 64 three to eight -- and N = 128, 129, 200 at d = 1, 3, 8.  Inputs per
case, one batched call with per-input s: u between the points, bit-equal to training row 5 and far outside the data (every c_i <= 1e-130)
under s drawn in [0.01, 4]; u between the points under s with zeros in every other coordinate (those entries == 0.0 exactly; the
compacted slots give the sweep counts of d / 2), s = 1e-10 everywhere (E_k - m_k cancels to 1e-10 of its terms: judged on the scale) and
s = 100.

With GPX_DENSE_BOUNDS_RECORD=<file> every comparison appends its rho_ref, the bound and each group's worst ratio to both
(profiles/r24_sensitivity.txt holds such a record)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from skgpuppy_amd.GaussianProcess import _DeviceModel

import _dense_ld as dl
import _sensitivity_model as sm
import _spgp_ld as sl

pytestmark = pytest.mark.gpu

IDS = ["n%d_d%d" % c for c in dl.CASES]
FILL = -7.25
GPX_ERR_BAD_ARG, GPX_ERR_STATE = -1, -4


class Fit(object):
    def __init__(self, N, d, sharp=False):
        self.N, self.d = N, d
        self.seed = dl.seed_of(N, d)
        self.x, self.t, self.theta = dl.make_case(N, d, self.seed, sharp)
        self.name = "N=%d d=%d%s" % (N, d, " sharp" if sharp else "")
        self.model = _DeviceModel(_gpx.f64(self.x), _gpx.f64(self.t), _gpx.f64(self.theta))
        self.alpha = self.model.alpha()
        self.h = self.model.handle


@contextlib.contextmanager
def fit(N, d, sharp=False):
    f = None
    try:
        f = Fit(N, d, sharp)
        yield f
    finally:
        if f is not None and getattr(f, "model", None) is not None:
            f.model.close()
        _gpx.lib.gpx_pool_trim()


def sens(h, U, S, total=True, status=False):
    """{"mean": [b], "V": [b], "first": [b, d], "total": [b, d]} of gpx_sensitivity_many; S [d] = one set for all inputs; the outputs enter
    holding FILL"""
    U, S = _gpx.f64(U), _gpx.f64(S)
    b, d = U.shape
    out = {"mean": np.full(b, FILL), "V": np.full(b, FILL), "first": np.full((b, d), FILL), "total": np.full((b, d), FILL)}
    st = _gpx.lib.gpx_sensitivity_many(h, _gpx.ptr(U), _gpx.ptr(S), int(S.ndim == 1), b, _gpx.ptr(out["mean"]), _gpx.ptr(out["V"]),
                                       _gpx.ptr(out["first"]), _gpx.ptr(out["total"]) if total else None)
    if status:
        return st, out
    _gpx.check(st, "gpx_sensitivity_many")
    if not total:
        assert np.all(out.pop("total") == FILL)
    return out


def check(title, name, got, want, ref):
    """got {group: values} against want {group: (values, scales)} under the bound of ref, the float64 evaluation of the same sums"""
    ref_dist = {k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in got}
    rho = dl.rho_of(ref_dist)
    for k, g in got.items():
        assert np.all(np.isfinite(g)), (title, name, k, g)
    dist = {k: dl.distances(g, want[k][0], want[k][1]) for k, g in got.items()}
    dl.record(title, name, rho, dist, ref_dist)
    dl.assert_within(dist, rho, what=title + " " + name)
    return rho


def one(out, i):
    return {"mean": out["mean"][i:i + 1], "V": out["V"][i:i + 1], "first": out["first"][i], "total": out["total"][i]}


def run_combos(f):
    cs = sm.combos(f.x, f.theta, f.seed)
    out = sens(f.h, np.stack([u for _n, u, _s in cs]), np.stack([s for _n, _u, s in cs]))
    for i, (cn, u, s) in enumerate(cs):
        want, ref = sm.both(f.x, f.theta, f.alpha, u, s)
        got = one(out, i)
        check("sensitivity " + cn, f.name, got, want, ref)
        for key in ("first", "total"):
            assert np.all(got[key][s == 0] == 0.0), (cn, key, got[key])


# ------------------------------------------------------------------------------------------------
# 3. every output entry under the rule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", dl.CASES, ids=IDS)
def test_sums(N, d):
    with fit(N, d) as f:
        run_combos(f)


def test_sums_sharp_w():
    """w in [2, 8]: om sg up to 32, the kernel a few grid cells wide"""
    with fit(*dl.SHARP_CASE, sharp=True) as f:
        run_combos(f)


# ------------------------------------------------------------------------------------------------
# 4. batching
# ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def chunk_of(n):
    old = os.environ.get("GPX_SENS_CHUNK")
    os.environ["GPX_SENS_CHUNK"] = str(n)
    try:
        yield
    finally:
        if old is None:
            del os.environ["GPX_SENS_CHUNK"]
        else:
            os.environ["GPX_SENS_CHUNK"] = old


def same_bits(a, b, keys=("mean", "V", "first", "total")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])


@pytest.mark.parametrize("N,d", [(200, 3), (700, 9)])
def test_an_inputs_result_does_not_depend_on_the_batch(N, d):
    with fit(N, d) as f:
        rng = np.random.RandomState(f.seed + 5)
        U = dl._grid(rng.uniform(1, 9, (130, d)))
        S = rng.uniform(0.01, 4.0, (130, d))
        S[1, 0] = 0.0                                   # one of the three with fewer active slots than its neighbours
        alone = [sens(f.h, U[i:i + 1], S[i:i + 1]) for i in range(3)]
        three = sens(f.h, U[:3], S[:3])
        rev = sens(f.h, U[::-1], S[::-1])               # the three are the LAST of 130, reversed
        with chunk_of(7):                               # 19 chunks, the three in the last one
            rev7 = sens(f.h, U[::-1], S[::-1])
        for i in range(3):
            for other, at in ((three, i), (rev, 129 - i), (rev7, 129 - i)):
                same_bits(one(alone[i], 0), one(other, at))
        same_bits(rev, rev7)
        # one shared s against the same s repeated per input
        shared = sens(f.h, U, S[0])
        same_bits(shared, sens(f.h, U, np.repeat(S[:1], 130, axis=0)))
        # total == NULL leaves the rest bit-equal
        same_bits(rev, sens(f.h, U[::-1], S[::-1], total=False), keys=("mean", "V", "first"))


# ------------------------------------------------------------------------------------------------
# 5. identities
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(200, 3), (700, 9)])
def test_identities(N, d):
    with fit(N, d) as f:
        u = dl.inputs_u(f.x, f.theta, f.seed)["between"]
        drawn = sm.variances(d, f.seed)["drawn"]
        lim = None
        # exactly one s_k > 0: first_k, total_k and V are one number, the other entries 0.0
        S = np.zeros((d, d))
        S[np.arange(d), np.arange(d)] = drawn
        out = sens(f.h, np.repeat(u[None, :], d, axis=0), S)
        for k in range(d):
            want, ref = sm.both(f.x, f.theta, f.alpha, u, S[k])
            rho = check("identity one s_%d > 0" % k, f.name, one(out, k), want, ref)
            lim = sm.bound(rho)
            off = np.arange(d) != k
            assert np.all(out["first"][k][off] == 0.0) and np.all(out["total"][k][off] == 0.0)
            for key in ("first", "total"):
                assert abs(out[key][k][k] - out["V"][k]) <= lim * float(want[key][1][k] + want["V"][1][0]), (k, key)
        # all s = 0: nothing varies
        none = sens(f.h, u[None, :], np.zeros(d))
        assert none["V"][0] == 0.0 and np.all(none["first"] == 0.0) and np.all(none["total"] == 0.0)
        v, _vt, w = dl.params(f.theta, d)
        terms = f.alpha.astype(dl.LD) * v * np.exp(-(w * (u.astype(dl.LD) - f.x.astype(dl.LD)) ** 2).sum(1) / 2)
        assert abs(none["mean"][0] - terms.sum()) <= lim * float(np.abs(terms).sum())
        # sum first <= V <= sum total, up to the summed bounds
        want, ref = sm.both(f.x, f.theta, f.alpha, u, drawn)
        full = sens(f.h, u[None, :], drawn)
        lim = sm.bound(check("identity ordering", f.name, one(full, 0), want, ref))
        slack_f = lim * float(want["first"][1].sum() + want["V"][1][0])
        slack_t = lim * float(want["total"][1].sum() + want["V"][1][0])
        assert full["first"][0].sum() <= full["V"][0] + slack_f
        assert full["V"][0] <= full["total"][0].sum() + slack_t


# ------------------------------------------------------------------------------------------------
# 6. against merged code: V is the beta beta^T part of Girard's exact variance for a diagonal Sigma
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [200, 700])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_against_the_exact_propagation(N, d):
    """gpx_propagate_exact_matrix with an explicit K^-1 = 0, beta = alpha, C_ux the plain kernel and cuu = 0 returns mean and
    var = nc2 sum_ij beta_i beta_j L_ij - mean^2 = V.  That path subtracts mean^2 at the end: its rounding sits on the scale of V's terms
    PLUS (sum |g_i|)^2, and the allowed difference is twice the rule's bound on that scale."""
    with fit(N, d) as f:
        u = dl.inputs_u(f.x, f.theta, f.seed)["between"]            # off the training rows
        s = sm.variances(d, f.seed)["drawn"]
        v, _vt, w = dl.params(f.theta, d, np.float64)
        C = v * np.exp(-0.5 * (w * (f.x - u) ** 2).sum(1))
        mean, var = ctypes.c_double(), ctypes.c_double()
        zeros = np.zeros((N, N))
        _gpx.check(_gpx.lib.gpx_propagate_exact_matrix(None, _gpx.ptr(zeros), _gpx.ptr(f.alpha), _gpx.ptr(_gpx.f64(f.x)), N, d, _gpx.ptr(_gpx.f64(w)),
                                                       _gpx.ptr(_gpx.f64(C)), _gpx.ptr(_gpx.f64(u)), _gpx.ptr(_gpx.f64(np.diag(s))), 0.0,
                                                       ctypes.byref(mean), ctypes.byref(var)), "gpx_propagate_exact_matrix")
        want, ref = sm.both(f.x, f.theta, f.alpha, u, s)
        out = sens(f.h, u[None, :], s)
        rho = check("against Exact", f.name, one(out, 0), want, ref)
        lim = 2 * sm.bound(rho)
        scale_v = float(want["V"][1][0] + want["mean"][1][0] ** 2)
        print("N=%d d=%d: V %.15g, Exact's %.15g, difference %.3e = %.4f of the allowed %.3e; mean %.15g against %.15g"
              % (N, d, out["V"][0], var.value, abs(out["V"][0] - var.value), abs(out["V"][0] - var.value) / (lim * scale_v), lim * scale_v,
                 out["mean"][0], mean.value))
        assert abs(out["V"][0] - var.value) <= lim * scale_v
        assert abs(out["mean"][0] - mean.value) <= lim * float(want["mean"][1][0])


# ------------------------------------------------------------------------------------------------
# 7. the pseudo-input handle of an SPGP model; 8. the Python class
# ------------------------------------------------------------------------------------------------
def test_pseudo_handle():
    N, d, m = 300, 3, 40
    x, t, theta, _xs = sl.make_case(N, d, m, 0.03, 0.06, 0.3)
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), theta.copy())
    pgp = gp.pseudo_gp()
    try:
        beta = pgp._get_beta()
        xb, th_gc = pgp.x, pgp.theta_min
        sa = sk.SensitivityAnalysis(pgp)
        rng = np.random.RandomState(77)
        U = dl._grid(rng.uniform(2, 8, (5, d)))
        S = rng.uniform(0.01, 4.0, (5, d))
        S[2, 1] = 0.0
        mean, V, first, total = sa.variances_many(U, S)
        assert mean.shape == V.shape == (5,) and first.shape == total.shape == (5, d)
        for i in range(5):
            want, ref = sm.both(xb, th_gc, beta, U[i], S[i])
            got = {"mean": mean[i:i + 1] - gp.meant, "V": V[i:i + 1], "first": first[i], "total": total[i]}
            check("pseudo input %d" % i, "N=%d m=%d d=%d" % (N, m, d), got, want, ref)
        assert first[2, 1] == 0.0 and total[2, 1] == 0.0
        # a fitted SPGP GaussianProcess itself is refused: its dense route is another quantity
        with pytest.raises(TypeError, match="pseudo_gp"):
            sk.SensitivityAnalysis(gp)
    finally:
        pgp.close()
        gp.cov.clear_cache()
        _gpx.lib.gpx_pool_trim()


class PlainGaussian(sk.GaussianCovariance):
    """the built-in kernel behind the generic route (gpx_fit_matrix): an overridden matrix builder"""

    def cov_matrix_ij(self, xi, xj, theta):
        return sk.GaussianCovariance.cov_matrix_ij(self, xi, xj, theta)


def small_problem():
    rng = np.random.RandomState(12)
    x = dl._grid(rng.uniform(0, 10, (60, 2)))
    t = np.sin(0.4 * x[:, 0]) + 0.3 * x[:, 1] + 3.0
    return x, t


def test_python_class():
    x, t = small_problem()
    d = 2
    theta = np.log(np.array([2.0, 0.01, 0.3, 0.1]))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    sa = sk.SensitivityAnalysis(gp)
    u, s = np.array([4.5, 5.25]), np.array([0.8, 0.0])
    mean, V, first, total = sa.variances(u, s)
    assert np.ndim(mean) == 0 and np.ndim(V) == 0 and first.shape == total.shape == (d,)
    want, ref = sm.both(x, theta, gp._dev().alpha(), u, s)
    check("class", "N=60 d=2", {"mean": np.array([mean - gp.meant]), "V": np.array([V]), "first": first, "total": total}, want, ref)
    assert first[1] == 0.0 and total[1] == 0.0 and first[0] > 0
    # the same through every accepted form of Sigma_x, bit for bit; meant is added to the mean alone
    for form in (np.diag(s), list(s)):
        again = sa.variances(u, form)
        assert again[0] == mean and again[1] == V and np.array_equal(again[2], first) and np.array_equal(again[3], total)
    U = np.stack([u, u + 0.5, u - 1.0])
    many = sa.variances_many(U, s)
    assert many[0].shape == many[1].shape == (3,) and many[2].shape == many[3].shape == (3, d)
    assert many[0][0] == mean and many[1][0] == V and np.array_equal(many[2][0], first)
    per = sa.variances_many(U, np.stack([np.diag(s)] * 3))
    for a, b in zip(many, per):
        assert np.array_equal(a, b)
    raw = sens(gp._dev().handle, U, s)
    assert np.array_equal(raw["mean"] + gp.meant, many[0]) and np.array_equal(raw["V"], many[1])
    # indices: the shares, zeros where V == 0
    fi, ti = sa.indices(u, s)
    assert np.array_equal(fi, first / V) and np.array_equal(ti, total / V) and fi.shape == (d,)
    fz, tz = sa.indices(u, np.zeros(d))
    assert np.array_equal(fz, np.zeros(d)) and np.array_equal(tz, np.zeros(d))
    fm, tm = sa.indices_many(U, np.array([[0.8, 0.0], [0.0, 0.0], [0.5, 0.5]]))
    assert fm.shape == tm.shape == (3, d) and np.all(fm[1] == 0) and np.all(tm[1] == 0) and fm[0, 0] > 0 and np.all(fm[2] > 0)
    assert fm[2].sum() <= 1 + 1e-9 <= tm[2].sum() + 2e-9
    # refusals
    with pytest.raises(ValueError, match="independent"):
        sa.variances(u, np.array([[1.0, 0.2], [0.2, 1.0]]))
    with pytest.raises(ValueError):
        sa.variances_many(U[:, :1], s)
    for cov, th in ((sk.MaternCovariance(2.5), theta), (sk.PeriodicCovariance(), np.concatenate([theta, np.log([3.0, 4.0, 0.5, 0.5])])),
                    (PlainGaussian(), theta)):
        other = sk.GaussianProcess(x, t, cov, th.copy())
        with pytest.raises(TypeError, match="GaussianCovariance"):
            sk.SensitivityAnalysis(other)
    with pytest.raises(TypeError):
        sk.SensitivityAnalysis(object())


def test_c_abi_refusals_leave_the_outputs_untouched():
    x, t = small_problem()
    theta = np.log(np.array([2.0, 0.01, 0.3, 0.1]))
    U = np.array([[4.5, 5.25], [1.0, 2.0]])
    lib = _gpx.lib

    def untouched(out):
        return all(np.all(a == FILL) for a in out.values())

    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    h = gp._dev().handle
    for bad in (np.array([[0.5, 0.5], [0.5, -1e-300]]), np.array([[0.5, np.nan], [0.5, 0.5]]), np.array([[np.inf, 0.5], [0.5, 0.5]])):
        st, out = sens(h, U, bad, status=True)
        assert st == GPX_ERR_BAD_ARG and untouched(out), (st, bad)
        assert "variances" in _gpx.last_error()
    st, out = sens(h, U, np.array([0.5, -2.0]), status=True)
    assert st == GPX_ERR_BAD_ARG and untouched(out)
    o = {k: np.full(s, FILL) for k, s in (("mean", 2), ("V", 2), ("first", (2, 2)), ("total", (2, 2)))}
    S = _gpx.f64(np.full((2, 2), 0.5))
    P = _gpx.ptr
    for args in ((None, P(S), 0, 2, P(o["mean"]), P(o["V"]), P(o["first"]), P(o["total"])),
                 (P(U), None, 0, 2, P(o["mean"]), P(o["V"]), P(o["first"]), P(o["total"])),
                 (P(U), P(S), 0, 2, None, P(o["V"]), P(o["first"]), P(o["total"])),
                 (P(U), P(S), 0, 2, P(o["mean"]), None, P(o["first"]), P(o["total"])),
                 (P(U), P(S), 0, 2, P(o["mean"]), P(o["V"]), None, P(o["total"])),
                 (P(U), P(S), 0, -1, P(o["mean"]), P(o["V"]), P(o["first"]), P(o["total"]))):
        assert lib.gpx_sensitivity_many(h, *args) == GPX_ERR_BAD_ARG
        assert untouched(o)
    assert lib.gpx_sensitivity_many(None, P(U), P(S), 0, 2, P(o["mean"]), P(o["V"]), P(o["first"]), P(o["total"])) == GPX_ERR_BAD_ARG
    assert lib.gpx_sensitivity_many(h, None, None, 0, 0, None, None, None, None) == 0          # b = 0 is a no-op
    assert untouched(o)
    # the kinds without the closed form: GPX_ERR_STATE, the text names the kernel
    for cov, th, word in ((sk.MaternCovariance(2.5), theta, "MaternCovariance"),
                          (sk.PeriodicCovariance(), np.concatenate([theta, np.log([3.0, 4.0, 0.5, 0.5])]), "PeriodicCovariance"),
                          (PlainGaussian(), theta, "gpx_fit_matrix")):
        other = sk.GaussianProcess(x, t, cov, th.copy())
        st, out = sens(other._dev().handle, U, S, status=True)
        assert st == GPX_ERR_STATE and untouched(out), (word, st)
        assert word in _gpx.last_error(), _gpx.last_error()
