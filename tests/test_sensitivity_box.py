"""gpx_sensitivity_box_many, SensitivityAnalysis(distribution="uniform") and UncertaintyPropagationUniform on the device: the variance
decomposition of the predictor mean, its mean and E[k^T K^-1 k] under independent uniform inputs against the model of
tests/_sensitivity_box_model.py (mpmath erf at 30 digits, long double sums), each sum on the scale of its own absolute terms, under
32 max(rho_ref, 1000 u) with rho_ref from the float64 scipy evaluation of the same case (the project's one rule, tests/_dense_ld.py).
Every sum is judged on the device's OWN alpha and K^-1.

Shapes: d = 1, 3, 8, 9, 17 -- one slot, one sweep, a full sweep, two sweeps with one slot in the second, three sweeps.  N is what the mpmath
model evaluates in a few seconds (N^2 d / 2 erf differences a box): 260 at d = 1 (npad 384: two build blocks, whose partials make the
mean, and a second pass of the pair kernel's 256 lanes over the columns), 129 at d = 1 and 3, 81 at d = 8 and 9, 57 at d = 17, none a
multiple of the 8 rows of a row block."""
import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _dense_ld as dl
import _sensitivity_box_model as bm
import _spgp_ld as sl
from test_sensitivity import FILL, GPX_ERR_BAD_ARG, GPX_ERR_STATE, chunk_of, fit, small_problem

pytestmark = pytest.mark.gpu

SHAPES = [(260, 1), (129, 1), (129, 3), (81, 8), (81, 9), (57, 17)]
THETA2 = np.log(np.array([2.0, 0.01, 0.3, 0.1]))


def box(h, lo, hi, total=True, quad=True, status=False):
    """{"mean", "V", "first", "total", "quad"} of gpx_sensitivity_box_many; lo, hi [d]: one box for the b = 3 inputs of a shared call;
    the outputs enter holding FILL"""
    lo, hi = _gpx.f64(lo), _gpx.f64(hi)
    b, d = (3, len(lo)) if lo.ndim == 1 else lo.shape
    out = {"mean": np.full(b, FILL), "V": np.full(b, FILL), "first": np.full((b, d), FILL), "total": np.full((b, d), FILL), "quad": np.full(b, FILL)}
    st = _gpx.lib.gpx_sensitivity_box_many(h, _gpx.ptr(lo), _gpx.ptr(hi), int(lo.ndim == 1), b, _gpx.ptr(out["mean"]), _gpx.ptr(out["V"]),
                                           _gpx.ptr(out["first"]), _gpx.ptr(out["total"]) if total else None, _gpx.ptr(out["quad"]) if quad else None)
    if status:
        return st, out
    _gpx.check(st, "gpx_sensitivity_box_many")
    return out


def boxes(x, theta):
    """[(name, lo, hi)]: around the data's bounding box; lo bit-equal to training row 5; wholly outside by 30 / sqrt(w); zero width in every
    other coordinate; width 1e-6 / sqrt(w); width 200 / sqrt(w)"""
    d = x.shape[1]
    sw = np.sqrt(dl.params(theta, d, np.float64)[2])
    mid = dl._grid(np.random.RandomState(d).uniform(3, 7, d))
    pin_hi = mid + 1.0
    pin_hi[::2] = (mid - 1.0)[::2]
    return [("bounding", x.min(0) - 0.5, x.max(0) + 0.5), ("equal", x[dl.QUIRK_ROW].copy(), x[dl.QUIRK_ROW] + 3.0),
            ("outside", x.max(0) + 30.0 / sw, x.max(0) + 30.0 / sw + 1.0), ("pinned", mid - 1.0, pin_hi), ("narrow", mid, mid + 1e-6 / sw),
            ("wide", 5.0 - 100.0 / sw, 5.0 + 100.0 / sw)]


def check(title, got, want, ref):
    ref_dist = {k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in got}
    rho = dl.rho_of(ref_dist)
    dist = {k: dl.distances(g, want[k][0], want[k][1]) for k, g in got.items()}
    dl.record("sensitivity box", title, rho, dist, ref_dist)
    dl.assert_within(dist, rho, what=title)


def one(out, i):
    return {k: (a[i] if a.ndim == 2 else a[i:i + 1]) for k, a in out.items()}


def against_model(title, x, theta, beta, Kinv, out, i, lo, hi):
    args = (x, theta, beta, Kinv, lo, hi)
    check(title, one(out, i), bm.sums(*args), bm.sums(*args, dt=np.float64))


@pytest.mark.parametrize("N,d", SHAPES, ids=["n%d_d%d" % c for c in SHAPES])
def test_sums(N, d):
    with fit(N, d) as f:
        bs = boxes(f.x, f.theta)
        out = box(f.h, np.stack([lo for _n, lo, _h in bs]), np.stack([hi for _n, _l, hi in bs]))
        Kinv = f.model.kinv()
        for i, (name, lo, hi) in enumerate(bs):
            got = one(out, i)
            assert all(np.all(np.isfinite(g)) for g in got.values()), (name, got)
            if name == "outside":          # every m carries erfc(30 / sqrt(2)) = 1e-197, every E erfc(30) = 1e-393 < the double range: no NaN comes of either
                assert all(np.all(np.abs(g) <= 1e-190) for g in got.values()), got
                continue
            against_model("%s N=%d d=%d" % (name, N, d), f.x, f.theta, f.alpha, Kinv, out, i, lo, hi)
            for key in ("first", "total"):
                assert np.all(got[key][lo == hi] == 0.0), (name, key, got[key])


def test_null_outputs_shared_box_and_chunking_keep_the_bits():
    with fit(129, 9) as f:
        bs = boxes(f.x, f.theta)
        LO, HI = np.stack([lo for _n, lo, _h in bs]), np.stack([hi for _n, _l, hi in bs])
        full = box(f.h, LO, HI)
        for kw, keys in (({"total": False}, ("mean", "V", "first", "quad")), ({"quad": False}, ("mean", "V", "first", "total")),
                         ({"total": False, "quad": False}, ("mean", "V", "first"))):
            part = box(f.h, LO, HI, **kw)
            for k in part:
                assert np.array_equal(part[k], full[k] if k in keys else np.full_like(full[k], FILL)), (kw, k)
        with chunk_of(1):
            one_by_one = box(f.h, LO, HI)
        shared = box(f.h, LO[0], HI[0])
        dev = [torch.tensor(a, device="cuda") for a in (LO, HI)]     # the bounds in device memory
        torch.cuda.synchronize()
        o = box(f.h, LO, HI)
        st = _gpx.lib.gpx_sensitivity_box_many(f.h, dev[0].data_ptr(), dev[1].data_ptr(), 0, len(LO), *[_gpx.ptr(o[k]) for k in bm.KEYS])
        assert st == 0
        for k in full:
            assert np.array_equal(one_by_one[k], full[k]) and np.array_equal(o[k], full[k]), k
            assert np.array_equal(shared[k], np.repeat(full[k][:1], 3, axis=0)), k


def test_argument_errors_leave_the_outputs_untouched():
    x, t = small_problem()
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), THETA2.copy())
    h = gp._dev().handle
    lo, hi = np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([[2.0, 2.0], [3.5, 6.0]])
    for at, val in (((1, 0), 2.9), ((0, 1), np.nan), ((1, 1), np.inf)):
        bad = hi.copy()
        bad[at] = val
        st, out = box(h, lo, bad, status=True)
        assert st == GPX_ERR_BAD_ARG and all(np.all(a == FILL) for a in out.values()), (at, val, st)
    o = box(h, lo, hi)
    P = _gpx.ptr
    for args in ((None, P(hi)) + tuple(P(o[k]) for k in bm.KEYS), (P(lo), P(hi), None) + tuple(P(o[k]) for k in bm.KEYS[1:])):
        assert _gpx.lib.gpx_sensitivity_box_many(h, args[0], args[1], 0, 2, *args[2:]) == GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_sensitivity_box_many(h, None, None, 0, 0, None, None, None, None, None) == 0
    other = sk.GaussianProcess(x, t, sk.MaternCovariance(2.5), THETA2.copy())
    st, out = box(other._dev().handle, lo, hi, status=True)
    assert st == GPX_ERR_STATE and "MaternCovariance" in _gpx.last_error() and all(np.all(a == FILL) for a in out.values())


def test_pseudo_handle():
    N, d, m = 300, 3, 40
    x, t, theta, _xs = sl.make_case(N, d, m, 0.03, 0.06, 0.3)
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), theta.copy())
    pgp = gp.pseudo_gp()
    try:
        lo, hi = np.array([[2.0, 3.0, 1.0], [4.0, 4.0, 4.0]]), np.array([[7.0, 3.0, 9.0], [4.5, 6.0, 5.0]])
        out = box(pgp._dev().handle, lo, hi)
        for i in range(2):
            against_model("pseudo input %d N=%d m=%d d=%d" % (i, N, m, d), pgp.x, pgp.theta_min, pgp._get_beta(), pgp.Kinv, out, i, lo[i], hi[i])
        assert out["first"][0, 1] == 0.0 and out["total"][0, 1] == 0.0
    finally:
        pgp.close()
        gp.cov.clear_cache()
        _gpx.lib.gpx_pool_trim()


def test_python_classes():
    x, t = small_problem()
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), THETA2.copy())
    u, s = np.array([4.5, 5.25]), np.array([0.8, 0.0])
    lo, hi = u - np.sqrt(3 * s), u + np.sqrt(3 * s)
    raw = box(gp._dev().handle, lo[None, :], hi[None, :])
    prior = gp._get_v() + gp._get_vt()
    mean, var = sk.UncertaintyPropagationUniform(gp).propagate_GA(u, np.diag(s))
    assert mean == raw["mean"][0] + gp.meant and var == raw["V"][0] + prior - raw["quad"][0]
    many = sk.UncertaintyPropagationUniform(gp).propagate_GA_many(np.stack([u, u + 1.0]), s)
    assert many[0][0] == mean and many[1][0] == var and many[0].shape == many[1].shape == (2,)
    assert sk.UncertaintyPropagationUniform(gp).propagate_mean(u, s) == mean
    with pytest.raises(ValueError, match="independent"):
        sk.UncertaintyPropagationUniform(gp).propagate_GA(u, np.array([[1.0, 0.2], [0.2, 1.0]]))
    sa = sk.SensitivityAnalysis(gp, distribution="uniform")
    for got in (sa.variances(u, s), sa.variances_box(lo, hi), [a[0] for a in sa.variances_box_many(lo[None, :], hi[None, :])]):
        assert got[0] == mean and got[1] == raw["V"][0] and np.array_equal(got[2], raw["first"][0]) and np.array_equal(got[3], raw["total"][0])
    fi, ti = sa.indices_box(lo, hi)
    assert np.array_equal(fi, raw["first"][0] / raw["V"][0]) and np.array_equal(ti, raw["total"][0] / raw["V"][0]) and fi[1] == 0.0
    assert np.array_equal(sa.indices(u, s)[0], fi) and np.array_equal(sa.indices_box_many(lo[None, :], hi[None, :])[1][0], ti)
    # the default distribution is the Gaussian call, untouched
    assert sk.SensitivityAnalysis(gp).variances(u, s)[1] != raw["V"][0]


def gaussian_law(x, theta, beta, Kinv, u, s):
    """(mean, variance) of the GP output under x_k ~ N(u_k, s_k) in long double, from the per-coordinate factors of include/gpx.h"""
    d = x.shape[1]
    v, vt, w = dl.params(theta, d)
    a = u.astype(dl.LD) - x.astype(dl.LD)
    ws = w * s.astype(dl.LD)
    g = np.exp((-np.log1p(ws) / 2 - w * a * a / (1 + ws) / 2).sum(1))
    lE = (-np.log1p(2 * ws) / 2 - w * (a[:, None, :] - a[None, :, :]) ** 2 / 4 - w * (a[:, None, :] + a[None, :, :]) ** 2 / (1 + 2 * ws) / 4).sum(2)
    be = beta.astype(dl.LD)
    mean = v * (be * g).sum()
    return mean, (v + vt) + (v * v) * ((np.outer(be, be) - Kinv.astype(dl.LD)) * np.exp(lE)).sum() - mean * mean


@pytest.mark.parametrize("s0", [0.4, 0.1])
def test_convergence_to_the_gaussian_law(s0):
    """Uniform and Gaussian inputs of equal mean and variance share their first three moments: the two variances differ by the fourth
    (kurtosis 1.8 against 3) and beyond, O(s^2).  The allowed difference is TWICE the difference of the two long-double models at this size,
    computed here from the definitions, not from the device: 2 * 1.42e-3 at s = 0.4 and 2 * 9.4e-5 at s = 0.1 (a factor 15 for a factor 4
    in s; the rounding of either variance, 1e-13 beside a prior of 2.01, is far below both)."""
    x, t = small_problem()
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), THETA2.copy())
    u, s = np.array([4.5, 5.25]), np.full(2, s0)
    beta, Kinv = gp._dev().alpha(), gp._dev().kinv()
    half = np.sqrt(3 * s)
    w = bm.sums(x, THETA2, beta, Kinv, u - half, u + half)
    v, vt, _w = dl.params(THETA2, 2)
    var_uniform = w["V"][0][0] + (v + vt) - w["quad"][0][0]
    tol = 2 * abs(float(var_uniform - gaussian_law(x, THETA2, beta, np.tril(Kinv) + np.tril(Kinv, -1).T, u, s)[1]))
    got = abs(sk.UncertaintyPropagationUniform(gp).propagate_GA(u, np.diag(s))[1] - sk.UncertaintyPropagationExact(gp).propagate_GA(u, np.diag(s))[1])
    print("s = %g: |uniform - Gaussian| %.6e, allowed %.6e" % (s0, got, tol))
    assert 0 < got <= tol        # tol = 2 |model difference|: 2.8e-3 at s = 0.4, 1.9e-4 at s = 0.1
