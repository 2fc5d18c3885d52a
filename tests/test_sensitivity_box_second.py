"""gpx_sensitivity_box_second_many and SensitivityAnalysis.second_order_box* on the device: the pair interaction terms under uniform inputs
    second_kl = sum_ij b_ij (prod_{q != k,l} m_iq m_jq) (E_k - m_ik m_jk) (E_l - m_il m_jl)
against the plain long-double evaluation of that definition over all pairs in the LINEAR domain (`second_sums` below: E and M as
tests/_sensitivity_box_model.py builds them, D from mpmath; the leave-two-out products as test_sensitivity_second.second_sums takes them),
each sum on the scale sum |b_ij| prod_{q != k,l}(m m) (E_k + M_k)(E_l + M_l), under 32 max(rho_ref, 1000 u) with rho_ref from the float64
evaluation of the same function.  Every sum is judged on the device's OWN alpha.  Shapes: those of test_sensitivity_second.py (every
kernel instance); boxes: those of test_sensitivity_box.py.  At most 77 k mpmath error-function pairs a box."""
import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _dense_ld as dl
import _sensitivity_box_model as bm
import _sensitivity_model as sm
import _spgp_ld as sl
from test_sensitivity import FILL, GPX_ERR_BAD_ARG, GPX_ERR_STATE, chunk_of, fit, small_problem
from test_sensitivity_box import box, boxes

pytestmark = pytest.mark.gpu

SHAPES = [(260, 2), (129, 3), (129, 8), (130, 9), (81, 17), (57, 33)]


def second_sums(x, theta, beta, lo, hi, dt=dl.LD):
    """(values [d, d], scales [d, d]) of the definition over the pairs j <= i with weight 2 / 1; the diagonal and the pinned coordinates stay 0"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, _vt, w = dl.params(theta, d, dt)
    D, pi = (bm._D_mp, bm.PI) if dt is dl.LD else (bm._D_f64, dt(np.pi))
    X, lo, hi = xr.astype(dt), np.asarray(lo, dtype=np.float64).astype(dt), np.asarray(hi, dtype=np.float64).astype(dt)
    L = hi - lo
    act = [int(k) for k in np.flatnonzero(L > 0)]
    be = np.asarray(beta, dtype=np.float64).astype(dt) * np.exp(-(w * (lo - X) ** 2)[:, L == 0].sum(1) / 2)
    ii, jj = np.tril_indices(N)
    b = (v * v) * be[ii] * be[jj] * np.where(ii == jj, 1.0, 2.0).astype(dt)
    E, M = {}, {}
    for k in act:
        r2, r = np.sqrt(w[k] / 2), np.sqrt(w[k])
        m = np.sqrt(pi / (2 * w[k])) / L[k] * D(r2 * (lo[k] - X[:, k]), r2 * L[k])
        mid = (X[ii, k] + X[jj, k]) / 2
        E[k] = np.exp(-w[k] * (X[ii, k] - X[jj, k]) ** 2 / 4) * (np.sqrt(pi / w[k]) / 2 / L[k]) * D(r * (lo[k] - mid), r * L[k])
        M[k] = m[ii] * m[jj]
    val, sc = np.zeros((d, d), dt), np.zeros((d, d), dt)
    for k in act:
        others = [q for q in act if q != k]
        suf, run = {}, np.ones(len(ii), dt)
        for q in reversed(others):                         # suf[q] = prod of M over the others after q
            suf[q] = run
            run = run * M[q]
        pre = np.ones(len(ii), dt)                         # the product of M over the others before l
        for l in others:
            if l > k:
                loo = pre * suf[l]
                val[k, l] = val[l, k] = (b * loo * (E[k] - M[k]) * (E[l] - M[l])).sum()
                sc[k, l] = sc[l, k] = (np.abs(b) * loo * (E[k] + M[k]) * (E[l] + M[l])).sum()
            pre = pre * M[l]
    return val, sc


def second(h, lo, hi, status=False):
    """[b, d, d] of gpx_sensitivity_box_second_many; lo, hi [d]: one box for the b = 3 inputs of a shared call; the output enters holding FILL"""
    lo, hi = _gpx.f64(lo), _gpx.f64(hi)
    b, d = (3, len(lo)) if lo.ndim == 1 else lo.shape
    out = np.full((b, d, d), FILL)
    st = _gpx.lib.gpx_sensitivity_box_second_many(h, _gpx.ptr(lo), _gpx.ptr(hi), int(lo.ndim == 1), b, _gpx.ptr(out))
    if status:
        return st, out
    _gpx.check(st, "gpx_sensitivity_box_second_many")
    return out


def shape_of(got, lo, hi, name):
    assert np.all(np.isfinite(got)), (name, got)
    assert np.array_equal(got, got.T) and np.all(np.diagonal(got) == 0.0), name
    assert np.all(got[lo == hi] == 0.0) and np.all(got[:, lo == hi] == 0.0), name


def judged(f, name, got, lo, hi):
    """got [d, d] under the rule; returns (rho_ref, scales)"""
    want, scale = second_sums(f.x, f.theta, f.alpha, lo, hi)
    ref = second_sums(f.x, f.theta, f.alpha, lo, hi, dt=np.float64)[0]
    ref_dist = {"second": dl.distances(ref, want, scale)}
    rho = dl.rho_of(ref_dist)
    dist = {"second": dl.distances(got, want, scale)}
    dl.record("box second order " + name, f.name, rho, dist, ref_dist)
    shape_of(got, lo, hi, name)
    dl.assert_within(dist, rho, what="box second order %s %s" % (name, f.name))
    return rho, scale


@pytest.mark.parametrize("which", range(6), ids=["bounding", "equal", "outside", "pinned", "narrow", "wide"])
@pytest.mark.parametrize("N,d", SHAPES, ids=["n%d_d%d" % c for c in SHAPES])
def test_sums(N, d, which):
    """one box a case: its long-double model is what takes the time (3 to 4 s)"""
    with fit(N, d) as f:
        name, lo, hi = boxes(f.x, f.theta)[which]
        got = second(f.h, lo[None, :], hi[None, :])[0]
        if name == "outside":              # every m is 1e-197 and below, every E below the double range: zeros, and no NaN comes of the logs
            shape_of(got, lo, hi, name)
            assert np.all(np.abs(got) <= 1e-190), got
        else:
            judged(f, name, got, lo, hi)


def test_a_refusal_leaves_the_output_untouched():
    with fit(129, 3) as f:
        bs = boxes(f.x, f.theta)
        LO, HI = np.stack([lo for _n, lo, _h in bs]), np.stack([hi for _n, _l, hi in bs])
        HI[-1, -1] = LO[-1, -1] - 1e-3
        st, o = second(f.h, LO, HI, status=True)
        assert st == GPX_ERR_BAD_ARG and np.all(o == FILL) and "bounds" in _gpx.last_error()


@pytest.mark.parametrize("N,d", [(129, 3), (130, 9)])
def test_two_active_coordinates_close_the_decomposition(N, d):
    """all but two coordinates pinned: V = first_k + first_l + second_kl, within the sum of the three sums' bounds"""
    with fit(N, d) as f:
        lo = dl.inputs_u(f.x, f.theta, f.seed)["between"] - 1.0
        hi = lo.copy()
        k, l = 0, d - 1
        hi[[k, l]] += 2.0
        got = second(f.h, lo[None, :], hi[None, :])[0]
        rho2, scale2 = judged(f, "identity", got, lo, hi)
        out = box(f.h, lo[None, :], hi[None, :], quad=False)
        want, ref = bm.sums(f.x, f.theta, f.alpha, None, lo, hi), bm.sums(f.x, f.theta, f.alpha, None, lo, hi, dt=np.float64)
        rho1 = dl.rho_of({key: dl.distances(ref[key][0], want[key][0], want[key][1]) for key in ("V", "first")})
        allowed = sm.bound(rho2) * float(scale2[k, l]) + sm.bound(rho1) * float(want["V"][1][0] + want["first"][1][k] + want["first"][1][l])
        rest = out["V"][0] - out["first"][0, k] - out["first"][0, l]
        print("N=%d d=%d: V - first_k - first_l = %.15g, second_kl = %.15g, difference %.3e of the allowed %.3e"
              % (N, d, rest, got[k, l], abs(rest - got[k, l]), allowed))
        assert got[k, l] != 0.0 and abs(rest - got[k, l]) <= allowed


@pytest.mark.parametrize("N,d", [(129, 8), (81, 17)])
def test_bits_do_not_depend_on_the_batch(N, d):
    with fit(N, d) as f:
        rng = np.random.RandomState(f.seed + 5)
        LO = dl._grid(rng.uniform(1, 6, (9, d)))
        HI = LO + dl._grid(rng.uniform(0.5, 4.0, (9, d)))
        HI[1, :d - 3] = LO[1, :d - 3]                       # three active slots between neighbours with d: another kernel instance
        HI[2] = LO[2]                                       # none
        whole = second(f.h, LO, HI)
        assert np.all(whole[2] == 0.0) and np.all(whole[1][d - 3:, d - 3:][~np.eye(3, dtype=bool)] != 0.0)
        for i in range(4):
            assert np.array_equal(second(f.h, LO[i:i + 1], HI[i:i + 1])[0], whole[i]), i
        assert np.array_equal(second(f.h, LO[::-1], HI[::-1])[::-1], whole)
        with chunk_of(1):
            assert np.array_equal(second(f.h, LO, HI), whole)
        shared = second(f.h, LO[0], HI[0])
        assert np.array_equal(shared, second(f.h, np.repeat(LO[:1], 3, axis=0), np.repeat(HI[:1], 3, axis=0))) and np.array_equal(shared[0], whole[0])


def test_pseudo_handle():
    N, d, m = 300, 3, 40
    x, t, theta, _xs = sl.make_case(N, d, m, 0.03, 0.06, 0.3)
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), theta.copy())
    pgp = gp.pseudo_gp()
    try:
        lo, hi = np.array([2.0, 3.0, 1.0]), np.array([7.0, 3.0, 9.0])
        got = sk.SensitivityAnalysis(pgp).second_order_box(lo, hi)
        assert got.shape == (d, d)
        f = type("PseudoFit", (), {"x": pgp.x, "theta": pgp.theta_min, "alpha": pgp._get_beta(), "name": "pseudo N=%d m=%d d=%d" % (N, m, d)})
        judged(f, "pseudo", got, lo, hi)
        assert got[0, 2] != 0.0
    finally:
        pgp.close()
        gp.cov.clear_cache()
        _gpx.lib.gpx_pool_trim()


def test_python_methods():
    x, t = small_problem()
    theta = np.log(np.array([2.0, 0.01, 0.3, 0.1]))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    sa = sk.SensitivityAnalysis(gp)
    LO, HI = np.array([[3.0, 4.0], [1.0, 2.0], [5.0, 5.0]]), np.array([[6.0, 6.5], [1.0, 2.0], [7.0, 5.0]])
    raw = second(gp._dev().handle, LO, HI)
    many = sa.second_order_box_many(LO, HI)
    assert many.shape == (3, 2, 2) and np.array_equal(many, raw) and raw[0, 0, 1] > 0 and np.all(raw[1:] == 0.0)
    one = sa.second_order_box(LO[0], HI[0])
    assert one.shape == (2, 2) and np.array_equal(one, raw[0])
    V = sa.variances_box_many(LO, HI)[1]
    idx = sa.second_order_indices_box_many(LO, HI)
    assert idx.shape == (3, 2, 2) and np.array_equal(idx[0], raw[0] / V[0]) and np.all(idx[1:] == 0.0) and V[1] == 0.0
    assert np.array_equal(sa.second_order_indices_box(LO[0], HI[0]), idx[0])
    assert np.array_equal(sk.SensitivityAnalysis(gp, distribution="uniform").second_order_box(LO[0], HI[0]), one)
    with pytest.raises(ValueError):
        sa.second_order_box_many(LO, HI[:, ::-1] - 5.0)
    assert _gpx.lib.gpx_sensitivity_box_second_many(gp._dev().handle, None, None, 0, 0, None) == 0      # b = 0 is a no-op
    other = sk.GaussianProcess(x, t, sk.MaternCovariance(2.5), theta.copy())
    st, o = second(other._dev().handle, LO, HI, status=True)
    assert st == GPX_ERR_STATE and np.all(o == FILL) and "MaternCovariance" in _gpx.last_error()
