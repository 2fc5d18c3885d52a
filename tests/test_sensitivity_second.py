"""gpx_sensitivity_second_many and SensitivityAnalysis.second_order* on the device: the pair interaction terms
    second_kl = sum_ij b_ij (prod_{q != k,l} m_iq m_jq) (E_k - m_ik m_jk) (E_l - m_il m_jl)
against the plain long-double evaluation of that definition over all pairs (`second_sums` below; notation of tests/_sensitivity_model.py),
each sum on the scale sum |b_ij| prod_{q != k,l}(m m) (E_k + M_k)(E_l + M_l), under 32 max(rho_ref, 1000 u) with rho_ref from the float64
evaluation of the same function (the project's one rule, tests/_spgp_ld.py).  Every sum is judged on the device's OWN alpha.

Shapes (N, d): (260, 2) four pair groups packed, more than 256 columns; (129, 3) an odd slot count; (129, 8) two groups packed; (130, 9) one
padded block; (81, 17) two blocks with the off-diagonal accumulator; (57, 33) three blocks -- N no multiple of 4, 8 or 16, several row blocks."""
import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _dense_ld as dl
import _sensitivity_model as sm
import _spgp_ld as sl
from test_sensitivity import FILL, GPX_ERR_BAD_ARG, GPX_ERR_STATE, chunk_of, fit, sens, small_problem

pytestmark = pytest.mark.gpu

SHAPES = [(260, 2), (129, 3), (129, 8), (130, 9), (81, 17), (57, 33)]


def second_sums(x, theta, beta, u, s, dt=dl.LD):
    """(values [d, d], scales [d, d]) of the definition over the pairs j <= i with weight 2 / 1; the diagonal stays 0"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, _vt, w = dl.params(theta, d, dt)
    sg = np.asarray(s, dtype=np.float64).astype(dt)
    a = np.asarray(u, dtype=np.float64).astype(dt) - xr.astype(dt)
    be = np.asarray(beta, dtype=np.float64).astype(dt)
    ws = w * sg
    m = np.exp(-np.log1p(ws) / 2 - w * a * a / (1 + ws) / 2)                                    # [N, d]
    A, B = w * (1 + ws) / (1 + 2 * ws) / 2, w * w * sg / (1 + 2 * ws)
    wgt = np.tril(np.full((N, N), 2.0)) - np.eye(N)
    b = (v * v) * np.outer(be, be) * wgt.astype(dt)
    M = np.stack([np.outer(m[:, k], m[:, k]) for k in range(d)])
    E = np.stack([np.exp(-np.log1p(2 * ws[k]) / 2 - A[k] * (a[:, k, None] ** 2 + a[None, :, k] ** 2) + B[k] * np.outer(a[:, k], a[:, k]))
                  for k in range(d)])
    val, sc = np.zeros((d, d), dt), np.zeros((d, d), dt)
    for k in range(d):
        others = [q for q in range(d) if q != k]
        suf = {}
        run = np.ones((N, N), dt)
        for q in reversed(others):                         # suf[q] = prod of M over the others after q
            suf[q] = run
            run = run * M[q]
        pre = np.ones((N, N), dt)                          # the product of M over the others before l
        for l in others:
            if l > k:
                loo = pre * suf[l]
                val[k, l] = val[l, k] = (b * loo * (E[k] - M[k]) * (E[l] - M[l])).sum()
                sc[k, l] = sc[l, k] = (np.abs(b) * loo * (E[k] + M[k]) * (E[l] + M[l])).sum()
            pre = pre * M[l]
    return val, sc


def second(h, U, S, status=False):
    """[b, d, d] of gpx_sensitivity_second_many; S [d] = one set for all inputs; the output enters holding FILL"""
    U, S = _gpx.f64(U), _gpx.f64(S)
    b, d = U.shape
    out = np.full((b, d, d), FILL)
    st = _gpx.lib.gpx_sensitivity_second_many(h, _gpx.ptr(U), _gpx.ptr(S), int(S.ndim == 1), b, _gpx.ptr(out))
    if status:
        return st, out
    _gpx.check(st, "gpx_sensitivity_second_many")
    return out


def two_active(s):
    out = np.zeros_like(s)
    out[[0, -1]] = s[[0, -1]]
    return out


def judged(f, name, got, u, s):
    """got [d, d] under the rule; returns (rho_ref, scales)"""
    want, scale = second_sums(f.x, f.theta, f.alpha, u, s)
    ref = second_sums(f.x, f.theta, f.alpha, u, s, dt=np.float64)[0]
    ref_dist = {"second": dl.distances(ref, want, scale)}
    rho = dl.rho_of(ref_dist)
    dist = {"second": dl.distances(got, want, scale)}
    dl.record("second order " + name, f.name, rho, dist, ref_dist)
    assert np.all(np.isfinite(got)), (name, got)
    dl.assert_within(dist, rho, what="second order %s %s" % (name, f.name))
    assert np.array_equal(got, got.T) and np.all(np.diagonal(got) == 0.0), name
    assert np.all(got[s == 0] == 0.0) and np.all(got[:, s == 0] == 0.0), name
    return rho, scale


@pytest.mark.parametrize("N,d", SHAPES, ids=["n%d_d%d" % c for c in SHAPES])
def test_sums(N, d):
    with fit(N, d) as f:
        cs = sm.combos(f.x, f.theta, f.seed)
        cs.append(("between/two", cs[0][1], two_active(cs[0][2])))
        out = second(f.h, np.stack([u for _n, u, _s in cs]), np.stack([s for _n, _u, s in cs]))
        for i, (cn, u, s) in enumerate(cs):
            judged(f, cn, out[i], u, s)
        # a refusal leaves the output as it was
        bad = np.stack([s for _n, _u, s in cs])
        bad[-1, -1] = -1e-300
        st, o = second(f.h, np.stack([u for _n, u, _s in cs]), bad, status=True)
        assert st == GPX_ERR_BAD_ARG and np.all(o == FILL) and "variances" in _gpx.last_error()


@pytest.mark.parametrize("N,d", [(129, 3), (130, 9)])
def test_two_active_coordinates_close_the_decomposition(N, d):
    """all but two variances zero: V = first_k + first_l + second_kl, within the sum of the three sums' bounds"""
    with fit(N, d) as f:
        u = dl.inputs_u(f.x, f.theta, f.seed)["between"]
        s = two_active(sm.variances(d, f.seed)["drawn"])
        k, l = 0, d - 1
        got = second(f.h, u[None, :], s)[0]
        rho2, scale2 = judged(f, "identity", got, u, s)
        got2 = got[k, l]
        out = sens(f.h, u[None, :], s)
        want, ref = sm.both(f.x, f.theta, f.alpha, u, s)
        rho1 = dl.rho_of({key: dl.distances(ref[key][0], want[key][0], want[key][1]) for key in ("V", "first")})
        allowed = sm.bound(rho2) * float(scale2[k, l]) + sm.bound(rho1) * float(want["V"][1][0] + want["first"][1][k] + want["first"][1][l])
        diff = abs((out["V"][0] - out["first"][0, k] - out["first"][0, l]) - got2)
        print("N=%d d=%d: V - first_k - first_l = %.15g, second_kl = %.15g, difference %.3e of the allowed %.3e"
              % (N, d, out["V"][0] - out["first"][0, k] - out["first"][0, l], got2, diff, allowed))
        assert diff <= allowed


@pytest.mark.parametrize("N,d", [(129, 8), (81, 17)])
def test_bits_do_not_depend_on_the_batch(N, d):
    with fit(N, d) as f:
        rng = np.random.RandomState(f.seed + 5)
        U = dl._grid(rng.uniform(1, 9, (9, d)))
        S = rng.uniform(0.01, 4.0, (9, d))
        S[1, :d - 3] = 0.0                                  # three active slots between neighbours with d: another kernel variant
        S[2] = 0.0                                          # none
        whole = second(f.h, U, S)
        assert np.all(whole[2] == 0.0)
        for i in range(4):
            assert np.array_equal(second(f.h, U[i:i + 1], S[i:i + 1])[0], whole[i]), i
        assert np.array_equal(second(f.h, U[::-1], S[::-1])[::-1], whole)
        with chunk_of(1):
            assert np.array_equal(second(f.h, U, S), whole)
        shared = second(f.h, U, S[0])
        assert np.array_equal(shared, second(f.h, U, np.repeat(S[:1], 9, axis=0))) and np.array_equal(shared[0], whole[0])


def test_pseudo_handle():
    N, d, m = 300, 3, 40
    x, t, theta, _xs = sl.make_case(N, d, m, 0.03, 0.06, 0.3)
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), theta.copy())
    pgp = gp.pseudo_gp()
    try:
        u, s = dl._grid(np.array([4.0, 5.5, 3.25])), np.array([0.7, 0.0, 1.9])
        got = sk.SensitivityAnalysis(pgp).second_order(u, s)
        assert got.shape == (d, d)
        f = type("PseudoFit", (), {"x": pgp.x, "theta": pgp.theta_min, "alpha": pgp._get_beta(), "name": "pseudo N=%d m=%d d=%d" % (N, m, d)})
        judged(f, "pseudo", got, u, s)
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
    u, s = np.array([4.5, 5.25]), np.array([0.8, 0.3])
    U = np.stack([u, u + 0.5, u - 1.0])
    S = np.array([[0.8, 0.3], [0.0, 0.0], [0.5, 0.0]])
    raw = second(gp._dev().handle, U, s)                   # meant plays no part: the raw call's bits
    many = sa.second_order_many(U, s)
    assert many.shape == (3, 2, 2) and np.array_equal(many, raw) and raw[0, 0, 1] > 0
    one = sa.second_order(u, np.diag(s))
    assert one.shape == (2, 2) and np.array_equal(one, raw[0])
    V = sa.variances_many(U, S)[1]
    per = sa.second_order_many(U, S)
    idx = sa.second_order_indices_many(U, S)
    assert idx.shape == (3, 2, 2) and np.array_equal(idx[0], per[0] / V[0]) and np.all(idx[1:] == 0.0) and V[1] == 0.0
    assert np.array_equal(sa.second_order_indices(u, s), idx[0])
    with pytest.raises(NotImplementedError, match="[Gg]aussian"):
        sk.SensitivityAnalysis(gp, distribution="uniform").second_order(u, s)
    with pytest.raises(ValueError):
        sa.second_order_many(U[:, :1], s)
    assert _gpx.lib.gpx_sensitivity_second_many(gp._dev().handle, None, None, 0, 0, None) == 0          # b = 0 is a no-op
    other = sk.GaussianProcess(x, t, sk.MaternCovariance(2.5), theta.copy())
    st, o = second(other._dev().handle, U, s, status=True)
    assert st == GPX_ERR_STATE and np.all(o == FILL) and "MaternCovariance" in _gpx.last_error()
