"""gpx_sensitivity_anova_many and SensitivityAnalysis.anova* / shapley* / closed_variance on the device: every term
    D_S = sum_ij b_ij prod_{q in S} (E_q - M_q) prod_{q not in S} M_q
of the ANOVA decomposition of the predictor mean against the plain long-double evaluation of that definition over all pairs and all
masks (`anova_sums` below; notation of tests/_sensitivity_model.py), each sum on the scale sum |b_ij| prod_{q in S} (E_q + M_q)
prod_{q not in S} M_q, under 32 max(rho_ref, 1000 u) with rho_ref from the float64 evaluation of the same function (the project's one
rule, tests/_spgp_ld.py), on the device's OWN alpha.  Shapes (N, d): (260, 2) more than 256 columns; (129, 3) an odd split; (129, 8) the
full single tile, two pair groups; (130, 9) 16 x 32; (81, 10) 32 x 32; (57, 33) seven spread-out variances kept: a non-trivial slot map."""
import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _dense_ld as dl
import _sensitivity_model as sm
import _spgp_ld as sl
from test_sensitivity import FILL, GPX_ERR_BAD_ARG, GPX_ERR_STATE, chunk_of, fit, sens, small_problem
from test_sensitivity_second import second, second_sums

pytestmark = pytest.mark.gpu

SHAPES = [(260, 2), (129, 3), (129, 8), (130, 9), (81, 10), (57, 33)]
KEPT = [0, 5, 11, 16, 22, 27, 32]                            # the coordinates of d = 33 that keep their variance


def anova_sums(x, theta, beta, u, s, dt=dl.LD):
    """(values [2^na], scales [2^na]) of the definition over the pairs j <= i with weight 2 / 1; bit q of the index is the q-th
    coordinate with s > 0; entry 0 (no variance at all) is set to 0"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, _vt, w = dl.params(theta, d, dt)
    sg = np.asarray(s, dtype=np.float64).astype(dt)
    a = np.asarray(u, dtype=np.float64).astype(dt) - xr.astype(dt)
    be = np.asarray(beta, dtype=np.float64).astype(dt)
    ws = w * sg
    m = np.exp(-np.log1p(ws) / 2 - w * a * a / (1 + ws) / 2)                                    # [N, d]
    A, B = w * (1 + ws) / (1 + 2 * ws) / 2, w * w * sg / (1 + 2 * ws)
    i, j = np.tril_indices(N)
    b = (v * v) * be[i] * be[j] * np.where(i == j, 1.0, 2.0).astype(dt)
    val, sc = [b], [np.abs(b)]
    for k in range(d):
        M = m[i, k] * m[j, k]
        if not s[k] > 0:                                     # E_k = M_k: the factor of every term
            val, sc = [t * M for t in val], [t * M for t in sc]
            continue
        E = np.exp(-np.log1p(2 * ws[k]) / 2 - A[k] * (a[i, k] ** 2 + a[j, k] ** 2) + B[k] * a[i, k] * a[j, k])
        val = [t * M for t in val] + [t * (E - M) for t in val]                                 # the slot's bit clear, then set
        sc = [t * M for t in sc] + [t * (E + M) for t in sc]
    val, sc = np.array([t.sum() for t in val]), np.array([t.sum() for t in sc])
    val[0] = 0
    return val, sc


def anova(h, U, S, tstride, status=False):
    """[b, tstride] of gpx_sensitivity_anova_many; S [d] = one set for all inputs; the output enters holding FILL"""
    U, S = _gpx.f64(U), _gpx.f64(S)
    out = np.full((len(U), tstride), FILL)
    st = _gpx.lib.gpx_sensitivity_anova_many(h, _gpx.ptr(U), _gpx.ptr(S), int(S.ndim == 1), len(U), _gpx.ptr(out), tstride)
    if status:
        return st, out
    _gpx.check(st, "gpx_sensitivity_anova_many")
    return out


def judged(f, name, got, u, s):
    """a row of the call under the rule; returns (its 2^na terms, rho_ref, scales)"""
    want, scale = anova_sums(f.x, f.theta, f.alpha, u, s)
    ref = anova_sums(f.x, f.theta, f.alpha, u, s, dt=np.float64)[0]
    nt = len(want)
    ref_dist = {"anova": dl.distances(ref, want, scale)}
    rho = dl.rho_of(ref_dist)
    dist = {"anova": dl.distances(got[:nt], want, scale)}
    dl.record("anova " + name, f.name, rho, dist, ref_dist)
    assert np.all(np.isfinite(got)), (name, got)
    dl.assert_within(dist, rho, what="anova %s %s" % (name, f.name))
    assert got[0] == 0.0 and np.all(got[nt:] == 0.0), name
    return got[:nt], rho, scale


@pytest.mark.parametrize("N,d", SHAPES, ids=["n%d_d%d" % c for c in SHAPES])
def test_sums(N, d):
    with fit(N, d) as f:
        cs = sm.combos(f.x, f.theta, f.seed)
        one = np.zeros(d)
        one[d // 2] = cs[0][2][d // 2]
        cs.append(("between/one", cs[0][1], one))
        if d == 33:
            cs = [(cn, u, np.where(np.isin(np.arange(d), KEPT), s, 0.0)) for cn, u, s in cs]
        U, S = np.stack([u for _n, u, _s in cs]), np.stack([s for _n, _u, s in cs])
        ts = (1 << (len(KEPT) if d == 33 else d)) + 3
        out = anova(f.h, U, S, ts)
        for i, (cn, u, s) in enumerate(cs):
            judged(f, cn, out[i], u, s)
        # a refusal leaves the output as it was: a stride one short of the widest input's terms, a negative variance
        st, o = anova(f.h, U, S, ts - 4, status=True)
        assert st == GPX_ERR_BAD_ARG and np.all(o == FILL) and "tstride" in _gpx.last_error()
        S[-1, -1] = -1e-300
        st, o = anova(f.h, U, S, ts, status=True)
        assert st == GPX_ERR_BAD_ARG and np.all(o == FILL) and "variances" in _gpx.last_error()


def test_eleven_uncertain_coordinates_are_refused():
    with fit(57, 12) as f:
        s = sm.variances(12, f.seed)["drawn"]
        s[3] = 0.0
        u = dl.inputs_u(f.x, f.theta, f.seed)["between"]
        st, o = anova(f.h, np.stack([u, u]), np.stack([np.where(np.arange(12) < 10, s, 0.0), s]), 1 << 11, status=True)
        assert st == GPX_ERR_BAD_ARG and np.all(o == FILL) and "input 1" in _gpx.last_error() and "GPX_ANOVA_MAX_ACTIVE" in _gpx.last_error()


@pytest.mark.parametrize("N,d", [(129, 3), (130, 9)])
def test_the_decomposition_closes(N, d):
    """D_{k} = first_k, D_{k,l} = second_kl, sum_S D_S = V, sum_{S contains k} D_S = total_k against the existing calls on the same
    handle, each within the sum of the bounds of the sums involved"""
    with fit(N, d) as f:
        u = dl.inputs_u(f.x, f.theta, f.seed)["between"]
        s = sm.variances(d, f.seed)["drawn"]
        D, rhoA, scA = judged(f, "closes", anova(f.h, u[None, :], s, 1 << d)[0], u, s)
        out, sec = sens(f.h, u[None, :], s), second(f.h, u[None, :], s)[0]
        want, ref = sm.both(f.x, f.theta, f.alpha, u, s)
        rho1 = dl.rho_of({key: dl.distances(ref[key][0], want[key][0], want[key][1]) for key in ("V", "first", "total")})
        w2, sc2 = second_sums(f.x, f.theta, f.alpha, u, s)
        rho2 = dl.rho_of({"second": dl.distances(second_sums(f.x, f.theta, f.alpha, u, s, dt=np.float64)[0], w2, sc2)})
        bA, b1, b2 = sm.bound(rhoA), sm.bound(rho1), sm.bound(rho2)
        masks = np.arange(1 << d)
        worst = 0.0
        for k in range(d):
            has = (masks >> k & 1) == 1
            checks = [(D[1 << k], out["first"][0, k], bA * scA[1 << k] + b1 * want["first"][1][k]),
                      (D[has].sum(), out["total"][0, k], bA * scA[has].sum() + b1 * want["total"][1][k])]
            checks += [(D[1 << k | 1 << l], sec[k, l], bA * scA[1 << k | 1 << l] + b2 * sc2[k, l]) for l in range(k + 1, d)]
            for mine, theirs, allowed in checks:
                worst = max(worst, abs(mine - theirs) / float(allowed))
                assert abs(mine - theirs) <= allowed, (k, mine, theirs, allowed)
        allowed = bA * scA[1:].sum() + b1 * want["V"][1][0]
        print("N=%d d=%d: sum D_S = %.15g, V = %.15g, difference %.3e of the allowed %.3e; worst entry at %.3f of its allowance"
              % (N, d, D.sum(), out["V"][0], abs(D.sum() - out["V"][0]), allowed, worst))
        assert abs(D.sum() - out["V"][0]) <= allowed


@pytest.mark.parametrize("N,d", [(129, 8), (81, 10)])
def test_bits_do_not_depend_on_the_batch(N, d):
    with fit(N, d) as f:
        rng = np.random.RandomState(f.seed + 5)
        U = dl._grid(rng.uniform(1, 9, (9, d)))
        S = rng.uniform(0.01, 4.0, (9, d))
        S[1, :d - 3] = 0.0                                  # three active slots between neighbours with d: several variants share a chunk
        S[2] = 0.0                                          # none
        S[3, 0] = 0.0                                       # d - 1
        ts = 1 << d
        whole = anova(f.h, U, S, ts)
        assert np.all(whole[2] == 0.0) and np.all(whole[1, 8:] == 0.0) and np.all(whole[0, 1:] != 0.0)
        for i in range(4):
            assert np.array_equal(anova(f.h, U[i:i + 1], S[i:i + 1], ts)[0], whole[i]), i
        assert np.array_equal(anova(f.h, U[::-1], S[::-1], ts)[::-1], whole)
        with chunk_of(1):
            assert np.array_equal(anova(f.h, U, S, ts), whole)
        shared = anova(f.h, U, S[0], ts)
        assert np.array_equal(shared, anova(f.h, U, np.repeat(S[:1], 9, axis=0), ts)) and np.array_equal(shared[0], whole[0])


def check_methods(sa, h, u, s, alpha, x, theta):
    """anova / shapley / closed_variance of one input against the raw call's bits"""
    d = len(u)
    act = [k for k in range(d) if s[k] > 0]
    raw = anova(h, u[None, :], s, 1 << len(act))[0]
    terms = sa.anova(u, np.diag(s))
    keys = [tuple(act[q] for q in range(len(act)) if m >> q & 1) for m in range(1, 1 << len(act))]
    assert list(terms) == keys and np.array_equal(np.array(list(terms.values())), raw[1:]) and raw[-1] != 0.0
    assert sa.anova_many(np.stack([u, u]), s)[1] == terms
    wantA, scale = anova_sums(x, theta, alpha, u, s)
    rho = dl.rho_of({"anova": dl.distances(anova_sums(x, theta, alpha, u, s, dt=np.float64)[0], wantA, scale)})
    sh = sa.shapley(u, s)
    V = sa.variances(u, s)[1]
    want, ref = sm.both(x, theta, alpha, u, s)
    rho1 = dl.rho_of({"V": dl.distances(ref["V"][0], want["V"][0], want["V"][1])})
    assert sh.shape == (d,) and np.all(sh[s == 0] == 0.0) and np.array_equal(sa.shapley_many(u[None, :], s)[0], sh)
    assert abs(sh.sum() - V) <= sm.bound(rho) * scale[1:].sum() + sm.bound(rho1) * want["V"][1][0]
    assert sa.closed_variance(u, s, range(d)) == sum(raw[1:]) and sa.closed_variance(u, s, [act[0]]) == raw[1]
    assert sa.closed_variance(u, s, []) == 0.0


def test_python_methods():
    x, t = small_problem()
    theta = np.log(np.array([2.0, 0.01, 0.3, 0.1]))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    sa = sk.SensitivityAnalysis(gp)
    u, s = np.array([4.5, 5.25]), np.array([0.8, 0.3])
    check_methods(sa, gp._dev().handle, u, s, gp._get_beta(), x, theta)
    many = sa.anova_many(np.stack([u, u + 0.5, u - 1.0]), np.array([[0.8, 0.3], [0.0, 0.0], [0.0, 0.5]]))
    assert [list(m) for m in many] == [[(0,), (1,), (0, 1)], [], [(1,)]]
    with pytest.raises(NotImplementedError, match="[Gg]aussian"):
        sk.SensitivityAnalysis(gp, distribution="uniform").anova(u, s)
    with pytest.raises(ValueError):
        sa.anova_many(u[None, :1], s)
    assert _gpx.lib.gpx_sensitivity_anova_many(gp._dev().handle, None, None, 0, 0, None, 0) == 0          # b = 0 is a no-op
    other = sk.GaussianProcess(x, t, sk.MaternCovariance(2.5), theta.copy())
    st, o = anova(other._dev().handle, u[None, :], s, 4, status=True)
    assert st == GPX_ERR_STATE and np.all(o == FILL) and "MaternCovariance" in _gpx.last_error()
    rng = np.random.RandomState(3)
    wide = sk.GaussianProcess(dl._grid(rng.uniform(0, 10, (30, 11))), rng.randn(30), sk.GaussianCovariance(), np.log(np.r_[2.0, 0.01, np.full(11, 0.02)]))
    with pytest.raises(ValueError, match="GPX_ANOVA_MAX_ACTIVE"):
        sk.SensitivityAnalysis(wide).shapley(np.full(11, 5.0), np.full(11, 0.5))


def test_pseudo_handle():
    N, d, m = 300, 3, 40
    x, t, theta, _xs = sl.make_case(N, d, m, 0.03, 0.06, 0.3)
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), theta.copy())
    pgp = gp.pseudo_gp()
    try:
        u, s = dl._grid(np.array([4.0, 5.5, 3.25])), np.array([0.7, 0.0, 1.9])
        check_methods(sk.SensitivityAnalysis(pgp), pgp._dev().handle, u, s, pgp._get_beta(), pgp.x, pgp.theta_min)
    finally:
        pgp.close()
        gp.cov.clear_cache()
        _gpx.lib.gpx_pool_trim()
