"""gpx_sensitivity_post_many and SensitivityAnalysis(..., posterior=True): var_post, first_post, total_post (include/gpx.h) against the plain
long-double evaluation of the formulas over ALL pairs (`model`), each on the scale of its absolute terms -- the prior constant plus v^2 sum
|W_ij| (.)(E + m) -- under 32 max(rho_ref, 1000 u), rho_ref from the float64 evaluation of the same function (the project's one rule,
tests/_spgp_ld.py), on the device's OWN K^-1.  Shapes: (260, 2) > 256 columns; (129, 8) N no multiple of SEN_R; (130, 9), (81, 17) 2, 3 sweeps."""
import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _dense_ld as dl
import _sensitivity_model as sm
import _spgp_ld as sl
from test_sensitivity import FILL, GPX_ERR_BAD_ARG, GPX_ERR_STATE, chunk_of, fit, sens, small_problem

SHAPES = [(260, 2), (129, 8), (130, 9), (81, 17)]


def model(x, theta, W, u, s, dt=dl.LD):
    """{"var": ([1], [1]), "first": ([d], [d]), "total": ([d], [d])}, each (values, scales): the prior constant - v^2 sum_ij W_ij (...)"""
    xr, d = np.asarray(x, dtype=np.float64), np.shape(x)[1]
    v, _vt, w = dl.params(theta, d, dt)
    ws = w * np.asarray(s, dtype=np.float64).astype(dt)
    a = np.asarray(u, dtype=np.float64).astype(dt) - xr.astype(dt)
    lm, lr = -np.log1p(ws) / 2 - w * a * a / (1 + ws) / 2, -np.log1p(2 * ws) / 2
    dm, sp = a[:, None, :] - a[None, :, :], a[:, None, :] + a[None, :, :]
    E, M = np.exp(lr - w * dm * dm / 4 - w * sp * sp / (1 + 2 * ws) / 4), np.exp(lm[:, None, :] + lm[None, :, :])
    Wv = (v * v) * np.asarray(W, dtype=np.float64).astype(dt)
    cV, PE, PM = -v * np.expm1(lr.sum()), E.prod(2), M.prod(2)
    out = {"var": (np.array([cV - (Wv * (PE - PM)).sum()], dt), np.array([cV + (np.abs(Wv) * (PE + PM)).sum()], dt)),
           "first": (np.empty(d, dt), np.empty(d, dt)), "total": (np.empty(d, dt), np.empty(d, dt))}
    for k in range(d):
        D, S = E[:, :, k] - M[:, :, k], E[:, :, k] + M[:, :, k]
        for key, F, c in (("first", M, -v * np.exp(lr.sum() - lr[k]) * np.expm1(lr[k])), ("total", E, -v * np.expm1(lr[k]))):
            loo = np.delete(F, k, axis=2).prod(2)
            out[key][0][k], out[key][1][k] = c - (Wv * loo * D).sum(), c + (np.abs(Wv) * loo * S).sum()
    return out


def test_model_is_the_definitions():
    """the model against tensor Gauss-Hermite quadrature (80 nodes; one for a coordinate with s = 0) of the definitions for the residual g of
    covariance c*(x, x') = c(x, x') - c(x)^T W c(x'): E[c*(x, x)] - E[c*(x, x')], and the same with x_k or x_~k shared, to 1e-12 of the scale"""
    z, q = (a.astype(dl.LD) / (1 if i == 0 else a.sum()) for i, a in enumerate(np.polynomial.hermite_e.hermegauss(80)))
    for d, s in ((1, [0.6]), (2, [0.5, 0.0]), (3, [0.7, 0.0, 0.3])):
        rng, N = np.random.RandomState(40 + d), 7 + d
        x, u = rng.uniform(0, 4, (N, d)), rng.uniform(1, 3, d)
        theta, W = np.log(np.concatenate([[1.7, 0.01], rng.uniform(0.2, 0.6, d)])), rng.randn(N, N)
        W = (W + W.T).astype(dl.LD)
        v, _vt, w = dl.params(theta, d)
        axes = [(dl.LD(u[k]) + np.sqrt(dl.LD(s[k])) * z, q) if s[k] > 0 else (np.array([u[k]], dl.LD), np.ones(1, dl.LD)) for k in range(d)]
        C = v * np.ones([len(ax[0]) for ax in axes] + [N], dl.LD)                                        # c_i on the tensor grid
        for k, (nodes, _q) in enumerate(axes):
            C = C * np.exp(-w[k] * (nodes[:, None] - x[:, k].astype(dl.LD)[None, :]) ** 2 / 2).reshape([-1 if l == k else 1 for l in range(d)] + [N])
        r = [(ax[1][:, None] * ax[1][None, :] * np.exp(-w[k] * (ax[0][:, None] - ax[0][None, :]) ** 2 / 2)).sum() for k, ax in enumerate(axes)]
        every = list(range(d))

        def mean_over(T, ks):                                     # the expectation over the coordinates ks of a grid tensor [..., N]
            for k in ks:
                T = (T * axes[k][1].reshape([-1 if l == k else 1 for l in range(d)] + [1])).sum(k, keepdims=True)
            return T

        def form(T, ks):                                          # E over the coordinates ks (kept by T) of T^T W T
            return mean_over(np.einsum("...i,ij,...j->...", T, W, T)[..., None], ks).ravel()[0]

        same, apart = v - form(C, every), v * np.prod(r) - form(mean_over(C, every), [])
        got = model(x, theta, W, u, np.array(s))
        for k in range(d):
            rest = [l for l in every if l != k]
            quad = {"var": same - apart, "first": v * np.prod([r[l] for l in rest]) - form(mean_over(C, rest), [k]) - apart,
                    "total": same - (v * r[k] - form(mean_over(C, [k]), rest))}
            for key, want in quad.items():
                err = float(abs(got[key][0][0 if key == "var" else k] - want) / got[key][1][0 if key == "var" else k])
                print("d=%d k=%d %s: model against quadrature %.3e of the scale" % (d, k, key, err))
                assert err <= 1e-12, (d, k, key, err)


def post(h, U, S, total=True, status=False):
    """the seven outputs of gpx_sensitivity_post_many by name; S [d] = one set for all inputs; the outputs enter holding FILL"""
    U, S = _gpx.f64(U), _gpx.f64(S)
    out = {k: np.full(U.shape if k[0] in "ft" else len(U), FILL) for k in ("mean", "V", "first", "total", "var_post", "first_post", "total_post")}
    P = {k: _gpx.ptr(a) for k, a in out.items()}
    st = _gpx.lib.gpx_sensitivity_post_many(h, _gpx.ptr(U), _gpx.ptr(S), int(S.ndim == 1), len(U), P["mean"], P["V"], P["first"], P["total"] if total else None,
                                            P["var_post"], P["first_post"], P["total_post"] if total else None)
    if status:
        return st, out
    _gpx.check(st, "gpx_sensitivity_post_many")
    if not total:
        assert np.all(out.pop("total") == FILL) and np.all(out.pop("total_post") == FILL)
    return out


def judged(x, theta, what, name, out, i, Kinv, u, s):
    """input i of `out` under the rule, then the inequalities within bound x scale; returns (bound, {key: values}, {key: scales})"""
    got = {k: np.atleast_1d(out[k + "_post"][i]) for k in ("var", "first", "total") if k + "_post" in out}
    want, ref = model(x, theta, Kinv, u, s), model(x, theta, Kinv, u, s, dt=np.float64)
    ref_dist, dist = ({k: dl.distances(o[k], want[k][0], want[k][1]) for k in got} for o in ({k: r[0] for k, r in ref.items()}, got))
    rho = dl.rho_of(ref_dist)
    dl.record("sensitivity post " + name, what, rho, dist, ref_dist)
    dl.assert_within(dist, rho, what="sensitivity post %s %s" % (name, what))
    lim, sc = sm.bound(rho), {k: np.asarray(want[k][1], dtype=np.float64) for k in got}
    assert all(np.all(g >= -lim * sc[k]) for k, g in got.items()), (name, got)
    assert got["first"].sum() <= got["var"][0] + lim * (sc["first"].sum() + sc["var"][0]), (name, got)
    assert "total" not in got or got["var"][0] <= got["total"].sum() + lim * (sc["total"].sum() + sc["var"][0]), (name, got)
    assert all(np.all(got[k][s == 0] == 0.0) for k in got if k != "var"), (name, got)
    return lim, got, sc


@pytest.mark.gpu
@pytest.mark.parametrize("total", [True, False], ids=["total", "first_only"])
@pytest.mark.parametrize("N,d", SHAPES, ids=["n%d_d%d" % c for c in SHAPES])
def test_sums(N, d, total):
    with fit(N, d) as f:
        cs = sm.combos(f.x, f.theta, f.seed)
        U, S = np.stack([u for _n, u, _s in cs]), np.stack([s for _n, _u, s in cs])
        out, Kinv, base = post(f.h, U, S, total), f.model.kinv(), sens(f.h, U, S, total)
        assert all(np.array_equal(out[k], base[k]) for k in base), "the mean part is gpx_sensitivity_many's, bit for bit"
        for i, (cn, u, s) in enumerate(cs):
            judged(f.x, f.theta, f.name, cn, out, i, Kinv, u, s)
        assert all(np.all(o == 0.0) for k, o in post(f.h, U[:1], np.zeros(d), total).items() if k != "mean")


@pytest.mark.gpu
@pytest.mark.parametrize("N,d", [(129, 8), (81, 17)])
def test_bits_do_not_depend_on_the_batch_the_chunking_s_shared_or_the_totals(N, d):
    with fit(N, d) as f:
        rng = np.random.RandomState(f.seed + 5)
        U, S = dl._grid(rng.uniform(1, 9, (130, d))), rng.uniform(0.01, 4.0, (130, d))
        S[1, ::2], S[2] = 0.0, 0.0
        whole = post(f.h, U, S)
        with chunk_of(7):
            chunked = post(f.h, U, S)
        alone, without, shared = post(f.h, U[77:78], S[77:78]), post(f.h, U, S, total=False), post(f.h, U[:3], S[0])
        for k in whole:
            assert np.array_equal(chunked[k], whole[k]) and np.array_equal(alone[k][0], whole[k][77]) and np.array_equal(shared[k][0], whole[k][0]), k
            assert k not in without or np.array_equal(without[k], whole[k]), k + " without the totals"


@pytest.mark.gpu
def test_with_one_active_coordinate_the_three_sums_agree_within_their_bounds():
    with fit(129, 3) as f:
        u, S, Kinv = dl.inputs_u(f.x, f.theta, f.seed)["between"], np.diag(sm.variances(3, f.seed)["drawn"]), f.model.kinv()
        out = post(f.h, np.repeat(u[None, :], 3, axis=0), S)
        for k in range(3):
            lim, got, sc = judged(f.x, f.theta, f.name, "one s_%d > 0" % k, out, k, Kinv, u, S[k])
            assert got["var"][0] > 0 and all(abs(got[key][k] - got["var"][0]) <= lim * (sc[key][k] + sc["var"][0]) for key in ("first", "total")), (k, got)


@pytest.mark.gpu
def test_pseudo_handle_python_methods_and_refusals():
    x, t, theta, _xs = sl.make_case(300, 3, 40, 0.03, 0.06, 0.3)
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(40), theta.copy())
    pgp = gp.pseudo_gp()
    try:
        u, s, sa, h = dl._grid(np.array([4.0, 5.5, 3.25])), np.array([0.7, 0.0, 1.9]), sk.SensitivityAnalysis(pgp), pgp._dev().handle
        raw = post(h, u[None, :], s)
        judged(pgp.x, pgp.theta_min, "pseudo N=300 m=40 d=3", "pseudo", raw, 0, pgp._dev().kinv(), u, s)
        mean, V, first, total = sa.variances(u, np.diag(s), posterior=True)
        assert (mean == raw["mean"][0] + gp.meant and V == raw["V"][0] + raw["var_post"][0] and np.array_equal(first, raw["first"][0] + raw["first_post"][0])
                and np.array_equal(total, raw["total"][0] + raw["total_post"][0]))
        assert all(np.array_equal(a[0], b) for a, b in zip(sa.variances_many(u[None, :], s, posterior=True), (mean, V, first, total)))
        fi, ti = sa.indices(u, s, posterior=True)
        assert np.array_equal(fi, first / V) and np.array_equal(ti, total / V) and np.array_equal(sa.indices_many(u[None, :], s, True)[0][0], fi)
        assert sa.variances(u, s)[1] == raw["V"][0]                                                          # the default is the mean part alone
        with pytest.raises(NotImplementedError, match="[Gg]aussian"):
            sk.SensitivityAnalysis(pgp, distribution="uniform").indices(u, s, posterior=True)
        st, o = post(h, u[None, :], np.array([0.7, -1e-300, 1.9]), status=True)
        assert st == GPX_ERR_BAD_ARG and all(np.all(a == FILL) for a in o.values()) and "variances" in _gpx.last_error()
        P = [_gpx.ptr(a) for a in o.values()]                                                                # total XOR total_post
        for args in (P[:3] + [None] + P[4:], P[:6] + [None]):
            assert _gpx.lib.gpx_sensitivity_post_many(h, _gpx.ptr(u), _gpx.ptr(s), 1, 1, *args) == GPX_ERR_BAD_ARG and all(np.all(a == FILL) for a in o.values())
        assert _gpx.lib.gpx_sensitivity_post_many(h, None, None, 0, 0, *[None] * 7) == 0                     # b = 0 is a no-op
    finally:
        pgp.close()
        gp.cov.clear_cache()
        _gpx.lib.gpx_pool_trim()
    other = sk.GaussianProcess(*small_problem(), sk.MaternCovariance(2.5), np.log(np.array([2.0, 0.01, 0.3, 0.1])))
    st, o = post(other._dev().handle, np.array([[4.5, 5.25]]), np.array([0.8, 0.3]), status=True)
    assert st == GPX_ERR_STATE and all(np.all(a == FILL) for a in o.values()) and "MaternCovariance" in _gpx.last_error()
