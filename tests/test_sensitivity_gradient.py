"""gpx_sensitivity_gradient_many and SensitivityAnalysis.gradient_moments / dgsm / active_subspace: gmean = E[grad mu], cmean =
E[grad mu grad mu^T] and cpost = E[Cov grad f] under x_k ~ N(u_k, s_k), against the plain long-double evaluation of the definitions of
include/gpx.h over ALL pairs (`model` below), every entry on the scale of its absolute terms -- sum |W_ij| G_ij (|p_k q_l| + delta_kl om^2
tau_k), W = beta beta^T or K^-1, plus delta_kl v w_k for cpost -- under 32 max(rho_ref, 1000 u) with rho_ref from the float64 evaluation of
the same function (the project's one rule, tests/_spgp_ld.py).  Judged on the device's OWN alpha and K^-1.

Shapes (N, d) -> instance of grad_pair_kernel: (260, 2), (129, 3), (129, 8), (130, 9) one block of 16 coordinates (1, 2 and 3 groups of
four in the exponent loop; more than 256 columns; N no multiple of 4 or 16); (81, 17) two blocks, four accumulators a weight; (57, 33) and
(41, 50) three and four blocks, the column blocks swept over grid.y.  Every shape runs with and without cpost."""
import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _dense_ld as dl
import _sensitivity_model as sm
import _spgp_ld as sl
from test_sensitivity import FILL, GPX_ERR_BAD_ARG, GPX_ERR_STATE, chunk_of, fit, sens, small_problem

SHAPES = [(260, 2), (129, 3), (129, 8), (130, 9), (81, 17), (57, 33), (41, 50)]
IDS = ["n%d_d%d" % c for c in SHAPES]
gpu = pytest.mark.gpu


def model(x, theta, beta, Kinv, u, s, dt=dl.LD):
    """{"gmean": ([d], [d]), "cmean": ([d, d], [d, d]), "cpost": the same unless Kinv is None}, each (values, scales)"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, _vt, w = dl.params(theta, d, dt)
    sg = np.asarray(s, dtype=np.float64).astype(dt)
    a = xr.astype(dt) - np.asarray(u, dtype=np.float64).astype(dt)
    be = np.asarray(beta, dtype=np.float64).astype(dt)
    ws = w * sg
    den = 1 + 2 * ws
    rho, tau = ws / den, sg / den
    gk = v * np.exp((-np.log1p(ws) / 2 - w * a * a / (1 + ws) / 2).sum(1))[:, None] * (w * a / (1 + ws))
    out = {"gmean": ((be[:, None] * gk).sum(0), (np.abs(be)[:, None] * np.abs(gk)).sum(0))}
    dm, sp = a[:, None, :] - a[None, :, :], a[:, None, :] + a[None, :, :]
    G = (v * v) * np.exp((-np.log1p(2 * ws) / 2 - w * dm * dm / 4 - w * sp * sp / den / 4).sum(2))
    P = (w * (rho * sp - a[:, None, :])).reshape(N * N, d)
    Q = (w * (rho * sp - a[None, :, :])).reshape(N * N, d)
    for key, W in (("cmean", np.outer(be, be)), ("cpost", Kinv)):
        if W is None:
            continue
        wg = (np.asarray(W, dtype=np.float64).astype(dt) * G).reshape(-1)
        val = (P * wg[:, None]).T @ Q + np.diag(w * w * tau * wg.sum())
        sc = (np.abs(P) * np.abs(wg)[:, None]).T @ np.abs(Q) + np.diag(w * w * tau * np.abs(wg).sum())
        out[key] = (val, sc) if key == "cmean" else (np.diag(v * w) - val, sc + np.diag(v * w))
    return out


def grad(h, U, S, post=True, status=False):
    """{"gmean": [b, d], "cmean": [b, d, d], "cpost": [b, d, d]} of gpx_sensitivity_gradient_many; S [d] = one set for all; outputs enter as FILL"""
    U, S = _gpx.f64(U), _gpx.f64(S)
    b, d = U.shape
    out = {"gmean": np.full((b, d), FILL), "cmean": np.full((b, d, d), FILL), "cpost": np.full((b, d, d), FILL)}
    st = _gpx.lib.gpx_sensitivity_gradient_many(h, _gpx.ptr(U), _gpx.ptr(S), int(S.ndim == 1), b, _gpx.ptr(out["gmean"]), _gpx.ptr(out["cmean"]),
                                                _gpx.ptr(out["cpost"]) if post else None)
    if status:
        return st, out
    _gpx.check(st, "gpx_sensitivity_gradient_many")
    if not post:
        assert np.all(out.pop("cpost") == FILL)
    return out


def judged(f, name, got, Kinv, u, s):
    """got {key: values of one input} under the rule; returns (rho_ref, the model)"""
    want, ref = model(f.x, f.theta, f.alpha, Kinv, u, s), model(f.x, f.theta, f.alpha, Kinv, u, s, dt=np.float64)
    ref_dist = {k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in got}
    rho = dl.rho_of(ref_dist)
    dist = {k: dl.distances(g, want[k][0], want[k][1]) for k, g in got.items()}
    dl.record("gradient moments " + name, f.name, rho, dist, ref_dist)
    assert all(np.all(np.isfinite(g)) for g in got.values()), (name, got)
    dl.assert_within(dist, rho, what="gradient moments %s %s" % (name, f.name))
    assert all(np.array_equal(got[k], got[k].T) for k in got if k != "gmean"), name
    return rho, want


def test_model_is_the_definitions():
    """the long-double model against tensor Gauss-Hermite quadrature (80 nodes; one node for a coordinate with s = 0) of E[grad mu],
    E[grad mu grad mu^T] and E[Cov grad f] = delta_kl v w_k - E[d_k c^T Kinv d_l c], to 1e-12 of the largest entry"""
    z, q = np.polynomial.hermite_e.hermegauss(80)
    z, q = z.astype(dl.LD), (q / q.sum()).astype(dl.LD)
    for d, s in ((1, [0.6]), (2, [0.5, 0.0]), (3, [0.7, 0.0, 0.3])):
        rng = np.random.RandomState(40 + d)
        N = 7 + d
        x, u, beta = rng.uniform(0, 4, (N, d)), rng.uniform(1, 3, d), rng.randn(N)
        theta = np.log(np.concatenate([[1.7, 0.01], rng.uniform(0.2, 0.6, d)]))
        Kinv = rng.randn(N, N)
        Kinv = Kinv + Kinv.T
        v, _vt, w = dl.params(theta, d)
        axes = [(dl.LD(u[k]) + np.sqrt(dl.LD(s[k])) * z, q) if s[k] > 0 else (np.array([u[k]], dl.LD), np.ones(1, dl.LD)) for k in range(d)]
        nodes = np.stack([m.ravel() for m in np.meshgrid(*[ax[0] for ax in axes], indexing="ij")], 1)           # [nodes, d]
        wt = np.prod(np.stack([m.ravel() for m in np.meshgrid(*[ax[1] for ax in axes], indexing="ij")], 1), axis=1)
        diff = nodes[:, None, :] - x.astype(dl.LD)[None, :, :]                                                   # [nodes, N, d]
        dc = -w * diff * (v * np.exp(-(w * diff * diff).sum(2) / 2))[:, :, None]                                 # d_k c_i at the nodes
        M = np.einsum("q,qik,qjl->ijkl", wt, dc, dc)
        be = beta.astype(dl.LD)
        quad = {"gmean": np.einsum("q,qik,i->k", wt, dc, be), "cmean": np.einsum("ijkl,i,j->kl", M, be, be),
                "cpost": np.diag(v * w) - np.einsum("ijkl,ij->kl", M, Kinv.astype(dl.LD))}
        got = model(x, theta, beta, Kinv, u, np.array(s))
        for key, want in quad.items():
            err = float(np.abs(got[key][0] - want).max() / np.abs(want).max())
            print("d=%d %s: model against quadrature %.3e of the largest entry" % (d, key, err))
            assert err <= 1e-12, (d, key, err)


@gpu
@pytest.mark.parametrize("N,d", SHAPES, ids=IDS)
def test_sums(N, d):
    with fit(N, d) as f:
        cs = sm.combos(f.x, f.theta, f.seed)
        U, S = np.stack([u for _n, u, _s in cs]), np.stack([s for _n, _u, s in cs])
        out, Kinv = grad(f.h, U, S), f.model.kinv()
        for i, (cn, u, s) in enumerate(cs):
            judged(f, cn, {k: o[i] for k, o in out.items()}, Kinv, u, s)
        S[-1, -1] = -1e-300                                 # a refusal leaves the outputs as they were
        st, o = grad(f.h, U, S, status=True)
        assert st == GPX_ERR_BAD_ARG and all(np.all(a == FILL) for a in o.values()) and "variances" in _gpx.last_error()


@gpu
@pytest.mark.parametrize("N,d", [(129, 8), (81, 17)])
def test_bits_do_not_depend_on_the_batch_the_chunking_or_cpost(N, d):
    with fit(N, d) as f:
        rng = np.random.RandomState(f.seed + 5)
        U, S = dl._grid(rng.uniform(1, 9, (130, d))), rng.uniform(0.01, 4.0, (130, d))
        S[1, ::2] = 0.0
        S[2] = 0.0
        whole = grad(f.h, U, S)
        with chunk_of(7):
            chunked = grad(f.h, U, S)
        alone, without = grad(f.h, U[77:78], S[77:78]), grad(f.h, U, S, post=False)
        for k in whole:
            assert np.array_equal(chunked[k], whole[k]) and np.array_equal(alone[k][0], whole[k][77]), k
            assert k == "cpost" or np.array_equal(without[k], whole[k]), k
        shared = grad(f.h, U[:3], S[0])
        assert all(np.array_equal(shared[k][0], whole[k][0]) for k in whole)


@gpu
@pytest.mark.parametrize("N,d", [(129, 3), (81, 17)])
def test_without_variance_it_is_the_gradient_at_u(N, d):
    """all s = 0: gmean = grad mu(u) and cmean = its outer product, within the sum of the two bounds (the scale of cmean_kl is then A_k A_l,
    A = the scale of the gradient, and the outer product of a gradient off by bound A is off by bound (A_k |g_l| + |g_k| A_l))"""
    with fit(N, d) as f:
        u, s = dl.inputs_u(f.x, f.theta, f.seed)["between"], np.zeros(d)
        out = grad(f.h, u[None, :], s, post=False)
        rho, want = judged(f, "no variance", {k: o[0] for k, o in out.items()}, None, u, s)
        mean, g = np.empty(1), np.empty((1, d))
        _gpx.check(_gpx.lib.gpx_predict_mean_grad(f.h, _gpx.ptr(_gpx.f64(u[None, :])), 1, _gpx.ptr(mean), _gpx.ptr(g)), "gpx_predict_mean_grad")
        A, g, lim = np.asarray(want["gmean"][1], dtype=np.float64), g[0], sm.bound(rho)
        assert np.all(np.abs(out["gmean"][0] - g) <= 2 * lim * A)
        assert np.all(np.abs(out["cmean"][0] - np.outer(g, g)) <= lim * (np.asarray(want["cmean"][1], dtype=np.float64) + np.outer(A, np.abs(g)) + np.outer(np.abs(g), A)))


@gpu
@pytest.mark.parametrize("N,d", [(129, 3), (130, 9)])
def test_poincare(N, d):
    """total_k <= s_k cmean_kk (Gaussian Poincare inequality for mu), within the two sums' bounds"""
    with fit(N, d) as f:
        for cn, u, s in [c for c in sm.combos(f.x, f.theta, f.seed) if c[0].endswith("/drawn")]:
            out = grad(f.h, u[None, :], s, post=False)
            rho2, want2 = judged(f, cn, {k: o[0] for k, o in out.items()}, None, u, s)
            want, ref = sm.both(f.x, f.theta, f.alpha, u, s)
            rho1 = dl.rho_of({"total": dl.distances(ref["total"][0], want["total"][0], want["total"][1])})
            total, nu = sens(f.h, u[None, :], s)["total"][0], np.diagonal(out["cmean"][0])
            slack = sm.bound(rho1) * np.asarray(want["total"][1], dtype=np.float64) + s * sm.bound(rho2) * np.asarray(np.diagonal(want2["cmean"][1]), dtype=np.float64)
            print("N=%d d=%d %s: min_k (s_k nu_k - total_k) / total_k = %.3e" % (N, d, cn, float(np.min((s * nu - total) / np.maximum(total, 1e-300)))))
            assert np.all(total <= s * nu + slack), (cn, total, s * nu)


@gpu
def test_pseudo_handle_and_python_methods():
    N, d, m = 300, 3, 40
    x, t, theta, _xs = sl.make_case(N, d, m, 0.03, 0.06, 0.3)
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), theta.copy())
    pgp = gp.pseudo_gp()
    try:
        u, s = dl._grid(np.array([4.0, 5.5, 3.25])), np.array([0.7, 0.0, 1.9])
        sa, h = sk.SensitivityAnalysis(pgp), pgp._dev().handle
        raw = grad(h, u[None, :], s)
        f = type("PseudoFit", (), {"x": pgp.x, "theta": pgp.theta_min, "alpha": pgp._get_beta(), "name": "pseudo N=%d m=%d d=%d" % (N, m, d)})
        judged(f, "pseudo", {k: o[0] for k, o in raw.items()}, pgp._dev().kinv(), u, s)
        g, C = sa.gradient_moments(u, np.diag(s))
        gp_, Cp = sa.gradient_moments_many(u[None, :], s, posterior=True)
        assert np.array_equal(g, raw["gmean"][0]) and np.array_equal(C, raw["cmean"][0]) and np.array_equal(gp_[0], g)
        assert np.array_equal(Cp[0], raw["cmean"][0] + raw["cpost"][0]) and np.array_equal(sa.dgsm(u, s), np.diagonal(C))
        assert np.array_equal(sa.dgsm_many(u[None, :], s, posterior=True)[0], np.diagonal(Cp[0]))
        lam, V = sa.active_subspace(u, s)
        assert np.all(np.diff(lam) <= 0) and np.abs((V * lam) @ V.T - Cp[0]).max() <= 1e-12 * np.linalg.norm(Cp[0])
        with pytest.raises(ValueError):
            sa.gradient_moments(u, np.diag(s) + 0.1)
        with pytest.raises(NotImplementedError, match="[Gg]aussian"):
            sk.SensitivityAnalysis(pgp, distribution="uniform").dgsm(u, s)
        assert _gpx.lib.gpx_sensitivity_gradient_many(h, None, None, 0, 0, None, None, None) == 0           # b = 0 is a no-op
    finally:
        pgp.close()
        gp.cov.clear_cache()
        _gpx.lib.gpx_pool_trim()
    x2, t2 = small_problem()
    other = sk.GaussianProcess(x2, t2, sk.MaternCovariance(2.5), np.log(np.array([2.0, 0.01, 0.3, 0.1])))
    st, o = grad(other._dev().handle, np.array([[4.5, 5.25]]), np.array([0.8, 0.3]), status=True)
    assert st == GPX_ERR_STATE and all(np.all(a == FILL) for a in o.values()) and "MaternCovariance" in _gpx.last_error()
