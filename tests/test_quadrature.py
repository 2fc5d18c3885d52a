"""Numerical propagation on the device: UncertaintyPropagationNumericalHG / UncertaintyPropagationMC, gpx_propagate_quadrature_many,
gpx_mixture_reduce and gpx_quadrature_nodes (csrc/quadrature.hip; the models and bounds: tests/_quadrature_model.py).

  (a) the reduction alone against the long-double model, within 8 max(rho, 4) units (rho measured on the float64 restatement);
  (b) the nodes against the stated fma chain, bit for bit;
  (c) the reference's recorded values through the Python classes, at the device tolerances 1e-9 k (mean), 1e-8 v k (variance);
  (d) ragged shapes against the oracle: every predicted row is held to 1e-9 / 1e-8 v by the parity tests, wq > 0 sums to 1, so
      |dm| <= 1e-9, |dvar| <= 1e-8 v + 4e-9 sqrt(c2) + 1e-16, and m3, m4 and the density lie within twice the first-order bound
      sum wq (|d/dmu| 1e-9 + |d/dsigma^2| 1e-8 v) + 64 u |value|;
  (e) an input that straddles a chunk seam; (f) five slabs and more (the left-looking emulated solve feeds the reduction);
  (g) the routes; (h) no side effects on the handle.
The CPU cases need no device.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import load_golden, torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from oracle import oracle as orc

import _periodic_ld as pl
import _quadrature_model as qm
from _operators import make_warped_gaussian

HERE = os.path.dirname(os.path.abspath(__file__))
LD = qm.LD
EMU, EVAR = 1e-9, 1e-8              # the parity tests' bounds on a predicted row: mean, variance / v
NEW = ("gpx_propagate_quadrature_many", "gpx_mixture_reduce", "gpx_quadrature_nodes")


# ------------------------------------------------------------------------------------------------
# without a device
# ------------------------------------------------------------------------------------------------
def test_symbols_classes_and_methods_exist():
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpx.h")).read()
    for name in NEW:
        assert name in _gpx.SIGNATURES and hasattr(_gpx.lib, name)
        assert "int %s(" % name in header
    assert _gpx.lib.gpx_abi_version() == 1      # additive
    assert issubclass(sk.UncertaintyPropagationNumericalHG, sk.UncertaintyPropagation)
    assert issubclass(sk.UncertaintyPropagationMC, sk.UncertaintyPropagationGA)
    for cls in (sk.UncertaintyPropagationNumericalHG, sk.UncertaintyPropagationMC):
        for m in ("propagate_mean", "propagate_GA", "propagate", "propagate_many", "propagate_GA_many", "propagate_moments_many",
                  "propagate_density_many"):
            assert callable(getattr(cls, m)), (cls, m)
    for m in ("propagate", "propagate_many"):
        assert callable(getattr(sk.UncertaintyPropagation, m))


def test_bad_arguments_are_refused_and_no_output_touched():
    U, A, z, wq, y = np.zeros((3, 2)), np.eye(2), np.zeros((4, 2)), np.full(4, 0.25), np.zeros(5)
    mom, dens = np.full((5, 3), 7.25), np.full((3, 5), 7.25)
    st = _gpx.lib.gpx_propagate_quadrature_many(None, _gpx.ptr(U), _gpx.ptr(A), 1, 3, _gpx.ptr(z), _gpx.ptr(wq), 4, _gpx.ptr(y), 5, 1, 0.0,
                                                _gpx.ptr(mom), _gpx.ptr(dens))
    assert st == _gpx.GPX_ERR_BAD_ARG and "null handle" in _gpx.last_error()
    mu, var = np.zeros((3, 4)), np.ones((3, 4))
    P = _gpx.ptr
    bad = [
        (None, P(var), P(wq), 4, 3, P(y), 5, 1, 0.0, P(mom), P(dens)),          # null arrays
        (P(mu), None, P(wq), 4, 3, P(y), 5, 1, 0.0, P(mom), P(dens)),
        (P(mu), P(var), None, 4, 3, P(y), 5, 1, 0.0, P(mom), P(dens)),
        (P(mu), P(var), P(wq), 4, 3, None, 5, 1, 0.0, P(mom), P(dens)),
        (P(mu), P(var), P(wq), 4, 3, P(y), 5, 1, 0.0, None, P(dens)),
        (P(mu), P(var), P(wq), 4, 3, P(y), 5, 1, 0.0, P(mom), None),           # dens null with ny > 0
        (P(mu), P(var), P(wq), 0, 3, P(y), 5, 1, 0.0, P(mom), P(dens)),         # S < 1
        (P(mu), P(var), P(wq), 4, -1, P(y), 5, 1, 0.0, P(mom), P(dens)),        # b < 0
        (P(mu), P(var), P(wq), 4, 3, P(y), -1, 1, 0.0, P(mom), P(dens)),        # ny < 0
    ]
    for args in bad:
        assert _gpx.lib.gpx_mixture_reduce(*args) == _gpx.GPX_ERR_BAD_ARG, args
    out = np.full((12, 2), 7.25)
    assert _gpx.lib.gpx_quadrature_nodes(P(U), None, 1, 3, P(z), 4, 2, P(out)) == _gpx.GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_quadrature_nodes(P(U), P(A), 1, 3, P(z), 4, 65, P(out)) == _gpx.GPX_ERR_BAD_ARG
    for o in (mom, dens, out):
        np.testing.assert_array_equal(o, np.full(o.shape, 7.25))


# ------------------------------------------------------------------------------------------------
# on the device
# ------------------------------------------------------------------------------------------------
def _reduce(mu, var, wq, y=None, y_shared=1, shift=0.0, device=False, pad=0):
    """gpx_mixture_reduce itself: (mom [5, b], dens [b, ny] or None); pad: sentinel doubles behind each output, checked untouched"""
    mu, var, wq = _gpx.f64(mu), _gpx.f64(var), _gpx.f64(wq)
    b, S = mu.shape
    ny = 0 if y is None else np.shape(y)[-1]
    mom = np.full(5 * b + pad, -7.25)
    dens = np.full(b * ny + pad, -7.25)
    yy = _gpx.f64(y) if ny else None
    if device:
        dev = [torch.from_numpy(a).cuda() for a in (mu, var, wq, mom, dens) + ((yy,) if ny else ())]
        p = [ctypes.c_void_p(t.data_ptr()) for t in dev]
        st = _gpx.lib.gpx_mixture_reduce(p[0], p[1], p[2], S, b, p[5] if ny else None, ny, int(y_shared), shift, p[3], p[4] if ny else None)
        torch.cuda.synchronize()
        mom, dens = dev[3].cpu().numpy(), dev[4].cpu().numpy()
    else:
        st = _gpx.lib.gpx_mixture_reduce(_gpx.ptr(mu), _gpx.ptr(var), _gpx.ptr(wq), S, b, _gpx.ptr(yy) if ny else None, ny, int(y_shared), shift,
                                         _gpx.ptr(mom), _gpx.ptr(dens) if ny else None)
    _gpx.check(st, "gpx_mixture_reduce")
    if pad:
        np.testing.assert_array_equal(mom[5 * b:], np.full(pad, -7.25))      # nothing written outside [5, b] and [b, ny]
        np.testing.assert_array_equal(dens[b * ny:], np.full(pad, -7.25))
    return mom[:5 * b].reshape(5, b), (dens[:b * ny].reshape(b, ny) if ny else None)


_RHO = []


def _reduce_bounds():
    if not _RHO:
        rm, rd = qm.reduce_rho()
        _RHO.extend([qm.reduce_bound_units(rm), qm.reduce_bound_units(rd)])
    return _RHO


@pytest.mark.gpu
@pytest.mark.parametrize("S", qm.REDUCE_S)
def test_reduce_against_long_double(S):
    """(a) every (b, ny, y form) of the shape list at this S; host pointers, and device pointers at ny = 0 and ny = 9"""
    bm, bd = _reduce_bounds()
    worst_m, worst_d, seen_b = 0.0, 0.0, set()
    for S_, b, ny, ysh in [c for c in qm.reduce_shapes() if c[0] == S]:
        mu, var, wq, y = qm.reduce_case(S, b, ny, ysh)
        device = ny in (0, 9) and (b, ny) not in seen_b
        seen_b.add((b, ny))
        mom, dens = _reduce(mu, var, wq, y, ysh, 0.25, device=device, pad=16)
        for i in range(b):
            yi = None if y is None else (y if ysh else y[i])
            lm, units, ld, du = qm.mixture_ld(mu[i], var[i], wq, yi, 0.25)
            assert np.all(np.isfinite(mom[:, i])), (S, b, ny, i)
            err = np.abs(LD(1) * mom[:, i] - lm)
            assert np.all(err <= bm * units), (S, b, ny, i, err, units)        # (a unit of 0 -- one node, sigma^2 = 0 -- asks for the exact 0)
            worst_m = max(worst_m, float(np.max(err[units > 0] / units[units > 0], initial=0.0)))
            if ny:
                if var[i].min() <= 0.0:
                    assert not np.any(np.isfinite(dens[i])), (S, b, ny, i)     # the sigma^2 = 0 node: non-finite, as the reference's expression
                    continue
                assert np.all(np.isfinite(dens[i])) and dens[i, -1] == 0.0, (S, b, ny, i, dens[i, -1])   # 40 sigma away: 0, not NaN
                rd = np.abs(LD(1) * dens[i] - ld) / du
                worst_d = max(worst_d, float(rd.max()))
                assert np.all(rd <= bd), (S, b, ny, i, rd)
    print("reduce S=%d: worst moments %.2f units (bound %.0f), density %.2f units (bound %.0f)" % (S, worst_m, bm, worst_d, bd))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [65, 4097])
def test_reduce_bits_do_not_depend_on_place_or_batch(S):
    mu, var, wq, y = qm.reduce_case(S, 3, 9, 0)
    var[-1, 0] = 1e-3
    alone = _reduce(mu[:1], var[:1], wq, y[:1], 0, 0.25)
    first = _reduce(mu, var, wq, y, 0, 0.25)
    order = [1, 2, 0]
    last = _reduce(mu[order], var[order], wq, y[order], 0, 0.25)
    big = _reduce(np.tile(mu, (44, 1))[:130], np.tile(var, (44, 1))[:130], wq, np.tile(y, (44, 1))[:130], 0, 0.25)
    for got, col in ((first, 0), (last, 2), (big, 129 - 129 % 3)):
        np.testing.assert_array_equal(got[0][:, col], alone[0][:, 0])
        np.testing.assert_array_equal(got[1][col], alone[1][0])


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 3, 8, 9, 64])
def test_nodes_are_the_stated_fma_chain(d):
    """(b) bit for bit, one A for all inputs and one per input"""
    rng = np.random.RandomState(40 + d)
    B, S = 3, 5
    U, z = rng.uniform(0, 10, (B, d)), rng.randn(S, d)
    for A in (rng.randn(d, d) * 0.3, rng.randn(B, d, d) * 0.3):
        out = np.full((B * S + 2, d), -7.25)
        _gpx.check(_gpx.lib.gpx_quadrature_nodes(_gpx.ptr(U), _gpx.ptr(_gpx.f64(A)), int(A.ndim == 2), B, _gpx.ptr(z), S, d, _gpx.ptr(out)), "gpx_quadrature_nodes")
        np.testing.assert_array_equal(out[B * S:], np.full((2, d), -7.25))
        np.testing.assert_array_equal(out[:B * S].reshape(B, S, d), qm.nodes_fma(U, A, z))


def _quad(gp, U, A, z, wq, Y=None, shift=0.0):
    """gpx_propagate_quadrature_many itself: (mom [5, B] -- the mean WITHOUT meant --, dens)"""
    U, A, z, wq = _gpx.f64(U), _gpx.f64(A), _gpx.f64(z), _gpx.f64(wq)
    B = len(U)
    ny = 0 if Y is None else np.shape(Y)[-1]
    YY = _gpx.f64(Y) if ny else None
    mom, dens = np.empty((5, B)), (np.empty((B, ny)) if ny else None)
    st = _gpx.lib.gpx_propagate_quadrature_many(gp._dev().handle, _gpx.ptr(U), _gpx.ptr(A), int(A.ndim == 2), B, _gpx.ptr(z), _gpx.ptr(wq), len(wq),
                                                _gpx.ptr(YY) if ny else None, ny, int(ny == 0 or YY.ndim == 1), shift, _gpx.ptr(mom),
                                                _gpx.ptr(dens) if ny else None)
    _gpx.check(st, "gpx_propagate_quadrature_many")
    return mom, dens


def _hold_to_first_order(tag, mom, dens, mu, var, wq, Y, v, worst):
    """(d)'s bounds for every input: mom [5, B] (mean as mu carries it), dens [B, ny]; mu, var [B, S] the oracle's; Y [B, ny] or None"""
    for i in range(mom.shape[1]):
        lm, _units, ld, _du = qm.mixture_ld(mu[i], var[i], wq, None if Y is None else Y[i], 0.0)
        bm, bvar, bm3, bm4, bdens = qm.first_order_bounds(mu[i], var[i], wq, None if Y is None else Y[i], 0.0, EMU, EVAR * v)
        err = np.abs(LD(1) * mom[:, i] - lm)
        ev_bound = EVAR * v + 64 * qm.U64 * abs(lm[2])         # E[sigma^2]: an average of the rows' variances
        for q, (e, bnd) in enumerate(zip(err, (bm, bvar, ev_bound, bm3, bm4))):
            worst[q] = max(worst[q], float(e / bnd))
            assert e <= bnd, (tag, i, q, float(e), float(bnd))
        if Y is not None:
            ed = np.abs(LD(1) * dens[i] - ld)
            worst[5] = max(worst[5], float(np.max(ed / bdens)))
            assert np.all(ed <= bdens), (tag, i, ed, bdens)


_RAGGED = {}     # N -> (gp, oracle gp, x)


def _ragged_gp(N):
    """the recipe of tests/test_propagate_many.py"""
    if N not in _RAGGED:
        d = {127: 3, 640: 6, 1500: 8, 5200: 8}[N]
        rng = np.random.RandomState(100 + N + d)
        x = rng.uniform(0, 10, (N, d))
        t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
        theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
        _RAGGED[N] = (sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy()), orc.OracleGP(x, t, theta), x)
    return _RAGGED[N]


def _ragged_inputs(x, B, S, seed, ny=9):
    """U (every 5th a training row), a full root A per input, S standard-normal nodes with positive weights that sum to 1, Y [B, ny]"""
    d = x.shape[1]
    rng = np.random.RandomState(seed)
    U = rng.uniform(2, 8, (B, d))
    U[::5] = x[rng.randint(0, len(x), len(U[::5]))]
    A = np.tril(rng.uniform(-0.1, 0.1, (B, d, d))) + 0.2 * np.eye(d)[None]
    z = rng.randn(S, d)
    if S > 1:
        z[0] = 0.0                                         # node 0 of the inputs above IS a training row (the +vt quirk is theirs alone)
    wq = rng.uniform(0.2, 1.0, S)
    wq /= wq.sum()
    return U, A, z, wq, rng.uniform(-1.5, 1.5, (B, ny))


def _against_oracle(tag, gp, og, x, B, S, seed, shared=False):
    U, A, z, wq, Y = _ragged_inputs(x, B, S, seed)
    if shared:
        A = A[0]
    meant = gp._get_mean_t()
    mom, dens = _quad(gp, U, A, z, wq, Y, meant)
    mu, var = og.estimate_many(qm.nodes_plain(U, A, z).reshape(B * S, -1))
    mom[0] += meant
    worst = [0.0] * 6
    _hold_to_first_order(tag, mom, dens, mu.reshape(B, S), var.reshape(B, S), wq, Y, float(np.exp(gp.theta_min[0])), worst)
    print("%s: worst fraction of the bound: m %.1e var %.1e Ev %.1e m3 %.1e m4 %.1e dens %.1e" % ((tag,) + tuple(worst)))
    return mom, dens


@pytest.mark.gpu
@pytest.mark.parametrize("B,S", [(1, 1), (1, 64), (3, 16), (130, 257)])
@pytest.mark.parametrize("N", [127, 640, 1500])
def test_against_oracle_ragged(N, B, S):
    """(d) every input and every y of every batch"""
    gp, og, x = _ragged_gp(N)
    _against_oracle("oracle N=%d B=%d S=%d" % (N, B, S), gp, og, x, B, S, N + B + S, shared=(B == 3))


@pytest.mark.gpu
def test_input_straddles_the_chunk_seam():
    """(e) N = 127, S = 257, B = 128: 32896 rows > the 32768 of a chunk, input 127 spans the seam (rows 32639 .. 32895).  A Gaussian handle has
    no chunk cap to force: the oracle, and the same input alone in a one-chunk call (the many-row solver's rows do not depend on their
    neighbours up to the parity bound: twice (d)'s bounds cover both).  The periodic predictor promises bits that do not depend on the
    chunking: there a capped run must reproduce the uncapped one bit for bit."""
    gp, og, x = _ragged_gp(127)
    B, S = 128, 257
    mom, dens = _against_oracle("seam", gp, og, x, B, S, 99)
    U, A, z, wq, Y = _ragged_inputs(x, B, S, 99)
    m1, d1 = _quad(gp, U[127:], A[127:], z, wq, Y[127:], gp._get_mean_t())
    m1[0] += gp._get_mean_t()
    assert abs(m1[0, 0] - mom[0, 127]) <= 2 * EMU and abs(m1[1, 0] - mom[1, 127]) <= 2 * (2 * EVAR + 4 * EMU)
    xp, tp, thp = pl.make_case(130, 1)
    pgp = sk.GaussianProcess(xp, tp, sk.PeriodicCovariance(), thp.copy())
    rng = np.random.RandomState(3)
    Up, Ap, zp, wp = rng.uniform(2, 8, (3, 1)), np.array([[0.3]]), rng.randn(257, 1), np.full(257, 1.0 / 257)
    free = _quad(pgp, Up, Ap, zp, wp, np.linspace(-1, 1, 9), 0.0)
    os.environ["GPX_PERIODIC_CHUNK"] = "256"
    try:
        capped = _quad(pgp, Up, Ap, zp, wp, np.linspace(-1, 1, 9), 0.0)      # 771 rows in chunks of 256: inputs 0 and 1 straddle seams
    finally:
        del os.environ["GPX_PERIODIC_CHUNK"]
    np.testing.assert_array_equal(capped[0], free[0])
    np.testing.assert_array_equal(capped[1], free[1])


@pytest.mark.gpu
def test_five_slabs_and_more():
    """(f) N = 5200 (six slabs of 1024 columns), d = 8, B = 8, S = 64: the left-looking emulated solve feeds the reduction"""
    gp, og, x = _ragged_gp(5200)
    _against_oracle("five slabs", gp, og, x, 8, 64, 5)


def _golden_gp(name):
    g = load_golden(name)
    return sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy()), orc.OracleGP(g["x"], g["t_raw"], g["theta"]), g


def _golden_through_class(key, gp, estimate_many, v, k=1.0):
    Q = load_golden("quadrature")
    u, Sigma, order = Q[key + "u"], Q[key + "Sigma"], int(Q[key + "order"])
    hg = sk.UncertaintyPropagationNumericalHG(gp, order=order)
    nu, nS = Q[key + "mean"].shape
    z, wq = qm.hg_rule(order, u.shape[1])
    worst = [0.0, 0.0, 0.0]
    for j in range(nS):
        bds = []
        mean, var = hg.propagate_GA_many(u[:nu], Sigma[j])
        dens = hg.propagate_density_many(Q[key + "y"][:, j], u[:nu], Sigma[j])
        for i in range(nu):
            ref_m, ref_v = Q[key + "ga"][i, j]
            worst = [max(worst[0], abs(mean[i] - ref_m)), max(worst[1], abs(var[i] - ref_v)), worst[2]]
            assert mean[i] == pytest.approx(ref_m, abs=1e-9 * k) and var[i] == pytest.approx(ref_v, abs=1e-8 * v * k), (key, i, j)
            assert hg.propagate_mean(u[i], Sigma[j]) == pytest.approx(Q[key + "mean"][i, j], abs=1e-9 * k)
            # the density: (d)'s first-order bound about the model's mu, sigma^2, plus the model's own distance from the reference
            mu, s2 = estimate_many(qm.nodes_plain(u[i:i + 1], qm.hg_root(Sigma[j]), z)[0])
            bd = qm.first_order_bounds(mu, s2, wq, Q[key + "y"][i, j], 0.0, EMU * k, EVAR * v * k)[4] + 1e-10 * Q[key + "dens"][i, j].max()
            bds.append(bd)
            ed = np.abs(dens[i] - Q[key + "dens"][i, j])
            worst[2] = max(worst[2], float(np.max(ed / bd)))
            assert np.all(ed <= bd), (key, i, j, ed, bd)
        # the single-input surface returns what the batch returns
        ga = hg.propagate_GA(u[0], Sigma[j])
        assert ga[0] == pytest.approx(mean[0], abs=2e-9 * k) and ga[1] == pytest.approx(var[0], abs=2e-8 * v * k)
        pm = hg.propagate_many(Q[key + "y"][0, j], u[0], Sigma[j])
        assert np.all(np.abs(pm - Q[key + "dens"][0, j]) <= bds[0])
        assert abs(hg.propagate(Q[key + "y"][0, j, 4], u[0], Sigma[j]) - Q[key + "dens"][0, j, 4]) <= bds[0][4]
    print("golden %s: worst dmean %.3e dvar %.3e, density %.1e of its bound" % ((key,) + tuple(worst)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n203_d3", "grid_int", "n256_d8"])
def test_golden_hg_through_the_classes(name):
    """(c) the reference's UncertaintyPropagationNumericalHG (n256_d8 recorded at order 2: tools/gen_quadrature_golden.py)"""
    gp, og, g = _golden_gp(name)
    _golden_through_class("hg_%s_" % name, gp, og.estimate_many, float(np.exp(g["theta"][0])))


@pytest.mark.gpu
def test_golden_hg_periodic():
    """(c) the reference's PeriodicCovariance model under HG: the one propagation that kernel has"""
    x, t, theta = pl.make_case(203, 3)
    gp = sk.GaussianProcess(x, t, sk.PeriodicCovariance(), theta.copy())
    assert gp._route() == "periodic"
    _golden_through_class("hgper_", gp, lambda xs: qm.periodic_estimate_many(x, t, theta, xs), float(np.exp(theta[0])))


def _class_equals_model_plus_reduce(gp, cls_kwargs, rule, root):
    rng = np.random.RandomState(8)
    d = gp.d
    lo, hi = np.min(gp.x, 0), np.max(gp.x, 0)
    U = lo + (hi - lo) * rng.uniform(0.3, 0.7, (4, d))
    Sigma = np.diag(((hi - lo) * 0.03) ** 2)
    Y = np.linspace(-1, 1, 7) + gp._get_mean_t()
    up = sk.UncertaintyPropagationNumericalHG(gp, **cls_kwargs)
    mean, var, m3, m4 = up.propagate_moments_many(U, Sigma)
    dens = up.propagate_density_many(Y, U, Sigma)
    z, wq = rule
    mu, s2 = gp.estimate_many(qm.nodes_plain(U, root(Sigma), z).reshape(4 * len(wq), d))
    mom, dd = _reduce(mu.reshape(4, -1), s2.reshape(4, -1), wq, Y, 1, 0.0)
    for got, ref in ((mean, mom[0]), (var, mom[1]), (m3, mom[3]), (m4, mom[4]), (dens, dd)):
        np.testing.assert_array_equal(got, ref)
    assert np.all(var > 0) and np.all(np.isfinite(dens))


@pytest.mark.gpu
def test_generic_and_spgp_routes():
    """(g) any other operator: the class is the model's own estimate_many on host-built nodes plus gpx_mixture_reduce, bit for bit; the
    generic route's gpx_fit_matrix handle is refused by the fused entry point"""
    g = load_golden("generic_ops")
    ggp = sk.GaussianProcess(g["wg_x"], g["wg_t"], make_warped_gaussian(sk.GaussianCovariance)(), g["wg_theta"].copy())
    assert ggp._route() == "generic"
    _class_equals_model_plus_reduce(ggp, dict(order=3), qm.hg_rule(3, ggp.d), qm.hg_root)
    d = ggp.d
    mom = np.full((5, 1), 7.25)
    st = _gpx.lib.gpx_propagate_quadrature_many(ggp._dev().handle, _gpx.ptr(np.zeros((1, d))), _gpx.ptr(np.eye(d)), 1, 1, _gpx.ptr(np.zeros((1, d))),
                                                _gpx.ptr(np.ones(1)), 1, None, 0, 1, 0.0, _gpx.ptr(mom), None)
    assert st == _gpx.GPX_ERR_STATE and "gpx_fit_matrix" in _gpx.last_error()
    np.testing.assert_array_equal(mom, np.full((5, 1), 7.25))
    rng = np.random.RandomState(5)
    N, d, m = 600, 3, 40
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    th = np.concatenate([np.log(np.array([2.0, 0.01] + [0.04] * d)), x[:m].ravel()])
    sgp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), th)
    assert sgp._route() == "spgp"
    _class_equals_model_plus_reduce(sgp, dict(order=4, full_sigma=True), qm.hg_rule(4, d), lambda S: qm.hg_root(S, True))


@pytest.mark.gpu
def test_mc_is_reproducible_and_agrees_with_hg():
    """(g) a fixed seed: the same bits twice; its mean within 5 standard errors sqrt(c2 / n) of order-8 Gauss-Hermite on the smooth d = 2 model
    (c2 = the variance of mu(x) under the input: what one sample of the mean scatters by), its density the same mixture's"""
    gp, og, g = _golden_gp("grid_int")
    Q = load_golden("quadrature")
    u, Sigma = Q["hg_grid_int_u"][0], Q["hg_grid_int_Sigma"][1]
    mc = sk.UncertaintyPropagationMC(gp, n=1000, seed=7)
    a, b = mc.propagate_GA(u, Sigma), mc.propagate_GA(u, Sigma)
    assert a == b
    hg = sk.UncertaintyPropagationNumericalHG(gp, order=8, full_sigma=True)
    m, var, _m3, _m4 = hg.propagate_moments_many(u[None], Sigma)
    ev = hg._reduce(u[None], Sigma)[0][2, 0]
    se = np.sqrt((var[0] - ev) / 1000)
    print("MC mean %.6f, HG order 8 %.6f, standard error %.2e" % (a[0], m[0], se))
    assert abs(a[0] - m[0]) <= 5 * se
    assert a[1] == pytest.approx(var[0], rel=5 * np.sqrt(2.0 / 1000))      # a variance estimate of n near-Gaussian draws scatters by sqrt(2 / n)
    # and the reduction is the model's: the class against the oracle on the same sample
    z, wq = qm.mc_rule(1000, 2, 7)
    mu, s2 = og.estimate_many(qm.nodes_plain(u[None], qm.mc_root(Sigma), z)[0])
    lm = qm.mixture_ld(mu, s2, wq)[0]
    assert a[0] == pytest.approx(float(lm[0]), abs=1e-9) and a[1] == pytest.approx(float(lm[1]), abs=1e-8 * 2 + 4e-9)


@pytest.mark.gpu
def test_no_side_effects_on_the_handle():
    """(h) Approx.propagate_GA with the single-u cache warm, and estimate_many, return the same bits before and after a quadrature call"""
    gp, og, g = _golden_gp("n203_d3")
    u, S = g["u0"], g["Sigma0"]
    ap = sk.UncertaintyPropagationApprox(gp)
    ap.propagate_GA(u, S)                       # warms the cache of u
    before = (ap.propagate_GA(u, S), gp.estimate_many(g["xs"]))
    sk.UncertaintyPropagationNumericalHG(gp).propagate_density_many(np.linspace(-1, 1, 5), g["xs"][:7], g["Sigma1"])
    after = (ap.propagate_GA(u, S), gp.estimate_many(g["xs"]))
    assert before[0] == after[0]
    np.testing.assert_array_equal(before[1][0], after[1][0])
    np.testing.assert_array_equal(before[1][1], after[1][1])
