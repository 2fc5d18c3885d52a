"""Batched Approx propagation: UncertaintyPropagationApprox.propagate_GA_many / propagate_mean_many and gpx_propagate_approx_many.

Every input's C, tr = tracedot(H, Sigma) and J_1..J_d are d + 2 right-hand sides of the many-right-hand-side triangular solver of
estimate_many; a caller's loop over propagate_GA (skgpuppy/UncertaintyPropagation.py:490-523) is what the call replaces, so the checks
are the single call's: the golden vectors and the oracle with the tolerances of tests/test_gpu_parity.py, and the single call itself.
Two device paths that are each held to 1e-9 (mean) and 1e-8 v (variance) of the oracle (test_c3_fit_and_propagation_against_oracle) may
differ by at most twice that: the bound of every batched-against-single comparison here.  Every input of every batch is compared.

The CPU cases need no device: the methods and the symbol exist, and a null handle is refused before anything is touched.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GP_CASES, load_golden, torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from oracle import oracle as orc

from _operators import make_warped_gaussian
from _propagate_many_worker import inputs as _inputs

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "_propagate_many_worker.py")
GPX_K_QUAD, GPX_K_EXACT = 5, 6      # include/gpx.h


# ------------------------------------------------------------------------------------------------
# without a device
# ------------------------------------------------------------------------------------------------
def test_batched_methods_and_symbol_exist():
    assert callable(getattr(sk.UncertaintyPropagationApprox, "propagate_GA_many"))
    assert callable(getattr(sk.UncertaintyPropagationApprox, "propagate_mean_many"))
    assert "gpx_propagate_approx_many" in _gpx.SIGNATURES
    assert hasattr(_gpx.lib, "gpx_propagate_approx_many")
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpx.h")).read()
    assert "int gpx_propagate_approx_many(" in header
    assert _gpx.lib.gpx_abi_version() == 1      # additive


def test_null_handle_is_refused_and_no_output_touched():
    U, S = np.zeros((3, 2)), np.eye(2)
    out = [np.full(3, 7.25) for _ in range(4)]
    st = _gpx.lib.gpx_propagate_approx_many(None, _gpx.ptr(U), _gpx.ptr(S), 1, 3, *[_gpx.ptr(o) for o in out])
    assert st == _gpx.GPX_ERR_BAD_ARG
    assert "null handle" in _gpx.last_error()
    for o in out:
        np.testing.assert_array_equal(o, np.full(3, 7.25))


# ------------------------------------------------------------------------------------------------
# on the device
# ------------------------------------------------------------------------------------------------
def _raw_many(gp, U, S, shared):
    """gpx_propagate_approx_many itself: (mean without meant, var, sigma2, rest)"""
    U, S = _gpx.f64(U), _gpx.f64(S)
    out = [np.empty(len(U)) for _ in range(4)]
    _gpx.check(_gpx.lib.gpx_propagate_approx_many(gp._dev().handle, _gpx.ptr(U), _gpx.ptr(S), int(shared), len(U), *[_gpx.ptr(o) for o in out]),
               "gpx_propagate_approx_many")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", GP_CASES)
def test_golden_one_call_for_all_pairs(name):
    """(1) ONE call with all nu x nS (u, Sigma) pairs of the fixture as a per-input-Sigma batch, test_propagation_golden's tolerances"""
    g = load_golden(name)
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    v = np.exp(g["theta"][0])
    k = 10.0 if name == "metis" else 1.0
    pairs = [(iu, iS) for iu in range(int(g["nu"])) for iS in range(int(g["nS"]))]
    U = np.array([g["u%d" % iu] for iu, _ in pairs])
    S = np.array([g["Sigma%d" % iS] for _, iS in pairs])
    up = sk.UncertaintyPropagationApprox(gp)
    mean, var = up.propagate_GA_many(U, S)
    mean_only = up.propagate_mean_many(U, S)
    assert mean.shape == var.shape == mean_only.shape == (len(pairs),)
    for i, (iu, iS) in enumerate(pairs):
        ref = g["approx_u%d_S%d" % (iu, iS)]
        print("golden %s u%d S%d: dmean %.3e dvar %.3e" % (name, iu, iS, abs(mean[i] - ref[0]), abs(var[i] - ref[1])))
        assert mean[i] == pytest.approx(ref[0], abs=1e-9 * k)
        assert var[i] == pytest.approx(ref[1], abs=1e-8 * v * k)
        assert mean_only[i] == pytest.approx(float(g["approx_mean_only_u%d_S%d" % (iu, iS)]), abs=1e-9 * k)


_RAGGED = {}     # N -> (gp, oracle gp, x)


def _ragged_gp(N):
    if N not in _RAGGED:
        d = {127: 3, 640: 6, 1500: 8}[N]
        rng = np.random.RandomState(100 + N + d)
        x = rng.uniform(0, 10, (N, d))
        t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
        theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
        _RAGGED[N] = (sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy()), orc.OracleGP(x, t, theta), x)
    return _RAGGED[N]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 130, 517])
@pytest.mark.parametrize("N", [127, 640, 1500])
def test_against_oracle_ragged_batches(N, B):
    """(2) random u (every 37th a copy of a training row: the quirk), a random SPD full Sigma per input, against oracle.approx_propagate with
    the tolerances of test_against_oracle_ragged's propagation asserts (mean 1e-9, variance 2e-8); sigma2 and rest against approx_parts
    (each is a part of the variance: the variance's tolerance)"""
    gp, og, x = _ragged_gp(N)
    U, S = _inputs(x, B, gp.d, N + B)
    mean, var = sk.UncertaintyPropagationApprox(gp).propagate_GA_many(U, S)
    m0, v0, s2, rest = _raw_many(gp, U, S, False)
    np.testing.assert_array_equal(m0 + gp.meant, mean)
    np.testing.assert_array_equal(v0, var)
    worst = [0.0] * 4
    for i in range(B):
        om, os2, orest = orc.approx_parts(og, U[i], S[i])
        oma, ova = orc.approx_propagate(og, U[i], S[i])
        worst = [max(a, b) for a, b in zip(worst, (abs(mean[i] - oma), abs(var[i] - ova), abs(s2[i] - os2), abs(rest[i] - orest)))]
        assert mean[i] == pytest.approx(oma, abs=1e-9) and var[i] == pytest.approx(ova, abs=2e-8), i
        assert m0[i] == pytest.approx(om, abs=1e-9), i
        assert s2[i] == pytest.approx(os2, abs=2e-8) and rest[i] == pytest.approx(orest, abs=2e-8), i
    print("oracle N=%d B=%d: worst dmean %.3e dvar %.3e dsigma2 %.3e drest %.3e" % ((N, B) + tuple(worst)))


_EDGE = {}       # d -> (gp, x)


def _edge_gp(d, N=640):
    """the ragged recipe with the length scales kept alive at large d (w = 0.04 * 3 / d)"""
    if d not in _EDGE:
        rng = np.random.RandomState(100 + N + d)
        x = rng.uniform(0, 10, (N, d))
        t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
        theta = np.log(np.array([2.0, 0.01] + [0.04 * 3.0 / d] * d))
        _EDGE[d] = (sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy()), x)
    return _EDGE[d]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 130])
@pytest.mark.parametrize("d", [1, 9, 64])
def test_ragged_batches_against_the_single_call_at_the_variant_edges(d, B):
    """(2b) d = 9 is the first d of approx_build_many_kernel<0> (differences recomputed from the LDS tile), d = 1 and d = 64 are the ends of
    the range (64: a 64 KB tile); N = 640, the inputs of (2), every input of the batch against propagate_GA.  Bound: twice the oracle
    tolerance of each device path (module docstring), v = 2."""
    gp, x = _edge_gp(d)
    U, S = _inputs(x, B, d, 640 + B)
    mean, var = sk.UncertaintyPropagationApprox(gp).propagate_GA_many(U, S)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    dm = dv = 0.0
    for i in range(B):
        m1, v1 = sk.UncertaintyPropagationApprox(gp).propagate_GA(U[i], S[i])
        dm, dv = max(dm, abs(mean[i] - m1)), max(dv, abs(var[i] - v1))
        assert mean[i] == pytest.approx(m1, abs=2 * 1e-9) and var[i] == pytest.approx(v1, abs=2 * 1e-8 * 2.0), i
    print("single call d=%d B=%d: worst dmean %.3e dvar %.3e" % (d, B, dm, dv))


def _child(args, extra, timeout=600):
    env = dict(os.environ)
    env.update(extra)
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args, extra, r.returncode, r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


@pytest.mark.gpu
@pytest.mark.parametrize("emu", ["1", "0"])
def test_full_size_against_the_single_call(emu):
    """(3) N = 16384, d = 8, B = 2048 (20480 solver rows: the K >= 4096 updates run emulated on the int8 matrix cores, or in fp64 with
    GPX_EMU_F64=0), 16 inputs of the batch also through propagate_GA one by one.  Bound: twice the oracle tolerance of each device path
    (module docstring), v = 2.  Measured (profiles/r08_propagate_many.txt): dmean 4.1e-13 / dvar 2.2e-15 emulated, 4.6e-13 / 2.9e-15 in fp64."""
    r = _child(["compare", 16384, 8, 2048, 16], {"GPX_EMU_F64": emu})
    print("full size vs single call, GPX_EMU_F64=%s: dmean %.3e dvar %.3e over %d inputs" % (emu, r["dmean"], r["dvar"], r["singles"]))
    assert r["finite"] and r["singles"] == 16
    assert r["dmean"] <= 2 * 1e-9 and r["dvar"] <= 2 * 1e-8 * 2.0


@pytest.mark.gpu
def test_independence_of_position_split_and_sigma_form():
    """(4) an input's result does not depend on its place in the batch, on the other inputs, or on how Sigma is passed.  The split holds
    bit for bit when both calls take the same route: each of them has more than 32 solver rows (B (d + 2) > 32; below that the
    few-right-hand-side solver serves the call) -- the many-right-hand-side solver computes every row the same way whatever the number of
    rows (tests/test_gpu_parity.py, test_full_size_properties (4))."""
    gp, _og, x = _ragged_gp(1500)
    B, d = 130, gp.d
    U, S = _inputs(x, B, d, 77)
    one = _raw_many(gp, U, S, False)
    rev = _raw_many(gp, U[::-1], S[::-1], False)
    for a, b in zip(one, rev):
        np.testing.assert_array_equal(a, b[::-1])
    cut = 47                                                # 47 * 10 and 83 * 10 rows: both many-right-hand-side calls
    assert cut * (d + 2) > 32 and (B - cut) * (d + 2) > 32
    head, tail = _raw_many(gp, U[:cut], S[:cut], False), _raw_many(gp, U[cut:], S[cut:], False)
    for a, h, t in zip(one, head, tail):
        np.testing.assert_array_equal(a, np.concatenate([h, t]))
    shared = _raw_many(gp, U, S[5], True)
    repeated = _raw_many(gp, U, np.repeat(S[5][None], B, 0), False)
    for a, b in zip(shared, repeated):
        np.testing.assert_array_equal(a, b)
    up = sk.UncertaintyPropagationApprox(gp)
    ms, vs = up.propagate_GA_many(U, S[5])                  # the (d, d) form of the Python call is the shared form
    np.testing.assert_array_equal(ms, shared[0] + gp.meant)
    np.testing.assert_array_equal(vs, shared[1])


def _fresh_gp(N=2200, d=5):
    rng = np.random.RandomState(9 + N)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    return sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy()), x


def _launches(gp, cls):
    n, ms, w = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_profile_read(gp._dev().handle, cls, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w)), "gpx_profile_read")
    return n.value


@pytest.mark.gpu
def test_no_side_effects_on_the_single_input_path():
    """(5) after a fresh fit a B = 256 batched call launches nothing of the K^-1 pass (GPX_K_QUAD) or the Exact sum (GPX_K_EXACT), leaves
    the Python object's single-input cache alone, and a following propagate_GA returns the bits it returns without the batched call"""
    gp, x = _fresh_gp()
    U, S = _inputs(x, 256, gp.d, 11)
    h = gp._dev().handle
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 2), "gpx_profile_enable")
    _gpx.check(_gpx.lib.gpx_profile_reset(h), "gpx_profile_reset")
    up = sk.UncertaintyPropagationApprox(gp)
    mean, var = up.propagate_GA_many(U, S)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert _launches(gp, GPX_K_QUAD) == 0 and _launches(gp, GPX_K_EXACT) == 0
    assert gp._Kinv is None
    assert up.u is None and up._cjh is None and up._kv is None
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 0), "gpx_profile_enable")
    after = up.propagate_GA(U[3], S[3])
    gp2, _x = _fresh_gp()
    plain = sk.UncertaintyPropagationApprox(gp2).propagate_GA(U[3], S[3])
    assert after == plain                                   # bit for bit
    # and the other way round: a batched call after single calls (cached u on the handle) is the batched call of a fresh fit
    m2, v2 = sk.UncertaintyPropagationApprox(gp2).propagate_GA_many(U, S)
    np.testing.assert_array_equal(m2, mean)
    np.testing.assert_array_equal(v2, var)


@pytest.mark.gpu
def test_edges():
    """(6) B = 0; B (d + 2) <= 32 (the few-right-hand-side route) against the single call within the two-device-paths bound; shape errors;
    a gpx_fit_matrix handle; a generic-route GP equals its own loop exactly"""
    gp, x = _fresh_gp()
    d, v = gp.d, 2.0
    up = sk.UncertaintyPropagationApprox(gp)
    m, var = up.propagate_GA_many(np.zeros((0, d)), np.eye(d))
    assert m.shape == var.shape == (0,)
    assert up.propagate_mean_many(np.zeros((0, d)), np.zeros((0, d, d))).shape == (0,)
    for B in (1, 4):                                        # 7 and 28 solver rows
        assert B * (d + 2) <= 32
        U, S = _inputs(x, B, d, 21 + B)
        U[0] = x[17]                                        # the quirk on this route too
        mean, var = up.propagate_GA_many(U, S)
        for i in range(B):
            m1, v1 = sk.UncertaintyPropagationApprox(gp).propagate_GA(U[i], S[i])
            print("few rows B=%d input %d: dmean %.3e dvar %.3e" % (B, i, abs(mean[i] - m1), abs(var[i] - v1)))
            assert mean[i] == pytest.approx(m1, abs=2 * 1e-9) and var[i] == pytest.approx(v1, abs=2 * 1e-8 * v)
    for bad_U, bad_S in [(np.zeros(d), np.eye(d)), (np.zeros((3, d + 1)), np.eye(d)), (np.zeros((3, d)), np.eye(d + 1)),
                         (np.zeros((3, d)), np.zeros((2, d, d))), (np.zeros((3, d)), np.zeros(d)), (np.zeros((2, 3, d)), np.eye(d))]:
        with pytest.raises(ValueError):
            up.propagate_GA_many(bad_U, bad_S)
        with pytest.raises(ValueError):
            up.propagate_mean_many(bad_U, bad_S)
    # a handle built from a supplied matrix has no inputs / theta to evaluate the kernel on
    from skgpuppy_amd.Covariance import _MatrixModel
    mm = _MatrixModel(np.eye(4) * 2.0, np.arange(4.0))
    out = [np.full(2, 7.25) for _ in range(4)]
    st = _gpx.lib.gpx_propagate_approx_many(mm.handle, _gpx.ptr(np.zeros((2, 1))), _gpx.ptr(np.eye(1)), 1, 2, *[_gpx.ptr(o) for o in out])
    assert st == _gpx.GPX_ERR_STATE and "gpx_fit_matrix" in _gpx.last_error()
    np.testing.assert_array_equal(out[0], np.full(2, 7.25))
    st = _gpx.lib.gpx_propagate_approx_many(gp._dev().handle, _gpx.ptr(np.zeros((2, d))), _gpx.ptr(np.eye(d)), 1, -1, *[_gpx.ptr(o) for o in out])
    assert st == _gpx.GPX_ERR_BAD_ARG
    st = _gpx.lib.gpx_propagate_approx_many(gp._dev().handle, _gpx.ptr(np.zeros((2, d))), _gpx.ptr(np.eye(d)), 1, 2, None, _gpx.ptr(out[1]), None, None)
    assert st == _gpx.GPX_ERR_BAD_ARG
    mm.close()
    # generic route (an operator that overrides a matrix builder): the documented loop over the single-input path
    g = load_golden("generic_ops")
    ggp = sk.GaussianProcess(g["wg_x"], g["wg_t"], make_warped_gaussian(sk.GaussianCovariance)(), g["wg_theta"].copy())
    gd = ggp.d
    rng = np.random.RandomState(4)
    GU = rng.uniform(g["wg_x"].min(0), g["wg_x"].max(0), (5, gd))
    GS = np.array([np.diag(rng.uniform(0.005, 0.05, gd)) for _ in range(5)])
    gup = sk.UncertaintyPropagationApprox(ggp)
    assert gup._generic()
    gm, gv = gup.propagate_GA_many(GU, GS)
    gmo = gup.propagate_mean_many(GU, GS[0])
    for i in range(5):
        one = sk.UncertaintyPropagationApprox(ggp)
        assert (gm[i], gv[i]) == one.propagate_GA(GU[i], GS[i])
        assert gmo[i] == one.propagate_mean(GU[i], GS[0])
    assert gup.u is None
