"""Batched inverse propagation: gpx_propagate_dvh_many, UncertaintyPropagationApprox._get_variance_dv_many and
InverseUncertaintyPropagationApprox.get_best_solution_many / _closed_form.

Every input's C, J_1..J_d and H_11..H_dd are 2 d + 1 right-hand sides of the many-right-hand-side triangular solver of estimate_many; a
caller's loop over get_best_solution (skgpuppy/InverseUncertaintyPropagation.py:139-173: d calls of _get_variance_dv_h and one _getFactor
per operating point) is what the call replaces.  The tolerances are the project's own: dvh against the oracle rtol 1e-6, atol 1e-8 v
(tests/test_gpu_parity.py, test_propagation_golden), sigma2 abs 2e-8 (tests/test_propagate_many.py); two device paths that are each held to
these may differ by twice as much (that module's docstring): the bound of every batched-against-single comparison here.

The solution itself is held to the first-order image of the two tolerances.  With c = I = 1 and no co-estimation
sol_k = (T - sigma2) sqrt(1 / dvh_k) / sum_j sqrt(dvh_j): a relative error e_j of dvh_j moves sqrt(1 / dvh_k) by e_k / 2 and the sum by at most
max_j e_j / 2, an absolute error a of sigma2 moves T - sigma2 by a / (T - sigma2), so
    rel <= 1.1 (2e-8 / (T - sigma2) + max_j (1e-6 + 1e-8 v / dvh_j)),     T - sigma2 = 0.05 here, 1.1 for the second-order terms.

The last test is the twin of the chunk-boundary test for gpx_propagate_approx_many, which had none at a small size.

The CPU cases need no device: the methods and the symbol exist, a null handle is refused before anything is touched, and the closed form
reproduces the golden solutions from the oracle's dvh and sigma2.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import GP_CASES, load_golden, torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx
from oracle import oracle as orc

from _operators import make_warped_gaussian
from _propagate_many_worker import inputs as _inputs
from test_propagate_many import GPX_K_EXACT, GPX_K_QUAD, _edge_gp, _fresh_gp, _launches, _ragged_gp

HERE = os.path.dirname(os.path.abspath(__file__))
GPX_K_GRAM, GPX_K_REDUCE = 0, 4     # include/gpx.h
V = 2.0                             # the signal variance of every recipe below
IUP = sk.InverseUncertaintyPropagationApprox


def _oracle_dvh_sigma2(og, u):
    cache = orc.cjh(og, u)
    dvh = np.array([orc.approx_dvh(og, u, h, cache) for h in range(og.d)])
    return dvh, orc.approx_parts(og, u, np.zeros((og.d, og.d)), cache)[1]


# ------------------------------------------------------------------------------------------------
# without a device
# ------------------------------------------------------------------------------------------------
def test_batched_methods_and_symbol_exist():
    """(1) the entry point in the binding, the library and the header; the three Python methods"""
    assert callable(getattr(sk.UncertaintyPropagationApprox, "_get_variance_dv_many"))
    assert callable(getattr(IUP, "get_best_solution_many"))
    assert callable(getattr(IUP, "_closed_form"))
    assert "gpx_propagate_dvh_many" in _gpx.SIGNATURES
    assert hasattr(_gpx.lib, "gpx_propagate_dvh_many")
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpx.h")).read()
    assert "int gpx_propagate_dvh_many(" in header
    assert _gpx.lib.gpx_abi_version() == 1      # additive


def test_null_handle_is_refused_and_no_output_touched():
    """(1) a null handle is GPX_ERR_BAD_ARG before anything is written"""
    U = np.zeros((3, 2))
    dvh, s2 = np.full((3, 2), 7.25), np.full(3, 7.25)
    st = _gpx.lib.gpx_propagate_dvh_many(None, _gpx.ptr(U), 3, _gpx.ptr(dvh), _gpx.ptr(s2))
    assert st == _gpx.GPX_ERR_BAD_ARG
    assert "null handle" in _gpx.last_error()
    np.testing.assert_array_equal(dvh, np.full((3, 2), 7.25))
    np.testing.assert_array_equal(s2, np.full(3, 7.25))


def test_closed_form_reproduces_the_golden_solutions_from_the_oracle():
    """(2) kat1_grid, u = [5.25, 4.75], c = [4, 1], target 0.02: the oracle's dvh and sigma2 through _closed_form against iup_approx
    (I = 1 / c) and iup_approx_coest (I = [0.25, 2], inputs 0 and 1 co-estimated) at test_inverse_uncertainty_propagation_golden's rtol;
    a row with one dvh <= 0 and a row whose target lies below sigma2 come back NaN, silently, and leave their neighbours alone"""
    g = load_golden("kat1_grid")
    og = orc.OracleGP(g["x"], g["t_raw"], g["theta"])
    u, c = np.array([5.25, 4.75]), np.array([4.0, 1.0])
    dvh, s2 = _oracle_dvh_sigma2(og, u)
    assert (dvh > 0).all() and s2 < 0.02
    one = IUP._closed_form(dvh[None], s2, c, 1 / c, [], 0.02)
    assert one.shape == (1, 2)
    np.testing.assert_allclose(one[0], g["iup_approx"], rtol=1e-6)
    coest = IUP._closed_form(dvh[None], np.array([s2]), c, np.array([0.25, 2.0]), [[0, 1]], np.array([0.02]))
    np.testing.assert_allclose(coest[0], g["iup_approx_coest"], rtol=1e-6)
    # rows 0, 2, 4 feasible, row 1 with dvh_1 < 0, row 3 with the target below sigma2 (as sigma2, then as a per-row target)
    D = np.array([dvh, dvh * [1.0, -1.0], dvh, dvh, dvh])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # no warning spam
        sol = IUP._closed_form(D, np.array([s2, s2, s2, 0.5, s2]), c, 1 / c, [], 0.02)
        sol_t = IUP._closed_form(D, s2, c, 1 / c, [], np.array([0.02, 0.02, 0.02, 0.5 * s2, 0.02]))
        sol_z = IUP._closed_form(np.array([dvh, [dvh[0], 0.0]]), s2, c, 1 / c, [], 0.02)
        sol_c = IUP._closed_form(D, np.array([s2, s2, s2, 0.5, s2]), c, np.array([0.25, 2.0]), [[0, 1]], 0.02)
    for s in (sol, sol_t):
        assert np.isnan(s[1]).all() and np.isnan(s[3]).all()
        for i in (0, 2, 4):
            np.testing.assert_array_equal(s[i], one[0])
    np.testing.assert_array_equal(sol_z[0], one[0])
    assert np.isnan(sol_z[1]).all()
    assert np.isnan(sol_c[3]).all()
    for i in (0, 2, 4):
        np.testing.assert_array_equal(sol_c[i], coest[0])
    # the folded derivative decides under co-estimation: dvh_0 - dvh_1 I_0 / I_1 > 0 here, so row 1 has a solution
    assert dvh[0] - dvh[1] * 0.25 / 2.0 > 0 and (sol_c[1] > 0).all()


# ------------------------------------------------------------------------------------------------
# on the device
# ------------------------------------------------------------------------------------------------
def _raw(gp, U, want_sigma2=True):
    """gpx_propagate_dvh_many itself on host pointers: (dvh [B, d], sigma2 [B] or None)"""
    U = _gpx.f64(U)
    dvh, s2 = np.empty((len(U), gp.d)), np.empty(len(U))
    _gpx.check(_gpx.lib.gpx_propagate_dvh_many(gp._dev().handle, _gpx.ptr(U), len(U), _gpx.ptr(dvh), _gpx.ptr(s2) if want_sigma2 else None),
               "gpx_propagate_dvh_many")
    return dvh, (s2 if want_sigma2 else None)


def _single(gp, u):
    """the single-input calls: (dvh [d] through _get_variance_dv_h for every h, sigma2 through _get_sigma2)"""
    up = sk.UncertaintyPropagationApprox(gp)
    return np.array([up._get_variance_dv_h(u, h) for h in range(gp.d)]), up._get_sigma2(u)


def _assert_two_paths(gp, U, dvh, s2, rows, what):
    dd = ds = 0.0
    for i in rows:
        d1, s1 = _single(gp, U[i])
        dd, ds = max(dd, np.abs(dvh[i] - d1).max()), max(ds, abs(s2[i] - s1))
        np.testing.assert_allclose(dvh[i], d1, rtol=2 * 1e-6, atol=2 * 1e-8 * V, err_msg="input %d" % i)
        assert s2[i] == pytest.approx(s1, abs=2 * 2e-8), i
    print("%s: %d inputs against the single calls, worst ddvh %.3e dsigma2 %.3e" % (what, len(rows), dd, ds))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GP_CASES)
def test_golden_one_call_for_all_inputs(name):
    """(3) ONE call with every u of the fixture, test_propagation_golden's tolerances; kat1_grid: the golden solutions as well"""
    g = load_golden(name)
    gp = sk.GaussianProcess(g["x"], g["t_raw"], sk.GaussianCovariance(), g["theta"].copy())
    v = np.exp(g["theta"][0])
    k = 10.0 if name == "metis" else 1.0
    nu = int(g["nu"])
    U = np.array([g["u%d" % iu] for iu in range(nu)])
    dvh, s2 = sk.UncertaintyPropagationApprox(gp)._get_variance_dv_many(U)
    assert dvh.shape == (nu, gp.d) and s2.shape == (nu,)
    for iu in range(nu):
        print("golden %s u%d: worst ddvh %.3e" % (name, iu, np.abs(dvh[iu] - g["dvh_u%d" % iu]).max()))
        np.testing.assert_allclose(dvh[iu], g["dvh_u%d" % iu], rtol=1e-6 * k, atol=1e-8 * v * k)
    if name == "kat1_grid":
        u3, c = np.tile([5.25, 4.75], (3, 1)), np.array([4.0, 1.0])
        sol = IUP(0.02, gp, None, c, 1 / c).get_best_solution_many(u3)
        sol_c = IUP(0.02, gp, None, c, np.array([0.25, 2.0]), coestimated=[[0, 1]]).get_best_solution_many(u3)
        assert sol.shape == sol_c.shape == (3, 2)
        for i in range(3):
            np.testing.assert_allclose(sol[i], g["iup_approx"], rtol=1e-6)
            np.testing.assert_allclose(sol_c[i], g["iup_approx_coest"], rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("N", [127, 640, 1500])
def test_against_oracle_ragged_batches(N, B):
    """(4) the inputs of test_propagate_many (every 37th a copy of a training row: the +vt quirk): dvh and sigma2 of every input against the
    oracle (N = 1500: the inputs with i % 4 == 0 or i % 37 == 0), then the solution for c = I = 1 and the target sigma2_oracle + 0.05 against
    _closed_form of the oracle's values within the first-order bound of the module docstring.  An input with an oracle dvh_k < 1e-3 is
    left out of the solution comparison only (at most 15 % of the compared inputs; CPU oracle at B = 130: 12.3 %, 6.9 %, 5.6 %); one with
    an oracle dvh_k < -1e-6 has no solution and must come back as a NaN row."""
    gp, og, x = _ragged_gp(N)
    d = gp.d
    U = _inputs(x, B, d, N + B)[0]
    rows = [i for i in range(B) if N < 1500 or i % 4 == 0 or i % 37 == 0]
    dvh, s2 = sk.UncertaintyPropagationApprox(gp)._get_variance_dv_many(U)
    odvh, os2 = np.empty((B, d)), np.empty(B)
    for i in rows:
        odvh[i], os2[i] = _oracle_dvh_sigma2(og, U[i])
    dd = ds = 0.0
    for i in rows:
        dd, ds = max(dd, np.abs(dvh[i] - odvh[i]).max()), max(ds, abs(s2[i] - os2[i]))
        np.testing.assert_allclose(dvh[i], odvh[i], rtol=1e-6, atol=1e-8 * V, err_msg="input %d" % i)
        assert s2[i] == pytest.approx(os2[i], abs=2e-8), i
    print("oracle N=%d B=%d: %d inputs, worst ddvh %.3e dsigma2 %.3e" % (N, B, len(rows), dd, ds))
    # the solution
    one = np.ones(d)
    T = np.full(B, np.nan)
    T[rows] = os2[rows] + 0.05
    iup = IUP(None, gp, None, one, one)
    sol = iup.get_best_solution_many(U, np.where(np.isnan(T), 1.0, T))
    again = IUP._closed_form(*sk.UncertaintyPropagationApprox(gp)._get_variance_dv_many(U), one, one, [], np.where(np.isnan(T), 1.0, T))
    np.testing.assert_array_equal(sol, again)               # bit for bit
    ref = IUP._closed_form(odvh[rows], os2[rows], one, one, [], T[rows])
    left_out, worst = 0, 0.0
    for r, i in enumerate(rows):
        if (odvh[i] < -1e-6).any():
            assert np.isnan(sol[i]).all(), i
        if (odvh[i] < 1e-3).any():
            left_out += 1
            continue
        bound = 1.1 * (2e-8 / 0.05 + (1e-6 + 1e-8 * V / odvh[i]).max())
        rel = np.abs(sol[i] - ref[r]) / np.abs(ref[r])
        worst = max(worst, (rel / bound).max())
        assert np.isfinite(sol[i]).all() and (rel <= bound).all(), (i, rel, bound)
    print("solution N=%d B=%d: %d of %d inputs left out (a dvh_k < 1e-3), worst error / bound %.3e" % (N, B, left_out, len(rows), worst))
    if B == 130:
        assert left_out <= 0.15 * len(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 130])
@pytest.mark.parametrize("d", [1, 8, 9, 64])
def test_ragged_batches_against_the_single_calls_at_the_variant_edges(d, B):
    """(5) d = 8 is the last d of the <8> templates of both kernels (differences and the 3 d + 1 sums in registers), d = 9 the first of the
    <0> ones, d = 1 and d = 64 the ends of the range (64: a 64 KB tile, 129 rows per input); N = 640, every input of the batch against
    _get_variance_dv_h (all h) and _get_sigma2 within the two-device-paths bound"""
    gp, x = _edge_gp(d)
    U = _inputs(x, B, d, 640 + B)[0]
    dvh, s2 = sk.UncertaintyPropagationApprox(gp)._get_variance_dv_many(U)
    assert dvh.shape == (B, d) and np.isfinite(dvh).all() and np.isfinite(s2).all()
    _assert_two_paths(gp, U, dvh, s2, range(B), "single call d=%d B=%d" % (d, B))


_SMALL = {}


def _small_gp(N=127, d=8):
    """the ragged recipe at N = 127, d = 8: 128 padded columns, so 32768 solver rows are 34 MB"""
    if (N, d) not in _SMALL:
        rng = np.random.RandomState(100 + N + d)
        x = rng.uniform(0, 10, (N, d))
        t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
        theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
        _SMALL[(N, d)] = (sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy()), x)
    return _SMALL[(N, d)]


@pytest.mark.gpu
def test_chunk_boundary():
    """(6) N = 127, d = 8, B = 2000: 34000 rows against the 32768-row chunk, so two chunks of 1927 and 73 inputs (an input never straddles
    them).  All finite; the inputs on both sides of the boundary, the ends and twelve random ones against the single calls; the first
    chunk's inputs equal, bit for bit, a call on them alone."""
    gp, x = _small_gp()
    B, first = 2000, 32768 // 17
    assert first == 1927 and B * 17 > 32768
    U = _inputs(x, B, gp.d, 127 + B)[0]
    dvh, s2 = _raw(gp, U)
    assert np.isfinite(dvh).all() and np.isfinite(s2).all()
    pick = [0, first - 1, first, B - 1] + [int(i) for i in np.random.RandomState(6).choice(B, 12, replace=False)]
    _assert_two_paths(gp, U, dvh, s2, pick, "chunk boundary")
    head_dvh, head_s2 = _raw(gp, U[:first])
    np.testing.assert_array_equal(dvh[:first], head_dvh)
    np.testing.assert_array_equal(s2[:first], head_s2)


@pytest.mark.gpu
def test_independence_of_position_split_and_pointer_kind():
    """(7) an input's result does not depend on its place in the batch, on the other inputs, or on where the arrays live.  The split holds
    bit for bit when both calls take the same route: each has more than 32 solver rows."""
    gp, _og, x = _ragged_gp(1500)
    B, d = 130, gp.d
    U = _inputs(x, B, d, 78)[0]
    one = _raw(gp, U)
    rev = _raw(gp, U[::-1])
    for a, b in zip(one, rev):
        np.testing.assert_array_equal(a, b[::-1])
    cut = 47
    assert cut * (2 * d + 1) > 32 and (B - cut) * (2 * d + 1) > 32
    head, tail = _raw(gp, U[:cut]), _raw(gp, U[cut:])
    for a, h, t in zip(one, head, tail):
        np.testing.assert_array_equal(a, np.concatenate([h, t]))
    Ud = torch.as_tensor(np.ascontiguousarray(U)).cuda()
    dvh_d = torch.empty((B, d), dtype=torch.float64, device="cuda")
    s2_d = torch.empty(B, dtype=torch.float64, device="cuda")
    vp = lambda tt: ctypes.c_void_p(tt.data_ptr())  # noqa: E731
    _gpx.check(_gpx.lib.gpx_propagate_dvh_many(gp._dev().handle, vp(Ud), B, vp(dvh_d), vp(s2_d)), "gpx_propagate_dvh_many")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dvh_d.cpu().numpy(), one[0])
    np.testing.assert_array_equal(s2_d.cpu().numpy(), one[1])


@pytest.mark.gpu
def test_no_side_effects_on_the_single_input_path():
    """(8) after a fresh fit a B = 256 call launches nothing of the K^-1 pass (GPX_K_QUAD) or the Exact sum (GPX_K_EXACT) -- its own two
    kernels count as gram and reduce --, builds no K^-1, leaves the Python object's single-input cache alone, and a following
    _get_variance_dv_h returns the bits it returns without the batched call"""
    gp, x = _fresh_gp()
    U = _inputs(x, 256, gp.d, 12)[0]
    h = gp._dev().handle
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 2), "gpx_profile_enable")
    _gpx.check(_gpx.lib.gpx_profile_reset(h), "gpx_profile_reset")
    up = sk.UncertaintyPropagationApprox(gp)
    dvh, s2 = up._get_variance_dv_many(U)
    assert np.isfinite(dvh).all() and np.isfinite(s2).all()
    assert _launches(gp, GPX_K_QUAD) == 0 and _launches(gp, GPX_K_EXACT) == 0
    assert _launches(gp, GPX_K_GRAM) >= 1 and _launches(gp, GPX_K_REDUCE) >= 1
    assert gp._Kinv is None
    assert up.u is None and up._cjh is None and up._kv is None
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 0), "gpx_profile_enable")
    after = [up._get_variance_dv_h(U[3], k) for k in range(gp.d)]
    gp2, _x = _fresh_gp()
    up2 = sk.UncertaintyPropagationApprox(gp2)
    plain = [up2._get_variance_dv_h(U[3], k) for k in range(gp.d)]
    assert after == plain                                   # bit for bit
    # and the other way round: a batched call after single calls (cached u on the handle) is the batched call of a fresh fit
    dvh2, s22 = up2._get_variance_dv_many(U)
    np.testing.assert_array_equal(dvh2, dvh)
    np.testing.assert_array_equal(s22, s2)


@pytest.mark.gpu
def test_edges():
    """(9) B = 0; B (2 d + 1) <= 32 (the few-right-hand-side route) against the single calls; shape errors; a gpx_fit_matrix handle; bad
    arguments; sigma2_out = NULL; a generic-route GP equals its own loop exactly"""
    gp, x = _fresh_gp()
    d = gp.d
    up = sk.UncertaintyPropagationApprox(gp)
    iup = IUP(0.5, gp, None, np.ones(d), np.ones(d))
    dvh, s2 = up._get_variance_dv_many(np.zeros((0, d)))
    assert dvh.shape == (0, d) and s2.shape == (0,)
    assert iup.get_best_solution_many(np.zeros((0, d))).shape == (0, d)
    for B in (1, 2):                                        # 11 and 22 solver rows
        assert B * (2 * d + 1) <= 32
        U = _inputs(x, B, d, 31 + B)[0]
        U[0] = x[17]                                        # the quirk on this route too
        dvh, s2 = up._get_variance_dv_many(U)
        _assert_two_paths(gp, U, dvh, s2, range(B), "few rows B=%d" % B)
    for bad_U in (np.zeros(d), np.zeros((3, d + 1)), np.zeros((2, 3, d))):
        with pytest.raises(ValueError):
            up._get_variance_dv_many(bad_U)
        with pytest.raises(ValueError):
            iup.get_best_solution_many(bad_U)
    # a handle built from a supplied matrix has no inputs / theta to evaluate the kernel on
    from skgpuppy_amd.Covariance import _MatrixModel
    mm = _MatrixModel(np.eye(4) * 2.0, np.arange(4.0))
    out, out2 = np.full((2, 1), 7.25), np.full(2, 7.25)
    st = _gpx.lib.gpx_propagate_dvh_many(mm.handle, _gpx.ptr(np.zeros((2, 1))), 2, _gpx.ptr(out), _gpx.ptr(out2))
    assert st == _gpx.GPX_ERR_STATE and "gpx_fit_matrix" in _gpx.last_error()
    np.testing.assert_array_equal(out, np.full((2, 1), 7.25))
    np.testing.assert_array_equal(out2, np.full(2, 7.25))
    mm.close()
    U = _inputs(x, 40, d, 5)[0]
    keep, keep2 = np.full((40, d), 7.25), np.full(40, 7.25)
    hd = gp._dev().handle
    assert _gpx.lib.gpx_propagate_dvh_many(hd, _gpx.ptr(U), -1, _gpx.ptr(keep), _gpx.ptr(keep2)) == _gpx.GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_propagate_dvh_many(hd, None, 40, _gpx.ptr(keep), _gpx.ptr(keep2)) == _gpx.GPX_ERR_BAD_ARG
    assert _gpx.lib.gpx_propagate_dvh_many(hd, _gpx.ptr(U), 40, None, _gpx.ptr(keep2)) == _gpx.GPX_ERR_BAD_ARG
    np.testing.assert_array_equal(keep, np.full((40, d), 7.25))
    np.testing.assert_array_equal(keep2, np.full(40, 7.25))
    with_s2, without = _raw(gp, U), _raw(gp, U, want_sigma2=False)
    assert without[1] is None
    np.testing.assert_array_equal(with_s2[0], without[0])
    # generic route (an operator that overrides a matrix builder): the documented loop over the single-input path
    g = load_golden("generic_ops")
    ggp = sk.GaussianProcess(g["wg_x"], g["wg_t"], make_warped_gaussian(sk.GaussianCovariance)(), g["wg_theta"].copy())
    gd = ggp.d
    GU = np.random.RandomState(4).uniform(g["wg_x"].min(0), g["wg_x"].max(0), (5, gd))
    gup = sk.UncertaintyPropagationApprox(ggp)
    assert gup._generic()
    gdvh, gs2 = gup._get_variance_dv_many(GU)
    for i in range(5):
        one = sk.UncertaintyPropagationApprox(ggp)
        assert [one._get_variance_dv_h(GU[i], k) for k in range(gd)] == list(gdvh[i])
        assert one._get_sigma2(GU[i]) == gs2[i]
    assert gup.u is None
    gsol = IUP(None, ggp, None, np.ones(gd), np.ones(gd)).get_best_solution_many(GU, gs2 + 0.05)
    np.testing.assert_array_equal(gsol, IUP._closed_form(gdvh, gs2, np.ones(gd), np.ones(gd), [], gs2 + 0.05))


@pytest.mark.gpu
def test_approx_many_chunk_boundary():
    """The twin of (6) for gpx_propagate_approx_many: N = 127, d = 8, B = 3300 inputs are 33000 rows against the 32768-row chunk, so two
    chunks of 3276 and 24 inputs.  All finite; the inputs on both sides of the boundary, the ends and twelve random ones against
    propagate_GA within test_propagate_many's two-device-paths bound (mean 2 * 1e-9, variance 2 * 1e-8 v, v = 2); the first
    chunk's inputs equal, bit for bit, a call on them alone."""
    gp, x = _small_gp()
    B, first = 3300, 32768 // 10
    assert first == 3276 and B * 10 > 32768
    U, S = _inputs(x, B, gp.d, 127 + B)
    up = sk.UncertaintyPropagationApprox(gp)
    mean, var = up.propagate_GA_many(U, S)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    pick = [0, first - 1, first, B - 1] + [int(i) for i in np.random.RandomState(7).choice(B, 12, replace=False)]
    dm = dv = 0.0
    for i in pick:
        m1, v1 = sk.UncertaintyPropagationApprox(gp).propagate_GA(U[i], S[i])
        dm, dv = max(dm, abs(mean[i] - m1)), max(dv, abs(var[i] - v1))
        assert mean[i] == pytest.approx(m1, abs=2 * 1e-9) and var[i] == pytest.approx(v1, abs=2 * 1e-8 * V), i
    print("approx_many chunk boundary: worst dmean %.3e dvar %.3e" % (dm, dv))
    head_mean, head_var = up.propagate_GA_many(U[:first], S[:first])
    np.testing.assert_array_equal(mean[:first], head_mean)
    np.testing.assert_array_equal(var[:first], head_var)
