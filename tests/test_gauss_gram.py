"""The Gaussian Gram kernel on the device (csrc/gram.hip; gpx_gram, gpx_dev_gram, gpx_dev_gram_scaled and the accessors of
GaussianCovariance) against the long-double model of tests/_gauss_ld.py (-m gpu).

Bound (not fitted to a device result; tests/_gauss_ld.py states the rule and derives its terms): every entry within
8 * max(rho, 4) = 32 units of u K (1 + q + sqrt(q) s), after a slack of (v + 1) 2^-1075 for the subnormal range; rho is the float64
restatement's own worst distance over all cases below (2.1).  tests/test_gauss_gram_model.py plants seven defects in the restatement
and shows that this bound, on these cases, catches each.  GPX_GRAM_RECORD=<file> appends the measured worst distances
(profiles/r17_gram_bounds.txt holds a run's: 2.4 units on the far family at d = 64, at most 1.4 everywhere else)."""
import ctypes
import functools
import math

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import _gauss_ld as gl

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

pytestmark = pytest.mark.gpu


def _vp(a):
    return ctypes.c_void_p(a) if isinstance(a, int) else _gpx.ptr(a)


def _gram(xi, n1, xj, n2, d, theta, add_diag=0.0, out=None):
    """gpx_gram on raw pointers (ints: device pointers)"""
    K = np.empty((n1, n2)) if out is None else out
    _gpx.check(_gpx.lib.gpx_gram(_vp(xi), n1, _vp(xj), n2, d, _gpx.ptr(_gpx.f64(theta)), float(add_diag), _vp(K)), "gpx_gram")
    return K


@functools.lru_cache(maxsize=None)
def _bound():
    rho, per = gl.rho_all()
    lim = gl.bound()
    gl.record("rho (float64 restatement, %d cases) = %.3f -> bound %.1f units of u K (1 + q + sqrt(q) s)" % (len(per), rho, lim))
    return lim


def _against_the_model(family, n1, n2, d):
    xi, xj, theta = gl.make_case(family, n1, n2, d)
    parts = gl.ld_parts(family, n1, n2, d)
    lim = _bound()
    K = _gram(xi, n1, xj, n2, d, theta)
    units = gl.units(K, parts)                                           # every entry: nothing is left out
    line = "gram %-6s (%3d, %3d) d=%-2d: worst %6.3f units = %.4f of the bound %.1f" % (family, n1, n2, d, units.max(), units.max() / lim, lim)
    if family == "offset":                                               # recorded, not asserted: what prescaling uncentred inputs costs
        line += "; in units of (1 + q) alone %.1f" % gl.units(K, parts, s_term=False).max()
    if family == "far":
        line += "; normal %d subnormal %d zero %d" % ((K >= gl.TINY).sum(), ((K > 0) & (K < gl.TINY)).sum(), (K == 0).sum())
    gl.record(line)
    assert units.shape == (n1, n2) and np.all(units <= lim), (family, n1, n2, d, float(units.max()), lim)
    eq = parts["eq"]
    if family != "far":
        assert eq.sum() >= len(range(3, n1, 7)) and np.all(K[eq] == gl.V)   # bit-equal rows: v exp(-0) = v exactly
    np.testing.assert_array_equal(sk.GaussianCovariance().cov_matrix_ij(xi, xj, theta), K)      # the class's accessor is the same call
    return K


# ------------------------------------------------------------------------------------------------
# a: gpx_gram against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", gl.D_ALL)
@pytest.mark.parametrize("n1,n2", gl.SHAPES)
def test_gram_against_the_model(n1, n2, d):
    _against_the_model("unit", n1, n2, d)


@pytest.mark.parametrize("d", gl.FAMILY_D)
@pytest.mark.parametrize("family", gl.FAMILIES[1:])
def test_gram_families_against_the_model(family, d):
    n1, n2 = gl.FAMILY_SHAPE
    K = _against_the_model(family, n1, n2, d)
    if family == "far":                                                  # the three classes reach the device's output as well
        assert min((K >= gl.TINY).sum(), ((K > 0) & (K < gl.TINY)).sum(), (K == 0).sum()) >= 100


def test_cov_matrix_adds_the_diagonal():
    """add_diag = vt on row == col of a square case, through cov_matrix: fl(v + vt) on the diagonal, v (no vt) on the off-diagonal pair of
    bit-equal rows"""
    n, d = gl.SQUARE
    x, theta = gl.make_square()
    vt = float(np.exp(theta[1]))
    parts = gl.ld_square()
    lim = _bound()
    K = sk.GaussianCovariance().cov_matrix(x, theta)
    units = gl.units(K, parts, "Kd")
    gl.record("gram square (%d, %d) d=%d add_diag=vt: worst %6.3f units = %.4f of the bound %.1f" % (n, n, d, units.max(), units.max() / lim, lim))
    assert np.all(units <= lim), (float(units.max()), lim)
    assert np.all(np.diag(K) == gl.V + vt) and K[n - 10, 4] == gl.V and K[4, n - 10] == gl.V
    np.testing.assert_array_equal(_gram(x, n, x, n, d, theta, vt), K)
    np.testing.assert_array_equal(_gram(x, n, x.copy(), n, d, theta, vt), K)                    # (xj is xi: one scaled copy serves both sides)
    off = ~np.eye(n, dtype=bool)
    np.testing.assert_array_equal(sk.GaussianCovariance().cov_matrix_ij(x, x, theta)[off], K[off])


# ------------------------------------------------------------------------------------------------
# b: bit equalities
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", gl.BITS_D)
def test_gram_bit_equalities(d):
    x, xj, theta = gl.make_case("unit", 257, 130, d)
    K = _gram(x, 257, x, 257, d, theta)
    np.testing.assert_array_equal(K, K.T)                                # K_ij == K_ji: the fit never computes the upper half
    assert np.all(np.diag(K) == gl.V)
    full = _gram(x, 257, xj, 130, d, theta)
    for a, b in ((0, 1), (63, 130), (129, 257)):                         # rows a:b of a call equal a call on rows a:b
        np.testing.assert_array_equal(_gram(np.ascontiguousarray(x[a:b]), b - a, xj, 130, d, theta), full[a:b])
    # the same pair on the interior fast path (rows 64..127 x columns 128..255 of the square call: a full tile off the diagonal) and on
    # the edge path (the same tile of the sub-call touches its diagonal)
    sub = _gram(np.ascontiguousarray(x[64:257]), 193, np.ascontiguousarray(x[128:257]), 129, d, theta)
    np.testing.assert_array_equal(sub, K[64:257, 128:257])
    xd, xjd = torch.from_numpy(x).cuda(), torch.from_numpy(xj).cuda()    # host and device pointers
    outd = torch.empty((257, 130), dtype=torch.float64, device="cuda")
    _gram(xd.data_ptr(), 257, xjd.data_ptr(), 130, d, theta, out=outd.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(outd.cpu().numpy(), full)


# ------------------------------------------------------------------------------------------------
# c: every launch mode of the device entry points
# ------------------------------------------------------------------------------------------------
SENTINEL = -7.0
GUARD, COL0, LD_EXTRA = 64, 64, 130       # a guard row tile above and below; the target starts COL0 columns in; ld = cols_pad + LD_EXTRA
# (n1, n2, rows_pad, cols_pad, the lower_only modes): the 1-D staircase grid with two and six row pairs; rows_pad % 128 != 0: the 2-D grid
# with the early return; rectangular (a panel: the rows from its diagonal down against its own columns)
LAUNCHES = [(200, 200, 256, 256, (0, 1)), (700, 700, 768, 768, (0, 1)), (150, 150, 192, 256, (1,)), (300, 200, 320, 256, (0, 1))]


@functools.lru_cache(maxsize=None)
def _launch_case(n1, n2, d):
    x, _xj, theta = gl._unit_like(np.random.RandomState(gl.seed_of("unit", n1, n2, d) + 2), n1, n1, d)
    vt = float(np.exp(theta[1]))
    return x, theta, vt, gl.kernel_parts(x, x[:n2], theta, add_diag=vt)


def _launch(entry, xd, xwd, n1, n2, d, theta, vt, lower, pad_identity, rp, cp):
    """one call into a sentinel-filled buffer; returns the whole buffer"""
    ld = cp + LD_EXTRA
    buf = torch.full((GUARD + rp + GUARD, ld), SENTINEL, dtype=torch.float64, device="cuda")
    out = ctypes.c_void_p(buf.data_ptr() + 8 * (GUARD * ld + COL0))
    if entry == "gpx_dev_gram":
        st = _gpx.lib.gpx_dev_gram(_vp(xd.data_ptr()), n1, _vp(xd.data_ptr()), n2, d, _gpx.ptr(theta), vt, lower, pad_identity, out, ld, rp, cp, None)
    else:
        st = _gpx.lib.gpx_dev_gram_scaled(_vp(xwd.data_ptr()), n1, _vp(xwd.data_ptr()), n2, d, gl.V, vt, lower, pad_identity, out, ld, rp, cp, None)
    _gpx.check(st, entry)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("d", (3, 8))
@pytest.mark.parametrize("pad_identity", (0, 1))
@pytest.mark.parametrize("n1,n2,rp,cp,lowers", LAUNCHES)
def test_every_launch_mode_of_the_device_entry_points(n1, n2, rp, cp, lowers, pad_identity, d):
    x, theta, vt, parts = _launch_case(n1, n2, d)
    lim = _bound()
    xd = torch.from_numpy(x).cuda()
    # the caller's prescaling with torch: fl(fl(sqrt(w_k)) x_k), w_k from the C library's exp as gpx_dev_gram takes it (numpy's differs
    # from it in the last bit for a few per cent of the arguments: under the rule's q term, but not the same bits)
    xwd = xd * torch.from_numpy(np.sqrt(np.array([math.exp(th) for th in theta[2:]]))).cuda()
    rows, cols = np.arange(rp)[:, None], np.arange(cp)[None, :]
    data = (rows < n1) & (cols < n2)
    pad_want = np.where(rows == cols, 1.0, 0.0) if pad_identity else np.zeros((rp, cp))
    above = 2 * (cols // 128) > rows // 64                               # 64 x 128 tiles strictly above the staircase: col0 > row0 + 63
    got = {}
    for entry in ("gpx_dev_gram_scaled", "gpx_dev_gram"):
        for lower in lowers:
            B = _launch(entry, xd, xwd, n1, n2, d, theta, vt, lower, pad_identity, rp, cp)
            T = B[GUARD:GUARD + rp, COL0:COL0 + cp].copy()
            B[GUARD:GUARD + rp, COL0:COL0 + cp] = SENTINEL
            assert np.all(B == SENTINEL), (entry, lower, "written outside [rows_pad, cols_pad]")
            written = ~above if lower else np.ones((rp, cp), bool)
            assert np.all(T[~written] == SENTINEL), (entry, lower, "a tile above the staircase was written")
            wd = written[:n1, :n2]                                       # every written entry of the data block, above the diagonal too
            units = gl.units(T[:n1, :n2], parts, "Kd")
            assert np.all(units[wd] <= lim), (entry, lower, float(units[wd].max()), lim)
            assert np.all(wd[np.tril_indices(n1, 0, n2)])                # every entry on and below the diagonal is among them
            pad = written & ~data
            assert np.array_equal(T[pad], pad_want[pad]), (entry, lower, "padding")
            got[(entry, lower)] = T
    tril = np.tril_indices(rp, 0, cp)
    ref = got[("gpx_dev_gram_scaled", lowers[0])]
    for key, T in got.items():                                           # lower_only 0 and 1, and both entry points: the same bits
        np.testing.assert_array_equal(T[tril], ref[tril], err_msg=str(key))
    worst = max(float(gl.units(T[:n1, :n2], parts, "Kd")[np.tril_indices(n1, 0, n2)].max()) for T in got.values())
    gl.record("dev gram n=(%d, %d) pad=(%d, %d) d=%d pad_identity=%d lower_only=%r: worst %6.3f units on and below the diagonal"
              % (n1, n2, rp, cp, d, pad_identity, lowers, worst))


# ------------------------------------------------------------------------------------------------
# d: argument checks (nothing is launched)
# ------------------------------------------------------------------------------------------------
def test_device_entry_points_refuse_bad_arguments():
    """padded rows without a single row (gram_kernel would read row n1 - 1 = -1 of xi for them), null inputs and a grid smaller than the
    data: GPX_ERR_BAD_ARG before anything is queued, the output untouched"""
    d = 3
    theta = np.log(np.array([2.0, 0.01, 0.04, 0.05, 0.06]))
    x = torch.zeros((128, d), dtype=torch.float64, device="cuda")
    buf = torch.full((128, 128), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    xp, out, th = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(buf.data_ptr()), _gpx.ptr(theta)
    lib = _gpx.lib
    cases = {"n1 == 0 with rows_pad > 0": (xp, 0, xp, 100, 64, 128),
             "null xi": (None, 100, xp, 100, 128, 128), "null xj": (xp, 100, None, 100, 128, 128),
             "rows_pad < n1": (xp, 100, xp, 100, 64, 128), "cols_pad < n2": (xp, 64, xp, 129, 64, 128),
             "negative n1": (xp, -1, xp, 100, 64, 128)}
    for what, (xi, n1, xj, n2, rp, cp) in cases.items():
        for lower in (0, 1):
            st = lib.gpx_dev_gram(xi, n1, xj, n2, d, th, 0.01, lower, 1, out, 128, rp, cp, None)
            assert st == _gpx.GPX_ERR_BAD_ARG and "gpx_dev_gram" in _gpx.last_error(), (what, st)
            st = lib.gpx_dev_gram_scaled(xi, n1, xj, n2, d, 2.0, 0.01, lower, 1, out, 128, rp, cp, None)
            assert st == _gpx.GPX_ERR_BAD_ARG and "gpx_dev_gram_scaled" in _gpx.last_error(), (what, st)
    assert lib.gpx_dev_gram(xp, 100, xp, 100, d, th, 0.01, 0, 1, None, 128, 128, 128, None) == _gpx.GPX_ERR_BAD_ARG
    assert lib.gpx_dev_gram_scaled(xp, 100, xp, 100, d, 2.0, 0.01, 0, 1, None, 128, 128, 128, None) == _gpx.GPX_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
