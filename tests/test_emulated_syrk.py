"""The symmetric emulated update of the factorisation's far columns (csrc/emu.hip, gpx_emu_syrk_lower_sub) on every entry of the lower
triangle, against the error-free reference of tests/_exact_product.py.

C[i, j] -= sum_k A[i, k] A[j, k] for j <= i.  Both roles of a row use ONE split: its own maximum and b = scale_bits(K, L) // 2 bits, so
sig_i = b - 1 - ilogb(max|row i|) scales row i as the left operand and as the right one.  The condition is the design bound of
tests/test_emulated_bound.py with both bit counts equal to b, restated here and not loosened:

    |E_ij - exact_ij| <= 1/2 sum_k (|a_ik| 2^-sig_j + |a_jk| 2^-sig_i) + K 2^-(sig_i + sig_j) / 4      (rounding of the split)
                         + ulp(X_ij 2^-(sig_i + sig_j))                                                (X -> fp64, two roundings)
                         + 1/2 ulp(E_ij)                                                               (the subtraction)

Nothing above the diagonal and nothing outside the window of C may be written.
"""
import ctypes

import numpy as np
import pytest

import _exact_product as xp
from _emu_model import scale_bits
from test_emulated_bound import _canary, error_ratio, row_scale

L = 16   # GPX_EMU_MODULI is not set by this file


def syrk_bound(A, E, prod):
    K = A.shape[1]
    b = scale_bits(K, L) // 2
    sg = row_scale(A, b)
    ld = np.longdouble
    sa = np.abs(A).sum(1, dtype=ld)
    i32 = lambda e: e.astype(np.int32)
    first = (np.ldexp(0.5 * sa[:, None], i32(-sg[None, :])) + np.ldexp(0.5 * sa[None, :], i32(-sg[:, None]))
             + np.ldexp(ld(K / 4.0), i32(-(sg[:, None] + sg[None, :]))))
    tail = np.maximum(np.spacing(np.abs(prod)).astype(ld), np.ldexp(ld(1), -1074)) + 0.5 * np.spacing(np.abs(E)).astype(ld)
    return (first + tail).astype(np.float64)


def operands(rows, K, seed, spread=0):
    """random rows; spread: row scales 2^-spread, 1, 2^spread in turn, so that entry (i, j) pairs a large row with a tiny one"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((rows, K))
    e = (spread * ((np.arange(rows) % 3) - 1)).astype(np.int32)
    A = np.ldexp(A, e[:, None])
    C = rng.standard_normal((rows, rows)) * np.ldexp(np.sqrt(K), e[:, None] + e[None, :])
    return A, C


def syrk(A, C, lda=None, ldc=None, oa=0, oc=0, pad=0, tile_rows=0):
    """gpx_emu_syrk_lower_sub on a window: A at column oa of a [rows + 2 pad, lda] matrix of NaN, C at column oc of a [rows + 2 pad, ldc]
    matrix of a canary pattern (the square's strict upper triangle holds the canary as well).  Returns the whole C matrix."""
    from conftest import torch
    from skgpuppy_amd import _gpx
    rows, K = A.shape
    lda, ldc = lda or K, ldc or rows
    ha = np.full((rows + 2 * pad, lda), np.nan)
    ha[pad:pad + rows, oa:oa + K] = A
    hc = _canary((rows + 2 * pad, ldc))
    win = hc[pad:pad + rows, oc:oc + rows]
    win[np.tril_indices(rows)] = C[np.tril_indices(rows)]
    a, c = torch.as_tensor(ha).cuda(), torch.as_tensor(hc).cuda()
    p = lambda t, off: ctypes.c_void_p(t.data_ptr() + 8 * off)
    fn = _gpx.lib.gpx_emu_syrk_lower_sub
    _gpx.check(fn(p(a, pad * lda + oa), lda, rows, K, p(c, pad * ldc + oc), ldc, tile_rows), "gpx_emu_syrk_lower_sub")
    return c.cpu().numpy()


def check(name, A, C, **window):
    rows = A.shape[0]
    pad, oc = window.get("pad", 0), window.get("oc", 0)
    out = syrk(A, C, **window)
    E = out[pad:pad + rows, oc:oc + rows].copy()
    # everything but the lower triangle of the window is the canary still, bit for bit
    want = _canary(out.shape)
    keep = want[pad:pad + rows, oc:oc + rows]
    keep[np.tril_indices(rows)] = E[np.tril_indices(rows)]
    assert out.tobytes() == want.tobytes(), "%s: a write above the diagonal or outside the window of C" % name
    hi, lo = xp.exact_sub(C, A, A)
    ph, _ = xp.exact_sub(np.zeros_like(C), A, A)
    low = np.tril(np.ones((rows, rows), dtype=bool))
    assert np.isfinite(E[low]).all(), name
    bound = syrk_bound(A, np.where(low, E, 0.0), -ph)
    ratio, at = error_ratio(np.where(low, E, hi), hi, np.where(low, lo, 0.0), bound)   # (above the diagonal: no error by construction)
    print("EMU-SYRK %-22s %5d x %5d  max error/bound %.4f at %s" % (name, rows, A.shape[1], ratio, at), flush=True)
    assert ratio <= 1.0, (name, ratio, at, float(E[at]), float(hi[at]), float(lo[at]), float(bound[at]))
    return E


@pytest.mark.gpu
@pytest.mark.parametrize("K", [128, 256, 4096])
@pytest.mark.parametrize("rows", [384, 1152])
def test_every_entry_within_the_bound(rows, K):
    """384 rows: one ragged tile of 256; 1152: a second column panel of 128 columns"""
    A, C = operands(rows, K, 1000 * rows + K)
    check("plain", A, C)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,K", [(384, 256), (1152, 128)])
def test_row_scales_forty_bits_apart(rows, K):
    A, C = operands(rows, K, 7 * rows + K, spread=40)
    check("scales 2^+-40", A, C)


@pytest.mark.gpu
def test_window_of_a_larger_matrix_with_canaries():
    A, C = operands(1152, 256, 3)
    check("window", A, C, lda=256 + 70, ldc=1152 + 37, oa=6, oc=9, pad=2)


@pytest.mark.gpu
def test_row_tiles_of_the_image():
    """2304 rows in row tiles of 1024: the panels' right operands come from the first, second and third tile's planes"""
    A, C = operands(2304, 128, 5)
    check("row tiles", A, C, tile_rows=1024)


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    A, C = operands(1152, 256, 11, spread=40)
    assert syrk(A, C).tobytes() == syrk(A, C).tobytes()


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    from conftest import torch
    from skgpuppy_amd import _gpx
    a, c = torch.zeros(256 * 128, dtype=torch.float64).cuda(), torch.zeros(256 * 256, dtype=torch.float64).cuda()
    fn = _gpx.lib.gpx_emu_syrk_lower_sub
    pa, pc = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(c.data_ptr())
    assert fn(pa, 128, 256, 100, pc, 256, 0) != 0      # K no multiple of 128
    assert fn(pa, 64, 256, 128, pc, 256, 0) != 0       # lda < K
    assert fn(pa, 128, 256, 128, pc, 255, 0) != 0      # ldc < rows
    assert fn(pa, 128, 0, 128, pc, 256, 0) == 0        # an empty update
