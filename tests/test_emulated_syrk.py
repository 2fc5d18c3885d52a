"""The symmetric emulated update of the factorisation's far columns (csrc/emu.hip, gpx_emu_syrk_lower_sub) on every entry of the lower
triangle, against the error-free reference of tests/_exact_product.py.

C[i, j] -= sum_k A[i, k] A[j, k] for j <= i.  Both roles of a row use ONE split: its own maximum and b = scale_bits(K, L) // 2 bits, so
sig_i = b - 1 - ilogb(max|row i|) scales row i as the left operand and as the right one.  The condition is the design bound of
tests/test_emulated_bound.py with both bit counts equal to b, restated here and not loosened:

    |E_ij - exact_ij| <= 1/2 sum_k (|a_ik| 2^-sig_j + |a_jk| 2^-sig_i) + K 2^-(sig_i + sig_j) / 4      (rounding of the split)
                         + ulp(X_ij 2^-(sig_i + sig_j))                                                (X -> fp64, two roundings)
                         + 1/2 ulp(E_ij)                                                               (the subtraction)

Nothing above the diagonal and nothing outside the window of C may be written -- by the test entry.  The factorisation calls the update
with diag_tile = 128 (gpx_emu_syrk_lower_sub_ex): row i ends at column min(rows - 1, i | (diag_tile - 1)), the last one of its diagonal
tile, so the diagonal tiles are updated in full.  The bound is symmetric in i and j and holds above the diagonal unchanged; there the
result is also symmetric to the bit (both entries come from the same integer X and the same scale sum), and the workspace the
factorisation planned for a larger update gives the same bytes.
"""
import collections
import ctypes
import hashlib

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


def region(rows, diag_tile=1):
    """what the update writes: row i up to column min(rows - 1, i | (diag_tile - 1))"""
    i, j = np.arange(rows)[:, None], np.arange(rows)[None, :]
    return j <= (i | (diag_tile - 1))


_REFS = collections.OrderedDict()


def exact(A, C):
    """(hi, lo) of C - A A^T and hi of -A A^T from tests/_exact_product.py, read-only; the last two operand pairs are kept, so that tests
    of the same operands that follow each other share one reference"""
    key = hashlib.sha1(A.tobytes() + C.tobytes()).hexdigest()
    if key not in _REFS:
        hi, lo = xp.exact_sub(C, A, A)
        ph, _ = xp.exact_sub(np.zeros_like(C), A, A)
        for v in (hi, lo, ph):
            v.setflags(write=False)
        _REFS[key] = (hi, lo, ph)
        while len(_REFS) > 2:
            _REFS.popitem(last=False)
    _REFS.move_to_end(key)
    return _REFS[key]


def syrk(A, C, lda=None, ldc=None, oa=0, oc=0, pad=0, tile_rows=0, diag_tile=1, plan_rows=0):
    """gpx_emu_syrk_lower_sub on a window: A at column oa of a [rows + 2 pad, lda] matrix of NaN, C at column oc of a [rows + 2 pad, ldc]
    matrix of a canary pattern (the square's strict upper triangle holds the canary as well).  Returns the whole C matrix.
    diag_tile, plan_rows other than (1, 0): gpx_emu_syrk_lower_sub_ex; the part of the diagonal tiles above the diagonal holds C as well."""
    from conftest import torch
    from skgpuppy_amd import _gpx
    rows, K = A.shape
    lda, ldc = lda or K, ldc or rows
    ha = np.full((rows + 2 * pad, lda), np.nan)
    ha[pad:pad + rows, oa:oa + K] = A
    hc = _canary((rows + 2 * pad, ldc))
    win = hc[pad:pad + rows, oc:oc + rows]
    reg = region(rows, diag_tile)
    win[reg] = C[reg]
    a, c = torch.as_tensor(ha).cuda(), torch.as_tensor(hc).cuda()
    p = lambda t, off: ctypes.c_void_p(t.data_ptr() + 8 * off)
    if (diag_tile, plan_rows) == (1, 0):
        st = _gpx.lib.gpx_emu_syrk_lower_sub(p(a, pad * lda + oa), lda, rows, K, p(c, pad * ldc + oc), ldc, tile_rows)
    else:
        st = _gpx.lib.gpx_emu_syrk_lower_sub_ex(p(a, pad * lda + oa), lda, rows, K, p(c, pad * ldc + oc), ldc, tile_rows, diag_tile, plan_rows)
    _gpx.check(st, "gpx_emu_syrk_lower_sub")
    return c.cpu().numpy()


def check(name, A, C, **window):
    """every entry of the written region (window["diag_tile"], default 1: the lower triangle) within syrk_bound, everything else the canary"""
    rows = A.shape[0]
    pad, oc = window.get("pad", 0), window.get("oc", 0)
    reg = region(rows, window.get("diag_tile", 1))
    out = syrk(A, C, **window)
    E = out[pad:pad + rows, oc:oc + rows].copy()
    # everything but the written region of the window is the canary still, bit for bit
    want = _canary(out.shape)
    keep = want[pad:pad + rows, oc:oc + rows]
    keep[reg] = E[reg]
    assert out.tobytes() == want.tobytes(), "%s: a write beyond a row's end or outside the window of C" % name
    hi, lo, ph = exact(A, C)
    assert np.isfinite(E[reg]).all(), name
    bound = syrk_bound(A, np.where(reg, E, 0.0), -ph)
    ratio, at = error_ratio(np.where(reg, E, hi), hi, np.where(reg, lo, 0.0), bound)   # (beyond the row's end: no error by construction)
    above = reg & ~region(rows)
    up = error_ratio(np.where(above, E, hi), hi, np.where(above, lo, 0.0), bound)[0] if above.any() else None
    print("EMU-SYRK %-22s %5d x %5d  max error/bound %.4f at %s%s" % (name, rows, A.shape[1], ratio, tuple(int(v) for v in at),
                                                                      "" if up is None else ", above the diagonal %.4f" % up), flush=True)
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
@pytest.mark.parametrize("rows,K", [(1152, 4096), (384, 256), (1152, 128)])
def test_whole_diagonal_tiles_every_entry_within_the_bound(rows, K):
    """diag_tile = 128, as the factorisation calls it: the operands of test_every_entry_within_the_bound, whose reference covers the
    entries above the diagonal already"""
    A, C = operands(rows, K, 1000 * rows + K)
    check("diag 128", A, C, diag_tile=128)


@pytest.mark.gpu
def test_whole_diagonal_tiles_row_scales_forty_bits_apart():
    A, C = operands(384, 256, 7 * 384 + 256, spread=40)
    check("diag 128 scales 2^+-40", A, C, diag_tile=128)


@pytest.mark.gpu
def test_whole_diagonal_tiles_ragged_last_tile():
    """300 rows: the last diagonal tile is 44 x 44, its rows end at column 299"""
    A, C = operands(300, 128, 300)
    assert region(300, 128)[299].all() and region(300, 128)[256, 299] and not region(300, 128)[255, 256]
    check("diag 128 ragged", A, C, diag_tile=128)


@pytest.mark.gpu
def test_diagonal_tiles_of_32():
    A, C = operands(384, 128, 32)
    check("diag 32", A, C, diag_tile=32)


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
def test_row_tiles_of_the_image_whole_diagonal_tiles():
    A, C = operands(2304, 128, 5)
    check("row tiles diag 128", A, C, tile_rows=1024, diag_tile=128)


@pytest.mark.gpu
def test_window_of_a_larger_matrix_whole_diagonal_tiles():
    A, C = operands(1152, 256, 3)
    check("window diag 128", A, C, lda=256 + 70, ldc=1152 + 37, oa=6, oc=9, pad=2, diag_tile=128)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,K,diag_tile,spread", [(1152, 256, 128, 40), (300, 128, 128, 0), (384, 128, 32, 0)])
def test_diagonal_tiles_stay_symmetric_to_the_bit(rows, K, diag_tile, spread):
    """C0 symmetric inside the diagonal tiles: E[i, j] and E[j, i] there come from the same integer X and the same scale sum and take
    one subtraction from equal values"""
    A, C = operands(rows, K, 13 * rows + K, spread=spread)
    reg = region(rows, diag_tile)
    above = reg & ~region(rows)
    C = np.where(above, C.T, C)
    assert above.sum() == sum(n * (n - 1) // 2 for n in [diag_tile] * (rows // diag_tile) + [rows % diag_tile])
    E = syrk(A, C, diag_tile=diag_tile)
    i, j = np.nonzero(above)
    assert (E[i, j] != C[i, j]).mean() > 0.99                  # written, not left at C0
    assert E[i, j].tobytes() == E[j, i].tobytes()
    assert E[~reg].tobytes() == _canary((rows, rows))[~reg].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,tile_rows", [(1152, 1024), (384, 1024), (1152, 0)])
def test_workspace_planned_for_more_rows_gives_the_same_bytes(rows, tile_rows):
    """planned and allocated for 2304 rows (three row tiles of 1024), planned again for the update's own rows (two tiles, one tile) before
    the split, as the factorisation does at every group boundary after its first"""
    A, C = operands(rows, 128, 17 * rows, spread=8)
    own = syrk(A, C, tile_rows=tile_rows, diag_tile=128)
    assert own.tobytes() == syrk(A, C, tile_rows=tile_rows, diag_tile=128, plan_rows=2304).tobytes()
    assert own.tobytes() == syrk(A, C, tile_rows=tile_rows, diag_tile=128, plan_rows=rows).tobytes()
    assert own.tobytes() != _canary(own.shape).tobytes()


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


@pytest.mark.gpu
def test_bad_diag_tile_and_plan_rows_are_refused():
    from conftest import torch
    from skgpuppy_amd import _gpx
    a = torch.ones(256 * 128, dtype=torch.float64).cuda()
    c = torch.full((256 * 256,), 2.5, dtype=torch.float64).cuda()
    fn = _gpx.lib.gpx_emu_syrk_lower_sub_ex
    pa, pc = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(c.data_ptr())
    for diag_tile in (3, 2048, 0, -128, 96):
        assert fn(pa, 128, 256, 128, pc, 256, 0, diag_tile, 0) == _gpx.GPX_ERR_BAD_ARG, diag_tile
        assert _gpx.last_error()
    for plan_rows in (255, 1, -1):
        assert fn(pa, 128, 256, 128, pc, 256, 0, 128, plan_rows) == _gpx.GPX_ERR_BAD_ARG, plan_rows
    assert bool((c == 2.5).all())                              # refused before anything is queued
    assert fn(pa, 128, 256, 128, pc, 256, 0, 1024, 256) == 0   # the largest diag_tile, plan_rows = rows
    assert bool((c == 2.5 - 128.0).all())                      # one diagonal block of 1024 covers the square: every entry updated
