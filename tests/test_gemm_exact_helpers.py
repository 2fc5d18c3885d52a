"""The exact comparison of tests/_gemm_exact.py passes on its own reference and sees each defect the GPU tests (tests/test_gemm_dispatch.py)
are meant to catch, made the way the kernel would make it; the Python copy of the launch codes agrees with include/gpx.h."""
import os
import re

import numpy as np
import pytest

import _gemm_exact as gx
from conftest import ROOT

from skgpuppy_amd import _gpx

M, N, K = 384, 512, 512          # a trapezoid: one full tile column on the left, then three tile rows of a triangle
ALPHA, BETA = -0.5, 2.0


@pytest.fixture(scope="module")
def case():
    rng = np.random.RandomState(5)
    A, B, C0 = gx.operands(rng, M, N, K)
    Bref, Bdev = gx.shaped(B, gx.zero_part(N, K, "lower"))
    wa, wb, wc = gx.windows(M, N, K)
    want = gx.reference(A, Bref, C0, ALPHA, BETA)
    written = gx.mask_lower(M, N)
    ok = np.where(gx.expand(written) != gx.UNTOUCHED, want, C0)      # what a correct launch leaves in C
    return dict(A=A, Bref=Bref, Bdev=Bdev, C0=C0, want=want, written=written, ok=ok, wc=wc)


def _check(case, got, cbuf=None):
    wc = case["wc"]
    buf = wc.new(got) if cbuf is None else cbuf
    gx.check(wc.view(buf), case["want"], case["C0"], case["written"], guards=[(buf, wc, "C")])


def test_reference_passes(case):
    _check(case, case["ok"])
    # the diagonal tiles of a lower-only launch on 64-row block tiles: the 64 x 64 piece above the diagonal stays at C0
    got = case["ok"].copy()
    got[0:64, 192:256] = case["C0"][0:64, 192:256]
    _check(case, got)


def test_poison_is_where_the_launch_does_not_read(case):
    nan = np.isnan(case["Bdev"])
    t = nan.reshape(N // 128, 128, K // 128, 128)
    assert (t.all(axis=(1, 3)) == t.any(axis=(1, 3))).all()                       # whole tiles only
    assert (t.all(axis=(1, 3)) == np.triu(np.ones((4, 4), bool), 1)).all()        # the tiles strictly above the diagonal
    assert not case["Bref"][nan].any() and not np.triu(case["Bref"], 1).any()
    # rectangular ktrim, shift 16: row tile r is not read in the columns below 128 r - 16, rounded down to a tile
    z = gx.unread_part(gx.zero_part(384, 512, "upper", shift=16))
    assert not z[:256].any() and z[256:, :128].all() and not z[256:, 128:].any()


def test_one_entry_off_by_one_fails(case):
    got = case["ok"].copy()
    got[300, 17] += 1.0
    with pytest.raises(AssertionError):
        _check(case, got)
    got = case["ok"].copy()
    got[130, 260] += 0.25                       # in the lower triangle of a diagonal tile, by the smallest step the data allows
    with pytest.raises(AssertionError):
        _check(case, got)


def test_sub_tile_left_at_c0_fails(case):
    got = case["ok"].copy()
    got[256:288, 32:64] = case["C0"][256:288, 32:64]
    with pytest.raises(AssertionError):
        _check(case, got)


def test_tile_with_the_product_applied_twice_fails(case):
    got = case["ok"].copy()
    blk = (slice(128, 256), slice(0, 128))
    got[blk] += ALPHA * case["A"][blk[0]].dot(case["Bref"][blk[1]].T)
    with pytest.raises(AssertionError):
        _check(case, got)


def test_one_stage_short_at_the_triangular_boundary_fails(case):
    """tile column 1 of a lower-triangular B contracts over k < 256; this one stops at 240"""
    got = case["ok"].copy()
    blk = (slice(256, 384), slice(128, 256))
    got[blk] -= ALPHA * case["A"][blk[0], 240:256].dot(case["Bref"][blk[1], 240:256].T)
    assert not np.array_equal(got, case["ok"])
    with pytest.raises(AssertionError):
        _check(case, got)


def test_guard_column_overwritten_fails(case):
    wc = case["wc"]
    buf = wc.new(case["ok"])
    buf.reshape(-1)[wc.offset + 5 * wc.ld + N] = 0.0          # the first column right of the window, row 5
    with pytest.raises(AssertionError, match="guard"):
        _check(case, None, cbuf=buf)
    buf = wc.new(case["ok"])
    buf[wc.offset - 1] = case["ok"][0, 0]                     # the entry in front of the window
    with pytest.raises(AssertionError, match="guard"):
        _check(case, None, cbuf=buf)


def test_unwritten_tile_written_fails(case):
    got = case["ok"].copy()
    blk = (slice(0, 128), slice(384, 512))                     # above the staircase
    assert (case["written"][0, 3] == gx.UNTOUCHED)
    got[blk] = case["want"][blk]
    with pytest.raises(AssertionError):
        _check(case, got)


def test_nan_in_the_written_part_fails(case):
    got = case["ok"].copy()
    got[200, 100] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        _check(case, got)


def test_reference_refuses_data_it_cannot_hold_exactly():
    rng = np.random.RandomState(1)
    A, B, C0 = gx.operands(rng, 128, 128, 16)
    with pytest.raises(AssertionError):
        gx.reference(A, B, C0, 0.75, 1.0)                      # no power of two
    with pytest.raises(AssertionError):
        gx.reference(A + 0.5, B, C0, 1.0, 1.0)
    with pytest.raises(AssertionError):
        gx.reference(A * 2.0 ** 30, B * 2.0 ** 30, C0, 1.0, 1.0)
    for alpha in gx.ALPHAS:
        for beta in gx.BETAS:
            want = gx.reference(A, B, C0, alpha, beta)
            np.testing.assert_array_equal(want, alpha * A.dot(B.T) + beta * C0)


def test_large_products_take_the_checked_fp64_route(monkeypatch):
    rng = np.random.RandomState(2)
    A, B, _ = gx.operands(rng, 256, 128, 64)
    P = gx.exact_product(A, B)
    monkeypatch.setattr(gx, "INT64_MACS", 0)
    np.testing.assert_array_equal(gx.exact_product(A, B), P)


def test_split_k_mask():
    m = gx.mask_splitk(384, 2)
    assert m.shape == (6, 3) and (m[:3] == m[3:]).all() and (m[:3] == gx.mask_lower(384, 384)).all()
    assert (gx.mask_trapezoid(256, 128) == np.array([[1, 2, 0], [1, 1, 2]])).all()


def test_trapezoid_mask_with_a_column_limit():
    import _trap_model as tm
    # 4 tile rows, one full column, the triangle cut behind its second tile column: the rows below the cut are written in full
    assert (gx.mask_trapezoid(512, 128, 256) == np.array([[1, 2, 0, 0, 0], [1, 1, 2, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]])).all()
    for tri_cols in (0, 512):                                  # no limit, either way of saying it
        assert (gx.mask_trapezoid(512, 128, tri_cols) == gx.mask_lower(512, 640)).all()
    for off, nt, wt in tm.DEVICE_CASES + ((2, 5, 0), (2, 5, 5), (1, 9, 1)):
        m = gx.mask_trapezoid(nt * 128, off * 128, wt * 128)
        assert ((m != gx.UNTOUCHED) == tm.mask(off, nt, wt)).all(), (off, nt, wt)
        lim_wt = tm.shape(off, nt, wt)[1]
        assert [tuple(t) for t in np.argwhere(m == gx.DIAGONAL)] == [(r, off + r) for r in range(lim_wt)]
    with pytest.raises(AssertionError):
        gx.mask_trapezoid(512, 128, 640)
    with pytest.raises(AssertionError):
        gx.mask_trapezoid(512, 128, 64)


def test_a_tile_right_of_the_column_limit_written_fails():
    """what a launch that ignored tri_cols would leave: the triangle's tiles right of the limit hold the result"""
    M, off_cols, tri_cols, K = 512, 128, 256, 16
    rng = np.random.RandomState(9)
    A, B, C0 = gx.operands(rng, M, off_cols + M, K)
    want = gx.reference(A, B, C0, ALPHA, BETA)
    lim, full = gx.mask_trapezoid(M, off_cols, tri_cols), gx.mask_trapezoid(M, off_cols)
    ok = np.where(gx.expand(lim) != gx.UNTOUCHED, want, C0)
    gx.check(ok, want, C0, lim)
    with pytest.raises(AssertionError):
        gx.check(np.where(gx.expand(full) != gx.UNTOUCHED, want, C0), want, C0, lim)
    with pytest.raises(AssertionError):                        # and the limited result does not pass for the whole trapezoid
        gx.check(ok, want, C0, full)


def test_launch_codes_match_the_header():
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    names = dict((n, tuple(int(v) for v in a.split(","))) for n, a in re.findall(r"GPX_GEMM_V_(\w+) = GPX_GEMM_VARIANT\(([^)]*)\)", text))
    assert "GPX_GEMM_V_NONE = 0" in text
    want = {"NONE": 0}
    want.update((n, _gpx.gemm_variant(*a)) for n, a in names.items())
    assert want == _gpx.GEMM_VARIANTS
    tri = dict((n, int(v)) for n, v in re.findall(r"GPX_GEMM_TRI_(\w+) = (\d)", text))
    assert tri == dict(NONE=_gpx.GEMM_TRI_NONE, A_UPPER=_gpx.GEMM_TRI_A_UPPER, A_LOWER=_gpx.GEMM_TRI_A_LOWER, B_LOWER=_gpx.GEMM_TRI_B_LOWER,
                       B_UPPER=_gpx.GEMM_TRI_B_UPPER)
