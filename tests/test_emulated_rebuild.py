"""The two integer kernels of the emulated fp64 update (csrc/emu.hip) on their own, to the last bit.

emu_rebuild_kernel (gpx_emu_rebuild): residue planes built here from chosen integers X must give C0 - ldexp(fl(X), -(sigma + tau))
with fl(X) modelled exactly as the kernel converts its 128-bit integer.  emu_i8_gemm_kernel (gpx_emu_i8_gemm): R_l must be the
balanced residue of A_l B_l^T mod p_l as the kernel stores it in one byte.  Both are integer computations, so every comparison is of
bit patterns.  tests/_emu_model.py stays the independent model: every X is checked against its garner() before it is used.
"""
import ctypes
import math

import numpy as np
import pytest

from _emu_model import MODULI, balanced, garner

NONFINITE = 0x7FFFFFFF
ROWS, COLS, LDR, LDC = 3, 9, 12, 11                                     # 9 columns: two full groups of four and a tail of one; ldc odd


def _centered(X, P):
    """the representative of X mod P in [-P/2, P/2) (P is even: 256 is always among the moduli)."""
    return (X + P // 2) % P - P // 2


def _chosen_integers(L, rng):
    P = math.prod(MODULI[:L])
    h = P // 2
    xs = [0, 1, -1, -h, -h + 1, -h + 2, h - 1, h - 2, h - 3]
    # every t_l = balanced(r_l c_l mod p_l) at its largest and at its smallest: X = sum_l t_l M_l mod P (largest |q|)
    M = [P // p for p in MODULI[:L]]
    xs.append(sum((127 if p == 256 else (p - 1) // 2) * m for p, m in zip(MODULI, M)))
    xs.append(sum((-128 if p == 256 else -(p - 1) // 2) * m for p, m in zip(MODULI, M)))
    for j in (1, 2, 3):                                                 # carries across the 40-bit limbs
        xs += [s * 2 ** (40 * j) + d for s in (1, -1) for d in (1, -1)]
    xs += [2 ** 63, -(2 ** 63), 2 ** 63 - 1, -(2 ** 63) - 1, 2 ** 64, -(2 ** 64), 2 ** 64 - 1, -(2 ** 64) + 1]   # the two conversion branches
    xs += [int.from_bytes(rng.bytes(17), "little", signed=True) for _ in range(2000)]
    xs = [_centered(x, P) for x in xs]                                  # what L residues can tell apart (the value itself wherever it fits)
    assert all(-h <= x < h for x in xs)
    return xs


def _convert(X):
    """fl(X) as emu_rebuild_kernel converts its __int128: the low word alone when the high word is its sign extension, else
    float(hi) 2^64 + float(lo) with one rounding of the sum."""
    hi, lo = X >> 64, X % 2 ** 64
    slo = lo - 2 ** 64 if lo >= 2 ** 63 else lo
    if hi == (-1 if slo < 0 else 0):
        return float(slo)
    return float(hi) * 2.0 ** 64 + float(lo)


def _crt_sum(res, L):
    """the kernel's direct CRT sum in Python integers and floats: (X, largest |limb sum|, |q|)."""
    P = math.prod(MODULI[:L])
    S, t_over_p = [0, 0, 0], 0.0
    for l, p in enumerate(MODULI[:L]):
        M = P // p
        t = balanced(res[l] * pow(M, -1, p), p)
        for j in range(3):
            S[j] += t * ((M >> (40 * j)) & (2 ** 40 - 1))
    q = round(float(S[0] + (S[1] << 40) + (S[2] << 80)) / float(P))
    X = S[0] + (S[1] << 40) + (S[2] << 80) - q * P
    X = X - P if X >= P // 2 else (X + P if X < -(P // 2) else X)
    return X, max(abs(s) for s in S), abs(q)


@pytest.mark.parametrize("L", [2, 8, 12, 16])
def test_crt_sum_model_equals_garner(L):
    """CPU: the linear-time sum recovers the integer Garner's digits give, its limb sums are exact in fp64 and |q| is small."""
    xs = _chosen_integers(L, np.random.default_rng(L))[:400]
    worst_s = worst_q = 0
    for X in xs:
        res = [balanced(X, p) for p in MODULI[:L]]
        Y, s, q = _crt_sum(res, L)
        assert Y == X == garner([r % p for r, p in zip(res, MODULI)], L)
        worst_s, worst_q = max(worst_s, s), max(worst_q, q)
    assert worst_s < 2 ** 51 and worst_q <= 8
    assert all(math.prod(MODULI[:L]) // p < 2 ** 120 for p in MODULI[:L])   # three 40-bit limbs hold every M_l


def _rebuild_case(L, seed):
    """(residues [batch][L][ROWS][LDR] int8, sigma [batch][ROWS], tau [batch][COLS], fl(X) [batch][ROWS][COLS])"""
    rng = np.random.default_rng(seed)
    xs = _chosen_integers(L, rng)
    for X in xs[:40] + xs[-20:]:
        assert garner([X % p for p in MODULI[:L]], L) == X
    per = ROWS * COLS
    nb = -(-len(xs) // per)
    xs += [0] * (nb * per - len(xs))
    res = rng.integers(-128, 128, (nb, L, ROWS, LDR), dtype=np.int8)    # the padding columns hold junk the kernel must not use
    xd = np.empty((nb, ROWS, COLS))
    for n, X in enumerate(xs):
        b, i, j = n // per, n % per // COLS, n % COLS
        for l in range(L):
            res[b, l, i, j] = balanced(X, MODULI[l])
        xd[b, i, j] = _convert(X)
    sig = rng.integers(-30, 70, (nb, ROWS)).astype(np.int32)
    tau = rng.integers(-30, 70, (nb, COLS)).astype(np.int32)
    return res, sig, tau, xd


def _run_rebuild(res, sig, tau, C0):
    from conftest import torch
    from skgpuppy_amd import _gpx
    nb, L = res.shape[:2]
    r, s, t, c = (torch.as_tensor(np.ascontiguousarray(v)).cuda() for v in (res, sig, tau, C0))
    for b in range(nb):
        _gpx.check(_gpx.lib.gpx_emu_rebuild(ctypes.c_void_p(r[b].data_ptr()), LDR, ROWS * LDR, L, ctypes.c_void_p(s[b].data_ptr()),
                                            ctypes.c_void_p(t[b].data_ptr()), ctypes.c_void_p(c[b].data_ptr()), LDC, ROWS, COLS), "gpx_emu_rebuild")
    return c.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 8, 12, 16])
def test_rebuild_bit_for_bit(L):
    res, sig, tau, xd = _rebuild_case(L, 100 + L)
    nb = res.shape[0]
    term = np.ldexp(xd, -(sig[:, :, None] + tau[:, None, :]))
    rng = np.random.default_rng(L)
    for kind in ("zero", "random"):
        C0 = np.zeros((nb, ROWS, LDC))
        if kind == "random":                                            # of the term's size, so that the subtraction rounds
            C0[:, :, :COLS] = term * rng.standard_normal(term.shape) + rng.standard_normal(term.shape)
        C0[:, :, COLS:] = 7.25                                          # beyond the row: untouched
        got = _run_rebuild(res, sig, tau, C0)
        want = C0.copy()
        want[:, :, :COLS] = C0[:, :, :COLS] - term
        bad = _bits(got) != _bits(want)
        print("L=%d C0 %s: %d of %d entries differ" % (L, kind, bad.sum(), bad.size))
        assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 16])
def test_rebuild_nonfinite_scale_marks_its_row_or_column(L):
    res, sig, tau, xd = _rebuild_case(L, 200 + L)
    res, sig, tau, xd = res[:2], sig[:2].copy(), tau[:2].copy(), xd[:2]
    sig[0, 1] = NONFINITE
    tau[1, 8] = NONFINITE                                               # the tail column
    tau[0, 2] = NONFINITE
    C0 = np.random.default_rng(L).standard_normal((2, ROWS, LDC))
    got = _run_rebuild(res, sig, tau, C0)
    nan = np.zeros((2, ROWS, LDC), bool)
    nan[0, 1, :COLS] = nan[1, :, 8] = nan[0, :, 2] = True
    np.testing.assert_array_equal(np.isnan(got), nan)
    ok = ~nan
    ok[:, :, COLS:] = False
    with np.errstate(over="ignore"):
        want = C0[:, :, :COLS] - np.ldexp(xd, -(sig[:, :, None].astype(np.int64) + tau[:, None, :]))
    assert (_bits(got[:, :, :COLS])[ok[:, :, :COLS]] == _bits(want)[ok[:, :, :COLS]]).all()
    assert (got[:, :, COLS:] == C0[:, :, COLS:]).all()


# ---- the row end of the symmetric update: row i stops behind column (i + diag) | dmask -------------------------------------
DIAGS, DMASKS = (0, 5, 256, -3), (0, 31, 127)


def row_end_mask(rows, cols, diag, dmask):
    """True where gpx_emu_rebuild_ex updates: column j of row i for j <= (i + diag) | dmask (Python's | on negative integers is the
    two's-complement one the kernel computes: (-3) | 31 = -1, a row that ends before column 0)"""
    return np.array([[j <= ((i + diag) | dmask) for j in range(cols)] for i in range(rows)])


def test_row_end_mask():
    m = row_end_mask(12, 5, -3, 0)
    assert not m[:3].any() and m[3].tolist() == [True, False, False, False, False] and m[7:].all()
    assert not row_end_mask(12, 5, -3, 31)[:3].any() and row_end_mask(12, 5, -3, 31)[3:].all()
    assert (row_end_mask(12, 5, 0, 0) == np.tril(np.ones((12, 5), bool))).all()
    m = row_end_mask(140, 130, 0, 127)
    assert m[:128, :128].all() and not m[:128, 128:].any() and m[128:].all()
    assert row_end_mask(140, 130, 256, 0).all() and row_end_mask(140, 130, 5, 31).sum(1)[[0, 26, 27, 122, 123]].tolist() == [32, 32, 64, 128, 130]
    # diag = 0, -3 and 5 without a mask end a row at every position inside a thread's four columns, in both shapes
    for rows, cols in ((12, 5), (140, 130)):
        ends = set(int(e) % 4 for d in (0, 5, -3) for e in row_end_mask(rows, cols, d, 0).sum(1) if 0 < e < cols)
        assert ends == {0, 1, 2, 3}, (rows, cols, ends)


def _shaped_case(rows, cols, ldr, seed):
    """(residues [16][rows][ldr] int8, sigma [rows], tau [cols], fl(X) [rows][cols]): the chosen integers, row by row, as often as they fit"""
    rng = np.random.default_rng(seed)
    xs = _chosen_integers(16, rng)
    res = rng.integers(-128, 128, (16, rows, ldr), dtype=np.int8)      # the padding columns hold junk the kernel must not use
    xd = np.empty((rows, cols))
    for n in range(rows * cols):
        X = xs[n % len(xs)]
        i, j = divmod(n, cols)
        res[:, i, j] = [balanced(X, p) for p in MODULI[:16]]
        xd[i, j] = _convert(X)
    return res, rng.integers(-30, 70, rows).astype(np.int32), rng.integers(-30, 70, cols).astype(np.int32), xd


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,ldr,ldc", [(12, 5, 12, 7), (140, 130, 136, 133)])
def test_rebuild_row_end_bit_for_bit(rows, cols, ldr, ldc):
    """16 moduli; cols no multiple of 4, so that a row's end falls at every position inside a thread's four columns: up to the row end
    the existing model to the bit, behind it C0's bits -- NaN, then a sentinel pattern"""
    from conftest import torch
    from skgpuppy_amd import _gpx
    res, sig, tau, xd = _shaped_case(rows, cols, ldr, 300 + cols)
    term = np.ldexp(xd, -(sig[:, None] + tau[None, :]))
    rng = np.random.default_rng(cols)
    inside = term * rng.standard_normal(term.shape) + rng.standard_normal(term.shape)
    r, s, t = (torch.as_tensor(np.ascontiguousarray(v)).cuda() for v in (res, sig, tau))
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    sentinel = 3.0 + (np.arange(rows * cols) % 509).reshape(rows, cols) / 512.0
    for dmask in DMASKS:
        for diag in DIAGS:
            m = row_end_mask(rows, cols, diag, dmask)
            for name, beyond in (("NaN", np.full((rows, cols), np.nan)), ("sentinel", sentinel)):
                C0 = np.full((rows, ldc), 7.25)                          # beyond the row of the window: untouched
                C0[:, :cols] = np.where(m, inside, beyond)
                want = C0.copy()
                want[:, :cols] = np.where(m, C0[:, :cols] - term, beyond)
                c = torch.as_tensor(C0).cuda()
                _gpx.check(_gpx.lib.gpx_emu_rebuild_ex(p(r), ldr, rows * ldr, 16, p(s), p(t), p(c), ldc, rows, cols, diag, dmask), "gpx_emu_rebuild_ex")
                got = c.cpu().numpy()
                bad = _bits(got) != _bits(want)
                assert not bad.any(), (diag, dmask, name, int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
            print("%d x %d diag %d dmask %d: %d of %d entries updated" % (rows, cols, diag, dmask, m.sum(), m.size))
    # the full rectangle through the new entry is gpx_emu_rebuild
    C0 = np.full((rows, ldc), 7.25)
    C0[:, :cols] = inside
    c1, c2 = torch.as_tensor(C0).cuda(), torch.as_tensor(C0).cuda()
    _gpx.check(_gpx.lib.gpx_emu_rebuild(p(r), ldr, rows * ldr, 16, p(s), p(t), p(c1), ldc, rows, cols), "gpx_emu_rebuild")
    _gpx.check(_gpx.lib.gpx_emu_rebuild_ex(p(r), ldr, rows * ldr, 16, p(s), p(t), p(c2), ldc, rows, cols, 2 ** 40, 0), "gpx_emu_rebuild_ex")
    assert (_bits(c1.cpu().numpy()) == _bits(c2.cpu().numpy())).all()


@pytest.mark.gpu
def test_rebuild_ex_refuses_a_mask_that_is_no_power_of_two_minus_one():
    from conftest import torch
    from skgpuppy_amd import _gpx
    r, s, c = torch.zeros(16 * 4 * 8, dtype=torch.int8).cuda(), torch.zeros(8, dtype=torch.int32).cuda(), torch.full((4 * 8,), 1.5, dtype=torch.float64).cuda()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    for diag, dmask in ((0, 2), (0, 126), (0, -1), (2 ** 41, 0), (-2 ** 41, 0)):
        assert _gpx.lib.gpx_emu_rebuild_ex(p(r), 8, 32, 16, p(s), p(s), p(c), 8, 4, 8, diag, dmask) == _gpx.GPX_ERR_BAD_ARG, (diag, dmask)
    assert bool((c == 1.5).all())


# ---- the int8 product --------------------------------------------------------------------------------------------------
_MAXR, _MAXC, _MAXK = 512, 768, 384


def _planes(kind, n, K, L):
    if kind == "random":
        full = np.random.default_rng(n).integers(-128, 128, (16, max(_MAXR, _MAXC), _MAXK), dtype=np.int8)
        return np.ascontiguousarray(full[:L, :n, :K])
    if kind == "min":
        return np.full((L, n, K), -128, np.int8)
    return np.ascontiguousarray(np.broadcast_to(np.where(np.arange(K) % 2 == 0, 127, -127).astype(np.int8), (L, n, K)))


def _stored_residue(S, p):
    """the byte the kernel stores for the integer sum S: the balanced residue, 128 (mod 256) wrapping to -128."""
    r = S % p
    r = np.where(r > (p - 1) // 2, r - p, r)
    return r.astype(np.int8)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "min", "alternating"])
@pytest.mark.parametrize("L", [1, 16])
@pytest.mark.parametrize("K", [128, 256, 384])
@pytest.mark.parametrize("rows, cols", [(256, 256), (512, 768)])
def test_int8_product_exact(rows, cols, K, L, kind):
    from conftest import torch
    from skgpuppy_amd import _gpx
    A, B = _planes(kind, rows, K, L), _planes(kind, cols, K, L)
    a, b = torch.as_tensor(A).cuda(), torch.as_tensor(B).cuda()
    r = torch.full((L, rows, cols), 99, dtype=torch.int8, device="cuda")
    _gpx.check(_gpx.lib.gpx_emu_i8_gemm(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), rows, cols, K, L,
                                        ctypes.c_void_p(r.data_ptr())), "gpx_emu_i8_gemm")
    got = r.cpu().numpy()
    for l in range(L):
        # |sum| <= K 2^14 < 2^53: the fp64 product of the integer planes is the integer product, and BLAS computes it quickly;
        # a corner of it is recomputed in int64 as the definition states it
        S = (A[l].astype(np.float64) @ B[l].astype(np.float64).T).astype(np.int64)
        np.testing.assert_array_equal(S[:16, :16], A[l, :16].astype(np.int64) @ B[l, :16].astype(np.int64).T)
        want = _stored_residue(S, MODULI[l])
        bad = got[l] != want
        assert not bad.any(), (l, int(bad.sum()), np.argwhere(bad)[:5], got[l][bad][:5], want[bad][:5])
