"""The emulated fp64 update (csrc/emu.hip) held to the per-entry error bound of DESIGN.md section 6, on every entry.

CPU: the error-free reference of tests/_exact_product.py against Fraction arithmetic on small instances of every operand family
below, and a planted defect of one unit in one slice product.  GPU (-m gpu): gpx_emu_gemm_nt_sub against that reference at the
operands where an exact-integer scheme goes wrong -- integers at the capacity P/2, extreme residues and Garner digits, power-of-two
and range edges of the row scales, in-row dynamic range, cancellation, windows of larger matrices, workspace tiles -- its argument
checks, and the call site: estimate_many, gpx_predict_kv and propagate_GA_many with every update of the recursion from K = 1024
emulated (GPX_EMU_MIN_K), against the oracle, in child processes.

The condition, for every entry (sig_i, tau_j: the scale exponents the split chooses, computed here from the row maxima):

    |E_ij - exact_ij| <= 1/2 sum_k (|a_ik| 2^-tau_j + |b_jk| 2^-sig_i) + K 2^-(sig_i + tau_j) / 4      (rounding of the split)
                         + ulp(X_ij 2^-(sig_i + tau_j))                                                (X -> fp64, two roundings)
                         + 1/2 ulp(E_ij)                                                               (the subtraction)

For the families called exact the operands are integers after scaling: the first line is asserted to be zero and left out.
GPX_EMU_MODULI is read once per process, so the 8- and 12-modulus cases run this file as a child process (main() below).
"""
import ctypes
import json
import math
import os
import subprocess
import sys
import time
from fractions import Fraction

import numpy as np
import pytest

import _exact_product as xp
from _emu_model import MODULI, emulated_product, garner, scale_bits, split_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------------------------
def row_scale(X, bits):
    """sig_i of emu_split_kernel: bits - 1 - ilogb(max|row|), 0 for an all-zero row"""
    m = np.abs(X).max(axis=1)
    return np.where(m > 0, bits - np.frexp(m)[1], 0).astype(np.int64)


def split_is_exact(X, bits):
    s = row_scale(X, bits)[:, None].astype(np.int32)
    with np.errstate(over="ignore"):
        y = np.ldexp(X, s)
    return bool(np.array_equal(np.rint(y), y))


def design_bound(A, B, E, prod, L, exact, shift=0):
    """the right-hand side above for every entry, times 2^shift (an integer or one per entry); prod = fl(A B^T) 2^shift (for the ulp
    of X 2^-(sig + tau)), E the kernel's result.  Extended precision (x87: 15 exponent bits) carries the terms that leave fp64's range
    before the shift brings them back; an ulp is never below 2^-1074."""
    K = A.shape[1]
    bits = scale_bits(K, L)
    sg, tu = row_scale(A, bits - bits // 2), row_scale(B, bits // 2)
    ld = np.longdouble
    assert np.finfo(ld).maxexp >= 16384, "design_bound needs an extended type with 15 exponent bits (x87 long double)"
    sh = np.broadcast_to(np.asarray(shift, dtype=np.int32), E.shape)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        tail = np.maximum(np.spacing(np.abs(prod)).astype(ld), np.ldexp(ld(1), sh - 1074)) + np.ldexp(0.5 * np.spacing(np.abs(E)).astype(ld), sh)
        if exact:
            assert split_is_exact(A, bits - bits // 2) and split_is_exact(B, bits // 2)      # the first line is zero
            return tail.astype(np.float64)
        sa, sb = np.abs(A).sum(1, dtype=ld), np.abs(B).sum(1, dtype=ld)
        i32 = lambda e: e.astype(np.int32)
        first = (np.ldexp(0.5 * sa[:, None], i32(sh - tu[None, :])) + np.ldexp(0.5 * sb[None, :], i32(sh - sg[:, None]))
                 + np.ldexp(ld(K / 4.0), i32(sh - (sg[:, None] + tu[None, :]))))
        return np.minimum(first + tail, ld(sys.float_info.max)).astype(np.float64)   # (clamped where 2^shift takes it out of range)


def error_ratio(E, hi, lo, bound):
    """max over the entries of |E - (hi + lo)| / bound (0 / 0 counts as 0), and where it is reached"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs((E - hi) - lo)
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    k = np.unravel_index(np.argmax(r), r.shape)
    return float(r[k]), k


# ------------------------------------------------------------------------------------------------------------------------
# operand families (plain numpy; small instances run on the CPU against Fraction)
# ------------------------------------------------------------------------------------------------------------------------
def bits_ab(K, L):
    b = scale_bits(K, L)
    return b - b // 2, b // 2


def largest(bits):
    """the largest magnitude a split of `bits` bits can hold that is a double"""
    return float((2 ** bits - 1) if bits <= 53 else (2 ** 53 - 1) * 2 ** (bits - 53))


def fam_capacity(rng, rows, cols, K, L):
    """every entry of a row at the largest magnitude: A rows all + / all -, B rows all +, all - or alternating along k, so that X
    lands near +P/2, -P/2 and 0"""
    ab, bb = bits_ab(K, L)
    X = K * int(largest(ab)) * int(largest(bb))
    PL = math.prod(MODULI[:L])
    assert X < PL // 2                                                   # fits with the kernel's scale_bits ...
    ab1, bb1 = (ab + bb + 1) - (ab + bb + 1) // 2, (ab + bb + 1) // 2
    assert K * int(largest(ab1)) * int(largest(bb1)) >= PL // 2          # ... and not with one bit more
    A = np.full((rows, K), largest(ab)) * np.where(np.arange(rows) % 2, -1.0, 1.0)[:, None]
    B = np.full((cols, K), largest(bb))
    B[1::3] *= -1.0
    B[2::3] *= np.where(np.arange(K) % 2, -1.0, 1.0)[None, :]
    A = np.ldexp(A, rng.integers(-30, 31, (rows, 1)).astype(np.int32))
    B = np.ldexp(B, rng.integers(-30, 31, (cols, 1)).astype(np.int32))
    C = rng.standard_normal((rows, cols)) * np.abs(A[:, :1]) * np.abs(B[:, :1]).T * K
    C[:, ::4] = 0.0
    return A, B, C


def with_residue(bits, r, p):
    """the smallest double-representable integer in [2^(bits-1), 2^bits) congruent to r mod p"""
    step = 2 ** max(0, bits - 53)
    v = 2 ** (bits - 1)
    while v % p != r % p:
        v += step
    assert v < 2 ** bits
    return v


def fam_residue(rng, K, L, which):
    """integer operands, one entry per row fixing the scale (a' = a).  which = 'p256': every a', b' = 128 mod 256 (the byte wraps to
    -128, the int32 accumulator reaches K 2^14); 'odd': per odd modulus rows at +(p-1)/2 and -(p-1)/2 mod p"""
    ab, bb = bits_ab(K, L)
    if which == "p256":
        targets = [(256, 128)] * 6
    else:
        targets = [(p, s * (p - 1) // 2) for p in MODULI[1:L] for s in (1, -1)]

    def make(bits, sign_mix):
        M = np.empty((len(targets), K))
        for i, (p, r) in enumerate(targets):
            m = rng.integers(0, min(2 ** 20, 2 ** (bits - 2) // p), K)
            row = (m * p + (r % p)).astype(np.float64)
            if sign_mix == 1 or (sign_mix == 2 and i % 2):               # negatives: -(r + p m) has residue -r; use p - r to keep r
                neg = rng.random(K) < 0.5
                row = np.where(neg, -(m * p + ((-r) % p)).astype(np.float64), row)
            row[rng.integers(0, K)] = float(with_residue(bits, r, p))
            M[i] = row
        return M
    A, B = make(ab, 2), make(bb, 1 if which == "odd" else 2)
    for M, bits in ((A, ab), (B, bb)):
        assert (row_scale(M, bits) == 0).all()
    for i, (p, r) in enumerate(targets):
        assert all(int(v) % p == r % p for v in A[i, :64]) and all(int(v) % p == r % p for v in B[i, :64])
    C = rng.standard_normal((len(targets), len(targets))) * 2.0 ** (ab + bb)
    sc = rng.integers(-20, 21, (len(targets), 1)).astype(np.int32)
    return np.ldexp(A, sc), np.ldexp(B, sc[::-1]), np.ldexp(C, sc + sc[::-1].T)


def fam_garner(rng, K, L):
    """rows of A whose integer X against the one row pattern of B has each mixed-radix digit in turn at its extreme balanced value
    (-128 / 127 for p = 256, +-(p - 1) / 2 for the odd moduli).  The top digit is bounded by K 2^(alpha + beta) < P / 2, so it takes
    the largest magnitude the capacity allows.  B's row is [bmax] * (K - 3), 1, 1, 0 and A's row spreads X // bmax over the first
    K - 3 entries, X mod bmax over the two next and fixes its scale with the last."""
    ab, bb = bits_ab(K, L)
    amax, bmax = int(largest(ab)), int(largest(bb))
    radix = [math.prod(MODULI[:k]) for k in range(L)]
    cap = (K - 4) * amax * bmax
    top = min((MODULI[L - 1] - 1) // 2, cap // radix[L - 1] - 1)

    def chunks(S, n, lim):
        out, sign = [], 1 if S >= 0 else -1
        S = abs(S)
        while S:
            c = min(S, lim)
            if c.bit_length() > 53:
                c = c >> (c.bit_length() - 53) << (c.bit_length() - 53)
            out.append(sign * c)
            S -= c
        assert len(out) <= n, (len(out), n)
        return out + [0] * (n - len(out))

    rowsA, Xs = [], []
    for k in range(L):
        for ext in ((-128, 127) if k == 0 else (-(MODULI[k] - 1) // 2, (MODULI[k] - 1) // 2)):
            for _rep in range(2):
                v = [int(rng.integers(-(p // 2) + 1, p // 2)) for p in MODULI[:L]]
                v[L - 1] = int(rng.integers(-top, top + 1))
                v[k] = ext if k < L - 1 else (top if ext > 0 else -top)
                X = sum(d * r for d, r in zip(v, radix))
                assert abs(X) <= cap and garner([X % p for p in MODULI[:L]], L) == X
                S, r = divmod(X, bmax)
                row = chunks(S, K - 3, amax) + chunks(r, 2, amax) + [amax]
                assert sum(a * b for a, b in zip(row, [bmax] * (K - 3) + [1, 1, 0])) == X
                rowsA.append(row)
                Xs.append(X)
    A = np.array([[float(a) for a in row] for row in rowsA])
    assert all(int(A[i, j]) == rowsA[i][j] for i in range(len(rowsA)) for j in range(0, K, max(1, K // 50)))
    Brow = np.array([float(bmax)] * (K - 3) + [1.0, 1.0, 0.0])
    B = np.stack([Brow, -Brow, Brow * 0.5, -Brow * 4.0, Brow * 2.0 ** -40])
    C = np.zeros((len(rowsA), len(B)))
    C[:, 1::2] = rng.standard_normal((len(rowsA), len(B[1::2]))) * 2.0 ** (ab + bb)
    return A, B, C, Xs


def fam_edges(rng, K, L):
    """rows for the edges of the row scale; the same kinds on both sides, so every pair meets"""
    def kinds(n_bits):
        R = []
        for e in (0, 17, -33):
            r = rng.uniform(-1, 1, K) * 2.0 ** e
            r[rng.integers(0, K)] = 2.0 ** e                             # maximum exactly a power of two
            R.append(r)
            r = rng.uniform(-1, 1, K) * 2.0 ** (e - 1)
            r[rng.integers(0, K)] = -np.nextafter(2.0 ** e, 0.0)        # one below it: rounds to 2^bits when bits < 53
            R.append(r)
        R.append(rng.integers(-2 ** 12, 2 ** 12, K) * 2.0 ** -1074)      # a subnormal row
        R.append(rng.uniform(-1, 1, K) * 1.7 * 2.0 ** 1020)              # a few binades below DBL_MAX
        R.append(rng.uniform(-1, 1, K) * 2.0 ** 1023)
        R.append(rng.uniform(-1, 1, K) * 2.0 ** -495)                    # tiny x tiny: sig + tau near 1100, the product near 2^-990
        R.append(rng.uniform(-1, 1, K) * 2.0 ** -560)                    # sig + tau far beyond 1100, the product subnormal or 0
        R.append(rng.uniform(-1, 1, K) * 2.0 ** -1000)
        r = np.zeros(K)
        r[rng.integers(0, K)] = -3.0 * 2.0 ** 40                          # a single non-zero entry
        R.append(r)
        R.append(np.zeros(K))                                            # an all-zero row
        R.append(rng.standard_normal(K))
        return np.array(R)
    A, B = kinds(0), kinds(1)
    C = rng.standard_normal((len(A), len(B)))
    C[:, ::2] = 0.0
    return A, B, C


def fam_range(rng, rows, cols, K):
    A = rng.standard_normal((rows, K)) * np.exp2(rng.integers(-30, 31, (rows, 1))) * np.exp2(-rng.uniform(0, 70, (rows, K)))
    B = rng.standard_normal((cols, K)) * np.exp2(rng.integers(-30, 31, (cols, 1))) * np.exp2(-rng.uniform(0, 70, (cols, K)))
    C = rng.standard_normal((rows, cols)) * np.abs(A).max(1, keepdims=True) * np.abs(B).max(1)[None, :]
    return A, B, C


def fam_random(rng, rows, cols, K):
    A = rng.standard_normal((rows, K)) * np.exp2(rng.integers(-30, 31, (rows, 1))) * np.exp2(-rng.uniform(0, 40, (rows, K)))
    B = rng.standard_normal((cols, K)) * np.exp2(rng.integers(-30, 31, (cols, 1)))
    C = rng.standard_normal((rows, cols)) * np.abs(A).max(1, keepdims=True) * np.abs(B).max(1)[None, :]
    return A, B, C


def fam_few_bits(rng, rows, cols, K, nbits):
    """integers of nbits bits times a power of two per row (exact; one or two slices in the reference)"""
    A = np.ldexp(rng.integers(-2 ** nbits + 1, 2 ** nbits, (rows, K)).astype(np.float64), rng.integers(-30, 31, (rows, 1)).astype(np.int32))
    B = np.ldexp(rng.integers(-2 ** nbits + 1, 2 ** nbits, (cols, K)).astype(np.float64), rng.integers(-30, 31, (cols, 1)).astype(np.int32))
    C = rng.standard_normal((rows, cols)) * np.abs(A).max(1, keepdims=True) * np.abs(B).max(1)[None, :] * np.sqrt(K)
    return A, B, C


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the reference against Fraction
# ------------------------------------------------------------------------------------------------------------------------
def fraction_sub(C0, A, B):
    FA = [[Fraction(v) for v in r] for r in A.tolist()]
    FB = [[Fraction(v) for v in r] for r in B.tolist()]
    return [[Fraction(C0[i, j]) - sum(x * y for x, y in zip(FA[i], FB[j])) for j in range(len(FB))] for i in range(len(FA))]


def fraction_bound(A, B, i, j, K, L, exact_family, x, prod):
    """the section 6 bound of entry (i, j) in rational arithmetic (x: the exact result, prod: the exact product)"""
    ulp = lambda f: Fraction(math.ulp(float(f))) if abs(f) < Fraction(2) ** 1023 else Fraction(2) ** 971
    tail = ulp(prod) + ulp(x) / 2
    if exact_family:
        return tail
    ab, bb = bits_ab(K, L)
    si, tj = int(row_scale(A[i:i + 1], ab)[0]), int(row_scale(B[j:j + 1], bb)[0])
    first = sum(abs(Fraction(a)) / Fraction(2) ** tj + abs(Fraction(b)) / Fraction(2) ** si for a, b in zip(A[i].tolist(), B[j].tolist())) / 2
    return first + Fraction(K, 4) / Fraction(2) ** (si + tj) + tail


SHIFTS = (0, 1100, -1100, 2200)       # the scales at which the edges family is compared: each entry is normal at one of them


def _small_families():
    rng = np.random.default_rng(21)
    K, L = 128, 16
    out = []
    A, B, C = fam_capacity(rng, 6, 7, K, L)
    out.append(("capacity", A, B, C, True, 0))
    A, B, C = fam_capacity(rng, 4, 6, K, 8)
    out.append(("capacity L=8", A, B, C, True, 0))
    A, B, C = fam_residue(rng, K, L, "p256")
    out.append(("residue 128 mod 256", A, B, C, True, 0))
    A, B, C = fam_residue(rng, K, L, "odd")
    out.append(("residue odd moduli", A[:8], B[:8], C[:8, :8], True, 0))
    A, B, C, _ = fam_garner(rng, 256, L)
    out.append(("garner digits", A[::7], B, C[::7], True, 0))
    A, B, C = fam_edges(rng, K, L)
    for shift in SHIFTS:
        out.append(("edges, scale_exp %d" % shift, A, B, C, False, shift))
    A, B, C = fam_range(rng, 6, 5, K)
    out.append(("in-row range", A, B, C, False, 0))
    A, B, C = fam_random(rng, 6, 5, K)
    hi, _lo = xp.exact_sub(np.zeros_like(C), A, B)
    out.append(("cancellation", A, B, -hi, False, 0))
    A, B, C = fam_few_bits(rng, 5, 6, K, 19)
    out.append(("few bits", A, B, C, True, 0))
    return out


@pytest.mark.parametrize("case", _small_families(), ids=lambda c: c[0])
def test_reference_against_fractions(case):
    """|hi + lo - exact| <= 2^-40 of the section 6 bound of that entry, wherever hi is finite and normal at this scale_exp (the edges
    family is covered by its scales together: test_reference_edges_every_entry_reached)."""
    name, A, B, C, exact_family, shift = case
    K = A.shape[1]
    L = 8 if "L=8" in name else 16
    hi, lo = xp.exact_sub(C, A, B, scale_exp=shift)
    F = fraction_sub(C, A, B)
    F0 = fraction_sub(np.zeros_like(C), A, B)
    two = Fraction(2)
    checked = 0
    for i in range(A.shape[0]):
        for j in range(B.shape[0]):
            x = F[i][j] * two ** shift
            if not (math.isfinite(hi[i, j]) and math.isfinite(lo[i, j])) or (x != 0 and abs(x) < two ** -900):
                assert name.startswith("edges")                          # (the GPU test's rule: _reference_multi_scale)
                continue
            checked += 1
            bound = fraction_bound(A, B, i, j, K, L, exact_family, F[i][j], -F0[i][j]) * two ** shift
            assert abs(Fraction(float(hi[i, j])) + Fraction(float(lo[i, j])) - x) * two ** 40 <= bound, (name, i, j)
            assert hi[i, j] == float(x)                                  # hi is the correctly rounded result
    assert checked > 0 and (checked == A.shape[0] * B.shape[0] or name.startswith("edges"))


def test_reference_edges_every_entry_reached():
    """each entry of the edges family is finite and normal (or exactly zero) at one of the scales the GPU test uses"""
    A, B, C = fam_edges(np.random.default_rng(21), 128, 16)
    hi, lo, _prod, shift = _reference_multi_scale(C, A, B)
    assert np.isfinite(hi).all() and np.isfinite(lo).all() and np.isin(shift, SHIFTS).all()
    F = fraction_sub(C, A, B)
    for i in range(len(A)):
        for j in range(len(B)):
            assert hi[i, j] == float(F[i][j] * Fraction(2) ** int(shift[i, j]))


def test_reference_sees_one_unit_of_one_slice_product():
    """one unit added to one entry of one slice product (weight 2^-((s + t + 2) q) of the row scales: 2^-40 .. 2^-80 of max|a| max|b|
    here) fails the criterion of test_reference_against_fractions at that entry and at no other"""
    rng = np.random.default_rng(4)
    K = 128
    q = xp.slice_bits(K)
    for exact_family, (A, B, C) in ((False, fam_random(rng, 4, 5, K)), (True, fam_capacity(rng, 4, 5, K, 16)), (False, fam_range(rng, 4, 5, K))):
        F = fraction_sub(C, A, B)
        F0 = fraction_sub(np.zeros_like(C), A, B)
        ea, eb = xp.row_exponents(A), xp.row_exponents(B)
        for s, t in ((0, 0), (1, 0), (0, 1), (1, 1)):
            hi, lo = xp.exact_sub(C, A, B, perturb=(s, t, 2, 3))
            for i in range(4):
                for j in range(5):
                    d = Fraction(float(hi[i, j])) + Fraction(float(lo[i, j])) - F[i][j]
                    passes = abs(d) * 2 ** 40 <= fraction_bound(A, B, i, j, K, 16, exact_family, F[i][j], -F0[i][j])
                    assert passes == ((i, j) != (2, 3)), (s, t, i, j)
                    if (i, j) == (2, 3):                                 # the planted unit at its weight, and nothing else
                        w = Fraction(2) ** (int(ea[2] + eb[3]) - (s + t + 2) * q)
                        assert abs(d + w) <= abs(F[i][j]) / 2 ** 100


@pytest.mark.parametrize("L", [8, 12, 16])
def test_model_exact_at_capacity_and_residue_extremes(L):
    """the Python-integer model of the scheme (test_emulated_update.emulated_product: its own assertion that the Garner digits give back
    sum a' b') on the capacity, residue and Garner-digit operands: they are exact families, so the model returns the exact product"""
    rng = np.random.default_rng(L)
    K = 128
    fams = [fam_capacity(rng, 4, 6, K, L)[:2], fam_residue(rng, K, L, "p256")[:2], fam_garner(rng, K, L)[:2]]
    A, B = fam_residue(rng, K, L, "odd")[:2]
    fams.append((A[::5], B[1::5]))
    for A, B in fams:
        A, B = A[:7], B[:6]
        ab, bb = bits_ab(K, L)
        assert split_is_exact(A, ab) and split_is_exact(B, bb)
        M = emulated_product(A.tolist(), B.tolist(), L)
        F = fraction_sub(np.zeros((len(A), len(B))), A, B)
        assert all(M[i][j] == -F[i][j] for i in range(len(A)) for j in range(len(B)))


@pytest.mark.parametrize("L", [8, 12, 16])
def test_model_exact_at_the_int32_accumulator_edge(L):
    """K = 130944, every a', b' = 128 mod 256: the mod-256 residue sum of the model is K 2^14 = 2^31 - 2^21; one row pair"""
    A, B = fam_residue(np.random.default_rng(L), 130944, L, "p256")[:2]
    A, B = A[:1], B[1:2]
    ab, bb = bits_ab(130944, L)
    a, b = split_row(A[0].tolist(), ab)[0], split_row(B[0].tolist(), bb)[0]
    assert all(v % 256 == 128 for v in a) and all(v % 256 == 128 for v in b) and 130944 * 128 * 128 == 2 ** 31 - 2 ** 21
    M = emulated_product(A.tolist(), B.tolist(), L)
    assert M[0][0] == -fraction_sub(np.zeros((1, 1)), A, B)[0][0]


def test_capacity_overflows_with_one_more_scale_bit():
    """what the capacity family claims to test: with alpha + beta one larger the same operands' integer leaves [-P/2, P/2) and the
    Garner digits give back X -+ P (fam_capacity asserts the same inequality for every case it builds)"""
    for L, K in ((16, 128), (16, 130944), (12, 8192), (8, 128)):
        ab, bb = bits_ab(K, L)
        s1 = ab + bb + 1
        X = K * int(largest(s1 - s1 // 2)) * int(largest(s1 // 2))
        PL = math.prod(MODULI[:L])
        assert garner([X % p for p in MODULI[:L]], L) == X - PL and garner([-X % p for p in MODULI[:L]], L) == PL - X


def test_reference_refuses_what_it_cannot_do_exactly():
    A = np.ones((2, 128))
    A[0, 0], A[0, 1] = 2.0 ** 1000, 2.0 ** -1000                         # 2000 bits in one row
    with pytest.raises(ValueError):
        xp.exact_sub(np.zeros((2, 2)), A, np.ones((2, 128)))
    A[0, 1] = np.nan
    with pytest.raises(ValueError):
        xp.exact_sub(np.zeros((2, 2)), A, np.ones((2, 128)))


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def _moduli():
    return int(os.environ.get("GPX_EMU_MODULI", "16"))


def _canary(shape):
    """a NaN-free pattern no kernel would write: 1.5 + (index mod 1021) / 1024"""
    n = int(np.prod(shape))
    return (1.5 + (np.arange(n) % 1021) / 1024.0).reshape(shape)


def _emu(A, B, C, lda=None, ldb=None, ldc=None, oa=0, ob=0, oc=0, pad=2):
    """gpx_emu_gemm_nt_sub on windows of larger device matrices: A at column oa of a [rows + 2 pad, lda] matrix of NaN (from row pad),
    likewise B; C at column oc of a [rows + 2 pad, ldc] matrix of a canary pattern, which must come back bit-unchanged."""
    from conftest import torch
    from skgpuppy_amd import _gpx
    (rows, K), cols = A.shape, B.shape[0]
    lda, ldb, ldc = lda or K, ldb or K, ldc or cols
    plain = (lda, ldb, ldc, oa, ob, oc) == (K, K, cols, 0, 0, 0)
    if plain:
        pad = 0
    assert oa + K <= lda and ob + K <= ldb and oc + cols <= ldc

    def host(X, ld, off, fill):
        H = fill((X.shape[0] + 2 * pad, ld))
        H[pad:pad + X.shape[0], off:off + X.shape[1]] = X
        return H
    nan = lambda s: np.full(s, np.nan)
    ha, hb, hc = (A, B, C) if plain else (host(A, lda, oa, nan), host(B, ldb, ob, nan), host(C, ldc, oc, _canary))
    a, b, c = (torch.as_tensor(np.ascontiguousarray(v)).cuda() for v in (ha, hb, hc))
    p = lambda t, off: ctypes.c_void_p(t.data_ptr() + 8 * off)
    rc = _gpx.lib.gpx_emu_gemm_nt_sub(p(a, pad * lda + oa), lda, p(b, pad * ldb + ob), ldb, p(c, pad * ldc + oc), ldc, rows, cols, K)
    _gpx.check(rc, "emu")
    out = c.cpu().numpy()
    if plain:
        return out
    E = out[pad:pad + rows, oc:oc + cols].copy()
    out[pad:pad + rows, oc:oc + cols] = _canary(out.shape)[pad:pad + rows, oc:oc + cols]
    assert out.tobytes() == _canary(out.shape).tobytes(), "a write outside the window of C"
    return E


def _reference(C, A, B, shift=0):
    hi, lo = xp.exact_sub(C, A, B, scale_exp=shift)
    ph, _pl = xp.exact_sub(np.zeros_like(C), A, B, scale_exp=shift)
    return hi, lo, -ph


def _reference_multi_scale(C, A, B):
    """(hi, lo, prod, shift) per entry, at the first scale_exp of SHIFTS where the result is finite and at least 2^-900 or exactly zero
    (zero: C0 = 0 and a product that is still 0 at 2^2200, where the smallest non-zero product of two doubles is normal)"""
    true_zero = (C == 0) & (_reference(C, A, B, 2200)[2] == 0)
    out = [np.full(C.shape, np.nan) for _ in range(3)] + [np.full(C.shape, 9999)]
    for shift in SHIFTS:
        hi, lo, prod = _reference(C, A, B, shift)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(hi) & np.isfinite(lo) & np.isfinite(prod) & ((np.abs(hi) >= 2.0 ** -900) | true_zero) & (out[3] == 9999)
        for k, v in enumerate((hi, lo, prod, shift)):
            out[k] = np.where(ok, v, out[k])
    return out


def _check(name, A, B, C, exact, E=None, **window):
    """every entry of the kernel's result against the reference and the bound; prints and returns the largest error / bound"""
    L = _moduli()
    t0 = time.time()
    if E is None:
        E = _emu(A, B, C, **window)
    t1 = time.time()
    hi, lo, prod = _reference(C, A, B)
    assert np.isfinite(hi).all() and np.isfinite(E).all(), name
    bound = design_bound(A, B, E, prod, L, exact)
    ratio, at = error_ratio(E, hi, lo, bound)
    print("EMU-BOUND %-34s L=%2d %5d x %5d x %6d  max error/bound %.4f at %s  (gpu %.1f s, reference %.1f s)"
          % (name, L, A.shape[0], B.shape[0], A.shape[1], ratio, at, t1 - t0, time.time() - t1), flush=True)
    assert ratio <= 1.0, (name, ratio, at, float(E[at]), float(hi[at]), float(lo[at]), float(bound[at]))
    return ratio, E


CAPACITY_K = {16: (128, 256, 4096, 8192, 32768, 130944), 12: (128, 8192, 130944), 8: (128, 8192, 130944)}


def run_capacity(K):
    A, B, C = fam_capacity(np.random.default_rng(K), 150, 71, K, _moduli())
    return _check("capacity", A, B, C, True)[0]


def run_edges(K=256):
    """power-of-two and range edges: compared at the scale_exp where each entry is normal; +-inf exactly where the exact result
    rounds to it; all-zero rows and columns leave C bit-unchanged"""
    L = _moduli()
    A, B, C = fam_edges(np.random.default_rng(8), K, L)
    E = _emu(A, B, C)
    hi, lo, prod, shift = _reference_multi_scale(C, A, B)
    assert np.isin(shift, SHIFTS).all() and not np.isnan(E).any()
    za, zb = ~A.any(1), ~B.any(1)
    assert za.any() and zb.any()
    assert E[za].tobytes() == C[za].tobytes() and E[:, zb].tobytes() == C[:, zb].tobytes()
    sh = shift.astype(np.int32)
    big = 2.0 ** (1024 - 1100) * (1 - 2.0 ** -54)                        # DBL_MAX + 1/2 ulp = 2^1024 - 2^970, in the shifted scale
    over = (shift == -1100) & (np.abs(hi) >= big) & ((np.abs(hi) > big) | (np.sign(lo) * np.sign(hi) >= 0))
    fin = ~over
    assert np.array_equal(np.isinf(E), over) and np.array_equal(np.sign(E[over]), np.sign(hi[over]))
    assert over.any() and (shift == 1100).any() and (shift == 2200).any() and (np.abs(E[fin]) > 2.0 ** 1000).any()
    Es = np.ldexp(E, sh)                                                  # exact: the shift moves away from the range's ends
    assert np.array_equal(np.ldexp(Es, -sh)[fin], E[fin])
    bound = design_bound(A, B, E, prod, L, False, sh)
    assert (bound[fin] > 0).all()
    ratio, at = error_ratio(np.where(fin, Es, 0.0), np.where(fin, hi, 0.0), np.where(fin, lo, 0.0), np.where(fin, bound, 1.0))
    print("EMU-BOUND %-34s L=%2d %5d x %5d x %6d  max error/bound %.4f at %s" % ("range edges", L, len(A), len(B), K, ratio, at), flush=True)
    assert ratio <= 1.0, (ratio, at, float(E[at]), float(hi[at]), float(lo[at]), int(shift[at]))
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("K", CAPACITY_K[16])
def test_capacity(K):
    run_capacity(K)


@pytest.mark.gpu
@pytest.mark.parametrize("which, K", [("p256", 130944), ("p256", 128), ("odd", 4096), ("odd", 128)])
def test_residue_extremes(which, K):
    A, B, C = fam_residue(np.random.default_rng(K), K, 16, which)
    _check("residues " + which, A, B, C, True)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [256, 4096])
def test_garner_digit_extremes(K):
    A, B, C, _Xs = fam_garner(np.random.default_rng(K), K, 16)
    _check("garner digits", A, B, C, True)


@pytest.mark.gpu
def test_range_edges():
    run_edges()


@pytest.mark.gpu
def test_in_row_dynamic_range():
    rng = np.random.default_rng(12)
    rows, cols, K = 300, 130, 1024
    A, B, C = fam_range(rng, rows, cols, K)
    _ratio, E = _check("in-row range 2^70", A, B, C, False)
    # an entry below 2^-(alpha + 1) of its row's largest is rounded to zero by the split: changing it changes nothing
    ab, bb = bits_ab(K, 16)
    A2, B2 = A.copy(), B.copy()
    deadA = np.abs(A) < np.abs(A).max(1, keepdims=True) * 2.0 ** -(ab + 1)
    deadB = np.abs(B) < np.abs(B).max(1, keepdims=True) * 2.0 ** -(bb + 1)
    assert deadA.sum() > 1000 and deadB.sum() > 1000
    A2[deadA] *= -0.75
    B2[deadB] = 0.0
    assert _emu(A2, B2, C).tobytes() == E.tobytes()


@pytest.mark.gpu
def test_cancellation():
    """C0 = fl(A B^T): the result is rounding residue only, and the absolute bound is unchanged"""
    rng = np.random.default_rng(13)
    A, B, _C = fam_random(rng, 640, 384, 4096)
    hi, _lo = xp.exact_sub(np.zeros((640, 384)), A, B)
    ratio, E = _check("cancellation C0 = fl(A B^T)", A, B, -hi, False)
    assert np.abs(E).max() < 1e-10 * np.abs(hi).max()


WINDOWS = [  # rows, cols, K, lda, ldb, ldc, oa, ob, oc
    (1, 1, 128, 128 * 3, 128 * 2, 1, 128, 128, 0),
    (3, 384, 256, 256 + 128, 256 + 3 * 128, 384 + 129, 128, 3 * 128, 128),
    (255, 2, 256, 256 + 2 * 128, 256 + 128, 2 + 5, 256, 128, 5),
    (256, 129, 256, 256 + 3 * 128, 256 + 2 * 128, 129 + 2 * 128, 3 * 128, 128, 128),
    (257, 5, 384, 384 + 128, 384 + 128, 5 + 128, 128, 0, 128),
    (513, 128, 128, 128 * 8, 128 * 5, 128 * 3, 128 * 5, 128 * 3, 128 * 2),
    (3, 3, 1024, 1024 + 128, 1024 + 128, 3 + 384, 0, 128, 384),
    (513, 384, 256, 256 + 5 * 128, 256 + 4 * 128, 384 + 3 * 128, 5 * 128, 3 * 128, 3 * 128),
    # ldc = cols, not a multiple of 4: the rebuild thread of a row's last columns sits next to the cells of the next row, which another
    # thread (from row 512 on: another workgroup) updates -- without the j0 + e >= cols guard it stores back a stale value there
    (515, 5, 256, 256 + 128, 256 + 128, 5, 128, 0, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("w", WINDOWS, ids=lambda w: "%dx%dx%d" % w[:3])
def test_windows_of_larger_matrices(w):
    """the way tsolve.hip calls it: sub-blocks at column offsets that are multiples of 128, leading dimensions larger than the window
    (even and odd multiples of 128; ldc also odd).  NaN around A and B, a canary around C."""
    rows, cols, K, lda, ldb, ldc, oa, ob, oc = w
    A, B, C = fam_random(np.random.default_rng(rows * 1000 + cols), rows, cols, K)
    _ratio, E = _check("windows", A, B, C, False, lda=lda, ldb=ldb, ldc=ldc, oa=oa, ob=ob, oc=oc)
    assert E.tobytes() == _emu(A, B, C).tobytes()                        # and the same bits as the contiguous call


@pytest.mark.gpu
def test_workspace_tiles_k130944():
    """K = 130944, 16 moduli: emu_cap = (2^31 / (130944 * 16)) rounded down to 256 = 1024, so 1100 x 1060 runs as 2 x 2 tiles,
    ragged both ways.  Operands of 12 bits: one slice each in the reference."""
    assert _moduli() == 16                                               # (the shape is derived for 16 moduli)
    rng = np.random.default_rng(14)
    A, B, C = fam_few_bits(rng, 1100, 1060, 130944, 12)
    _ratio, E = _check("tiles 2 x 2 at K = 130944", A, B, C, True)
    assert E[1000:1060].tobytes() == _emu(A[1000:1060], B, C[1000:1060]).tobytes()   # rows across the tile boundary, alone


@pytest.mark.gpu
def test_workspace_column_tile_shortened():
    """K = 128, 16 moduli: emu_cap = 2^20, so the row tile is round_up(46000, 256) = 46080 and the column tile starts at
    round_up(3000, 256) = 3072; 46080 * 3072 * 16 > 2^31, so the loop shortens it once to 2816 (46080 * 2816 * 16 < 2^31): one row tile,
    two column tiles of 2816 and 184 columns."""
    assert _moduli() == 16                                               # (the shape is derived for 16 moduli)
    rows, cols, K, L = 46000, 3000, 128, 16
    rt, ct = -(-rows // 256) * 256, -(-cols // 256) * 256
    assert rt <= (2 ** 31 // (K * L)) // 256 * 256 and rt * ct * L > 2 ** 31 and rt * (ct - 256) * L <= 2 ** 31 and cols > ct - 256
    rng = np.random.default_rng(15)
    A, B, C = fam_few_bits(rng, rows, cols, K, 19)
    _ratio, E = _check("column tile shortened", A, B, C, True)
    assert E[:300, 2700:].tobytes() == _emu(A[:300], B[2700:], np.ascontiguousarray(C[:300, 2700:])).tobytes()


def _child(args, env, timeout=900):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=timeout, cwd=ROOT)
    sys.stdout.write(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("L", [8, 12])
def test_fewer_moduli_capacity_and_edges(L):
    """GPX_EMU_MODULI = 8 and 12 (alpha, beta < 53: nextafter(2^e, 0) scales to 2^bits itself) in a process of their own"""
    r = _child(["bound", L], {"GPX_EMU_MODULI": str(L)})
    assert r["L"] == L and r["cases"] == len(CAPACITY_K[L]) + 1 and max(r["ratios"]) <= 1.0


# ---- argument checks ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_arguments_leave_c_untouched():
    from conftest import torch
    from skgpuppy_amd import _gpx
    K, rows, cols = 256, 4, 6
    a = torch.ones((rows + 1, 2 * K), dtype=torch.float64).cuda()
    b = torch.ones((cols + 1, 2 * K), dtype=torch.float64).cuda()
    c0 = torch.as_tensor(_canary((rows, 2 * cols))).cuda()
    c = c0.clone()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 8 * off)
    good = dict(A=P(a), lda=2 * K, B=P(b), ldb=2 * K, C=P(c), ldc=2 * cols, rows=rows, cols=cols, K=K)
    refused = [dict(lda=K - 2), dict(ldb=K - 128), dict(ldc=cols - 1), dict(K=K + 64, lda=4 * K, ldb=4 * K), dict(K=100), dict(K=1 << 17, lda=1 << 17, ldb=1 << 17),
               dict(K=(1 << 17) + 128, lda=1 << 18, ldb=1 << 18), dict(K=0), dict(lda=2 * K + 1), dict(ldb=2 * K - 1), dict(A=P(a, 1)), dict(B=P(b, 3))]
    for bad in refused:
        g = dict(good, **bad)
        rc = _gpx.lib.gpx_emu_gemm_nt_sub(g["A"], g["lda"], g["B"], g["ldb"], g["C"], g["ldc"], g["rows"], g["cols"], g["K"])
        assert rc == _gpx.GPX_ERR_BAD_ARG, (bad, rc)
        assert "emu_gemm_nt_sub" in _gpx.last_error(), bad
        torch.cuda.synchronize()
        assert torch.equal(c, c0), bad


# ---- the call site: the emulated recursion of tsolve.hip at small N against the oracle ------------------------------------
# GPX_EMU_MIN_K = 1024 lets trsm_right_lt_squares emulate every update of its recursion: rows padded to 128, slabs of 1024 columns, the
# left half the largest power of two below the slab count.  The emulated products are windows of the solver's own buffers (ldz, ld), their
# workspace is sized by trsm_emu_need, and the column counts c1 - cm are the recursion's ragged last slabs.
EST_CASES = [(1100, 257), (2200, 300), (3000, 129), (4224, 517), (5000, 130), (7300, 1000)]      # N, M (ragged; > 32: the many-row solver)
KV_CASE = (2200, 300)
PROP_CASES = [(1500, 3), (1500, 517), (2200, 3), (2200, 517)]                                    # N, B; d = 9: 3 (d + 2) = 33 rows > 32
PROP_D = 9


def emulated_updates(N, min_k=1024, slab=1024, tile=128):
    """(K, columns) of every update of trsm_right_lt_squares(0, P) that emu_enabled(K) sends to emu_gemm_nt_sub, in order"""
    npad = -(-N // tile) * tile
    out = []

    def rec(p0, p1):
        if p1 - p0 <= 1:
            return
        h = 1
        while h * 2 < p1 - p0:
            h *= 2
        pm = p0 + h
        rec(p0, pm)
        c0, cm, c1 = p0 * slab, pm * slab, min(p1 * slab, npad)
        if min_k <= cm - c0 < 2 ** 17 and (cm - c0) % 128 == 0:
            out.append((cm - c0, c1 - cm))
        rec(pm, p1)
    rec(0, -(-npad // slab))
    return out


def test_recursion_shapes_of_the_small_cases():
    """what the cases below put through the emulated product: K = 1024, 2048 and 4096 with 128, 256, 1024 and 3328 columns among them"""
    want = {1100: [(1024, 128)], 2200: [(1024, 1024), (2048, 256)], 3000: [(1024, 1024), (2048, 1024)],
            4224: [(1024, 1024), (2048, 2048), (1024, 1024), (4096, 128)], 5000: [(1024, 1024), (2048, 2048), (1024, 1024), (4096, 1024)],
            7300: [(1024, 1024), (2048, 2048), (1024, 1024), (4096, 3328), (1024, 1024), (2048, 1280), (1024, 256)],
            1500: [(1024, 512)]}
    for N, shapes in want.items():
        assert emulated_updates(N) == shapes, N
    assert all(not emulated_updates(N, 4096) for N in (1100, 2200, 3000))            # the default threshold leaves them native
    assert emulated_updates(16384, 4096) == [(4096, 4096), (8192, 8192), (4096, 4096)]


def _est_problem(N, M, d=8):
    rng = np.random.RandomState(100 + N + d)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (M, d))
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    return x, t, xs, theta


def _prop_inputs(x, B, d, seed):
    """as tests/_propagate_many_worker.inputs: every 37th input a copy of a training row, a full SPD Sigma for each"""
    rng = np.random.RandomState(seed)
    U = rng.uniform(0, 10, (B, d))
    U[::37] = x[rng.randint(0, len(x), len(U[::37]))]
    A = rng.uniform(-0.1, 0.1, (B, d, d))
    return U, np.einsum("bij,bkj->bik", A, A) + 0.005 * np.eye(d)


def run_recursion(out):
    """child process: every case on the device with this process's GPX_EMU_* settings -> one .npz"""
    try:
        import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)
    except Exception:
        pass
    import skgpuppy_amd as sk
    from skgpuppy_amd import _gpx
    from oracle import oracle as orc
    res = {}
    for N, M in EST_CASES:
        x, t, xs, theta = _est_problem(N, M)
        gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
        res["est%d" % N] = np.stack(gp.estimate_many(xs))
        gp._dev().close()
    N, M = KV_CASE
    x, t, xs, theta = _est_problem(N, M)
    K, kv = orc.gram(x, theta), np.ascontiguousarray(orc.gram_ij(xs, x, theta))
    kd = np.full(M, np.exp(theta[0]) + np.exp(theta[1]))
    tc = np.ascontiguousarray(t - t.mean())
    h = ctypes.c_void_p()
    _gpx.check(_gpx.lib.gpx_fit_matrix(_gpx.ptr(K), _gpx.ptr(tc), N, None, ctypes.byref(h)), "gpx_fit_matrix")
    mean, var = np.empty(M), np.empty(M)
    _gpx.check(_gpx.lib.gpx_predict_kv(h, _gpx.ptr(kv), M, _gpx.ptr(kd), _gpx.ptr(mean), _gpx.ptr(var)), "gpx_predict_kv")
    _gpx.lib.gpx_free(h)
    res["kv%d" % N] = np.stack([mean + t.mean(), var])
    for N in sorted({n for n, _b in PROP_CASES}):
        x, t, _xs, theta = _est_problem(N, 1, PROP_D)
        gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
        for B in [b for n, b in PROP_CASES if n == N]:
            U, S = _prop_inputs(x, B, PROP_D, N + B)
            res["prop%d_%d" % (N, B)] = np.stack(sk.UncertaintyPropagationApprox(gp).propagate_GA_many(U, S))
        gp._dev().close()
    np.savez(out, **res)


_RUNS = {}


def _recursion_run(tmp_path_factory, name):
    """one child per setting, one after the other, each under its own time limit; kept for the tests of this module"""
    env = {"emu16": {"GPX_EMU_F64": "1", "GPX_EMU_MIN_K": "1024", "GPX_EMU_MODULI": "16"},
           "emu12": {"GPX_EMU_F64": "1", "GPX_EMU_MIN_K": "1024", "GPX_EMU_MODULI": "12"},
           "native": {"GPX_EMU_F64": "0"}}[name]
    if name not in _RUNS:
        out = str(tmp_path_factory.mktemp("recursion") / (name + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "recursion", out], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        with np.load(out) as z:
            _RUNS[name] = {k: z[k] for k in z.files}
    return _RUNS[name]


def _oracle_values():
    """the oracle's answer to every case (CPU), and the tolerance of each: (value [2, n], rtol, atol mean, atol var)"""
    if "oracle" not in _RUNS:
        from oracle import oracle as orc
        ref = {}
        for N, M in EST_CASES:
            x, t, xs, theta = _est_problem(N, M)
            og = orc.OracleGP(x, t, theta)
            ref["est%d" % N] = (np.stack(og.estimate_many(xs)), 1e-6, 1e-9, 2e-9)          # test_against_oracle_ragged
            if (N, M) == KV_CASE:
                ref["kv%d" % N] = ref["est%d" % N]
        for N in sorted({n for n, _b in PROP_CASES}):
            x, t, _xs, theta = _est_problem(N, 1, PROP_D)
            og = orc.OracleGP(x, t, theta)
            for B in [b for n, b in PROP_CASES if n == N]:
                U, S = _prop_inputs(x, B, PROP_D, N + B)
                ref["prop%d_%d" % (N, B)] = (np.array([orc.approx_propagate(og, U[i], S[i]) for i in range(B)]).T, 0.0, 1e-9, 2e-8)   # test_propagate_many
        _RUNS["oracle"] = ref
    return _RUNS["oracle"]


def _excess(got, ref):
    """max over the outputs of |got - oracle| / (atol + rtol |oracle|) for mean and variance, and the largest absolute differences"""
    val, rtol, am, av = ref
    dm, dv = np.abs(got[0] - val[0]), np.abs(got[1] - val[1])
    return max((dm / (am + rtol * np.abs(val[0]))).max(), (dv / (av + rtol * np.abs(val[1]))).max()), dm.max(), dv.max()


@pytest.mark.gpu
def test_emulated_recursion_against_oracle(tmp_path_factory):
    """estimate_many at N = 1100 .. 7300, gpx_predict_kv on a gpx_fit_matrix handle and propagate_GA_many with every update from K = 1024
    emulated (16 moduli): the tolerances of test_against_oracle_ragged and of test_propagate_many's oracle test, and outputs that differ
    from the GPX_EMU_F64 = 0 run (the emulated path was taken)"""
    emu, nat, ref = _recursion_run(tmp_path_factory, "emu16"), _recursion_run(tmp_path_factory, "native"), _oracle_values()
    assert sorted(emu) == sorted(nat) == sorted(ref)
    for k in sorted(ref):
        (xe, dme, dve), (xn, dmn, dvn) = _excess(emu[k], ref[k]), _excess(nat[k], ref[k])
        print("EMU-RECURSION %-12s 16 moduli: |dmean| %.3e |dvar| %.3e (%.3g of tolerance)   native: %.3e %.3e (%.3g)" % (k, dme, dve, xe, dmn, dvn, xn), flush=True)
        assert np.isfinite(emu[k]).all() and not np.array_equal(emu[k], nat[k]), k
        assert xe <= 1.0 and xn <= 1.0, k


@pytest.mark.gpu
def test_emulated_recursion_12_moduli(tmp_path_factory):
    """GPX_EMU_MODULI = 12 (alpha + beta = 83 at K = 1024, 41 + 42 bits): held to four times the larger of the 16-modulus and the native
    difference to the oracle, or to the existing tolerance where that is looser.  Measured on an MI355X (profiles/r09_emu_bound.txt),
    worst case over all outputs of all cases in units of the existing tolerance: 12 moduli 0.0815, 16 moduli 0.000848, native fp64
    0.000826 (largest |dmean| 5.0e-10 / 4.4e-12 / 4.4e-12 at N = 7300, largest |dvar| 4.6e-12 / 4.0e-12 / 4.0e-12): the existing
    tolerance is the looser of the two here, and 12 moduli use 8 % of it."""
    e12, e16, nat = (_recursion_run(tmp_path_factory, n) for n in ("emu12", "emu16", "native"))
    ref = _oracle_values()
    worst = [0.0, 0.0, 0.0]
    for k in sorted(ref):
        x12, x16, xn = _excess(e12[k], ref[k]), _excess(e16[k], ref[k]), _excess(nat[k], ref[k])
        print("EMU-RECURSION %-12s 12 moduli: |dmean| %.3e |dvar| %.3e (%.3g of tolerance; 16 moduli %.3g, native %.3g)" % (k, x12[1], x12[2], x12[0], x16[0], xn[0]),
              flush=True)
        assert not np.array_equal(e12[k], nat[k]) and not np.array_equal(e12[k], e16[k]), k
        assert x12[0] <= max(4.0 * max(x16[0], xn[0]), 1.0), k
        worst = [max(a, b[0]) for a, b in zip(worst, (x12, x16, xn))]
    print("EMU-RECURSION worst of tolerance: 12 moduli %.3g, 16 moduli %.3g, native %.3g" % tuple(worst), flush=True)


def main(argv):
    """child process: the families that depend on GPX_EMU_MODULI (one JSON line last), or the cases of the recursion (one .npz)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-gpuppy_amd"), os.path.join(ROOT, "tests")]
    if argv[0] == "recursion":
        return run_recursion(argv[1])
    L = int(argv[1])
    assert argv[0] == "bound" and _moduli() == L
    ratios = [run_capacity(K) for K in CAPACITY_K[L]] + [run_edges()]
    print(json.dumps({"L": L, "cases": len(ratios), "ratios": ratios}))


if __name__ == "__main__":
    main(sys.argv[1:])
