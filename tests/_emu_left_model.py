"""A Python-integer model of the fixed-scale split of the left-looking solve (csrc/emu.hip, emu_split_fixed_kernel and
emu_scale_from_bound_kernel) and the error bound of DESIGN.md section 6 that follows from it.  It imports nothing from the product.

The row scale comes from a bound on the row that is known before the row is: s_i = abits - 1 - ilogb(2 bound_i).  An entry
|x| <= bound_i scales below 2^(abits - 1); the rounding a' = rint(x 2^s_i) moves it by at most 2^-s_i / 2 <= 2^-abits 2 bound_i.  With
row j of B split as before (tau_j from its largest entry and bbits), every entry of C = C0 - A B^T obeys

    |E_ij - exact_ij| <= 1/2 sum_k (|a_ik| 2^-tau_j + |b_jk| 2^-s_i) + K 2^-(s_i + tau_j) / 4      (rounding of the two splits)
                         + ulp(X_ij 2^-(s_i + tau_j))                                              (X -> fp64, two roundings)
                         + 1/2 ulp(E_ij)                                                           (the subtraction)

whose second term is at most 2^-abits 2 bound_i |b_j|_1: the statement of the issue per A entry, summed over the row of B.
"""
import math
from fractions import Fraction

import numpy as np

from _emu_model import MODULI, balanced, garner, scale_bits, split_row

ZERO_BOUND_SCALE = 1000          # the scale of a row whose bound is 0: a double of magnitude 2^(abits - 1000) or more overflows 2^abits (status); smaller
                                 # ones are held exactly or rounded to an integer, below about 2^-1000 to 0 unseen -- harmless next to a bound of 0


def left_bits(slabs, L=16, slab=1024):
    """(abits, bbits) of a solve over `slabs` slabs: from the deepest update, K = slab (slabs - 1)"""
    b = scale_bits(slab * (slabs - 1), L)
    return b - b // 2, b // 2


def fixed_scale(bound, abits):
    """s of emu_scale_from_bound_kernel, or None where the bound is no bound (negative, NaN, Inf: the status word)"""
    if not (bound >= 0.0) or math.isinf(bound):
        return None
    if bound == 0.0:
        return ZERO_BOUND_SCALE
    return abits - 2 - (math.frexp(bound)[1] - 1)


def split_fixed(x, s, abits):
    """(integers a', overflow) of emu_split_fixed_kernel for a finite row: a' = rint(x 2^s), 0 and the flag where |a'| > 2^abits"""
    out, over = [], False
    for v in x:
        a = Fraction(v) * Fraction(2) ** s
        a = int(round(a))                                   # round half to even, as rint
        if abs(a) > 2 ** abits:
            a, over = 0, True
        out.append(a)
    return out, over


def fixed_product(A, bounds, B, abits, bbits, L=16, defect=None):
    """A B^T as the scheme computes it: A's rows split with their fixed scales, B's rows with their own, the integer product rebuilt from
    its L residues (Python integers).  defect = (i, j, l): one unit added to residue l of entry (i, j).  Returns rows of Fraction."""
    out = []
    sb = [split_row(r, bbits) for r in B]
    for i, (row, bd) in enumerate(zip(A, bounds)):
        s = fixed_scale(bd, abits)
        ai, over = split_fixed(row, s, abits)
        assert not over
        line = []
        for j, (bj, tj) in enumerate(sb):
            res = [sum(balanced(a, p) * balanced(b, p) for a, b in zip(ai, bj)) % p for p in MODULI[:L]]
            if defect is not None and defect[:2] == (i, j):
                res[defect[2]] = (res[defect[2]] + 1) % MODULI[defect[2]]
            X = garner([balanced(r, p) for r, p in zip(res, MODULI[:L])], L)
            if defect is None:
                assert X == sum(a * b for a, b in zip(ai, bj))         # K 2^(abits + bbits) < P / 2: the residues determine X
            line.append(Fraction(X) / Fraction(2) ** (s + tj))
        out.append(line)
    return out


def fraction_bound(a_row, bound, b_row, abits, bbits):
    """the first line of the bound above for one entry, in rational arithmetic"""
    s = fixed_scale(bound, abits)
    tj = split_row(b_row, bbits)[1]
    two = Fraction(2)
    first = sum(abs(Fraction(a)) / two ** tj + abs(Fraction(b)) / two ** s for a, b in zip(a_row, b_row)) / 2
    return first + Fraction(len(a_row), 4) / two ** (s + tj)


def b_scale(B, bbits):
    """tau_j of emu_split_kernel: bbits - 1 - ilogb(max|row|), 0 for an all-zero row"""
    m = np.abs(B).max(axis=1)
    return np.where(m > 0, bbits - np.frexp(m)[1], 0).astype(np.int64)


def a_scale(bounds, abits):
    b = np.asarray(bounds, dtype=np.float64)
    return np.where(b > 0, abits - 1 - np.frexp(np.where(b > 0, b, 1.0))[1], ZERO_BOUND_SCALE).astype(np.int64)


def left_bound(A, bounds, B, E, prod, abits, bbits):
    """the whole right-hand side above for every entry (numpy, extended precision for the sums); prod = fl(A B^T), E the kernel's result"""
    ld = np.longdouble
    K = A.shape[1]
    sg, tu = a_scale(bounds, abits), b_scale(B, bbits)
    sa, sb = np.abs(A).sum(1, dtype=ld), np.abs(B).sum(1, dtype=ld)
    i32 = lambda e: e.astype(np.int32)
    first = (np.ldexp(0.5 * sa[:, None], i32(-tu[None, :] + 0 * sg[:, None])) + np.ldexp(0.5 * sb[None, :], i32(-sg[:, None] + 0 * tu[None, :]))
             + np.ldexp(ld(K / 4.0), i32(-(sg[:, None] + tu[None, :]))))
    tail = np.spacing(np.abs(prod)).astype(ld) + 0.5 * np.spacing(np.abs(E)).astype(ld)
    return (first + tail).astype(np.float64)
