"""An error-free CPU reference for C0 - A B^T (row-major A [rows, K], B [cols, K], fp64), every entry, in plain numpy.

Each row of A and of B is scaled by a power of two so that its largest entry lies in [1/2, 1), and is then peeled into integer slices of
q bits (t = rint(r 2^q), r <- r 2^q - t: every step exact).  With 2 q + ceil(log2 K) + 4 <= 52 every slice-by-slice product is a sum of
integers that stays below 2^48, so fp64 BLAS computes it exactly in any order, and up to 16 such products of one weight 2^-(d q) add
exactly as well.  The weighted sums are added to C0, largest first, in a three-term expansion (TwoSum on the leading and on the second
term), and the result is returned as an unevaluated pair (hi, lo): hi = fl(exact), |hi + lo - exact| <~ 2^-104 |exact| + 2^-150 of the
largest partial sum.  Nothing is approximated silently: operands whose rows need more than `max_slices` slices, or whose scaling is not
exact (an in-row range beyond fp64's exponent range), raise.

scale_exp returns (C0 - A B^T) 2^scale_exp instead, for results outside fp64's range (the caller picks it so that nothing it cares about
is subnormal or overflows).  Nothing here imports the product or the oracle.
"""
import math

import numpy as np


def two_sum(a, b):
    """s = fl(a + b) and e with a + b = s + e exactly (Knuth; no overflow assumed)."""
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    return s, e


def slice_bits(K):
    return (52 - 4 - max(0, math.ceil(math.log2(K)))) // 2


def row_exponents(X):
    """e with max|row| in [2^(e-1), 2^e); 0 for an all-zero row"""
    m = np.abs(X).max(axis=1)
    return np.where(m > 0, np.frexp(m)[1], 0).astype(np.int64)


def slices(X, q, max_slices=16):
    """(list of integer-valued arrays T_s, row exponents e): X[i, k] = 2^e_i sum_s T_s[i, k] 2^-((s + 1) q) exactly"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if not np.isfinite(X).all():
        raise ValueError("exact reference: non-finite operand")
    e = row_exponents(X)
    r = np.ldexp(X, (-e)[:, None].astype(np.int32))
    if not np.array_equal(np.ldexp(r, e[:, None].astype(np.int32)), X):
        raise ValueError("exact reference: a row's range exceeds what one power-of-two scale can hold")
    out = []
    while r.any():
        if len(out) == max_slices:
            raise ValueError("exact reference: more than %d slices of %d bits needed" % (max_slices, q))
        r = np.ldexp(r, q)
        t = np.rint(r)
        r = r - t                                   # exact: |r| <= 1/2, a multiple of the operand's last bit
        out.append(t)
    return out or [np.zeros_like(X)], e


def exact_sub(C0, A, B, scale_exp=0, max_slices=16, perturb=None):
    """(hi, lo) with hi + lo = (C0 - A B^T) 2^scale_exp for every entry (see the module docstring for the residual).

    perturb = (s, t, i, j): entry (i, j) of the product of slice s of A with slice t of B is changed by 1 -- the defect the CPU tests
    plant to show that the comparison against exact rational arithmetic sees one unit of one slice product."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    C0 = np.asarray(C0, dtype=np.float64)
    rows, K = A.shape
    cols = B.shape[0]
    assert B.shape[1] == K and C0.shape == (rows, cols)
    q = slice_bits(K)
    Sa, ea = slices(A, q, max_slices)
    Sb, eb = slices(B, q, max_slices)
    if min(len(Sa), len(Sb)) > 16:
        raise ValueError("exact reference: more than 16 products of one weight")
    # all slice pairs in one product: block (s, t) of [Sa_0; Sa_1; ...] [Sb_0; Sb_1; ...]^T
    P = np.concatenate(Sa, 0) @ np.concatenate(Sb, 0).T
    if perturb is not None:
        s, t, i, j = perturb
        P[s * rows + i, t * cols + j] += 1.0
    E = (ea[:, None] + eb[None, :] + scale_exp).astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = np.ldexp(C0, scale_exp) if scale_exp else C0.copy()
        lo = np.zeros_like(hi)
        lo2 = np.zeros_like(hi)
        for d in range(len(Sa) + len(Sb) - 1):      # weight 2^-((d + 2) q): largest first
            Pd = None
            for s in range(max(0, d - len(Sb) + 1), min(d, len(Sa) - 1) + 1):
                blk = P[s * rows:(s + 1) * rows, (d - s) * cols:(d - s + 1) * cols]
                Pd = blk.copy() if Pd is None else Pd + blk          # integers below 2^52: exact
            T = np.ldexp(Pd, np.clip(E - (d + 2) * q, -4000, 4000).astype(np.int32))
            hi, e1 = two_sum(hi, -T)
            lo, e2 = two_sum(lo, e1)
            lo2 += e2
        hi, lo = two_sum(hi, lo)
        lo = lo + lo2
        hi, lo = two_sum(hi, lo)
    return hi, lo
