"""The fixed-scale split of the left-looking solve on the CPU (tests/_emu_left_model.py: integer residues by the kernel's rule, the
product rebuilt by Python integers): the bound of DESIGN.md section 6 holds on every entry, one unit of error in one residue is seen,
and a bound that is too small is reported instead of wrapping."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _emu_left_model as lm
from _emu_model import MODULI, scale_bits


def _operands(seed, rows=7, cols=5, K=128):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((rows, K)) * np.exp2(-rng.uniform(0, 30, (rows, K))) * np.exp2(rng.integers(-20, 21, (rows, 1)))
    B = rng.standard_normal((cols, K)) * np.exp2(rng.integers(-20, 21, (cols, 1)))
    m = np.abs(A).max(1)
    bounds = m * np.array([1.0, 1.5, 2.0 ** 30, 3.0, 1.0, 2.0 ** 10, 1.9999])[:rows]     # the largest entry at, and up to 2^30 below, its bound
    A[4] = 0.0
    bounds[4] = 0.0                                                                    # an all-zero row with bound 0
    return A, bounds, B


@pytest.mark.parametrize("slabs, L", [(5, 16), (16, 16), (9, 12)])
def test_bound_holds_on_every_entry(slabs, L):
    abits, bbits = lm.left_bits(slabs, L)
    assert abits + bbits == scale_bits(1024 * (slabs - 1), L)
    A, bounds, B = _operands(slabs)
    M = lm.fixed_product(A.tolist(), bounds.tolist(), B.tolist(), abits, bbits, L)
    worst = Fraction(0)
    for i in range(len(A)):
        for j in range(len(B)):
            exact = sum(Fraction(a) * Fraction(b) for a, b in zip(A[i].tolist(), B[j].tolist()))
            bound = lm.fraction_bound(A[i].tolist(), float(bounds[i]), B[j].tolist(), abits, bbits)
            assert abs(M[i][j] - exact) <= bound, (i, j)
            if bound:
                worst = max(worst, abs(M[i][j] - exact) / bound)
    assert all(v == 0 for v in M[4])                                                   # the zero row
    assert worst > Fraction(1, 1000)                                                   # the bound is not vacuous
    # the issue's form of the A term: 2^-abits 2 bound_i per entry of A
    for i in (0, 1, 2, 3, 5, 6):
        s = lm.fixed_scale(float(bounds[i]), abits)
        assert Fraction(1, 2) / Fraction(2) ** s <= Fraction(2) ** -abits * 2 * Fraction(float(bounds[i]))


def test_an_entry_below_its_bound_keeps_its_bits():
    """a row 2^-30 below its bound keeps abits - 31 bits: the rounding step is 2^(31 - abits) of the row's largest entry at most"""
    abits, _ = lm.left_bits(16)
    assert abits == 55
    x = [1.0 + 2.0 ** -20, -0.75, 2.0 ** -21 * 1.5]
    s = lm.fixed_scale(2.0 ** 30, abits)
    a, over = lm.split_fixed(x, s, abits)
    assert not over and s == abits - 2 - 30
    assert [Fraction(v) / Fraction(2) ** s for v in a] == [Fraction(v) for v in x]      # down to 2^-23: held exactly
    y = [1.0 + 2.0 ** -30]
    assert Fraction(lm.split_fixed(y, s, abits)[0][0]) / Fraction(2) ** s == 1          # 30 bits: rounded at 2^-(abits - 32)


def test_one_unit_in_one_residue_is_seen():
    abits, bbits = lm.left_bits(5)
    A, bounds, B = _operands(3)
    good = lm.fixed_product(A.tolist(), bounds.tolist(), B.tolist(), abits, bbits)
    for l in (0, 7, 15):
        bad = lm.fixed_product(A.tolist(), bounds.tolist(), B.tolist(), abits, bbits, defect=(2, 3, l))
        for i in range(len(A)):
            for j in range(len(B)):
                if (i, j) != (2, 3):
                    assert bad[i][j] == good[i][j]
        exact = sum(Fraction(a) * Fraction(b) for a, b in zip(A[2].tolist(), B[3].tolist()))
        bound = lm.fraction_bound(A[2].tolist(), float(bounds[2]), B[3].tolist(), abits, bbits)
        assert abs(bad[2][3] - exact) > bound                                          # M_l = P / p_l units of X: far outside


def test_wrong_bounds_are_reported():
    abits, _ = lm.left_bits(16)
    x = [0.3, -1.0, 0.999]
    for f, want in ((1.0, False), (0.5, False), (0.26, False), (0.125, True), (2.0 ** -40, True)):
        # |x| <= 2 bound never overflows; from 4 bound on it always does (between the two the binade of the bound decides)
        assert lm.split_fixed(x, lm.fixed_scale(f, abits), abits)[1] == want, f
    for b in np.exp2(np.arange(-3.0, 3.0, 0.37)):
        assert not lm.split_fixed([2 * b], lm.fixed_scale(float(b), abits), abits)[1]
        assert lm.split_fixed([4.0001 * b], lm.fixed_scale(float(b), abits), abits)[1]
    a, over = lm.split_fixed([0.0, 1e-3], lm.fixed_scale(0.0, abits), abits)
    assert over and a == [0, 0]                                                        # bound 0, an entry that is not
    for b in (-1.0, float("nan"), float("inf")):
        assert lm.fixed_scale(b, abits) is None
    assert math.prod(MODULI) > 2 ** 125
