"""A Python-integer model of the emulated fp64 update (csrc/emu.hip, Ozaki scheme II): the moduli, the scale bits, the row split, the
balanced residues, Garner's mixed-radix digits and the whole product in exact arithmetic.  Shared by tests/test_emulated_update.py and
tests/test_emulated_bound.py; it imports nothing from the product."""
import math
from fractions import Fraction

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 211, 199, 197, 193, 191]


def scale_bits(K, L):
    """alpha + beta as emu.hip computes it: the largest s with K 2^s < P / 2."""
    return math.floor(sum(math.log2(p) for p in MODULI[:L]) - 1.0 - math.log2(K) - 1e-9)


def balanced(r, p):
    r %= p
    if p == 256:
        return r - 256 if r >= 128 else r
    return r - p if r > (p - 1) // 2 else r


def split_row(x, bits):
    """(integers a', exponent s): a' = rint(x 2^s) with the row's largest |x| in [2^(bits-1), 2^bits) after scaling."""
    m = max(abs(v) for v in x)
    if m == 0.0:
        return [0] * len(x), 0
    s = bits - 1 - (math.frexp(m)[1] - 1)
    return [int(round(math.ldexp(v, s))) for v in x], s


def garner(res, L):
    """balanced mixed-radix digits of the residues -> the integer in [-P/2, P/2) (what emu_rebuild_kernel evaluates)."""
    v = [balanced(res[0], MODULI[0])]
    for k in range(1, L):
        pk, t = MODULI[k], res[k]
        for j in range(k):
            t = (t - v[j]) * pow(MODULI[j], -1, pk)
        v.append(balanced(t, pk))
    x = 0
    for k in range(L - 1, -1, -1):
        x = x * MODULI[k] + v[k]
    return x


def emulated_product(A, B, L=16):
    K = len(A[0])
    bits = scale_bits(K, L)
    ab, bb = bits - bits // 2, bits // 2
    sa = [split_row(r, ab) for r in A]
    sb = [split_row(r, bb) for r in B]
    out = []
    for ai, si in sa:
        row = []
        for bj, tj in sb:
            res = [sum(balanced(a, p) * balanced(b, p) for a, b in zip(ai, bj)) for p in MODULI[:L]]
            X = garner([balanced(r, p) for r, p in zip(res, MODULI[:L])], L)
            assert X == sum(a * b for a, b in zip(ai, bj))             # the residues determine the integer product
            row.append(Fraction(X) / Fraction(2) ** (si + tj))
        out.append(row)
    return out
