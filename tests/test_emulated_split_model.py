"""No GPU: the residue routine of the splits (csrc/emu.hip: two 32-bit words of a' + 2^60, two byte dot products per modulus, a 24-bit
multiply-high for the quotient) modelled in numpy (tests/_emu_split_model.py) gives the balanced residue of every integer |a'| <= 2^59.
Exhaustive over every x the dot products can produce, for each modulus; against Python integers for random and extreme a'."""
import random

import numpy as np
import pytest

from _emu_model import MODULI, balanced
from _emu_split_model import BIAS, MAX_BITS, reachable_x, reduce_x, residues_exact, residues_model, split_constants, words


@pytest.mark.parametrize("p", MODULI[1:])
def test_every_reachable_x_reduces_to_its_balanced_residue(p):
    c, k0, m = split_constants(p)
    assert p % 2 == 1 and all(0 <= v < p for v in c) and 0 <= k0 < p and (k0 + 2 ** BIAS) % p == 0
    assert (m - 1) * p < 2 ** 31 <= m * p and m < 2 ** 24                # m = ceil(2^31 / p) fits the 24-bit multiply
    xmax = reachable_x(p)
    assert xmax < 2 ** 19 and 2 * xmax + p < 2 ** 21
    x = np.arange(xmax + 1, dtype=np.uint64)
    byte, r, q, y = reduce_x(x, p)
    assert (y < 2 ** 24).all() and (q < 2 ** 12).all()
    assert (np.abs(r) <= (p - 1) // 2).all()                             # the symmetric representative, no tie for odd p
    assert ((x.astype(np.int64) - r) % p == 0).all()
    assert (byte == r.astype(np.int8)).all()                             # the low byte of r + 256 q is r's
    assert (q == (2 * x.astype(np.int64) + p) // (2 * p)).all()          # the quotient is the exact floor


def _doubles_that_are_integers(bits, rng):
    """Python integers a', |a'| <= 2^bits, each exactly an fp64."""
    top = 2 ** bits
    ulp = max(1, 2 ** (bits - 53))                                      # spacing of the doubles just below 2^bits
    xs = [0, 1, -1, top, -top, top - ulp, -(top - ulp), 2 ** 32, -(2 ** 32), 2 ** 32 - 1, -(2 ** 32) + 1, 2 ** 31, -(2 ** 31)]
    for p in MODULI:
        k = top // p
        for v in (p, -p, 3 * p, k * p, -k * p):                          # multiples of p (rounded to a double below)
            xs.append(v)
    xs += [128, -128, 384, -384, 128 + 256 * 12345, -(128 + 256 * 12345), top - 128 if bits > 8 else 128, -(top - 128) if bits > 8 else -128]
    for _ in range(20000):
        e = rng.randint(0, bits)
        xs.append(rng.randint(-(2 ** e), 2 ** e))
    xs = [int(float(v)) for v in xs if abs(v) <= top]                   # the nearest double (only values past 2^53 move)
    assert all(abs(v) <= top and float(v) == v for v in xs)
    return xs


@pytest.mark.parametrize("bits", [24, 55, MAX_BITS])
def test_model_equals_python_integers(bits):
    xs = _doubles_that_are_integers(bits, random.Random(bits))
    a = np.array([float(v) for v in xs])
    lo, hi = words(a)
    assert all(int(h) * 2 ** 32 + int(l) == v + 2 ** BIAS for v, l, h in zip(xs[:200], lo[:200], hi[:200]))
    got = residues_model(a, 16)
    for l, p in enumerate(MODULI):
        want = np.array([balanced(v, p) for v in xs], np.int64).astype(np.int8)   # 128 mod 256: balanced() gives -128 itself
        assert (got[l] == want).all(), (p, [xs[i] for i in np.flatnonzero(got[l] != want)[:5]])
    assert (got == residues_exact(np.array(xs, np.int64), 16)).all()     # the GPU test's host reference agrees as well
    if bits > 8:
        i = xs.index(128)
        assert got[0][i] == -128 and got[0][xs.index(-128)] == -128      # +-128 mod 256 share the byte
