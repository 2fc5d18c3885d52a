"""(Goes with r20_emu_epilogue_int_wide.patch, which did not ship: pytest this file directly.)
The integer reduction of the int8 product's epilogue (emu_prod_word of the patch) restated in NumPy, against the fp64 formula it
replaced, (int8_t)(int)fma(-rint(v / p), p, v), for every modulus:

    u = v + 2^31 (v ^ 0x80000000), bytes d_0 .. d_3;  x = k0 + sum_k d_k (2^(8k) mod p),  k0 = (-2^31) mod p;
    q = ((2 x + p) m) >> 32,  m = ceil(2^31 / p);  byte = (x + (256 - p) q) & 255.

The quotient is exact (x < 2^18, so (2 x + p) m / 2^32 exceeds (2 x + p) / (2 p) by less than 2^-12 while the next integer is at least
1 / (2 p) > 2^-9 away): this arithmetic has no correction step, and m off by one either way changes no byte -- asserted below, because a
reduction that needed its reciprocal to the last unit would be the more fragile one.  The two planted defects are therefore the two this
arithmetic CAN have: a reciprocal that is one place off (the neighbouring modulus's m), and the missing correction k0 of the 2^31 offset.
No GPU is needed."""
import numpy as np
import pytest

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 211, 199, 197, 193, 191]


def constants(p):
    w = [pow(256, k, p) for k in range(4)]
    return w, (-(1 << 31)) % p, -(-(1 << 31) // p)


def reduce_integer(v, p, m=None, k0=None):
    """the kernel's arithmetic, in uint64 with the widths of the instructions checked"""
    w, k0_, m_ = constants(p)
    m = m_ if m is None else m
    k0 = k0_ if k0 is None else k0
    u = (v.astype(np.int64) + (1 << 31)).astype(np.uint64)
    assert (u < (1 << 32)).all()
    x = np.full(v.shape, k0, np.uint64)
    for k in range(4):
        x += ((u >> np.uint64(8 * k)) & np.uint64(255)) * np.uint64(w[k])
    y = np.uint64(2) * x + np.uint64(p)
    assert (x < (1 << 18)).all() and (y < (1 << 24)).all() and m < (1 << 24)      # v_mul_hi_u32_u24 takes both whole
    q = (y * np.uint64(m)) >> np.uint64(32)
    assert (q < (1 << 24)).all()                                                   # v_mad_u32_u24
    return ((x + q * np.uint64(256 - p)) & np.uint64(255)).astype(np.uint8).view(np.int8)


def reduce_fp64(v, p):
    """(int8_t)(int)fma(-rint(v * (1 / p)), p, v): rint(..) p is an integer below 2^53, so the fma is the exact difference"""
    vd = v.astype(np.float64)
    r = vd - np.rint(vd * (1.0 / float(p))) * float(p)
    assert (np.abs(r) <= p / 2).all()
    return r.astype(np.int64).astype(np.uint8).view(np.int8)                       # (128 mod 256 wraps to -128)


def _values(p):
    rng = np.random.default_rng(20 + p)
    top = ((1 << 31) - 1) // p
    ks = np.concatenate([[top, top - 1, top + 1, -top, -top + 1, -top - 1], rng.integers(-top, top + 1, 4096)]).astype(np.int64)
    v = (ks[:, None] * p + np.arange(-p, p + 1, dtype=np.int64)[None, :]).ravel()
    v = v[np.abs(v) < (1 << 31)]                                                   # the kernel's sums: |v| < 2^31
    return np.concatenate([np.arange(-(1 << 17), (1 << 17) + 1, dtype=np.int64), v,
                           [(1 << 31) - 1, -(1 << 31) + 1, 2145386496, -2145386496, -2128625664]])


@pytest.mark.parametrize("p", MODULI)
def test_integer_reduction_is_the_fp64_formula(p):
    v = _values(p)
    want = reduce_fp64(v, p)
    got = reduce_integer(v, p)
    bad = got != want
    assert not bad.any(), (p, v[bad][:5], got[bad][:5], want[bad][:5])
    if p == 256:
        np.testing.assert_array_equal(got, (v & 255).astype(np.uint8).view(np.int8))
    # the reciprocal has three bits to spare: one unit either way is the same quotient
    _, _, m = constants(p)
    for dm in (-1, 1):
        np.testing.assert_array_equal(reduce_integer(v, p, m=m + dm), want)


@pytest.mark.parametrize("l", range(1, len(MODULI)))
def test_planted_defects_fail(l):
    p = MODULI[l]
    v = _values(p)
    want = reduce_fp64(v, p)
    neighbour = constants(MODULI[l - 1] if l > 1 else MODULI[l + 1])[2]            # the reciprocal one place off in the table
    assert (reduce_integer(v, p, m=neighbour) != want).any()
    assert (reduce_integer(v, p, k0=0) != want).any()                             # the 2^31 offset left uncorrected
