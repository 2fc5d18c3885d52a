"""A numpy model of the residue routine of the emulated update's splits (csrc/emu.hip, emu_words / emu_plane_bytes), step by step as the
kernel computes it, and the exact residues it must equal.  The constants are derived here from the moduli, not copied from the kernel.
Shared by tests/test_emulated_split_model.py (no GPU) and tests/test_emulated_split.py; it imports nothing from the product."""
import numpy as np

from _emu_model import MODULI

NONFINITE = 0x7FFFFFFF
MAX_BITS = 59                                                           # |a'| <= 2^59: emu_scale_bits(128, 16) = 117, abits = 59
BIAS = 60                                                               # a'' = a' + 2^60 >= 0


def split_constants(p):
    """(c_0 .. c_7, k0, m): c_k = 2^(8k) mod p, k0 = (-2^60) mod p, m = ceil(2^31 / p)."""
    return [pow(2, 8 * k, p) for k in range(8)], (-(2 ** BIAS)) % p, -((-2 ** 31) // p)


def reachable_x(p):
    """the largest x = k0 + sum_k d_k c_k over the bytes d_k of a'' in [2^60 - 2^59, 2^60 + 2^59] (d_7 <= 0x18)."""
    c, k0, _m = split_constants(p)
    return k0 + 255 * sum(c[:7]) + 0x18 * c[7]


def words(a):
    """(lo, hi) of a'' = a' + 2^60 = 2^32 hi + lo for an fp64 array of integers, in the kernel's fp64 steps (h 2^32 and the
    difference are exact, so the fma of the kernel and the two operations here agree)."""
    a = np.asarray(a, np.float64)
    h = np.floor(a * 2.0 ** -32)
    lo = a - h * 2.0 ** 32
    assert ((lo >= 0) & (lo < 2.0 ** 32)).all() and (np.abs(h) <= 2.0 ** 27).all()
    return lo.astype(np.uint64), (h.astype(np.int64) + (1 << 28)).astype(np.uint64)


def reduce_x(x, p):
    """the byte the kernel keeps of x (uint64 array, x = a' mod p): q = (y m) >> 32 with y = 2 x + p, then the low byte of
    q (256 - p) + x = r + 256 q, r = x - p q.  Returns (byte as int8, r, q, y)."""
    _c, _k0, m = split_constants(p)
    y = 2 * x + p
    q = (y * np.uint64(m)) >> np.uint64(32)
    r = x.astype(np.int64) - q.astype(np.int64) * p
    byte = ((q & np.uint64(0xFFFFFF)) * np.uint64(256 - p) + x) & np.uint64(0xFF)
    return byte.astype(np.uint8).view(np.int8), r, q, y


def plane_bytes(lo, hi, p):
    if p == 256:
        return (lo & np.uint64(0xFF)).astype(np.uint8).view(np.int8)
    c, k0, _m = split_constants(p)
    x = np.full(lo.shape, k0, np.uint64)
    for k in range(4):
        x += ((lo >> np.uint64(8 * k)) & np.uint64(0xFF)) * np.uint64(c[k])
        x += ((hi >> np.uint64(8 * k)) & np.uint64(0xFF)) * np.uint64(c[4 + k])
    assert int(x.max(initial=0)) <= reachable_x(p)
    return reduce_x(x, p)[0]


def residues_model(a, L):
    """[L, ...] int8: the kernel's arithmetic on the fp64 integers a."""
    lo, hi = words(a)
    return np.stack([plane_bytes(lo, hi, p) for p in MODULI[:L]])


def residues_exact(a, L):
    """[L, ...] int8 from exact integers (int64 array): the balanced residue a mod p (numpy's % on int64 is Python's: the result has
    the sign of p), 128 mod 256 as -128."""
    a = np.asarray(a, np.int64)
    out = []
    for p in MODULI[:L]:
        r = a % p
        half = 127 if p == 256 else (p - 1) // 2
        out.append(np.where(r > half, r - p, r).astype(np.int8))
    return np.stack(out)
