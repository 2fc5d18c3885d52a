"""emu_i8_gemm_kernel (csrc/emu.hip) through gpx_emu_i8_gemm / gpx_emu_i8_gemm_ld, byte for byte against the residues of the exact
integer product: every stage count the k loop distinguishes (one stage, an even count, an odd count that ends in buffer 0), one and
several tiles in either direction, one to sixteen moduli, the largest sums the kernel admits, the row strides of the residue image
(lda > K) and of a wider result (ldr > cols), a result that is not 16-byte aligned, and guard bytes around and between the rows of R.
The file does not know which MFMA shape the library was built with (EMU_MFMA_16): it must pass with both."""
import ctypes
import functools

import numpy as np
import pytest

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 211, 199, 197, 193, 191]
GUARD, PAD = 99, 256


@functools.lru_cache(maxsize=None)
def _planes():
    """uniform full-range bytes, -128 included, for the largest case; smaller cases take the leading part"""
    rng = np.random.default_rng(2020)
    A = rng.integers(-128, 128, (16, 512, 1024), dtype=np.int8)
    B = rng.integers(-128, 128, (16, 512, 1024), dtype=np.int8)
    A[:, :, 0] = -128
    B[:, ::2, 0] = -128
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def _stored(S, p):
    """the byte of the integer S: the balanced residue, 128 (mod 256) stored as -128"""
    r = S % p
    return np.where(r > (p - 1) // 2, r - p, r).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _want(rows, cols, K, l):
    A, B = _planes()
    # |sum| <= K 2^14 < 2^53: the fp64 product of the integer planes IS the integer product; a corner is recomputed in int64
    S = (A[l, :rows, :K].astype(np.float64) @ B[l, :cols, :K].astype(np.float64).T).astype(np.int64)
    np.testing.assert_array_equal(S[:8, :8], A[l, :8, :K].astype(np.int64) @ B[l, :8, :K].astype(np.int64).T)
    w = _stored(S, MODULI[l])
    w.setflags(write=False)
    return w


def _run(a_dev, lda, b_dev, rows, cols, K, L, ldr=None, roff=0):
    """launches on device planes a_dev [L][rows][lda], b_dev [L][cols][K]; R sits `PAD + roff` bytes into a guarded buffer.
    Returns R as [L, rows, cols] after checking every byte the kernel had no business writing."""
    from conftest import torch
    from skgpuppy_amd import _gpx
    ldr = cols if ldr is None else ldr
    n = L * rows * ldr
    buf = torch.full((PAD + roff + n + PAD,), GUARD, dtype=torch.int8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    r_ptr = buf.data_ptr() + PAD + roff
    if ldr == cols and roff == 0 and lda == K:
        rc = _gpx.lib.gpx_emu_i8_gemm(ctypes.c_void_p(a_dev.data_ptr()), ctypes.c_void_p(b_dev.data_ptr()), rows, cols, K, L, ctypes.c_void_p(r_ptr))
    else:
        rc = _gpx.lib.gpx_emu_i8_gemm_ld(ctypes.c_void_p(a_dev.data_ptr()), lda, ctypes.c_void_p(b_dev.data_ptr()), rows, cols, K, L,
                                         ctypes.c_void_p(r_ptr), ldr)
    _gpx.check(rc, "gpx_emu_i8_gemm")
    out = buf.cpu().numpy()
    assert (out[:PAD + roff] == GUARD).all() and (out[PAD + roff + n:] == GUARD).all(), "bytes around R were written"
    body = out[PAD + roff:PAD + roff + n].reshape(L, rows, ldr)
    assert (body[:, :, cols:] == GUARD).all(), "bytes between the rows of R were written"
    return body[:, :, :cols]


def _compare(got, rows, cols, K, L):
    for l in range(L):
        want = _want(rows, cols, K, l)
        bad = got[l] != want
        assert not bad.any(), (l, int(bad.sum()), np.argwhere(bad)[:5], got[l][bad][:5], want[bad][:5])


def _device_planes(rows, cols, K, L, lda=None):
    from conftest import torch
    A, B = _planes()
    lda = K if lda is None else lda
    a = torch.full((L, rows, lda), 77, dtype=torch.int8, device="cuda")     # (what lies beyond column K is never read into a sum)
    a[:, :, :K] = torch.as_tensor(A[:L, :rows, :K].copy()).cuda()
    b = torch.as_tensor(B[:L, :cols, :K].copy()).cuda()
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("L", [16, 1, 2, 15])
@pytest.mark.parametrize("K", [128, 256, 384, 1024])
@pytest.mark.parametrize("rows, cols", [(256, 256), (512, 256), (256, 512)])
def test_product_bytes(rows, cols, K, L):
    a, b = _device_planes(rows, cols, K, L)
    _compare(_run(a, K, b, rows, cols, K, L), rows, cols, K, L)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [128, 384])
def test_row_strides(K):
    """lda = K + 1024 (a product that reads the leading columns of a wider residue image) and ldr > cols, 16-byte aligned"""
    rows, cols, L, lda = 512, 512, 3, K + 1024
    a, b = _device_planes(rows, cols, K, L, lda)
    _compare(_run(a, lda, b, rows, cols, K, L, ldr=cols + 64), rows, cols, K, L)


@pytest.mark.gpu
@pytest.mark.parametrize("roff, pad", [(4, 4), (0, 4), (4, 0), (1, 3)])
def test_unaligned_result(roff, pad):
    rows, cols, K, L = 256, 512, 384, 3
    a, b = _device_planes(rows, cols, K, L)
    _compare(_run(a, K, b, rows, cols, K, L, ldr=cols + pad, roff=roff), rows, cols, K, L)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 16], ids=["first_two_moduli", "all_sixteen_with_the_last_two"])
@pytest.mark.parametrize("bval", [-128, 127])
def test_largest_sums(bval, L):
    """K = 130944 = 2^17 - 128, the largest the kernel admits (1023 stages: an odd count), every entry of A -128 and of B -128 or 127:
    the sums 2 145 386 496 and -2 128 625 664 are the largest |v| an accumulator can hold here.  Planes 14 and 15 are the last two moduli."""
    from conftest import torch
    rows = cols = 256
    K = 130944
    a = torch.full((L, rows, K), -128, dtype=torch.int8, device="cuda")
    b = torch.full((L, cols, K), bval, dtype=torch.int8, device="cuda")
    got = _run(a, K, b, rows, cols, K, L)
    S = np.int64(K) * -128 * bval
    assert S == (2145386496 if bval == -128 else -2128625664) and abs(int(S)) < 2 ** 31
    for l in range(L):
        want = _stored(np.full((rows, cols), S, np.int64), MODULI[l])
        bad = got[l] != want
        assert not bad.any(), (l, MODULI[l], int(bad.sum()), got[l][bad][:5], want[bad][:5])
