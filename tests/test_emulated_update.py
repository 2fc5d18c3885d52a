"""The emulated fp64 update of estimate_many (csrc/emu.hip, Ozaki scheme II on int8 matrix cores).

CPU: a Python-integer model of the whole scheme (split, residues, exact residue products, Garner digits, rescale) against exact
arithmetic, the bit budget for every K the kernel accepts, and the moduli.  GPU (-m gpu): the product against exact sums and
against the native fp64 kernel, its reproducibility across runs and row orders, and estimate_many with GPX_EMU_F64=1 against
GPX_EMU_F64=0 in fresh processes.
"""
import ctypes
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from _emu_model import MODULI, emulated_product, garner, scale_bits, split_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_moduli_pairwise_coprime():
    for i in range(16):
        for j in range(i):
            assert math.gcd(MODULI[i], MODULI[j]) == 1
    assert abs(sum(math.log2(p) for p in MODULI) - 125.2) < 0.05


def test_bit_budget_every_k():
    P = math.prod(MODULI)
    for L in range(2, 17):                                              # every count of moduli emu_moduli() accepts
        PL = math.prod(MODULI[:L])
        for K in range(128, 1 << 17, 128):
            s = scale_bits(K, L)
            assert K * Fraction(2) ** s < PL // 2 <= K * Fraction(2) ** (s + 1)   # largest such s (negative for few moduli and deep K)
            assert K * 128 * 128 < 2 ** 31                              # int32 accumulation of int8 residues is exact
    assert scale_bits(8192, 16) == 111 and (111 - 111 // 2, 111 // 2) == (56, 55)
    assert P.bit_length() == 126


def test_garner_roundtrip_extremes():
    rng = np.random.default_rng(1)
    P = math.prod(MODULI)
    for X in [0, 1, -1, P // 2 - 1, -(P // 2), 2 ** 100, -(2 ** 117) + 12345] + [int(v) for v in rng.integers(-2 ** 62, 2 ** 62, 50)]:
        assert garner([X % p for p in MODULI], 16) == X


def test_scheme_against_exact_arithmetic():
    rng = np.random.default_rng(7)
    K = 256
    A = (rng.standard_normal((6, K)) * np.exp2(rng.integers(-30, 30, (6, 1))) * np.exp2(-rng.uniform(0, 40, (6, K)))).tolist()
    B = (rng.standard_normal((5, K)) * np.exp2(rng.integers(-30, 30, (5, 1)))).tolist()
    A[3] = [0.0] * K                                                    # an all-zero (padding) row
    E = emulated_product(A, B)
    for i in range(6):
        for j in range(5):
            exact = sum(Fraction(a) * Fraction(b) for a, b in zip(A[i], B[j]))
            # truncation bound: each a'_ik is within 1/2 of a_ik 2^sig_i (likewise b), so the error is at most
            # sum_k (|a_ik| 2^-tau_j + |b_jk| 2^-sig_i) / 2 + 2^-(sig_i + tau_j) / 4
            bits = scale_bits(K, 16)                                    # the kernel's split (K = 256: 58 + 58)
            _, si = split_row(A[i], bits - bits // 2)
            _, tj = split_row(B[j], bits // 2)
            bound = sum(abs(Fraction(a)) / 2 ** tj + abs(Fraction(b)) / 2 ** si for a, b in zip(A[i], B[j])) / 2 + Fraction(K, 4) / 2 ** (si + tj)
            assert abs(E[i][j] - exact) <= bound
            if i == 3:
                assert E[i][j] == 0


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def _exact_entry(a, b, C0):
    """C0 - a.b exactly, as a Fraction (doubles are dyadic: one common denominator 2^2200)."""
    D = 2200
    s = 0
    for x, y in zip(a.tolist(), b.tolist()):
        nx, dx = x.as_integer_ratio()
        ny, dy = y.as_integer_ratio()
        s += nx * ny * ((1 << D) // (dx * dy))
    return Fraction(C0) - Fraction(s, 1 << D)


def _operands(rng, rows, cols, K):
    A = rng.standard_normal((rows, K)) * np.exp2(rng.integers(-30, 31, (rows, 1))) * np.exp2(-rng.uniform(0, 40, (rows, K)))
    B = rng.standard_normal((cols, K)) * np.exp2(rng.integers(-30, 31, (cols, 1)))
    C = rng.standard_normal((rows, cols)) * np.abs(A).max(1, keepdims=True) * np.abs(B).max(1)[None, :]
    return A, B, C


def _emu(A, B, C):
    from conftest import torch
    from skgpuppy_amd import _gpx
    a, b, c = (torch.as_tensor(np.ascontiguousarray(v)).cuda() for v in (A, B, C))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _gpx.check(_gpx.lib.gpx_emu_gemm_nt_sub(p(a), A.shape[1], p(b), B.shape[1], p(c), C.shape[1], A.shape[0], B.shape[0], A.shape[1]), "emu")
    return c.cpu().numpy()


def _native(A, B, C):
    from conftest import torch
    from skgpuppy_amd import _gpx
    a, b, c = (torch.as_tensor(np.ascontiguousarray(v)).cuda() for v in (A, B, C))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _gpx.check(_gpx.lib.gpx_dev_gemm_nt(p(a), A.shape[1], p(b), B.shape[1], p(c), C.shape[1], A.shape[0], B.shape[0], A.shape[1], -1.0, 1.0, 0,
                                        None), "gemm")
    torch.cuda.synchronize()
    return c.cpu().numpy()


@pytest.mark.gpu
def test_emulated_product_exact_sums_and_reproducible():
    rng = np.random.default_rng(3)
    rows, cols, K = 640, 384, 4096
    A, B, C = _operands(rng, rows, cols, K)
    A[5, 17] = np.nan
    A[9, 3] = np.inf
    B[11, 2] = -np.inf
    E = _emu(A, B, C)
    N = _native(A, B, C)
    # non-finite rows / columns of the operands give non-finite outputs exactly where the native kernel's are
    np.testing.assert_array_equal(~np.isfinite(E), ~np.isfinite(N))
    assert (~np.isfinite(E)).sum() == 2 * cols + rows - 2
    # against exact sums on a sample of entries: no worse than twice the native kernel's error (plus one rounding of the result)
    idx = [(i, j) for i, j in zip(rng.integers(0, rows, 64), rng.integers(0, cols, 64)) if i not in (5, 9) and j != 11]
    ee, en = [], []
    for i, j in idx:
        x = _exact_entry(A[i], B[j], C[i, j])
        ulp = math.ulp(float(x))
        ee.append(abs(Fraction(E[i, j]) - x) / ulp)
        en.append(abs(Fraction(N[i, j]) - x) / ulp)
    print("max error in ulps of the result: emulated %.3g, native %.3g" % (max(ee), max(en)))
    assert max(ee) <= 2 * max(en) + 1
    # bit-identical across runs, row permutations and row subsets of A
    np.testing.assert_array_equal(E, _emu(A, B, C))
    perm = rng.permutation(rows)
    np.testing.assert_array_equal(E[perm], _emu(A[perm], B, C[perm]))
    np.testing.assert_array_equal(E[100:300], _emu(A[100:300], B, C[100:300]))


@pytest.mark.gpu
def test_emulated_product_tiled_workspace_k32768():
    """K = 32768: at most 4096 rows / columns per workspace tile, so 4608 x 4352 runs as 2 x 2 tiles (ragged both ways), with the
    K = 32768 bit budget (alpha = 55, beta = 54)."""
    rng = np.random.default_rng(5)
    rows, cols, K = 4608, 4352, 32768
    A, B, C = _operands(rng, rows, cols, K)
    E = _emu(A, B, C)
    N = _native(A, B, C)
    assert np.isfinite(E).all()
    # one entry in each of the four tiles at least, plus random ones
    idx = [(0, 0), (4095, 4095), (4096, 0), (0, 4096), (4607, 4351), (4100, 4200)] + list(zip(rng.integers(0, rows, 14), rng.integers(0, cols, 14)))
    ee, en = [], []
    for i, j in idx:
        x = _exact_entry(A[i], B[j], C[i, j])
        ulp = math.ulp(float(x))
        ee.append(abs(Fraction(E[i, j]) - x) / ulp)
        en.append(abs(Fraction(N[i, j]) - x) / ulp)
    print("K=32768 max error in ulps of the result: emulated %.3g, native %.3g" % (max(ee), max(en)))
    assert max(ee) <= 2 * max(en) + 1
    # every entry: close to the native kernel (both within a few ulps of |a|.|b| of the exact sum)
    scale = np.abs(A).max(1, keepdims=True) * np.abs(B).max(1)[None, :] * np.sqrt(K)
    assert (np.abs(E - N) <= 1e-13 * scale + 4 * np.spacing(np.abs(N))).all()
    np.testing.assert_array_equal(E[4000:4300], _emu(A[4000:4300], B, C[4000:4300]))   # rows across the tile boundary


_E2E = r"""
import sys, numpy as np
sys.path[:0] = [%(root)r, %(pkg)r]
import torch
import skgpuppy_amd as sk
N, M, d = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
rng = np.random.default_rng(11)
x = rng.uniform(0.0, 10.0, (N, d))
t = np.sin(x).sum(1) + 0.1 * rng.standard_normal(N)
xs = rng.uniform(0.0, 10.0, (M, d))
xs[7, 0] = np.nan
theta = np.log(np.array([1.0, 0.01] + [0.5] * d))
gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta)
m, v = gp.estimate_many(xs)
np.save(sys.argv[4], np.stack([m, v]))
"""


def _run_e2e(tmp_path, N, M, d, emu):
    env = dict(os.environ, GPX_EMU_F64=str(emu))
    out = str(tmp_path / ("e2e_%d_%d.npy" % (N, emu)))
    code = _E2E % {"root": ROOT, "pkg": os.path.join(ROOT, "scikit-gpuppy_amd")}
    r = subprocess.run([sys.executable, "-c", code, str(N), str(M), str(d), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("N, M, d", [(16384, 16384, 8), (8200, 6000, 8), (65536, 3000, 16)])
def test_estimate_many_emulated_against_native(tmp_path, N, M, d):
    e = _run_e2e(tmp_path, N, M, d, 1)
    n = _run_e2e(tmp_path, N, M, d, 0)
    bad = ~np.isfinite(n)
    np.testing.assert_array_equal(~np.isfinite(e), bad)                 # (a NaN query: the same rows either way)
    ok = ~bad.any(0)
    assert not np.array_equal(e[:, ok], n[:, ok])                        # the emulated updates were taken
    dm = np.abs(e[0, ok] - n[0, ok]).max()
    dv = np.abs(e[1, ok] - n[1, ok]).max()
    print("N=%d M=%d: max|dmean| %.3g max|dvar| %.3g" % (N, M, dm, dv))
    assert dm <= 1e-11 * max(1.0, np.abs(n[0, ok]).max())
    assert dv <= 1e-11 * 1.0                                            # v = exp(theta[0]) = 1
