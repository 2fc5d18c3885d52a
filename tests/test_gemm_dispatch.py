"""Every launch form of the fp64 GEMM (csrc/gemm.hip, gemm_tile.h), one at a time and exact.

The cases are integer-valued with power-of-two alpha and beta (tests/_gemm_exact.py): the kernel's result equals the integer reference bit
for bit, tiles a launch must leave alone still hold C0, the sentinel around every window is intact, operands are unchanged, and whatever
a launch promises not to read holds NaN.  Each case names the launch it is meant to take -- read off launch_gemm_nt -- and asserts that
gpx_dev_gemm_nt_ex reports it: when a threshold moves, the assertion fails and the shape has to be picked again.  The five roundoff cases
at the end are the only comparisons with a tolerance."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from conftest import torch

import _gemm_exact as gx
import _trap_model as tm
from skgpuppy_amd import _gpx

pytestmark = pytest.mark.gpu

V = _gpx.GEMM_VARIANTS
NONE, A_UPPER, A_LOWER, B_LOWER, B_UPPER = (_gpx.GEMM_TRI_NONE, _gpx.GEMM_TRI_A_UPPER, _gpx.GEMM_TRI_A_LOWER, _gpx.GEMM_TRI_B_LOWER,
                                            _gpx.GEMM_TRI_B_UPPER)
lib = _gpx.lib


def _up(buf):
    return torch.from_numpy(np.ascontiguousarray(buf)).cuda()


def _down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _at(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + 8 * offset)


def _seed(*v):
    return sum((i + 1) * 7919 * int(x) for i, x in enumerate(v)) % (2 ** 31)


# ---- gpx_dev_gemm_nt_ex: one table -----------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "M N K lower ktrim tri small variant")


def C(M, N, K, variant, lower=0, ktrim=0, tri=NONE, small=0):
    return Case(M, N, K, lower, ktrim, tri, small, variant)


CASES = [
    # plain 128 x 128, >= 192 tiles: 13 x 15 tiles (a ragged last group of the 8-row walk, 195 = 3 mod 8 workgroups), 3, 1 and 2 stages
    C(1664, 1920, 48, "128X128"), C(1664, 1920, 16, "128X128"), C(1664, 1920, 32, "128X128"),
    # plain 64 x 64
    C(384, 256, 128, "64X64"), C(2048, 1536, 128, "64X64", small=1),
    # one column tile
    C(12288, 128, 16, "64X128"), C(256, 128, 48, "32X128"),
    # lower-only
    C(2560, 2560, 32, "LOWER_128X128", lower=1),        # 210 tiles
    C(2432, 2432, 32, "LOWER_64X64", lower=1),          # 190 tiles of 128: 38 tile rows of 64, a ragged last group
    C(1024, 1024, 528, "LOWER_32X32", lower=1), C(1024, 1024, 496, "LOWER_64X64", lower=1),
    # trapezoids (the shapes of test_gpu_parity.py::test_gemm_nt_trapezoid)
    C(256, 384, 48, "LOWER_64X64", lower=1), C(384, 1408, 64, "LOWER_64X64", lower=1), C(2048, 3072, 32, "LOWER_128X128", lower=1),
    C(512, 1024, 640, "LOWER_32X32", lower=1),
    # ktrim, lower-only: both operands upper triangular, K = M = N
    C(384, 384, 384, "LOWER_64X64", lower=1, ktrim=1), C(2560, 2560, 2560, "LOWER_128X128", lower=1, ktrim=1),
    # ktrim, rectangular: A upper triangular, its diagonal ktrim - 1 columns to the left
    C(384, 256, 512, "64X64", ktrim=1), C(384, 256, 512, "64X64", ktrim=17), C(384, 256, 512, "64X64", ktrim=145),
    C(2048, 1536, 2048, "128X128", ktrim=1),
    # triangular B (K = N), lower and upper
    C(256, 384, 384, "TRIB_SMALL_64X64", tri=B_LOWER), C(256, 384, 384, "TRIB_SMALL_64X64", tri=B_UPPER),
    C(256, 128, 128, "TRIB_SMALL_32X128", tri=B_LOWER), C(12288, 128, 128, "TRIB_SMALL_64X128", tri=B_UPPER),
    C(3072, 1024, 1024, "TRIB_FINE", tri=B_LOWER), C(3072, 1024, 1024, "TRIB_FINE", tri=B_UPPER),
    C(11520, 640, 640, "TRIB_LONGEST_FIRST", tri=B_LOWER), C(11520, 640, 640, "TRIB_LONGEST_FIRST", tri=B_UPPER),   # an odd column count
    C(14336, 1024, 1024, "TRIB_PAIRED", tri=B_LOWER), C(14336, 1024, 1024, "TRIB_PAIRED", tri=B_UPPER),
    # triangular A (K = M) through the plain launches
    C(384, 256, 384, "64X64", tri=A_UPPER), C(384, 256, 384, "64X64", tri=A_LOWER),
]


def _case_id(c):
    s = "%dx%dx%d" % (c.M, c.N, c.K)
    s += "-lower" if c.lower else ""
    s += "-ktrim%d" % c.ktrim if c.ktrim else ""
    s += "-tri%d" % c.tri if c.tri else ""
    s += "-small" if c.small else ""
    return s + "-" + c.variant


def _shape_operands(c, A, B):
    """(A, B) as the reference multiplies them and as the kernel gets them, for the case's triangular declarations"""
    za, zb = np.zeros(A.shape, bool), np.zeros(B.shape, bool)
    if c.ktrim and c.lower:
        za, zb = gx.zero_part(c.M, c.K, "upper"), gx.zero_part(c.N, c.K, "upper")
    elif c.ktrim:
        za = gx.zero_part(c.M, c.K, "upper", shift=c.ktrim - 1)
    elif c.tri == A_UPPER:
        za = gx.zero_part(c.M, c.K, "upper")
    elif c.tri == A_LOWER:
        za = gx.zero_part(c.M, c.K, "lower")
    elif c.tri == B_LOWER:
        zb = gx.zero_part(c.N, c.K, "lower")
    elif c.tri == B_UPPER:
        zb = gx.zero_part(c.N, c.K, "upper")
    return gx.shaped(A, za), gx.shaped(B, zb)


def _launch_ex(da, wa, db, wb, dc, wc, c, alpha, beta):
    v = ctypes.c_int(-1)
    st = lib.gpx_dev_gemm_nt_ex(_at(da, wa.offset), wa.ld, _at(db, wb.offset), wb.ld, _at(dc, wc.offset), wc.ld, c.M, c.N, c.K, alpha, beta,
                                c.lower, c.ktrim, c.tri, c.small, ctypes.byref(v), None)
    return st, v.value


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_launch_form_exact(c):
    rng = np.random.RandomState(_seed(*c[:7]))
    A, B, C0 = gx.operands(rng, c.M, c.N, c.K)
    alpha, beta = gx.scalars(rng)                              # beta != 0: a tile computed twice must show
    (Aref, Adev), (Bref, Bdev) = _shape_operands(c, A, B)
    wa, wb, wc = gx.windows(c.M, c.N, c.K)
    want = gx.reference(Aref, Bref, C0, alpha, beta)
    written = gx.mask_lower(c.M, c.N) if c.lower else gx.mask_plain(c.M, c.N)
    abuf, bbuf = wa.new(Adev), wb.new(Bdev)
    da, db, dc = _up(abuf), _up(bbuf), _up(wc.new(C0))
    st, variant = _launch_ex(da, wa, db, wb, dc, wc, c, alpha, beta)
    _gpx.check(st, "gpx_dev_gemm_nt_ex")
    got = _down(dc)
    print("alpha %g beta %g variant 0x%x (expected %s = 0x%x)" % (alpha, beta, variant, c.variant, V[c.variant]))
    gx.check(wc.view(got), want, C0, written, guards=[(got, wc, "C")])
    assert gx.same_bits(_down(da), abuf) and gx.same_bits(_down(db), bbuf)
    assert variant == V[c.variant]


def test_poison_reaches_the_cases_that_promise_not_to_read():
    """every case with a triangular operand of more than one 128-tile per side holds NaN where the launch must not read"""
    for c in CASES:
        if not (c.ktrim or c.tri):
            continue
        (_, Adev), (_, Bdev) = _shape_operands(c, np.ones((c.M, c.K)), np.ones((c.N, c.K)))
        tri_side = c.N if c.tri in (B_LOWER, B_UPPER) else c.M
        if tri_side > 128 and c.ktrim != 145:                  # (ktrim = 145: the shifted diagonal leaves no whole tile in 384 rows)
            assert np.isnan(Adev).any() or np.isnan(Bdev).any(), _case_id(c)


@pytest.mark.parametrize("M,variant", [(256, "32X128"), (12288, "64X128")])
def test_in_place_leaf(M, variant):
    """C == A with one column tile (K = N = 128): the in-place TRSM leaf.  The reference is taken before the call."""
    rng = np.random.RandomState(M)
    A, B, _ = gx.operands(rng, M, 128, 128)
    alpha, beta = gx.scalars(rng)
    wa, wb = gx.Window(M, 128, 144, 6), gx.Window(128, 128, 130, 10)
    want = gx.reference(A, B, A, alpha, beta)
    bbuf = wb.new(B)
    da, db = _up(wa.new(A)), _up(bbuf)
    c = Case(M, 128, 128, 0, 0, NONE, 0, variant)
    st, got_variant = _launch_ex(da, wa, db, wb, da, wa, c, alpha, beta)
    _gpx.check(st, "gpx_dev_gemm_nt_ex")
    got = _down(da)
    gx.check(wa.view(got), want, A, gx.mask_plain(M, 128), guards=[(got, wa, "A = C")])
    assert gx.same_bits(_down(db), bbuf)
    assert got_variant == V[variant]


def test_lower_only_65_tile_rows_on_the_device():
    """8320 x 8320, K = 16 (one stage): 2145 tiles of the grouped triangular walk, compared on the device.  The fp64 product of the same
    integers is exact for the reason the kernel's is; 128 of its rows are compared with the int64 product."""
    M = N = 8320
    K = 16
    rng = np.random.RandomState(8320)
    A, B = gx.integers(rng, (M, K), 8), gx.integers(rng, (N, K), 8)
    alpha, beta = -0.5, 2.0
    assert (abs(beta / alpha) * 1024 + K * 64) * 16 < gx.EXACT
    wa, wb, wc = gx.windows(M, N, K)
    abuf, bbuf = wa.new(A), wb.new(B)
    da, db = _up(abuf), _up(bbuf)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(8320)
    buf = torch.full((wc.size,), gx.SENTINEL, dtype=torch.float64, device="cuda")
    view = buf[wc.offset:wc.offset + M * wc.ld].view(M, wc.ld)[:, :N]
    view.copy_(torch.randint(-1024, 1025, (M, N), device="cuda", generator=gen).double())
    C0 = view.clone()
    P = torch.matmul(_up(A), _up(B).T)
    rows = np.unique(np.linspace(0, M - 1, 128).astype(int))
    np.testing.assert_array_equal(P[torch.as_tensor(rows, device="cuda")].cpu().numpy(), gx.exact_product(A[rows], B))
    want = alpha * P + beta * C0
    del P
    c = Case(M, N, K, 1, 0, NONE, 0, "LOWER_128X128")
    st, variant = _launch_ex(da, wa, db, wb, buf, wc, c, alpha, beta)
    _gpx.check(st, "gpx_dev_gemm_nt_ex")
    torch.cuda.synchronize()
    r = torch.arange(M, device="cuda")[:, None]
    col = torch.arange(N, device="cuda")[None, :]
    tr, tc = r // 128, col // 128
    is_want, is_c0 = view == want, view == C0
    must_write = (tc < tr) | ((tc == tr) & (col <= r))
    ok = torch.where(must_write, is_want, torch.where(tc > tr, is_c0, is_want | is_c0))
    bad = int((~ok).sum())
    assert bad == 0, "%d entries wrong, first at %s" % (bad, (~ok).nonzero()[0].tolist())
    view.fill_(gx.SENTINEL)
    assert bool((buf == gx.SENTINEL).all()), "the sentinel around C"
    assert gx.same_bits(_down(da), abuf) and gx.same_bits(_down(db), bbuf)
    assert variant == V["LOWER_128X128"]


# ---- the row-reduction epilogue --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(12288, 256), (8192, 384)], ids=["paired", "longest-first"])
def test_tri_reduce(M, N):
    rng = np.random.RandomState(M + N)
    A, B, C0 = gx.operands(rng, M, N, N)
    y = gx.integers(rng, (N,), 8)
    alpha = gx.scalars(rng)[0]
    Bref, Bdev = gx.shaped(B, gx.zero_part(N, N, "lower"))
    assert np.isnan(Bdev).any()
    wa, wb, wc = gx.windows(M, N, N)
    want = gx.reference(A, Bref, C0, alpha, 0.0)
    slot0, nslots = 3, 3 + N // 64 + 2
    # z multiples of 1/4 with |z| <= 2^17: the 64-term sums of z^2 and z y are exact in any order
    Z4 = (want * 4.0).astype(np.int64)
    assert np.array_equal(Z4 / 4.0, want) and np.abs(want).max() <= 2.0 ** 17
    Z4 = Z4.reshape(M, N // 64, 64)
    p2_want = np.full((M, nslots), gx.SENTINEL)
    py_want = np.full((M, nslots), gx.SENTINEL)
    p2_want[:, slot0:slot0 + N // 64] = (Z4 * Z4).sum(2) / 16.0
    py_want[:, slot0:slot0 + N // 64] = (Z4 * y.astype(np.int64).reshape(1, N // 64, 64)).sum(2) / 4.0
    abuf, bbuf = wa.new(A), wb.new(Bdev)
    da, db, dc, dy = _up(abuf), _up(bbuf), _up(wc.new(C0)), _up(y)
    p2, py = _up(np.full((M, nslots), gx.SENTINEL)), _up(np.full((M, nslots), gx.SENTINEL))
    st = lib.gpx_dev_gemm_nt_tri_reduce(_at(da, wa.offset), wa.ld, _at(db, wb.offset), wb.ld, _at(dc, wc.offset), wc.ld, M, N, alpha, _at(dy),
                                        _at(p2), _at(py), slot0, nslots, None)
    _gpx.check(st, "gpx_dev_gemm_nt_tri_reduce")
    got = _down(dc)
    gx.check(wc.view(got), want, C0, gx.mask_plain(M, N), guards=[(got, wc, "C")])
    np.testing.assert_array_equal(_down(p2), p2_want)          # the written slots and the sentinel in all others
    np.testing.assert_array_equal(_down(py), py_want)
    assert gx.same_bits(_down(da), abuf) and gx.same_bits(_down(db), bbuf)


def test_tri_reduce_refuses_fewer_than_192_tiles():
    M = N = 256
    rng = np.random.RandomState(1)
    A, B, C0 = gx.operands(rng, M, N, N)
    nslots = N // 64
    da, db, dc, dy = _up(A), _up(np.tril(B)), _up(C0), _up(np.ones(N))
    p2, py = _up(np.full((M, nslots), gx.SENTINEL)), _up(np.full((M, nslots), gx.SENTINEL))
    st = lib.gpx_dev_gemm_nt_tri_reduce(_at(da), N, _at(db), N, _at(dc), N, M, N, 1.0, _at(dy), _at(p2), _at(py), 0, nslots, None)
    assert st == _gpx.GPX_ERR_BAD_ARG
    # slots that would not fit are refused before the launcher sees them
    st2 = lib.gpx_dev_gemm_nt_tri_reduce(_at(da), N, _at(db), N, _at(dc), N, M, N, 1.0, _at(dy), _at(p2), _at(py), 1, nslots, None)
    assert st2 == _gpx.GPX_ERR_BAD_ARG
    np.testing.assert_array_equal(_down(dc), C0)
    assert (_down(p2) == gx.SENTINEL).all() and (_down(py) == gx.SENTINEL).all()


# ---- the batched launch: the three products of the square inverses' recursive doubling (tsolve.hip, invert_squares_into) ---------------------
@pytest.mark.parametrize("batch", [1, 6, 9])
@pytest.mark.parametrize("nq", [1, 3])
@pytest.mark.parametrize("h", [64, 128, 256])
def test_batched_products_of_the_square_inverse(h, nq, batch):
    """Squares of side S = 2 h nq hold nq pairs of h x h diagonal blocks each, as the caller's 1024-squares do: problem (p, q) works on
    the blocks at p S^2 + q 2 h (S + 1) of pl / pz and on tt[p][q] (dense h x h).  Each problem is compared on its own, everything else
    in the three buffers must stay as it was: the rotation of the tile coordinates with the problem index must not mix problems."""
    S = 2 * h * nq
    nsq = (batch + nq - 1) // nq
    rng = np.random.RandomState(_seed(h, nq, batch))
    sp, sq = S * S, 2 * h * (S + 1)
    tsp, tsq = nq * h * h, h * h

    def square_view(buf, first, p, q):   # the h x h block of problem (p, q) in a buffer of squares; first = offset of problem (0, 0)'s
        o = first + p * sp + q * sq
        return np.lib.stride_tricks.as_strided(buf[o:], shape=(h, h), strides=(8 * S, 8))

    def tt_view(buf, p, q):
        o = p * tsp + q * tsq
        return buf[o:o + h * h].reshape(h, h)

    def fill(view, zero=None, lim=8):
        X = gx.integers(rng, (h, h), lim)
        ref, dev = gx.shaped(X, zero) if zero is not None else (X, X)
        view[...] = dev
        return ref

    problems = [(z // nq, z % nq) for z in range(nsq * nq)]
    up, lo = gx.zero_part(h, h, "upper"), gx.zero_part(h, h, "lower")
    # (A operand: first offset, zero part, tri), (B operand), (C) per product; offsets inside pl / pz as in the caller
    products = [
        dict(name="T^T = Z11 L21^T", A=("pz", 0, up), B=("pl", h * S, None), C=("tt", 0), tri=A_UPPER),
        dict(name="inv21 = -inv22 T", A=("pl", h * S + h, lo), B=("tt", 0, None), C=("pl", h * S), tri=A_LOWER),
        dict(name="Z12 = -T^T inv22^T", A=("tt", 0, None), B=("pl", h * S + h, lo), C=("pz", h), tri=B_LOWER),
    ]
    for prod in products:
        host = dict(pl=np.full(nsq * sp, gx.SENTINEL), pz=np.full(nsq * sp, gx.SENTINEL), tt=np.full(nsq * tsp, gx.SENTINEL))

        def view(which, first, p, q):
            return tt_view(host[which], p, q) if which == "tt" else square_view(host[which], first, p, q)

        alpha, beta = gx.scalars(rng)
        refs = []
        for p, q in problems:
            Ar = fill(view(prod["A"][0], prod["A"][1], p, q), prod["A"][2])
            Br = fill(view(prod["B"][0], prod["B"][1], p, q), prod["B"][2])
            C0 = fill(view(prod["C"][0], prod["C"][1], p, q), lim=1024)
            refs.append((Ar, Br, C0))
        if h > 128 and prod["tri"]:
            assert np.isnan(host["pl"]).any() or np.isnan(host["pz"]).any()
        expect = dict((k, v.copy()) for k, v in host.items())
        for z, (p, q) in enumerate(problems):
            if z < batch:
                Ar, Br, C0 = refs[z]
                cname, cfirst = prod["C"]
                dst = tt_view(expect[cname], p, q) if cname == "tt" else square_view(expect[cname], cfirst, p, q)
                dst[...] = gx.reference(Ar, Br, C0, alpha, beta)
        dev = dict((k, _up(v)) for k, v in host.items())

        def arg(which, first):
            return (_at(dev[which], first), h, tsp, tsq) if which == "tt" else (_at(dev[which], first), S, sp, sq)

        a, b, c_ = arg(*prod["A"][:2]), arg(*prod["B"][:2]), arg(*prod["C"])
        st = lib.gpx_dev_gemm_nt_batched(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c_[0], c_[1], c_[2], c_[3], nq, prod["tri"], h, h, h,
                                         alpha, beta, batch, None)
        _gpx.check(st, "gpx_dev_gemm_nt_batched")
        for k in host:
            got = _down(dev[k])
            cname = prod["C"][0]
            if k == cname:
                for z, (p, q) in enumerate(problems):     # problem by problem first: the message names the one that is wrong
                    g = tt_view(got, p, q) if k == "tt" else square_view(got, prod["C"][1], p, q)
                    e = tt_view(expect[k], p, q) if k == "tt" else square_view(expect[k], prod["C"][1], p, q)
                    assert not np.isnan(g).any(), (prod["name"], z)
                    np.testing.assert_array_equal(g, e, err_msg="%s: problem %d = (%d, %d) of %d" % (prod["name"], z, p, q, batch))
            np.testing.assert_array_equal(got, expect[k], err_msg="%s: buffer %s outside the problems' results" % (prod["name"], k))


# ---- split-K SYRK --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_w2", [False, True], ids=["W", "W-W2"])
@pytest.mark.parametrize("nchunks", [1, 8])
@pytest.mark.parametrize("kchunk", [16, 272])
def test_syrk_splitk(kchunk, nchunks, with_w2):
    m, K = 384, kchunk * nchunks
    rng = np.random.RandomState(_seed(kchunk, nchunks, with_w2))
    W, W2, _ = gx.operands(rng, m, m, K)
    if not with_w2:
        W2 = W
    C0 = gx.integers(rng, (nchunks * m, m), 1024)
    alpha = gx.scalars(rng)[0]
    ww, ww2, wp = gx.Window(m, K, K + 16, 6), gx.Window(m, K, K + 16, 10), gx.Window(nchunks * m, m, m, 4)
    wbuf, w2buf = ww.new(W), ww2.new(W2)
    dw, dw2, dp = _up(wbuf), _up(w2buf), _up(wp.new(C0))
    st = lib.gpx_dev_syrk_splitk(_at(dw, ww.offset), ww.ld, _at(dw2, ww2.offset) if with_w2 else None, _at(dp, wp.offset), m, kchunk, nchunks,
                                 alpha, None)
    _gpx.check(st, "gpx_dev_syrk_splitk")
    got = _down(dp)
    want = np.concatenate([gx.reference(W[:, c * kchunk:(c + 1) * kchunk], W2[:, c * kchunk:(c + 1) * kchunk], C0[c * m:(c + 1) * m], alpha, 0.0)
                           for c in range(nchunks)])
    parts = wp.view(got)
    gx.check(parts, want, C0, gx.mask_splitk(m, nchunks), guards=[(got, wp, "parts")])
    il = np.tril_indices(m)
    whole = gx.reference(W, W2, C0[:m], alpha, 0.0)
    np.testing.assert_array_equal(sum(parts[c * m:(c + 1) * m][il] for c in range(nchunks)), whole[il])
    assert gx.same_bits(_down(dw), wbuf) and gx.same_bits(_down(dw2), w2buf)


# ---- the trapezoid launch with its counters --------------------------------------------------------------------------------------------------
def _trap_setup(M, off_cols, K, tri_cols=0):
    """tri_cols in (0, M): the rows of B behind the triangle's last column hold NaN -- the launch must not read them"""
    rng = np.random.RandomState(_seed(M, off_cols, K))
    N = off_cols + M
    A, B, C0 = gx.operands(rng, M, N, K)
    alpha, beta = gx.scalars(rng)
    wa, wb, wc = gx.windows(M, N, K)
    Bdev = B.copy()
    if 0 < tri_cols < M:
        Bdev[off_cols + tri_cols:] = np.nan
    return dict(N=N, A=A, B=B, C0=C0, alpha=alpha, beta=beta, wa=wa, wb=wb, wc=wc, abuf=wa.new(A), bbuf=wb.new(Bdev))


def _trap_launch(s, M, off_cols, K, count, tri_cols=None):
    """tri_cols None: gpx_dev_syrk_trap, else gpx_dev_syrk_trap_cols"""
    da, db, dc = _up(s["abuf"]), _up(s["bbuf"]), _up(s["wc"].new(s["C0"]))
    args = (_at(da, s["wa"].offset), s["wa"].ld, _at(db, s["wb"].offset), s["wb"].ld, _at(dc, s["wc"].offset), s["wc"].ld, M, off_cols, K, s["alpha"],
            s["beta"])
    cnt = _at(count) if count is not None else None
    st = lib.gpx_dev_syrk_trap(*args, cnt, None) if tri_cols is None else lib.gpx_dev_syrk_trap_cols(*args, tri_cols, cnt, None)
    return st, da, db, dc


@pytest.mark.parametrize("M,off_cols,K", [(4096, 1024, 128), (4480, 1024, 48)])   # (the second: 35 tile rows, a ragged last group)
def test_syrk_trap(M, off_cols, K):
    s = _trap_setup(M, off_cols, K)
    want = gx.reference(s["A"], s["B"], s["C0"], s["alpha"], s["beta"])
    written = gx.mask_trapezoid(M, off_cols)
    off = off_cols // 128
    for with_count in (True, False):
        count = _up(np.array([0] * off + [7] * 4, dtype=np.int32)) if with_count else None
        st, da, db, dc = _trap_launch(s, M, off_cols, K, count)
        _gpx.check(st, "gpx_dev_syrk_trap")
        got = _down(dc)
        gx.check(s["wc"].view(got), want, s["C0"], written, guards=[(got, s["wc"], "C")])
        assert gx.same_bits(_down(da), s["abuf"]) and gx.same_bits(_down(db), s["bbuf"])
        if with_count:
            assert _down(count).tolist() == [M // 128] * off + [7] * 4


def test_syrk_trap_too_small_is_refused():
    M, off_cols, K = 2048, 1024, 128
    s = _trap_setup(M, off_cols, K)
    count = _up(np.array([0] * 8 + [7] * 4, dtype=np.int32))
    st, _da, _db, dc = _trap_launch(s, M, off_cols, K, count)
    assert st == _gpx.GPX_ERR_STATE
    assert gx.same_bits(_down(dc), s["wc"].new(s["C0"]))
    assert _down(count).tolist() == [0] * 8 + [7] * 4


def _trap_case_id(c):
    return "off%d-nt%d-wt%d" % c


@pytest.mark.parametrize("off,nt,wt", tm.DEVICE_CASES, ids=[_trap_case_id(c) for c in tm.DEVICE_CASES])
def test_syrk_trap_cols(off, nt, wt):
    """the column-limited launch (gemm_nt_f64_trap_signal_kernel<true>) alone, at the smallest shapes the launcher accepts: tile row r
    holds off + min(r + 1, wt) tiles, everything right of that keeps C0, the rows of B the launch has no tile for are NaN"""
    M, off_cols, tri_cols, K = nt * 128, off * 128, wt * 128, 48
    assert tm.accepts(off, nt, wt) and tm.shape(off, nt, wt)[0]
    s = _trap_setup(M, off_cols, K, tri_cols)
    assert np.isnan(s["bbuf"]).any()
    want = gx.reference(s["A"], s["B"], s["C0"], s["alpha"], s["beta"])
    written = gx.mask_trapezoid(M, off_cols, tri_cols)
    assert ((written != gx.UNTOUCHED) == tm.mask(off, nt, wt)).all()
    for with_count in (True, False):
        count = _up(np.array([0] * off + [7] * 4, dtype=np.int32)) if with_count else None
        st, da, db, dc = _trap_launch(s, M, off_cols, K, count, tri_cols)
        assert st == 0, "the launcher refuses a shape the model accepts: %d, %s" % (st, _gpx.last_error())
        got = _down(dc)
        gx.check(s["wc"].view(got), want, s["C0"], written, guards=[(got, s["wc"], "C")])
        assert gx.same_bits(_down(da), s["abuf"]) and gx.same_bits(_down(db), s["bbuf"])
        if with_count:
            assert _down(count).tolist() == [nt] * off + [7] * 4


@pytest.mark.parametrize("off,nt,wt", tm.REFUSED_CASES, ids=[_trap_case_id(c) for c in tm.REFUSED_CASES])
def test_syrk_trap_cols_one_tile_row_too_small_is_refused(off, nt, wt):
    """one tile row fewer than the smallest shape the rule accepts with this width: GPX_ERR_STATE, as the model decides, and nothing is touched"""
    M, off_cols, tri_cols, K = nt * 128, off * 128, wt * 128, 48
    assert not tm.accepts(off, nt, wt) and tm.accepts(off, nt + 1, wt)
    s = _trap_setup(M, off_cols, K, tri_cols)
    count = _up(np.array([0] * off + [7] * 4, dtype=np.int32))
    st, da, db, dc = _trap_launch(s, M, off_cols, K, count, tri_cols)
    assert st == _gpx.GPX_ERR_STATE
    assert gx.same_bits(_down(dc), s["wc"].new(s["C0"]))
    assert gx.same_bits(_down(da), s["abuf"]) and gx.same_bits(_down(db), s["bbuf"])
    assert _down(count).tolist() == [0] * off + [7] * 4


def test_syrk_trap_cols_without_a_limit_is_syrk_trap():
    """tri_cols = 0 and tri_cols = M: the bytes of gpx_dev_syrk_trap, counters included (10 tile rows, one full column: the smallest
    shape the rule accepts without a limit)"""
    off, nt, K = 1, 10, 48
    M, off_cols = nt * 128, off * 128
    assert tm.accepts(off, nt, nt) and not tm.accepts(off, nt - 1, nt - 1)
    s = _trap_setup(M, off_cols, K)
    out = []
    for tri_cols in (None, 0, M):
        count = _up(np.array([0] * off + [7] * 4, dtype=np.int32))
        st, _da, _db, dc = _trap_launch(s, M, off_cols, K, count, tri_cols)
        _gpx.check(st, "gpx_dev_syrk_trap_cols")
        out.append((_down(dc), _down(count).tolist()))
    gx.check(s["wc"].view(out[0][0]), gx.reference(s["A"], s["B"], s["C0"], s["alpha"], s["beta"]), s["C0"], gx.mask_trapezoid(M, off_cols),
             guards=[(out[0][0], s["wc"], "C")])
    for got, counters in out[1:]:
        assert gx.same_bits(got, out[0][0]) and counters == out[0][1] == [nt] * off + [7] * 4


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_c_untouched():
    M = N = K = 256
    rng = np.random.RandomState(3)
    A, B, C0 = gx.operands(rng, M, N, K)
    wa, wb, wc = gx.Window(M, K, K + 16, 6), gx.Window(N, K, K + 2, 10), gx.Window(M, N, N + 3, 4)
    cbuf = wc.new(C0)
    da, db, dc = _up(wa.new(A)), _up(wb.new(B)), _up(cbuf)

    def call(M=M, N=N, K=K, alpha=1.0, beta=1.0, lower=0, ktrim=0, tri=NONE, small=0, a_off=wa.offset, lda=wa.ld, c_is_a=False):
        v = ctypes.c_int(-1)
        cp, ldc = (_at(da, a_off), lda) if c_is_a else (_at(dc, wc.offset), wc.ld)
        st = lib.gpx_dev_gemm_nt_ex(_at(da, a_off), lda, _at(db, wb.offset), wb.ld, cp, ldc, M, N, K, alpha, beta, lower, ktrim, tri, small,
                                    ctypes.byref(v), None)
        return st, v.value

    refused = {
        "alpha = 0": dict(alpha=0.0),
        "odd lda": dict(lda=wa.ld + 1),
        "misaligned A": dict(a_off=wa.offset + 1),
        "tri with lower_only": dict(tri=B_LOWER, lower=1),
        "tri with ktrim": dict(tri=A_UPPER, ktrim=1),
        "tri B with K != N": dict(tri=B_LOWER, K=128),
        "tri A with K != M": dict(tri=A_UPPER, K=128),
        "ktrim shift no multiple of 16": dict(ktrim=2),
        "lower_only with N < M": dict(lower=1, N=128),
        "lower ktrim with K != M": dict(lower=1, ktrim=1, K=128),
        "internal paired value 4": dict(tri=4),
        "internal paired value 6": dict(tri=6),
        "unknown tri": dict(tri=7),
        "negative ktrim": dict(ktrim=-1),
        "M no multiple of 128": dict(M=192),
        "K no multiple of 16": dict(K=40),
        "C == A with N = 256": dict(c_is_a=True),
    }
    a0 = _down(da).copy()
    for name, kw in refused.items():
        st, variant = call(**kw)
        assert st == _gpx.GPX_ERR_BAD_ARG, name
        assert variant == V["NONE"], name
        assert _gpx.last_error(), name
    # the trapezoid's column limit: negative, no multiple of 128, beyond M (here M = 256 rows, no full columns: A, B and C as above)
    count = _up(np.array([7] * 4, dtype=np.int32))

    def trap(tri_cols, c=dc):
        return lib.gpx_dev_syrk_trap_cols(_at(da, wa.offset), wa.ld, _at(db, wb.offset), wb.ld, _at(c, wc.offset), wc.ld, M, 0, K, 1.0, 1.0, tri_cols,
                                          _at(count), None)

    for tri_cols in (-128, -1, 64, 129, 384):
        assert trap(tri_cols) == _gpx.GPX_ERR_BAD_ARG, tri_cols
        assert _gpx.last_error(), tri_cols
    assert gx.same_bits(_down(dc), cbuf) and gx.same_bits(_down(da), a0) and _down(count).tolist() == [7] * 4
    dc2 = _up(cbuf)                                             # the same call with a limit it can have goes through, on a copy of C
    assert trap(128, dc2) == 0
    gx.check(wc.view(_down(dc2)), gx.reference(A, B, C0, 1.0, 1.0), C0, gx.mask_trapezoid(M, 0, 128), guards=[(_down(dc2), wc, "C")])
    st, variant = call()                                       # and the same call without a defect goes through
    assert st == 0 and variant == V["64X64"]
    gx.check(wc.view(_down(dc)), gx.reference(A, B, C0, 1.0, 1.0), C0, gx.mask_plain(M, N), guards=[(_down(dc), wc, "C")])


def test_the_table_covers_every_launch_code():
    taken = set(c.variant for c in CASES) | {"NONE"}           # NONE: test_refusals_leave_c_untouched
    assert taken == set(V), sorted(set(V) ^ taken)


# ---- roundoff: one case per block tile ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,lower,variant", [(256, 128, 272, 0, "32X128"), (12288, 128, 272, 0, "64X128"), (384, 256, 272, 0, "64X64"),
                                                   (1024, 1024, 528, 1, "LOWER_32X32"),   # (this tile is taken for 512 <= K <= 2048 only)
                                                   (1664, 1920, 272, 0, "128X128")])
def test_roundoff_per_block_tile(M, N, K, lower, variant):
    """randn data, alpha = -0.75, beta = 1.25: |got - ref| <= (K + 4) 2^-53 (|alpha| |A| |B|^T + |beta| |C0|) on every entry, ref the
    numpy.longdouble product -- K fused multiply-adds, the roundings of beta / alpha, of its product with C and of the final scaling, one
    unit of slack.  Nothing measured enters the bound."""
    rng = np.random.RandomState(_seed(M, N, K))
    A, B, C0 = rng.randn(M, K), rng.randn(N, K), rng.randn(M, N)
    alpha, beta = -0.75, 1.25
    wa, wb, wc = gx.windows(M, N, K)
    da, db, dc = _up(wa.new(A)), _up(wb.new(B)), _up(wc.new(C0))
    st, got_variant = _launch_ex(da, wa, db, wb, dc, wc, Case(M, N, K, lower, 0, NONE, 0, variant), alpha, beta)
    _gpx.check(st, "gpx_dev_gemm_nt_ex")
    buf = _down(dc)
    wc.check_guard(buf, "C")
    got = wc.view(buf)
    ref = gx.longdouble_reference(A, B, C0, alpha, beta)
    bound = gx.roundoff_bound(A, B, C0, alpha, beta)
    w = gx.expand(gx.mask_lower(M, N) if lower else gx.mask_plain(M, N))
    r, col = np.arange(M)[:, None], np.arange(N)[None, :]
    must = (w == gx.WRITTEN) | ((w == gx.DIAGONAL) & (col <= r))
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    print("max |got - ref| / bound = %.3f over %d entries" % ((err[must] / bound[must]).max(), must.sum()))
    assert (err[must] <= bound[must]).all()
    np.testing.assert_array_equal(got[w == gx.UNTOUCHED], C0[w == gx.UNTOUCHED])
    above = (w == gx.DIAGONAL) & (col > r)
    assert ((err[above] <= bound[above]) | (got[above] == C0[above])).all()
    assert got_variant == V[variant]
