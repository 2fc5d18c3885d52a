"""Exact reference and comparison for the launch forms of the fp64 GEMM (csrc/gemm.hip); no GPU in here.

The faults of that code are discrete: a tile enumeration that visits a tile twice or not at all, a contraction range off by one 16-deep
stage at a triangular boundary, leading-dimension arithmetic.  On integer data with power-of-two alpha and beta every partial sum of
C = alpha A B^T + beta C is exact in fp64 in ANY order, so the kernel must reproduce an integer reference bit for bit and one dropped or
doubled stage shows as an integer-sized difference.  reference() asserts the exactness from the data it is given.

Operands live in windows of larger buffers (Window) filled with a sentinel; where a launch promises not to read (gpx_dev_gemm_nt_ex in
include/gpx.h) they hold NaN (shaped()); `written` masks say by 128 x 128 tiles what a launch must write and what it must leave alone."""
import numpy as np

TILE = 128
SENTINEL = 12345.678            # no multiple of 2^-4: nothing a launch computes here equals it
ALPHAS = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 0.25)
BETAS = ALPHAS + (0.0,)
UNTOUCHED, WRITTEN, DIAGONAL = 0, 1, 2   # DIAGONAL: a lower-only launch's diagonal tile -- the lower triangle is written, above it each entry
#                                          is either written or left alone (64- and 32-row block tiles skip their sub-tiles above the diagonal)
INT64_MACS = 1 << 30            # above this the integer product takes seconds: see exact_product
EXACT = 2.0 ** 53


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def integers(rng, shape, lim):
    return rng.randint(-lim, lim + 1, shape).astype(np.float64)


def operands(rng, M, N, K):
    """A [M, K], B [N, K] integer-valued in [-8, 8], C0 [M, N] in [-1024, 1024]"""
    return integers(rng, (M, K), 8), integers(rng, (N, K), 8), integers(rng, (M, N), 1024)


def scalars(rng, beta_zero=False):
    """(alpha, beta) from the powers of two of the issue; beta != 0 unless asked for: with beta = 0 a tile computed twice is invisible"""
    return ALPHAS[rng.randint(len(ALPHAS))], 0.0 if beta_zero else ALPHAS[rng.randint(len(ALPHAS))]


def zero_part(rows, K, kind, shift=0):
    """where an operand [rows, K] declared triangular is zero: 'upper': [i][k] = 0 for k < i - shift; 'lower': [i][k] = 0 for k > i"""
    i, k = np.arange(rows)[:, None], np.arange(K)[None, :]
    return k < i - shift if kind == "upper" else k > i


def unread_part(zero):
    """of a zero part, the 128 x 128 tiles that lie wholly inside it: what a launch does not read"""
    rows, K = zero.shape
    out = np.zeros_like(zero)
    r, c = rows // TILE, K // TILE
    if r and c:
        t = zero[:r * TILE, :c * TILE].reshape(r, TILE, c, TILE).all(axis=(1, 3))
        out[:r * TILE, :c * TILE] = np.repeat(np.repeat(t, TILE, 0), TILE, 1)
    return out


def shaped(X, zero):
    """(what the reference multiplies, what the kernel is given): zeros in the zero part; NaN where the launch must not read"""
    ref = np.where(zero, 0.0, X)
    return ref, np.where(unread_part(zero), np.nan, ref)


# ---- windows --------------------------------------------------------------------------------------------------------------------------------
class Window:
    """a [rows, cols] matrix with leading dimension ld, `offset` doubles into a flat buffer that holds SENTINEL everywhere else"""

    def __init__(self, rows, cols, ld, offset):
        assert ld >= cols and offset >= 0
        self.rows, self.cols, self.ld, self.offset = rows, cols, ld, offset
        self.size = offset + rows * ld + offset + 2

    def new(self, a):
        buf = np.full(self.size, SENTINEL)
        self.view(buf)[...] = a
        return buf

    def view(self, buf):
        return buf[self.offset:self.offset + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols]

    def check_guard(self, buf, what="window"):
        g = np.array(buf)
        self.view(g)[...] = SENTINEL
        bad = np.flatnonzero(g != SENTINEL)
        assert bad.size == 0, "%s: %d guard entries overwritten, first at flat index %d (window starts at %d, ld %d)" % (
            what, bad.size, bad[0], self.offset, self.ld)


def windows(M, N, K):
    """the embedding every case uses: even offsets, lda = K + 16, ldb = K + 2, ldc = N + 3 (odd: C has no alignment requirement)"""
    return Window(M, K, K + 16, 6), Window(N, K, K + 2, 10), Window(M, N, N + 3, 4)


def same_bits(a, b):
    """bitwise equality, NaN poison included (an operand a launch must not change)"""
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---- reference ------------------------------------------------------------------------------------------------------------------------------
def _as_int(X, what):
    Xi = X.astype(np.int64)
    assert np.array_equal(Xi.astype(np.float64), X), "%s is not integer-valued" % what
    return Xi


def exact_product(A, B):
    """A B^T of integer-valued A [M, K], B [N, K] as int64.  The int64 product on the host up to INT64_MACS multiply-adds; above that
    (numpy's integer matmul runs at ~1 GMAC/s: 15 s for the largest case) the fp64 product of the same integers, which is exact because
    every partial sum in any order is an integer below 2^53 -- asserted here from the data -- and is compared with the int64 product
    on 128 rows spread over A."""
    Ai, Bi = _as_int(A, "A"), _as_int(B, "B")
    M, K = A.shape
    N = B.shape[0]
    assert float(np.abs(Ai).sum(1).max()) * float(np.abs(Bi).max() if Bi.size else 0) < EXACT
    if M * N * K <= INT64_MACS:
        return Ai.dot(Bi.T)
    P = A.dot(B.T)
    Pi = P.astype(np.int64)
    assert np.array_equal(Pi.astype(np.float64), P)
    rows = np.unique(np.linspace(0, M - 1, 128).astype(int))
    assert np.array_equal(Pi[rows], Ai[rows].dot(Bi.T)), "fp64 product of integers differs from the int64 product"
    return Pi


def reference(A, B, C0, alpha, beta, P=None):
    """alpha A B^T + beta C0, exact.  The kernel forms acc = (beta / alpha) C0 + sum_k a b and stores alpha acc: asserted from the data,
    every intermediate of that route is a multiple of 2^-4 below 2^53 2^-4, whatever the order of the sum.  P: exact_product(A, B) if the
    caller has it."""
    if P is None:
        P = exact_product(A, B)
    C0i = _as_int(C0, "C0")
    bs16, a16 = beta / alpha * 16.0, alpha * 16.0
    assert bs16 == int(bs16) and a16 == int(a16) and alpha != 0.0, (alpha, beta)
    absprod = float(np.abs(A).sum(1).max()) * float(np.abs(B).max() if B.size else 0)
    assert (abs(bs16) * float(np.abs(C0i).max() if C0i.size else 0) + 16.0 * absprod) * max(1.0, abs(alpha)) < EXACT
    acc16 = int(bs16) * C0i + 16 * P
    res256 = int(a16) * acc16
    assert not (res256 % 16).any(), "the result is no multiple of 2^-4"
    return (res256 // 16).astype(np.float64) / 16.0


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------
def mask_plain(M, N):
    return np.full((M // TILE, N // TILE), WRITTEN, dtype=np.int8)


def mask_lower(M, N):
    """lower_only: square C (N == M) or a trapezoid whose first N - M columns are full; by 128-tiles"""
    assert N >= M
    i, j = np.arange(M // TILE)[:, None], np.arange(N // TILE)[None, :]
    off = (N - M) // TILE
    return np.where(j < i + off, WRITTEN, np.where(j == i + off, DIAGONAL, UNTOUCHED)).astype(np.int8)


def mask_trapezoid(M, off_cols, tri_cols=0):
    """tri_cols (0 or M: all): the triangle's columns end there -- tile row r holds off_cols / 128 + min(r + 1, tri_cols / 128) tiles, the
    last of them a diagonal tile only where the triangle still runs (r < tri_cols / 128); the rows below are written in full"""
    assert 0 <= tri_cols <= M and tri_cols % TILE == 0
    m = mask_lower(M, off_cols + M)
    if 0 < tri_cols < M:
        m[:, (off_cols + tri_cols) // TILE:] = UNTOUCHED
    return m


def mask_splitk(m, nchunks):
    """parts [nchunks, m, m] seen as one [nchunks m, m] matrix: the lower tiles of every part"""
    return np.tile(mask_lower(m, m), (nchunks, 1))


def expand(written):
    return np.repeat(np.repeat(written, TILE, 0), TILE, 1)


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------
def check(got, want, C0, written, guards=()):
    """got == want bit for bit on the written tiles, got == C0 on the untouched ones, no NaN in anything written;
    guards: (buffer after the launch, Window, name) -- the sentinel around every window"""
    got, want, C0 = np.asarray(got), np.asarray(want), np.asarray(C0)
    assert got.shape == want.shape == C0.shape == (written.shape[0] * TILE, written.shape[1] * TILE)
    w = expand(written)
    assert not np.isnan(got[w != UNTOUCHED]).any(), "NaN in the written part"
    full, un = w == WRITTEN, w == UNTOUCHED
    np.testing.assert_array_equal(got[full], want[full], err_msg="written tiles")
    np.testing.assert_array_equal(got[un], C0[un], err_msg="tiles the launch must leave alone")
    il, iu = np.tril_indices(TILE), np.triu_indices(TILE, 1)
    for bi, bj in zip(*np.nonzero(written == DIAGONAL)):
        blk = (slice(TILE * bi, TILE * bi + TILE), slice(TILE * bj, TILE * bj + TILE))
        g, x, c = got[blk], want[blk], C0[blk]
        np.testing.assert_array_equal(g[il], x[il], err_msg="diagonal tile (%d, %d)" % (bi, bj))
        assert ((g[iu] == x[iu]) | (g[iu] == c[iu])).all(), "diagonal tile (%d, %d): an entry above the diagonal is neither C0 nor the result" % (bi, bj)
    for buf, win, name in guards:
        win.check_guard(buf, name)


def roundoff_bound(A, B, C0, alpha, beta):
    """entrywise bound of the issue for the non-exact cases: K fused multiply-adds, one rounding of beta / alpha, one of its product with
    C, one of the final scaling, one unit of slack"""
    K = A.shape[1]
    return (K + 4) * 2.0 ** -53 * (abs(alpha) * np.abs(A).dot(np.abs(B).T) + abs(beta) * np.abs(C0))


def longdouble_reference(A, B, C0, alpha, beta):
    ld = np.longdouble
    return ld(alpha) * A.astype(ld).dot(B.astype(ld).T) + ld(beta) * C0.astype(ld)
