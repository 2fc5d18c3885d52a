"""The two splits of the emulated update (csrc/emu.hip) on their own, to the last byte: gpx_emu_split (emu_row_scale_kernel +
emu_split_kernel: each row scaled by its own largest entry) and gpx_emu_split_fixed (emu_split_fixed_kernel: the left-looking solve's
split with a given scale, into a column window of the residue image).  Every residue byte and every scale is compared with a host
reference built from exact integers, a' = rint(ldexp(x, s)) as int64 and its residues by integer %; everything around the written
windows carries sentinels that must be intact afterwards."""
import ctypes

import numpy as np
import pytest

from _emu_split_model import NONFINITE, residues_exact

ROWS, ROWS_PAD = 5, 256
SENT = 0x5A
SIG_SENT = -777


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _general_row(n, top_exp, s, rng):
    """n doubles x with |x 2^s| < 2^top_exp, spread over 70 binades, then the special entries: ties at +-0.5 before the rounding (even
    and odd neighbours), -0.0, 0.0 and the last double below +-2^top_exp."""
    x = np.ldexp(rng.uniform(-1.0, 1.0, n), rng.integers(top_exp - 70, top_exp + 1, n) - s)
    for j, k in enumerate((0, 1, 2, 3, -1, -2, -3, 254, 255, -255, 12345678)):
        x[8 + j] = np.ldexp(k + 0.5, -s)                                # 0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, ...: exact ties
    x[20], x[21] = -0.0, 0.0
    x[22] = np.ldexp(1.0 - 2.0 ** -53, top_exp - s)
    x[23] = -np.ldexp(1.0 - 2.0 ** -53, top_exp - s)
    return x


def _integers(x, s):
    """a' = rint(x 2^s) of the finite entries as int64 (0 where x is not finite), exact: |a'| <= 2^59."""
    fin = np.isfinite(x)
    a = np.rint(np.ldexp(np.where(fin, x, 0.0), s))
    assert (np.abs(a) <= 2.0 ** 62).all()
    return a.astype(np.int64)


# ---- the split with the row's own scale ------------------------------------------------------------------------------------------------
def _free_case(K, bits, seed):
    rng = np.random.default_rng(seed)
    ldx = K + 6
    X = np.full((ROWS, ldx), np.nan)                                    # beyond column K: NaN that must not be read into anything
    # row 0: its largest entry 2 - 2^-52 scales to 2^bits - 2^(bits - 53): for bits < 53 it ROUNDS to 2^bits exactly, the largest a' there is
    X[0, :K] = _general_row(K, bits, bits - 1, rng)
    X[0, 3], X[0, K - 1] = 2.0 - 2.0 ** -52, -(2.0 - 2.0 ** -52)
    X[1, :K] = 0.0                                                      # all zero: scale 0
    X[1, 5] = -0.0
    X[2, :K] = _general_row(K, bits, bits + 39, rng)
    X[2, K // 2 + 1] = np.nan
    X[3, :K] = _general_row(K, bits, bits - 11, rng)
    X[3, K - 2] = -np.inf
    X[4, :K] = _general_row(K, bits, bits - 301, rng)                   # another binade: the scale comes from ilogb of the maximum
    X[4, 7] = np.ldexp(1.5, 300)
    sig = np.zeros(ROWS, np.int64)
    a = np.zeros((ROWS, K), np.int64)
    for i in (0, 1, 4):
        m = np.abs(X[i, :K]).max()
        sig[i] = 0 if m == 0.0 else bits - 1 - (int(np.frexp(m)[1]) - 1)
        a[i] = _integers(X[i, :K], int(sig[i]))
        assert (np.abs(a[i]) <= 2 ** bits).all()
    sig[2] = sig[3] = NONFINITE                                         # zero residues
    if bits < 53:
        assert abs(a[0, 3]) == 2 ** bits and a[0, K - 1] == -(2 ** bits)
    return X, ldx, sig, a


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [24, 55, 59])
@pytest.mark.parametrize("L", [2, 16])
@pytest.mark.parametrize("K", [128, 1152])
def test_split_with_own_scale_every_byte(K, L, bits):
    from conftest import torch
    from skgpuppy_amd import _gpx
    X, ldx, sig, a = _free_case(K, bits, 1000 * K + bits)
    want = np.zeros((L, ROWS_PAD, K), np.int8)
    want[:, :ROWS] = residues_exact(a, L)
    gap = 48                                                            # sentinel bytes between the planes, in front and behind
    plane = ROWS_PAD * K + gap
    x = torch.as_tensor(X).cuda()
    buf = torch.full((gap + L * plane,), SENT, dtype=torch.int8, device="cuda")
    sg = torch.full((ROWS_PAD + 8,), SIG_SENT, dtype=torch.int32, device="cuda")
    _gpx.check(_gpx.lib.gpx_emu_split(_ptr(x), ldx, ROWS, ROWS_PAD, K, bits, L, ctypes.c_void_p(buf.data_ptr() + gap), plane, _ptr(sg)), "gpx_emu_split")
    got, gs = buf.cpu().numpy(), sg.cpu().numpy()
    assert (got[:gap] == SENT).all()
    pl = got[gap:].reshape(L, plane)
    assert (pl[:, ROWS_PAD * K:] == SENT).all()
    res = pl[:, :ROWS_PAD * K].reshape(L, ROWS_PAD, K)
    bad = res != want
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], res[bad][:5], want[bad][:5])
    np.testing.assert_array_equal(gs[:ROWS], sig.astype(np.int32))
    assert (gs[ROWS:ROWS_PAD] == 0).all() and (gs[ROWS_PAD:] == SIG_SENT).all()


# ---- the split with a given scale ------------------------------------------------------------------------------------------------------
def _fixed_case(width, bits, over, seed):
    rng = np.random.default_rng(seed)
    ldx = width + 10
    X = np.full((ROWS, ldx), np.nan)
    sig = np.array([bits - 11, 3, bits + 40, bits - 1, NONFINITE], np.int64)
    a = np.zeros((ROWS, width), np.int64)
    # row 0: up to the limit itself, +-2^bits after scaling (allowed: only |a'| > 2^bits is refused)
    X[0, :width] = _general_row(width, bits, int(sig[0]), rng)
    X[0, 1], X[0, width - 1] = np.ldexp(1.0, bits - int(sig[0])), -np.ldexp(1.0, bits - int(sig[0]))
    if over:                                                            # row 1: one entry just over the limit, its neighbours exact
        X[1, :width] = _general_row(width, bits, int(sig[1]), rng)
        X[1, 33] = np.ldexp(1.0 + 2.0 ** -20, bits - int(sig[1]))
    else:
        X[1, :width] = 0.0                                              # an all-zero row under an arbitrary scale
    X[2, :width] = _general_row(width, bits - 3, int(sig[2]), rng)
    X[2, 17] = np.nan                                                   # marks the row; the other entries are split all the same
    X[3, :width] = _general_row(width, bits - 1, int(sig[3]), rng)
    X[3, width - 16] = np.inf
    X[4, :width] = _general_row(width, bits - 2, 5, rng)          # marked at entry: zeros, whatever it holds
    for i in range(4):
        a[i] = _integers(X[i, :width], int(sig[i]))
    if over:
        assert abs(a[1, 33]) > 2 ** bits
        a[1, 33] = 0
    assert (np.abs(a) <= 2 ** bits).all() and a[0, 1] == 2 ** bits and a[0, width - 1] == -(2 ** bits)
    sig_after = sig.copy()
    sig_after[2] = sig_after[3] = NONFINITE
    return X, ldx, sig, sig_after, a


@pytest.mark.gpu
@pytest.mark.parametrize("over", [False, True])
@pytest.mark.parametrize("bits", [24, 55, 59])
@pytest.mark.parametrize("L", [2, 16])
@pytest.mark.parametrize("width", [1024, 256])
def test_split_with_given_scale_every_byte(width, L, bits, over):
    from conftest import torch
    from skgpuppy_amd import _gpx
    X, ldx, sig, sig_after, a = _fixed_case(width, bits, over, 7 * width + bits + int(over))
    off, ldr, gap = 48, width + 80, 32                                  # the window starts at column 48 of an image 80 columns wider
    plane = ROWS_PAD * ldr + gap
    want = np.full((L, plane), SENT, np.int8)
    win = want[:, :ROWS_PAD * ldr].reshape(L, ROWS_PAD, ldr)
    win[:, :, off:off + width] = 0
    win[:, :ROWS, off:off + width] = residues_exact(a, L)
    x = torch.as_tensor(X).cuda()
    buf = torch.full((gap + L * plane,), SENT, dtype=torch.int8, device="cuda")
    sg_host = np.full(ROWS_PAD + 8, SIG_SENT, np.int32)
    sg_host[:ROWS] = sig
    sg = torch.as_tensor(sg_host).cuda()
    st = torch.zeros(3, dtype=torch.int32, device="cuda")
    _gpx.check(_gpx.lib.gpx_emu_split_fixed(_ptr(x), ldx, ROWS, ROWS_PAD, width, bits, L, ctypes.c_void_p(buf.data_ptr() + gap + off), ldr, plane,
                                            _ptr(sg), ctypes.c_void_p(st.data_ptr() + 4)), "gpx_emu_split_fixed")
    got, gs = buf.cpu().numpy(), sg.cpu().numpy()
    assert (got[:gap] == SENT).all()
    bad = got[gap:].reshape(L, plane) != want                           # the window, and every sentinel beside, between and behind it
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])
    np.testing.assert_array_equal(gs[:ROWS], sig_after.astype(np.int32))
    assert (gs[ROWS:] == SIG_SENT).all()                                 # the padding rows' scales are neither read nor written
    assert st.cpu().tolist() == [0, int(over), 0]


@pytest.mark.gpu
def test_split_entries_refuse_what_the_kernels_take_for_granted():
    from conftest import torch
    from skgpuppy_amd import _gpx
    x = torch.zeros(4 * 1040, dtype=torch.float64, device="cuda")
    r = torch.zeros(16 * 4 * 1040, dtype=torch.int8, device="cuda")
    s = torch.zeros(8, dtype=torch.int32, device="cuda")
    ok = dict(X=_ptr(x), ldx=1040, rows=2, rows_pad=4, K=1024, bits=55, nmod=16, res=_ptr(r), plane=4 * 1040, sig=_ptr(s))
    for change in (dict(K=1000), dict(bits=60), dict(bits=0), dict(nmod=17), dict(ldx=1000), dict(ldx=1041), dict(rows=5), dict(plane=4 * 1024 - 16),
                   dict(X=ctypes.c_void_p(x.data_ptr() + 8)), dict(res=ctypes.c_void_p(r.data_ptr() + 4)), dict(sig=None)):
        args = dict(ok, **change)
        assert _gpx.lib.gpx_emu_split(*args.values()) == _gpx.GPX_ERR_BAD_ARG, change
    okf = dict(X=_ptr(x), ldx=1040, rows=2, rows_pad=4, width=512, bits=55, nmod=16, res=_ptr(r), ldr=1040, plane=4 * 1040, sig=_ptr(s), status=_ptr(s))
    for change in (dict(width=520), dict(width=2048, ldx=2048, ldr=2048), dict(ldr=1032), dict(ldr=496), dict(plane=4 * 1040 + 8), dict(status=None),
                   dict(bits=60), dict(res=ctypes.c_void_p(r.data_ptr() + 8))):
        args = dict(okf, **change)
        assert _gpx.lib.gpx_emu_split_fixed(*args.values()) == _gpx.GPX_ERR_BAD_ARG, change
    assert _gpx.lib.gpx_emu_split(*ok.values()) == 0 and _gpx.lib.gpx_emu_split_fixed(*okf.values()) == 0
    assert int(r.count_nonzero()) == 0 and s.cpu().tolist() == [0] * 8
