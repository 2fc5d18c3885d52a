"""The tile enumeration of the trapezoid launch (csrc/gemm.hip: gemm_nt_f64_trap_signal_kernel, launch_syrk_trap_signal; lower_tile of
csrc/gemm_tile.h) restated on numpy integers, every workgroup of a launch at once; no GPU in here.

A launch covers, by 128-tiles, tile rows r = 0 .. nt - 1 of C: `off` full ("narrow") tile columns, then the lower triangle limited to its
first wt tile columns -- row r holds off + min(r + 1, wt) tiles.  wt = nt is the unlimited launch (tri_cols = 0 or M); 0 < wt < nt the
LIM instantiation.  tiles() is the kernel's map from workgroup to tile, accepts() the launcher's rule; `defect` plants one index error
of the kind the map could have, for tests/test_trap_model.py to show that the property sees it."""
import numpy as np

# (off, nt, wt) of the launches tests/test_gemm_dispatch.py runs on the device, and per `off` one launch a tile row too small to be accepted
DEVICE_CASES = ((1, 10, 8),     # one ragged group of 2 rows below the triangle
                (1, 20, 2),     # triangle smaller than one group
                (1, 30, 1),
                (2, 15, 8),
                (2, 26, 3),
                (8, 34, 8),     # off = 8: the factorisation's own
                (8, 27, 16),
                (8, 35, 24),    # full groups plus a ragged one of 3
                (8, 40, 16),    # nt - wt a multiple of 8
                (8, 33, 32))    # wt = nt - 1: a single row below
REFUSED_CASES = ((1, 9, 8), (2, 14, 8), (8, 33, 8))
DEFECTS = ("ragged-group-as-8", "tri-with-nt", "group-stride-8nt", "bx-by-swapped", "start-without-narrow")


def _settle(guess, too_large, too_small):
    """the kernel's two correction loops behind a square-root guess"""
    v = guess
    while True:
        m = too_large(v)
        if not m.any():
            break
        v = v - m
    while True:
        m = too_small(v)
        if not m.any():
            break
        v = v + m
    return v


def lower_tile(lid, tri_off, nt):
    """(by, bx) of the lid-th tiles of a lower-only walk: groups of 8 tile rows, column-major left of the group's diagonal block, then that
    block's triangle row by row.  A lid past the walk's end gives whatever the arithmetic gives (a group without rows: (-1, -1))."""
    lid = np.asarray(lid, dtype=np.int64)
    negative, lid = lid < 0, np.maximum(lid, 0)
    b2 = 8.0 * tri_off + 4.0
    size = lambda g: g * (8 * tri_off + 32 * g + 4)              # tiles in front of group g
    g = _settle(((np.sqrt(b2 * b2 + 128.0 * lid) - b2) * (1.0 / 64.0)).astype(np.int64),
                lambda g: (g > 0) & (size(g) > lid), lambda g: (size(g + 1) <= lid) & ((g + 1) * 8 < nt))
    rem = lid - size(g)
    first = 8 * g
    rows = np.minimum(8, nt - first)
    ok = (rows > 0) & ~negative
    rows = np.where(ok, rows, 1)
    rect = rows * (tri_off + first)
    bx_r = rem // rows
    by_r = first + rem - bx_r * rows
    r2 = np.maximum(rem - rect, 0)
    j = _settle(((np.sqrt(8.0 * r2 + 1.0) - 1.0) * 0.5).astype(np.int64), lambda j: j * (j + 1) // 2 > r2, lambda j: (j + 1) * (j + 2) // 2 <= r2)
    in_rect = rem < rect
    by = np.where(in_rect, by_r, first + j)
    bx = np.where(in_rect, bx_r, tri_off + first + (r2 - j * (j + 1) // 2))
    return np.where(ok, by, -1), np.where(ok, bx, -1)


def shape(off, nt, wt):
    """(lim, wt, number of workgroups) as the launcher derives them from tri_cols = 128 wt: 0 and nt mean the whole triangle"""
    lim = 0 < wt < nt
    if not lim:
        wt = nt
    return lim, wt, wt * (wt + 1) // 2 + (nt - wt) * wt + off * nt


def _rows_of(g, nt):
    return np.minimum(8, nt - 8 * g)


def narrow_of(off, nt):
    """the narrow tiles of each XCD x: the groups g = x, x + 8, .. of 8 tile rows (the last one ragged), `off` columns each"""
    return np.array([sum(int(_rows_of(g, nt)) * off for g in range(x, (nt + 7) // 8, 8)) for x in range(8)], dtype=np.int64)


def accepts(off, nt, wt):
    """the launcher's rule: every XCD has at least as many workgroups as narrow tiles (else GPX_ERR_STATE)"""
    nwg = shape(off, nt, wt)[2]
    return bool(((nwg - np.arange(8) + 7) // 8 >= narrow_of(off, nt)).all())


def tiles(off, nt, wt, defect=None):
    """(by, bx, narrow) of the workgroups 0 .. nwg - 1 of an accepted launch"""
    assert defect is None or defect in DEFECTS
    lim, wt, nwg = shape(off, nt, wt)
    orig = np.arange(nwg, dtype=np.int64)
    xcd, idx = orig & 7, orig >> 3
    nar = narrow_of(off, nt)
    mine = nar[xcd]
    narrow = idx < mine
    # the narrow part: this XCD's groups one after the other, column-major inside a group
    g, k = xcd.copy(), np.where(narrow, idx, 0)
    while True:
        m = narrow & (k >= _rows_of(g, nt) * off)
        if not m.any():
            break
        k = k - np.where(m, _rows_of(g, nt) * off, 0)
        g = g + np.where(m, 8, 0)
    r = np.maximum(_rows_of(g, nt), 1)
    by_n, bx_n = 8 * g + k % r, k // r
    # the bulk: XCD x's contiguous chunk of the logical order starts behind the chunks of the XCDs before it
    per_xcd = (nwg - np.arange(8) + 7) // 8 - (0 if defect == "start-without-narrow" else nar)
    start = np.concatenate([[0], np.cumsum(per_xcd)[:-1]])[xcd]
    lid = np.where(narrow, 0, start + idx - mine)
    tri = (nt if defect == "tri-with-nt" else wt) * (wt + 1) // 2
    by_t, bx_t = lower_tile(np.where(lid < tri, lid, 0) if lim else lid, 0, wt if lim else nt)
    if lim:
        rr = np.maximum(lid - tri, 0)
        stride = 8 * (nt if defect == "group-stride-8nt" else wt)
        gg = rr // stride
        first = wt + 8 * gg
        rows = np.full_like(first, 8) if defect == "ragged-group-as-8" else np.minimum(8, nt - first)
        ok = rows > 0
        rows = np.where(ok, rows, 1)
        rem = rr - gg * stride
        bx_b = rem // rows
        by_b = first + rem - bx_b * rows
        if defect == "bx-by-swapped":
            by_b, bx_b = bx_b, by_b
        by_b, bx_b = np.where(ok, by_b, -1), np.where(ok, bx_b, -1 - off)
        by_t, bx_t = np.where(lid < tri, by_t, by_b), np.where(lid < tri, bx_t, bx_b)
    return np.where(narrow, by_n, by_t), np.where(narrow, bx_n, bx_t + off), narrow


def mask(off, nt, wt):
    """[nt, off + nt] by tiles: True where the launch writes -- row r holds its first off + min(r + 1, wt) tiles"""
    wt = shape(off, nt, wt)[1]
    r, c = np.arange(nt)[:, None], np.arange(off + nt)[None, :]
    return c < off + np.minimum(r + 1, wt)


def violations(off, nt, wt, defect=None):
    """what is wrong with the enumeration of an accepted shape, as a list of strings (empty: every tile of the trapezoid is taken exactly
    once, none lies outside it, the counting workgroups are exactly those of the first `off` tile columns and each of those columns counts nt)"""
    by, bx, narrow = tiles(off, nt, wt, defect)
    want = mask(off, nt, wt)
    out = []
    inside = (by >= 0) & (by < nt) & (bx >= 0) & (bx < off + nt)
    inside[inside] = want[by[inside], bx[inside]]
    if not inside.all():
        o = int(np.flatnonzero(~inside)[0])
        out.append("%d workgroups outside the trapezoid, first %d at (%d, %d)" % ((~inside).sum(), o, by[o], bx[o]))
    taken = np.bincount(by[inside] * (off + nt) + bx[inside], minlength=nt * (off + nt)).reshape(nt, off + nt)
    if (taken[want] == 0).any():
        out.append("%d tiles not taken, first %s" % ((want & (taken == 0)).sum(), np.argwhere(want & (taken == 0))[0].tolist()))
    if (taken > 1).any():
        out.append("%d tiles taken more than once, first %s" % ((taken > 1).sum(), np.argwhere(taken > 1)[0].tolist()))
    if (narrow != (bx < off)).any():
        out.append("%d workgroups count a tile outside the first %d tile columns, or do not count one inside" % ((narrow != (bx < off)).sum(), off))
    counts = np.bincount(bx[narrow & inside], minlength=off)[:off]
    if (counts != nt).any() or narrow.sum() != off * nt:
        out.append("counters %s, not %d each" % (counts.tolist(), nt))
    return out


def smallest_accepted(off, wt):
    """the smallest nt > wt the launcher accepts with this triangle width (a LIM launch)"""
    nt = wt + 1
    while not accepts(off, nt, wt):
        nt += 1
    return nt
