"""CPU: the trapezoid launch's map from workgroup to tile (tests/_trap_model.py, restated from csrc/gemm.hip) takes every tile of the
trapezoid exactly once and none outside it, for every shape the launcher's rule accepts; each planted index defect breaks that.

tests/test_gemm_dispatch.py runs the model's smallest accepted shapes on the device and holds the launcher to the model's decisions."""
import numpy as np
import pytest

import _trap_model as tm

OFFS = (1, 2, 8)
NTS = tuple(range(1, 140)) + (200, 263, 504, 512)


def _widths(nt):
    return sorted(set(w for w in (0, 1, 2, 3, 7, 8, 9, 16, 24, nt - 9, nt - 8, nt - 1, nt) if 0 <= w <= nt))


@pytest.fixture(scope="module")
def sweep():
    accepted, refused, wrong = [], [], []
    for off in OFFS:
        for nt in NTS:
            for wt in _widths(nt):
                if not tm.accepts(off, nt, wt):
                    refused.append((off, nt, wt))
                    continue
                accepted.append((off, nt, wt))
                v = tm.violations(off, nt, wt)
                if v:
                    wrong.append((off, nt, wt, v))
    return accepted, refused, wrong


def test_every_accepted_shape_takes_each_tile_once(sweep):
    accepted, refused, wrong = sweep
    print("%d shapes accepted, %d refused, %d with violations" % (len(accepted), len(refused), len(wrong)))
    assert not wrong, wrong[:5]
    assert (len(accepted), len(refused)) == (4554, 687)        # a moved acceptance rule changes the split


def test_the_sweep_reaches_both_instantiations_and_every_group_shape(sweep):
    accepted = sweep[0]
    lim = [(off, nt, wt) for off, nt, wt in accepted if tm.shape(off, nt, wt)[0]]
    assert len(lim) > 2000 and len(accepted) - len(lim) > 300
    assert set((nt - wt) % 8 for _off, nt, wt in lim) == set(range(8))        # every ragged last group, and none
    assert any(nt - wt < 8 for _off, nt, wt in lim) and any(wt < 8 for _off, nt, wt in lim) and any(wt % 8 for _off, nt, wt in lim)


@pytest.mark.parametrize("off,nt,wt", [(1, 10, 8), (8, 35, 24), (8, 139, 24), (2, 512, 503)])
def test_narrow_columns_count_nt(off, nt, wt):
    by, bx, narrow = tm.tiles(off, nt, wt)
    assert np.bincount(bx[narrow], minlength=off).tolist() == [nt] * off
    assert (bx[~narrow] >= off).all() and len(by) == tm.shape(off, nt, wt)[2]
    for c in range(off):                                                    # and each column's nt tiles are its nt rows
        assert sorted(by[narrow & (bx == c)].tolist()) == list(range(nt))


def test_unlimited_widths_are_one_launch():
    """tri_cols = 0 and tri_cols = M: the same enumeration, that of the launch without a limit"""
    for off, nt in ((1, 10), (8, 35)):
        a, b = tm.tiles(off, nt, 0), tm.tiles(off, nt, nt)
        assert all((x == y).all() for x, y in zip(a, b)) and not tm.shape(off, nt, 0)[0] and not tm.shape(off, nt, nt)[0]


def test_mask_rows():
    m = tm.mask(2, 5, 3)
    assert m.sum(1).tolist() == [3, 4, 5, 5, 5] and m.shape == (5, 7)
    assert (m == (np.arange(7)[None, :] < m.sum(1)[:, None])).all()        # every row is a prefix
    assert tm.mask(2, 5, 0).sum(1).tolist() == tm.mask(2, 5, 5).sum(1).tolist() == [3, 4, 5, 6, 7]


# where each planted defect must show: a shape of the device cases (the ones whose geometry the defect touches)
DEFECT_SHAPES = {
    "ragged-group-as-8": [(1, 10, 8), (8, 35, 24), (8, 33, 32)],            # (nt - wt a multiple of 8: no ragged group, no difference)
    "tri-with-nt": list(tm.DEVICE_CASES),
    "group-stride-8nt": [(8, 35, 24), (8, 40, 16), (2, 26, 3), (1, 20, 2)],   # (a single group below the triangle: the stride is never used)
    "bx-by-swapped": list(tm.DEVICE_CASES),
    "start-without-narrow": list(tm.DEVICE_CASES),
}


@pytest.mark.parametrize("defect", tm.DEFECTS)
def test_planted_defect_fails_the_property(defect):
    for off, nt, wt in DEFECT_SHAPES[defect]:
        assert tm.accepts(off, nt, wt) and not tm.violations(off, nt, wt)
        v = tm.violations(off, nt, wt, defect)
        print(defect, (off, nt, wt), v)
        assert v, (defect, off, nt, wt)


def test_defects_that_cannot_show_do_not():
    """the two shapes named above as blind to a defect are: the property is not failing for another reason"""
    assert not tm.violations(8, 40, 16, "ragged-group-as-8")
    assert not tm.violations(1, 10, 8, "group-stride-8nt")


def test_every_defect_is_planted():
    assert set(DEFECT_SHAPES) == set(tm.DEFECTS) and len(tm.DEFECTS) >= 4


def test_device_cases_are_the_smallest_the_rule_accepts():
    for off, nt, wt in tm.DEVICE_CASES:
        assert tm.accepts(off, nt, wt) and tm.shape(off, nt, wt)[0], (off, nt, wt)
    # all but the two that are there for their group shapes: one tile row fewer is refused
    for off, nt, wt in tm.DEVICE_CASES:
        if (off, nt, wt) not in ((8, 35, 24), (8, 40, 16)):
            assert tm.smallest_accepted(off, wt) == nt, (off, nt, wt)
    assert max(nt for _off, nt, _wt in tm.DEVICE_CASES) * 128 <= 5120
    assert set(off for off, _nt, _wt in tm.REFUSED_CASES) == set(OFFS)
    for off, nt, wt in tm.REFUSED_CASES:
        assert not tm.accepts(off, nt, wt) and tm.accepts(off, nt + 1, wt) and tm.smallest_accepted(off, wt) == nt + 1
