"""CPU-only: the long-double model of the Gaussian Gram kernel (tests/_gauss_ld.py) against the golden file of the genuine reference
(tests/golden/gram.npz), the float64 restatement's own distance rho that the device bound of tests/test_gauss_gram.py is built on, the
conditions the input families promise and the seeded defects that bound must catch.

Measured here (x86-64, numpy float64 against np.longdouble), printed by the tests with -s: rho <= 2.1 over all cases (the far family; the
others <= 1.5), so GRAM_FLOOR = 4 governs and the bound is 32 units of u K (1 + q + sqrt(q) s)."""
import math

import numpy as np
import pytest

from conftest import load_golden

import _gauss_ld as gl

GOLDEN_CASES = ["grid_int", "n257_d5", "n64_d16", "rect_33x257_d5", "n257_d5_vt0", "n130_d1"]      # test_gpu_parity.GRAM_CASES


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_model_reproduces_the_golden_gram(name):
    """K_ij and K (= K_ij + vt on the diagonal) at the tolerance test_gram_golden holds the device to"""
    g = load_golden("gram")
    xi, xj, th = g[name + "__xi"], g[name + "__xj"], g[name + "__theta"]
    with np.errstate(divide="ignore"):
        vt = float(np.exp(th[1]))
    np.testing.assert_allclose(gl.kernel_parts(xi, xj, th)["K"].astype(np.float64), g[name + "__K_ij"], rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(gl.restate(xi, xj, th), g[name + "__K_ij"], rtol=1e-13, atol=1e-300)
    if name + "__K" in g:
        np.testing.assert_allclose(gl.kernel_parts(xi, xi, th, add_diag=vt)["Kd"].astype(np.float64), g[name + "__K"], rtol=1e-13, atol=1e-300)


def test_golden_file_has_the_cases():
    g = load_golden("gram")
    assert all(n + "__K_ij" in g for n in GOLDEN_CASES) and sum(n + "__K" in g for n in GOLDEN_CASES) >= 1


def test_rho_of_the_float64_restatement():
    rho, per = gl.rho_all()
    for fam in gl.FAMILIES:
        print("%-7s rho %.3f" % (fam, max(r for c, r in per.items() if c[0] == fam)))
    print("square  rho %.3f" % per[("square",) + gl.SQUARE])
    print("rho = %.3f -> bound %.1f units of u K (1 + q + sqrt(q) s)" % (rho, gl.bound()))
    assert len(per) == 5 * len(gl.D_ALL) + 3 * len(gl.FAMILY_D) + 1
    assert np.isfinite(rho) and 0 < rho < gl.GRAM_FLOOR
    assert gl.bound() == 32.0


def test_the_s_term_is_needed_and_is_no_loosening():
    """in units of (1 + q) alone the restatement itself leaves the floor on the offset family (prescaled coordinates near 2^10 sqrt(w)
    lose their low bits before the difference), and the full scale stays within a small factor of (1 + q) on the unit family"""
    worst = 0.0
    for d in gl.FAMILY_D:
        case = ("offset",) + gl.FAMILY_SHAPE + (d,)
        xi, xj, theta = gl.make_case(*case)
        worst = max(worst, float(gl.units(gl.restate(xi, xj, theta), gl.ld_parts(*case), s_term=False).max()))
    print("offset family, restatement in units of (1 + q) alone: %.1f" % worst)
    assert worst > gl.bound()
    for d in gl.FAMILY_D:
        p = gl.ld_parts("unit", 130, 257, d)
        ratio = (1 + p["q"] + np.sqrt(p["q"]) * p["s"]) / (1 + p["q"])
        assert float(ratio.max()) < 8.0, (d, float(ratio.max()))


def test_parameters_are_the_ones_the_device_holds():
    """the exact comparisons (equal rows give v, the diagonal fl(v + vt)) need numpy's exp(theta) and the C library's to agree on v and vt"""
    theta = gl.make_case("unit", 130, 257, 3)[2]
    v, vt, _w = gl.params(theta, 3, np.float64)
    assert float(v) == math.exp(theta[0]) == gl.V and float(vt) == math.exp(theta[1])


@pytest.mark.parametrize("d", gl.FAMILY_D)
def test_far_family_populates_normal_subnormal_and_zero(d):
    n1, n2 = gl.FAMILY_SHAPE
    xi, xj, theta = gl.make_case("far", n1, n2, d)
    K = gl.restate(xi, xj, theta)
    normal, sub, zero = int((K >= gl.TINY).sum()), int(((K > 0) & (K < gl.TINY)).sum()), int((K == 0).sum())
    print("far d=%d: normal %d subnormal %d zero %d" % (d, normal, sub, zero))
    assert min(normal, sub, zero) >= 100 and normal + sub + zero == n1 * n2
    q = gl.ld_parts("far", n1, n2, d)["q"]
    assert float(q.max()) / 2 > 750.0 > float(q.min()) / 2          # both sides of the fmax(x, -750) clamp
    c = gl.far_ramp(theta, n2)
    assert np.array_equal(c, gl._grid(c)) and np.all(np.diff(c) > 0)


def test_equal_rows_exist_and_the_offset_is_exact():
    for fam in ("unit", "sharp", "offset"):
        for n1, n2 in gl.SHAPES if fam == "unit" else (gl.FAMILY_SHAPE,):
            for d in (1, 3, 64):
                xi, xj, theta = gl.make_case(fam, n1, n2, d)
                eq = gl.ld_parts(fam, n1, n2, d)["eq"]
                rows = list(range(3, n1, 7))
                assert all(eq[i, (5 * i) % n2] for i in rows) and eq.sum() >= len(rows) and (len(rows) > 0) == (n1 > 3)
                K = gl.restate(xi, xj, theta)
                assert np.all(K[eq] == gl.V)
    for d in gl.FAMILY_D:
        n1, n2 = gl.FAMILY_SHAPE
        xi, xj, theta = gl.make_case("offset", n1, n2, d)
        bi, bj, btheta = gl.offset_base(n1, n2, d)
        assert np.array_equal(xi - gl.OFFSET, bi) and np.array_equal(xj - gl.OFFSET, bj) and np.array_equal(theta, btheta)
        assert np.array_equal(bi, gl._grid(bi)) and np.array_equal(xi, gl._grid(xi)) and xi.min() >= gl.OFFSET
    x, theta = gl.make_square()
    assert np.array_equal(x[gl.SQUARE[0] - 10], x[4])
    p = gl.ld_square()
    assert np.array_equal(p["Kd"] != p["K"], np.eye(gl.SQUARE[0], dtype=bool))


def test_sharp_family_reaches_1e_130():
    for d in gl.FAMILY_D:
        p = gl.ld_parts("sharp", 130, 257, d)
        assert float(p["q"].max()) > 200.0, (d, float(p["q"].max()))
    assert min(float(gl.ld_parts("sharp", 130, 257, d)["K"].min()) for d in gl.FAMILY_D) < 1e-130


def _worst_of_defect(defect):
    """{case: the defective restatement's worst distance}: the families at (130, 257) for every d of FAMILY_D and the square case"""
    out = {}
    for fam in gl.FAMILIES:
        for d in gl.FAMILY_D:
            case = (fam,) + gl.FAMILY_SHAPE + (d,)
            xi, xj, theta = gl.make_case(*case)
            out[case] = float(gl.units(gl.restate(xi, xj, theta, defect=defect), gl.ld_parts(*case)).max())
    x, theta = gl.make_square()
    vt = float(np.exp(theta[1]))
    out[("square",) + gl.SQUARE] = float(gl.units(gl.restate(x, x, theta, add_diag=vt, defect=defect), gl.ld_square(), "Kd").max())
    return out


@pytest.mark.parametrize("defect", gl.DEFECTS)
def test_seeded_defects_fall_outside_the_bound(defect):
    """each defect planted in the restatement leaves the bound on at least one case that tests/test_gauss_gram.py runs on the device --
    the same case with the same rule would catch it in gram_kernel"""
    lim = gl.bound()
    worst = _worst_of_defect(defect)
    caught = {c: r for c, r in worst.items() if not r <= lim}
    top = max(worst, key=lambda c: worst[c])
    print("%-8s caught on %d of %d cases; worst %.3e units on %r (bound %.1f)" % (defect, len(caught), len(worst), worst[top], top, lim))
    assert caught, (defect, worst)
    # where each is expected to show
    expect = {"tail": [("unit", 130, 257, 1), ("unit", 130, 257, 3), ("unit", 130, 257, 9), ("unit", 130, 257, 17)],
              "col": [("unit", 130, 257, d) for d in gl.FAMILY_D], "nohalf": [("unit", 130, 257, d) for d in gl.FAMILY_D],
              "diag1": [("square",) + gl.SQUARE], "expanded": [("offset", 130, 257, d) for d in gl.FAMILY_D],
              "sqrt32": [("unit", 130, 257, d) for d in gl.FAMILY_D], "ftz": [("far", 130, 257, d) for d in gl.FAMILY_D]}[defect]
    assert all(c in caught for c in expect), (defect, [c for c in expect if c not in caught])
    if defect == "tail":                     # even d has no tail: the defect is the identity there
        assert all(worst[("unit", 130, 257, d)] <= lim for d in (2, 8, 64))
