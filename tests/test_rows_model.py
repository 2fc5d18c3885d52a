"""CPU-only: the long-double model of tests/_rows_ld.py is right, its float64 evaluation stays under the floor of each rule, and each rule
rejects every seeded defect at the shapes tests/test_rows.py runs on the device.

  model    the Gaussian C, J, H_kk and tr = tracedot(H, Sigma) against oracle.cjh; the Matern 5/2 J, H_kk and tr against
           _matern_ld.jacobian_hessian and C against _matern_ld.kernel_parts; C and J of every kind against _predict_grad_model.rows; J and H_kk
           against central differences of the kernel in long double; d = 1, 3, 9
  floor    rho of the rows (over every case of _rows_ld.all_cases()) and rho_ref of every reduction case, printed
  defects  _rows_ld.ROW_DEFECTS at N = 129 (127 padded columns), d = 3 and 9; _rows_ld.REDUCE_DEFECTS at npad = 768, d = 8 and 9
  build    the eight APPROX / DVH instantiations of the build frame (csrc/rows_tile.h) keep everything in registers and their occupancy"""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from oracle import oracle as orc

import _dense_ld as dl
import _matern_ld as ml
import _predict_grad_model as pg
import _rows_ld as rl

PKG_PARENT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scikit-gpuppy_amd")
LD = rl.LD
EPS_LD = float(np.finfo(LD).eps)
MODEL_D = (1, 3, 9)
MODEL_N = 40


def _small(d):
    x, _t, theta, Uin, Sig = rl.make_case(128, d)
    return x[:MODEL_N], theta, Uin, Sig               # rows 5, 7, 9 (equal, but_last, but_first) are among the first 40


def _split(block, layout, d, B, N):
    """{row kind: [B, rows of the kind, N]} of a (values | scales | q) block"""
    names = rl.row_kinds(layout, d, B)
    return {k: block[names == k][:, :N].reshape(B, -1, N) for k in ("C", "tr", "J", "H") if (names == k).any()}


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", MODEL_D)
def test_gaussian_rows_agree_with_the_oracle(d):
    """entry by entry within 1e-12 (1 + q) of the entry's scale: the oracle is float64"""
    x, theta, Uin, Sig = _small(d)
    gp = types.SimpleNamespace(x=x, theta_min=theta, n=len(x))
    B, N = len(Uin), len(x)
    got = {lay: [_split(a, lay, d, B, N) for a in rl.rows(x, theta, Uin, Sig, 0, lay)] for lay in (rl.APPROX, rl.DVH, rl.GRAD)}
    for b, u in enumerate(Uin):
        C, J, H = orc.cjh(gp, u)
        J, Hkk, tr = J[:, :, 0].T, np.diagonal(H, axis1=1, axis2=2).T, (H * Sig[b][None]).sum((1, 2))
        noise = float(np.exp(theta[1])) * (x == u).all(1)
        for lay, want in ((rl.APPROX, {"C": C, "tr": tr, "J": J}), (rl.DVH, {"C": C, "J": J, "H": Hkk}), (rl.GRAD, {"C": C - noise, "J": J})):
            val, sca, q = got[lay]
            for k, w in want.items():
                err = np.abs(val[k][b] - np.atleast_2d(w)).astype(np.float64)
                lim = (1e-12 * (1 + q[k][b]) * sca[k][b]).astype(np.float64)
                assert (err <= lim).all(), (d, b, rl.LAYOUT_NAMES[lay], k, float((err - lim).max()))


@pytest.mark.parametrize("d", MODEL_D)
def test_matern_rows_agree_with_the_matern_model(d):
    """long double against long double: within 256 eps (1 + q) of the entry's scale (the two evaluate in different orders)"""
    x, theta, Uin, Sig = _small(d)
    B, N = len(Uin), len(x)
    got = {lay: [_split(a, lay, d, B, N) for a in rl.rows(x, theta, Uin, Sig, 5, lay)] for lay in (rl.APPROX, rl.DVH, rl.GRAD)}
    for b, u in enumerate(Uin):
        J, H = ml.jacobian_hessian(u, x, theta)
        C = ml.kernel_parts(u[None, :], x, theta, 5)["K"][0]
        want = {"C": C, "J": J.T, "H": np.diagonal(H, axis1=1, axis2=2).T, "tr": (H * Sig[b].astype(LD)[None]).sum((1, 2))}
        for lay in (rl.APPROX, rl.DVH, rl.GRAD):
            val, sca, q = got[lay]
            for k in val:
                err, lim = np.abs(val[k][b] - np.atleast_2d(want[k])), 256 * EPS_LD * (1 + q[k][b]) * sca[k][b]
                assert (err <= lim).all(), (d, b, rl.LAYOUT_NAMES[lay], k, float((err - lim).max()))


@pytest.mark.parametrize("kind", rl.KINDS)
@pytest.mark.parametrize("d", MODEL_D)
def test_grad_rows_agree_with_the_predictor_model(d, kind):
    """C with the kind's own +vt convention and J = -d c / d u of _predict_grad_model.rows, every kind"""
    x, theta, Uin, Sig = _small(d)
    B, N = len(Uin), len(x)
    val, sca, q = [_split(a, rl.GRAD, d, B, N) for a in rl.rows(x, theta, Uin, Sig, kind, rl.GRAD)]
    C, dC, _kuu = pg.rows(x, theta, Uin, kind)
    for k, w in (("C", C[:, None, :]), ("J", -dC)):
        err, lim = np.abs(val[k] - w), 256 * EPS_LD * (1 + q[k]) * sca[k]
        assert (err <= lim).all(), (d, kind, k, float((err - lim).max()))


@pytest.mark.parametrize("kind", rl.KINDS)
@pytest.mark.parametrize("d", MODEL_D)
def test_rows_agree_with_central_differences(d, kind):
    """J_k = -d c / d u_k (step 2^-20: truncation 1e-12, rounding 1e-13 of c) and, where the kind has it, H_kk = d^2 c / d u_k^2 (step 2^-13:
    truncation 1e-8, rounding 1e-11), in long double at the inputs away from the kernel's origin"""
    x, theta, Uin, Sig = _small(d)
    Uin = Uin[[0, 3, 4, 6, 7]]                       # between, but_last, but_first, two random ones
    B, N = len(Uin), len(x)
    lay = rl.DVH if kind != 3 else rl.GRAD
    val, sca, _q = [_split(a, lay, d, B, N) for a in rl.rows(x, theta, Uin, Sig, kind, lay)]
    c_at = lambda V: rl.parts(x, theta, V, kind)["c"]  # noqa: E731  (values at exactly representable steps)
    c0 = c_at(Uin)
    for k in range(d):
        for name, h, tol in (("J", LD(2.0) ** -20, 1e-9), ("H", LD(2.0) ** -13, 1e-5)):
            if name not in val:
                continue
            e = np.zeros(d)
            e[k] = float(h)
            cp, cm = c_at(Uin + e), c_at(Uin - e)
            fd = -(cp - cm) / (2 * h) if name == "J" else (cp - 2 * c0 + cm) / (h * h)
            err, lim = np.abs(val[name][:, k] - fd), tol * (sca[name][:, k] + c0)
            assert (err <= lim).all(), (d, kind, name, k, float((err / lim).max()))


# ------------------------------------------------------------------------------------------------
# the float64 evaluations and the floors
# ------------------------------------------------------------------------------------------------
def test_float64_rows_stay_under_the_floor():
    rho, per = rl.rho_all()
    for kind in rl.KINDS:
        for lay in rl.LAYOUTS_OF[kind]:
            worst = max((r, c) for c, r in per.items() if c[2] == kind and c[3] == lay)
            print("rows %-8s %-6s rho %.3f units at N=%d d=%d" % (rl.KIND_NAMES[kind], rl.LAYOUT_NAMES[lay], worst[0], worst[1][0], worst[1][1]))
    print("rows: rho %.3f units, bound %.1f" % (rho, rl.bound()))
    assert rho <= rl.GRAM_FLOOR and rl.bound() == rl.GRAM_MARGIN * rl.GRAM_FLOOR


def _reduce_both(lay, d, npad, family, defect=None):
    Zs, y, Sig, kuu = rl.reduce_case(lay, d, npad, family)
    return rl.reduce_model(lay, d, Zs, y, Sig, kuu), rl.reduce_model(lay, d, Zs, y, Sig, kuu, dt=np.float64, defect=defect)


def test_float64_reductions_stay_under_the_floor():
    for lay in (rl.APPROX, rl.DVH, rl.GRAD):
        worst = 0.0
        for d in rl.REDUCE_D:
            for npad in rl.REDUCE_NPAD:
                for family in ("random", "cancel"):
                    want, ref = _reduce_both(lay, d, npad, family)
                    worst = max(worst, rl.rho_of({k: rl.distances(ref[k][0], want[k][0], want[k][1]) for k in want}))
        print("reduce %-6s rho_ref %.3e (floor %.3e)" % (rl.LAYOUT_NAMES[lay], worst, dl.FLOOR))
        assert worst <= dl.FLOOR


# ------------------------------------------------------------------------------------------------
# the seeded defects
# ------------------------------------------------------------------------------------------------
def _row_targets(defect):
    """the (kind, layout) pairs a defect changes"""
    every = [(k, lay) for k in rl.KINDS for lay in rl.LAYOUTS_OF[k]]
    return {"jsign": every, "exp32": every, "coord": every,
            "h_now": [(0, rl.DVH)], "h_nos": [(5, rl.DVH)], "vt_grad": [(0, rl.GRAD)],
            "tr_diag": [(0, rl.APPROX), (5, rl.APPROX)], "tr_sigma0": [(0, rl.APPROX), (5, rl.APPROX)],
            "flag0": [p for p in every if rl.has_vt(*p)], "vt_pad": [p for p in every if rl.has_vt(*p)]}[defect]


@pytest.mark.parametrize("d", [3, 9])
@pytest.mark.parametrize("defect", rl.ROW_DEFECTS)
def test_row_defects_are_rejected(defect, d):
    x, _t, theta, Uin, Sig = rl.make_case(129, d)
    lim = rl.bound()
    for kind, lay in _row_targets(defect):
        model = rl.rows(x, theta, Uin, Sig, kind, lay)
        clean = rl.units(rl.rows(x, theta, Uin, Sig, kind, lay, dt=np.float64)[0], model).max()
        bad = rl.units(rl.rows(x, theta, Uin, Sig, kind, lay, dt=np.float64, defect=defect)[0], model).max()
        print("%s %s %s d=%d: clean %.3f, with the defect %.3e units (bound %.1f)" % (defect, rl.KIND_NAMES[kind], rl.LAYOUT_NAMES[lay], d, clean, bad, lim))
        assert clean <= lim < bad, (defect, kind, lay)


@pytest.mark.parametrize("d", [8, 9])
@pytest.mark.parametrize("defect", rl.REDUCE_DEFECTS)
def test_reduce_defects_are_rejected(defect, d):
    targets = {"tail512": (rl.APPROX, rl.DVH, rl.GRAD), "quarter": (rl.APPROX, rl.DVH, rl.GRAD), "nosquare": (rl.APPROX, rl.DVH),
               "sigma0": (rl.APPROX,), "dvar1": (rl.GRAD,), "trhalf": (rl.APPROX,)}[defect]
    for lay in targets:
        want, clean = _reduce_both(lay, d, 768, "random")
        _w, bad = _reduce_both(lay, d, 768, "random", defect)
        rho = rl.rho_of({k: rl.distances(clean[k][0], want[k][0], want[k][1]) for k in want})
        rl.assert_within({k: rl.distances(clean[k][0], want[k][0], want[k][1]) for k in want}, rho)
        with pytest.raises(AssertionError):
            rl.assert_within({k: rl.distances(bad[k][0], want[k][0], want[k][1]) for k in want}, rho, defect)


# ------------------------------------------------------------------------------------------------
# the build kernels' resources
# ------------------------------------------------------------------------------------------------
# fragment of the mangled name -> (the least waves per SIMD, the most scalar registers spilled into vector lanes): the figures of the three
# separate kernel bodies that the frame replaced; the six GRAD instantiations are held by tests/test_predict_grad_model.py
BUILD_FLOORS = {"propagate.hip": {"approx_build_many_kernelILi8ELb0E": (6, 22), "approx_build_many_kernelILi0ELb0E": (7, 0),
                                  "dvh_build_many_kernelILi8E": (7, 0), "dvh_build_many_kernelILi0E": (8, 0)},
                "matern.hip": {"matern52_build_many_kernelILi8ELb0E": (7, 42), "matern52_build_many_kernelILi0ELb0E": (7, 19),
                               "matern52_build_many_kernelILi8ELb1E": (6, 24), "matern52_build_many_kernelILi0ELb1E": (6, 18)}}


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("src", sorted(BUILD_FLOORS))
def test_build_kernels_keep_everything_in_registers(src, tmp_path):
    """-Rpass-analysis=kernel-resource-usage (the recipe of tests/test_predict_grad_model.py): no scratch, no spilled vector register, an
    occupancy not below the floor of each APPROX / DVH instantiation, and no more scalar registers spilled into vector lanes than the
    separate bodies spilled (five of the eight did: 18 to 42; the other three spill none)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(PKG_PARENT, "csrc", src), "-o",
                          str(tmp_path / (src + ".o")), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" ")[0]] = int(m.group(2))
    missed = []
    for frag, (floor, sgpr_spill) in BUILD_FLOORS[src].items():
        hits = {k: u for k, u in usage.items() if frag in k}
        assert len(hits) == 1, (frag, sorted(usage))
        for k, u in hits.items():
            print(k, u, "floor", floor, "scalar spill at most", sgpr_spill)
            if not (u["ScratchSize"] == 0 and u["SGPRs"] <= sgpr_spill and u["VGPRs"] == 0 and u["Occupancy"] >= floor):
                missed.append((k, u, floor, sgpr_spill))
    assert not missed, missed
