"""CPU-only: the surface of the predictor's input gradients (gpx_predict_mean_grad, gpx_predict_grad, GaussianProcess.estimate_many_gradient,
UncertaintyPropagationLinear), the meaning of tests/_predict_grad_model.py -- its gradients against central differences of the oracle's
predictor, with the O(1) defects it must see planted and rejected -- and the register report of the new kernels."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_PARENT, ROOT

import skgpuppy_amd
from skgpuppy_amd import _gpx
from oracle import oracle as orc

import _predict_grad_model as pg

N, D, NQ, H = 60, 3, 5, 1e-4
RTOL, GMIN = 1e-6, 1e-3      # relative tolerance of max(|g|, GMIN): a check of meaning, the defects it must see are O(1)


# ---- surface -----------------------------------------------------------------------------------------------------
def test_symbols_header_and_signatures():
    text = open(os.path.join(ROOT, "include", "gpx.h")).read()
    for name, nargs in (("gpx_predict_mean_grad", 5), ("gpx_predict_grad", 7)):
        assert hasattr(_gpx.lib, name)
        assert re.search(r"\bint %s\(gpx_handle \*h, const double \*xs, int64_t m," % name, text)
        assert len(_gpx.SIGNATURES[name][1]) == nargs and _gpx.SIGNATURES[name][0] is ctypes.c_int
    assert "UncertaintyPropagation.py:214-227" in text and "Covariance.py:660-689" in text      # the reference lines the entries cite
    assert _gpx.lib.gpx_abi_version() == 1
    assert "#define GPX_ABI_VERSION 1" in text


def test_null_handle_is_refused_before_anything_is_written():
    xs = np.zeros((2, 3))
    outs = [np.full(6, 7.25) for _ in range(4)]
    st = _gpx.lib.gpx_predict_grad(None, _gpx.ptr(xs), 2, *[_gpx.ptr(o) for o in outs])
    assert st == _gpx.GPX_ERR_BAD_ARG and "null handle" in _gpx.last_error()
    st = _gpx.lib.gpx_predict_mean_grad(None, _gpx.ptr(xs), 2, _gpx.ptr(outs[0]), _gpx.ptr(outs[1]))
    assert st == _gpx.GPX_ERR_BAD_ARG and "null handle" in _gpx.last_error()
    for o in outs:
        assert (o == 7.25).all()


def test_python_surface():
    for m in ("estimate_many_gradient", "estimate_gradient"):
        assert callable(getattr(skgpuppy_amd.GaussianProcess, m))
    L = skgpuppy_amd.UncertaintyPropagationLinear
    assert "UncertaintyPropagationLinear" in skgpuppy_amd.__all__ and issubclass(L, skgpuppy_amd.UncertaintyPropagationGA)
    for m in ("propagate_mean", "propagate_GA", "_derivative", "propagate_GA_many", "propagate_mean_many"):
        assert callable(getattr(L, m))


# ---- meaning: the model's gradients are the derivatives of the oracle's predictor ------------------------------------
def _case():
    """N = 60 points in [0, 10]^3, v = 2, vt = 0.05, w in [0.3, 0.6] (length scales well under the cube: the variance moves by O(1) between
    the points, so both gradients are far above GMIN), five queries between the points"""
    rng = np.random.RandomState(2214)
    x = pg._grid(rng.uniform(0, 10, (N, D)))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.concatenate([[2.0, 0.05], rng.uniform(0.3, 0.6, D)]))
    return x, t, theta, pg._grid(rng.uniform(2, 8, (NQ, D)))


class _ScalarMatern(orc.OracleCovariance):
    """MaternCovariance's scalar __call__ (pure host code) under the oracle's generic operator: every matrix from N^2 scalar calls"""

    def __init__(self, nu):
        self.cov = skgpuppy_amd.MaternCovariance(nu)

    def __call__(self, xi, xj, theta):
        return self.cov(xi, xj, theta)


def _central(gp, xs):
    """central differences (h = 1e-4) of gp.estimate: (d mean [M, d], d var [M, d])"""
    dm, dv = np.empty(xs.shape), np.empty(xs.shape)
    for i, u in enumerate(xs):
        for k in range(xs.shape[1]):
            e = np.zeros(xs.shape[1])
            e[k] = H
            (m1, v1), (m0, v0) = gp.estimate(u + e), gp.estimate(u - e)
            dm[i, k], dv[i, k] = (m1 - m0) / (2 * H), (v1 - v0) / (2 * H)
    return dm, dv


_REF = {}


def _reference(nu2):
    """(x, theta, xs, alpha, Kinv, d mean, d var) of the case under the kind's oracle: computed once, shared, never changed"""
    if nu2 not in _REF:
        x, t, theta, xs = _case()
        gp = orc.OracleGP(x, t, theta) if nu2 == 0 else orc.OracleOperatorGP(x, t, _ScalarMatern(nu2 / 2.0), theta)
        dm, dv = _central(gp, xs)
        for a in (dm, dv):
            a.setflags(write=False)
        _REF[nu2] = (x, theta, xs, gp.beta(), gp.Kinv, dm, dv)
    return _REF[nu2]


def _worst(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), GMIN)))


def _model(nu2, defect=None):
    x, theta, xs, alpha, Kinv, _dm, _dv = _reference(nu2)
    return (pg.mean_grad(x, theta, alpha, xs, nu2, dt=np.float64, defect=defect)["dmean"][0],
            pg.var_grad(x, theta, Kinv, xs, nu2, dt=np.float64, defect=defect)["dvar"][0])


@pytest.mark.parametrize("nu2", pg.KINDS)
def test_model_gradients_are_central_differences_of_the_oracle(nu2):
    dm, dv = _reference(nu2)[5:]
    assert np.abs(dm).min() > GMIN and np.abs(dv).max() > 10 * GMIN        # the case exercises both gradients
    gm, gv = _model(nu2)
    print("nu2 %d: worst relative distance  d mean %.3e  d var %.3e" % (nu2, _worst(gm, dm), _worst(gv, dv)))
    assert _worst(gm, dm) <= RTOL and _worst(gv, dv) <= RTOL
    # and the long-double evaluation says the same
    x, theta, xs, alpha, Kinv = _reference(nu2)[:5]
    assert _worst(pg.mean_grad(x, theta, alpha, xs, nu2)["dmean"][0].astype(np.float64), dm) <= RTOL
    assert _worst(pg.var_grad(x, theta, Kinv, xs, nu2)["dvar"][0].astype(np.float64), dv) <= RTOL


@pytest.mark.parametrize("nu2", pg.KINDS)
@pytest.mark.parametrize("defect", pg.DEFECTS)
def test_the_check_rejects_each_planted_defect(nu2, defect):
    dm, dv = _reference(nu2)[5:]
    gm, gv = _model(nu2, defect)
    if defect != "half":                      # the factor 2 belongs to the variance alone
        assert _worst(gm, dm) > 100 * RTOL
    assert _worst(gv, dv) > 100 * RTOL


def test_model_values_are_the_oracles_and_the_quirk_is_in_C_alone():
    """mean and variance of the model are the oracle's estimate; at a query bit-equal to a training row the Matern rows carry +vt, the
    Gaussian ones do not (GaussianCovariance.cov_matrix_ij), and no gradient changes with the flag except through C in d var"""
    for nu2 in pg.KINDS:
        x, theta, xs, alpha, Kinv = _reference(nu2)[:5]
        x_, t_, _th, _xs = _case()
        gp = orc.OracleGP(x_, t_, theta) if nu2 == 0 else orc.OracleOperatorGP(x_, t_, _ScalarMatern(nu2 / 2.0), theta)
        q = np.vstack([xs[:2], x[7]])
        m = pg.mean_grad(x, theta, alpha, q, nu2, dt=np.float64)
        v = pg.var_grad(x, theta, Kinv, q, nu2, dt=np.float64)
        for i in range(3):
            mu, var = gp.estimate(q[i])
            assert m["mean"][0][i] + gp.meant == pytest.approx(mu, abs=1e-10) and v["var"][0][i] == pytest.approx(var, abs=1e-9)
        on = pg.mean_grad(x, theta, alpha, q, nu2, quirk=True, dt=np.float64)
        off = pg.mean_grad(x, theta, alpha, q, nu2, quirk=False, dt=np.float64)
        vt = np.exp(theta[1])
        assert on["mean"][0][2] - off["mean"][0][2] == pytest.approx(vt * alpha[7], rel=1e-9)
        assert (on["dmean"][0] == off["dmean"][0]).all() and (on["mean"][0][:2] == off["mean"][0][:2]).all()


# ---- the new kernels' resources --------------------------------------------------------------------------------------
NEW_KERNELS = {"predict_grad.hip": ("predict_mean_grad_kernel", "predict_mean_grad_sum_kernel", "grad_reduce_many_kernel"),
               "propagate.hip": ("approx_build_many_kernelILi8ELb1E", "approx_build_many_kernelILi0ELb1E"),
               "matern.hip": ("matern_grad_build_many_kernel",)}
COUNTS = {"predict_mean_grad_kernel": 6, "predict_mean_grad_sum_kernel": 1, "grad_reduce_many_kernel": 2, "approx_build_many_kernelILi8ELb1E": 1,
          "approx_build_many_kernelILi0ELb1E": 1, "matern_grad_build_many_kernel": 4}


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("src", sorted(NEW_KERNELS))
def test_new_kernels_keep_everything_in_registers(src, tmp_path):
    """-Rpass-analysis=kernel-resource-usage (the recipe of tests/test_kernel_resources.py): no scratch, no spilled register of either
    file, and the d <= 8 instantiations at two waves per SIMD or more"""
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
    for frag in NEW_KERNELS[src]:
        hits = {k: u for k, u in usage.items() if frag in k}
        assert len(hits) == COUNTS[frag], (frag, sorted(usage))
        for k, u in hits.items():
            print(k, u)
            assert u["ScratchSize"] == 0 and u["SGPRs"] == 0 and u["VGPRs"] == 0, (k, u)
            if "ILi8E" in k:
                assert u["Occupancy"] >= 2, (k, u)
