#!/usr/bin/env python3
"""Batched inverse propagation at C3 size (N = 16384, d = 8, B = 4096 operating points) on one GPU, three interleaved repetitions in one
process after a warm-up, wall time around each call with the device idle before and after (as bench.py times gpx_predict):

  many     ONE gpx_propagate_dvh_many call, device pointers in and out
  predict  gpx_predict with M = B (2 d + 1) queries: the same solver on the same number of rows
  loop     what the call replaces: InverseUncertaintyPropagationApprox.get_best_solution point by point with K^-1 already resident (the
           loop's best case), over min(B, 512) points and scaled to B.  c = I = 1, target 3 > v + vt >= sigma2, so only a point with
           a dvh_k <= 0 has no solution: there get_best_solution asserts (counted) and get_best_solution_many returns a NaN row

then the per-class device times of one batched call (gpx_profile_read: build = gram, solve = gemm + gemm_emu, reduce), and the worst
difference between the batched dvh / sigma2 / solution and the single calls' over the loop's points."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scikit-gpuppy_amd"))
import torch  # noqa: E402
import skgpuppy_amd as sk  # noqa: E402
from skgpuppy_amd import _gpx  # noqa: E402

lib = _gpx.lib
N, d, B = 16384, 8, int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = 3
TARGET = 3.0
rng = np.random.RandomState(20240 + N + d)
x = rng.uniform(0, 10, (N, d))
t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
U = rng.uniform(0, 10, (B, d))
U[::37] = x[rng.randint(0, N, len(U[::37]))]
M = B * (2 * d + 1)
NL = min(B, 512)
xs = rng.uniform(0, 10, (M, d))

dev = torch.device("cuda")
print("device: %s" % torch.cuda.get_device_name(0))
print("N=%d d=%d B=%d  (solver rows B (2 d + 1) = %d)  GPX_EMU_F64=%s" % (N, d, B, M, os.environ.get("GPX_EMU_F64", "1")))
gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
h = gp._dev().handle
vp = lambda tt: ctypes.c_void_p(tt.data_ptr())  # noqa: E731
Ud, xsd = torch.as_tensor(U).to(dev), torch.as_tensor(xs).to(dev)
dvh_d = torch.empty((B, d), dtype=torch.float64, device=dev)
s2_d = torch.empty(B, dtype=torch.float64, device=dev)
pm_d, pv_d = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)


def many():
    _gpx.check(lib.gpx_propagate_dvh_many(h, vp(Ud), B, vp(dvh_d), vp(s2_d)), "gpx_propagate_dvh_many")


def predict():
    _gpx.check(lib.gpx_predict(h, vp(xsd), M, vp(pm_d), vp(pv_d)), "gpx_predict")


one = np.ones(d)
loop_sol = np.full((NL, d), np.nan)
refused = [0]


def loop():
    refused[0] = 0
    with np.errstate(invalid="ignore"):                  # (the square root of a negative dvh, just before the assert)
        for i in range(NL):
            try:
                loop_sol[i] = sk.InverseUncertaintyPropagationApprox(TARGET, gp, U[i], one, one).get_best_solution()
            except AssertionError:
                loop_sol[i] = np.nan
                refused[0] += 1


def timed(f):
    torch.cuda.synchronize()
    a = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - a) * 1e3


sk.UncertaintyPropagationExact(gp).propagate_GA(U[1], 0.01 * np.eye(d))     # materialises K^-1: every single call below is one pass over it
many(); predict()                                                            # warm-up (buffers from the pool, kernels loaded)
for i in range(4):
    sk.UncertaintyPropagationApprox(gp)._get_variance_dv_h(U[i], 0)
best = {}
for r in range(REPS):
    row = {"many": timed(many), "predict": timed(predict), "loop": timed(loop)}
    print("rep %d: many %9.3f ms   predict(M=%d) %9.3f ms   loop of get_best_solution over %d points %9.1f ms"
          % (r + 1, row["many"], M, row["predict"], NL, row["loop"]), flush=True)
    for k, v in row.items():
        best[k] = min(best.get(k, v), v)
loop_scaled = best["loop"] * B / NL
print("best:  many %.3f ms = %.2f us per point = %.0f points/s" % (best["many"], best["many"] * 1e3 / B, B / best["many"] * 1e3))
print("       loop %.1f ms over %d points = %.1f us per point = %.0f points/s, scaled to B: %.1f ms   (%d of %d points refused by its assert)"
      % (best["loop"], NL, best["loop"] * 1e3 / NL, NL / best["loop"] * 1e3, loop_scaled, refused[0], NL))
print("ratio: batched / loop of get_best_solution (K^-1 resident)                = %.2fx points per second   [required >= 5]"
      % (loop_scaled / best["many"]))
print("ratio: batched time / gpx_predict time on the same number of rows         = %.3f   [required <= 1.25]" % (best["many"] / best["predict"]))

dvh, s2 = dvh_d.cpu().numpy(), s2_d.cpu().numpy()
up = sk.UncertaintyPropagationApprox(gp)
ddvh = ds2 = 0.0
for i in range(NL):
    ddvh = max(ddvh, np.abs(np.array([up._get_variance_dv_h(U[i], k) for k in range(d)]) - dvh[i]).max())
    ds2 = max(ds2, abs(up._get_sigma2(U[i]) - s2[i]))
print("worst |batched - loop| over %d points: dvh %.3e  sigma2 %.3e   (bound rtol 2e-6 + 4e-8 / 4e-8)" % (NL, ddvh, ds2))
sol = sk.InverseUncertaintyPropagationApprox._closed_form(dvh, s2, one, one, [], TARGET)
both = np.isfinite(loop_sol).all(1) & np.isfinite(sol[:NL]).all(1)
print("solutions: %d NaN rows of %d in the batch; over the loop's points %d rows where exactly one side has no solution, worst relative "
      "difference of the others %.3e" % (np.isnan(sol).any(1).sum(), B, (np.isfinite(loop_sol).all(1) != np.isfinite(sol[:NL]).all(1)).sum(),
                                         (np.abs(sol[:NL][both] - loop_sol[both]) / loop_sol[both]).max()))

names = {_gpx.K_GRAM: "build (gram class)", _gpx.K_GEMM: "solve: fp64 products", _gpx.K_GEMM_SMALL: "solve: fp64 products, small tiles",
         _gpx.K_GEMM_EMU: "solve: emulated updates", _gpx.K_REDUCE: "reduce"}
for label, f in (("gpx_propagate_dvh_many", many), ("gpx_predict, M = %d" % M, predict)):
    lib.gpx_profile_enable(h, 2)
    lib.gpx_profile_reset(h)
    f()
    print("device time by kernel class, one %s call:" % label)
    for k, nm in names.items():
        n_, ms_, w_ = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        lib.gpx_profile_read(h, k, ctypes.byref(n_), ctypes.byref(ms_), ctypes.byref(w_))
        if n_.value:
            print("   %-36s %4d launches %9.3f ms" % (nm, n_.value, ms_.value))
    lib.gpx_profile_enable(h, 0)
gp._dev().close()
