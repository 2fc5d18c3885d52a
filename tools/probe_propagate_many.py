#!/usr/bin/env python3
"""Batched Approx propagation at C3 size (N = 16384, d = 8, B = 4096 inputs, full Sigma per input) on one GPU, three interleaved
repetitions in one process after a warm-up, wall time around each call with the device idle before and after (as bench.py times
gpx_predict):

  many     ONE gpx_propagate_approx_many call, device pointers in and out
  predict  gpx_predict with M = B (d + 2) queries: the same solver on the same number of rows
  loop     what the call replaces: propagate_GA input by input with K^-1 already resident (the loop's best case), through the Python
           class and through the C entry point itself

then the per-class device times of one batched call (gpx_profile_read: build = gram, solve = gemm + gemm_emu, reduce) and the worst
difference between the batched results and the loop's over all B inputs."""
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
rng = np.random.RandomState(20240 + N + d)
x = rng.uniform(0, 10, (N, d))
t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
U = rng.uniform(0, 10, (B, d))
U[::37] = x[rng.randint(0, N, len(U[::37]))]
A = rng.uniform(-0.1, 0.1, (B, d, d))
S = np.ascontiguousarray(np.einsum("bij,bkj->bik", A, A) + 0.005 * np.eye(d))
M = B * (d + 2)
xs = rng.uniform(0, 10, (M, d))

dev = torch.device("cuda")
print("device: %s" % torch.cuda.get_device_name(0))
print("N=%d d=%d B=%d  (solver rows B (d + 2) = %d)  GPX_EMU_F64=%s" % (N, d, B, M, os.environ.get("GPX_EMU_F64", "1")))
gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
h = gp._dev().handle
vp = lambda tt: ctypes.c_void_p(tt.data_ptr())  # noqa: E731
Ud, Sd, xsd = torch.as_tensor(U).to(dev), torch.as_tensor(S).to(dev), torch.as_tensor(xs).to(dev)
out_d = [torch.empty(B, dtype=torch.float64, device=dev) for _ in range(4)]
pm_d, pv_d = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)


def many():
    _gpx.check(lib.gpx_propagate_approx_many(h, vp(Ud), vp(Sd), 0, B, *[vp(o) for o in out_d]), "gpx_propagate_approx_many")


def predict():
    _gpx.check(lib.gpx_predict(h, vp(xsd), M, vp(pm_d), vp(pv_d)), "gpx_predict")


up = sk.UncertaintyPropagationApprox(gp)
loop_mean, loop_var = np.empty(B), np.empty(B)


def loop_python():
    for i in range(B):
        loop_mean[i], loop_var[i] = up.propagate_GA(U[i], S[i])


def loop_c():
    o = [ctypes.c_double() for _ in range(4)]
    refs = [ctypes.byref(v) for v in o]
    for i in range(B):
        lib.gpx_propagate_approx(h, _gpx.ptr(U[i]), _gpx.ptr(S[i]), *refs)


def timed(f):
    torch.cuda.synchronize()
    a = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - a) * 1e3


sk.UncertaintyPropagationExact(gp).propagate_GA(U[1], S[1])     # materialises K^-1: every single call below is one pass over it
many(); predict()                                                 # warm-up (buffers from the pool, kernels loaded)
for i in range(4):
    up.propagate_GA(U[i], S[i])
best = {}
for r in range(REPS):
    row = {"many": timed(many), "predict": timed(predict), "loop_python": timed(loop_python), "loop_c": timed(loop_c)}
    print("rep %d: many %9.3f ms   predict(M=%d) %9.3f ms   loop (Python class) %9.1f ms   loop (C entry point) %9.1f ms"
          % (r + 1, row["many"], M, row["predict"], row["loop_python"], row["loop_c"]), flush=True)
    for k, v in row.items():
        best[k] = min(best.get(k, v), v)
print("best:  many %.3f ms = %.2f us per input = %.0f propagations/s" % (best["many"], best["many"] * 1e3 / B, B / best["many"] * 1e3))
print("       loop, Python class %.1f ms = %.0f propagations/s ; C entry point %.1f ms = %.0f propagations/s"
      % (best["loop_python"], B / best["loop_python"] * 1e3, best["loop_c"], B / best["loop_c"] * 1e3))
print("ratio: batched / loop of propagate_GA (Python class, K^-1 resident) = %.2fx propagations per second   [required >= 5]"
      % (best["loop_python"] / best["many"]))
print("       batched / loop of gpx_propagate_approx (C, K^-1 resident)     = %.2fx" % (best["loop_c"] / best["many"]))
print("ratio: batched time / gpx_predict time on the same number of rows    = %.3f   [required <= 1.25]" % (best["many"] / best["predict"]))

mean = out_d[0].cpu().numpy() + gp.meant
var = out_d[1].cpu().numpy()
print("worst |batched - loop| over all %d inputs: mean %.3e  variance %.3e   (bound 2e-9 / 4e-8)"
      % (B, np.abs(mean - loop_mean).max(), np.abs(var - loop_var).max()))

names = {_gpx.K_GRAM: "build (gram class)", _gpx.K_GEMM: "solve: fp64 products", _gpx.K_GEMM_SMALL: "solve: fp64 products, small tiles",
         _gpx.K_GEMM_EMU: "solve: emulated updates", _gpx.K_REDUCE: "reduce"}
for label, f in (("gpx_propagate_approx_many", many), ("gpx_predict, M = %d" % M, predict)):
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
