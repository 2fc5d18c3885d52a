#!/usr/bin/env python3
"""Numerical propagation (gpx_propagate_quadrature_many) at the size the project is measured at, N = 16384, d = 8:

  (a) 4096 inputs x 16 nodes, one shared A, no density          (b) one input, order-4 Gauss-Hermite (65536 nodes), 256 y
  (c) Monte Carlo, n = 1000, 64 inputs, 64 y

each against gpx_predict on the same number of rows (same process, interleaved, --reps runs each) and against a loop of gp.estimate over
the nodes of ONE input -- the shape of the reference's evaluation (at most --loop-nodes of them are timed, the rest is scaled).  The device
time by kernel class (gpx_profile_*) of both calls: the node build is the difference of the Gram class, the mixture reduction the
difference of the reduce class.

    python3 tools/probe_quadrature.py [--n 16384] [--reps 3]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")):
    sys.path.insert(0, p)
try:
    import torch  # noqa: F401
except Exception:
    pass
import skgpuppy_amd as sk  # noqa: E402
from skgpuppy_amd import _gpx  # noqa: E402


def classes(h):
    out = {}
    for c, name in enumerate(_gpx.KERNEL_CLASS_NAMES):
        n, ms, w = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_profile_read(h, c, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w)), "gpx_profile_read")
        if n.value:
            out[name] = (n.value, ms.value)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-nodes", type=int, default=256)
    a = ap.parse_args()
    N, d = a.n, a.d
    rng = np.random.RandomState(0)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    h = gp._dev().handle
    Sigma = np.diag(np.full(d, 0.05))
    hg2, hg4, mc = sk.UncertaintyPropagationNumericalHG(gp, order=2, full_sigma=True), sk.UncertaintyPropagationNumericalHG(gp), sk.UncertaintyPropagationMC(gp, 1000, seed=1)
    z16 = hg2._rule(d)[0][:16]
    cases = [
        ("(a) 4096 inputs x 16 nodes, shared A, ny = 0", rng.uniform(2, 8, (4096, d)), hg2._root(Sigma), z16, np.full(16, 1.0 / 16), None),
        ("(b) 1 input x 65536 nodes (order 4), ny = 256", rng.uniform(2, 8, (1, d)), hg4._root(Sigma), hg4._rule(d)[0], hg4._rule(d)[1], np.linspace(-2, 2, 256)),
        ("(c) MC n = 1000, 64 inputs, ny = 64", rng.uniform(2, 8, (64, d)), mc._root(Sigma), mc._rule(d)[0], mc._rule(d)[1], np.linspace(-2, 2, 64)),
    ]
    print("N = %d, d = %d, %d runs each, interleaved; times in ms" % (N, d, a.reps))
    for tag, U, A, z, wq, Y in cases:
        U, A, z, wq = _gpx.f64(U), _gpx.f64(A), _gpx.f64(z), _gpx.f64(wq)
        B, S = len(U), len(wq)
        ny = 0 if Y is None else len(Y)
        rows = B * S
        X = (U[:, None, :] + z.dot(A.T)[None]).reshape(rows, d)
        mom, dens = np.empty((5, B)), np.empty((B, max(ny, 1)))
        pm, pv = np.empty(rows), np.empty(rows)

        def quad():
            _gpx.check(_gpx.lib.gpx_propagate_quadrature_many(h, _gpx.ptr(U), _gpx.ptr(A), 1, B, _gpx.ptr(z), _gpx.ptr(wq), S, _gpx.ptr(_gpx.f64(Y)) if ny else None,
                                                              ny, 1, gp.meant, _gpx.ptr(mom), _gpx.ptr(dens) if ny else None), "gpx_propagate_quadrature_many")

        def pred():
            _gpx.check(_gpx.lib.gpx_predict(h, _gpx.ptr(X), rows, _gpx.ptr(pm), _gpx.ptr(pv)), "gpx_predict")

        quad(), pred()                                       # warm-up: buffers, kernels
        tq, tp = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); quad(); tq.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter(); pred(); tp.append(1e3 * (time.perf_counter() - t0))
        nl = min(S, a.loop_nodes)
        tl = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for s in range(nl):
                gp.estimate(X[s])
            tl.append(1e3 * (time.perf_counter() - t0) * S / nl)
        prof = {}
        for name, f in (("quadrature", quad), ("predict", pred)):
            _gpx.lib.gpx_profile_enable(h, 2)
            _gpx.lib.gpx_profile_reset(h)
            f()
            prof[name] = classes(h)
            _gpx.lib.gpx_profile_enable(h, 0)
        # the model check: the call's mean / variance against the same mixture of gpx_predict's rows in NumPy
        m = (pm.reshape(B, S) * wq).sum(1)
        c2 = ((pm.reshape(B, S) - m[:, None]) ** 2 * wq).sum(1)
        var = (pv.reshape(B, S) * wq).sum(1) + c2
        print("\n%s: %d rows" % (tag, rows))
        print("  gpx_propagate_quadrature_many  %s  median %.2f" % (" ".join("%.2f" % v for v in tq), np.median(tq)))
        print("  gpx_predict on the same rows   %s  median %.2f   ratio %.3f" % (" ".join("%.2f" % v for v in tp), np.median(tp), np.median(tq) / np.median(tp)))
        print("  loop of gp.estimate, one input's %d nodes (%d timed, scaled)  %s  median %.1f  -> x %d inputs = %.0f ms, %.0fx the call"
              % (S, nl, " ".join("%.1f" % v for v in tl), np.median(tl), B, np.median(tl) * B, np.median(tl) * B / np.median(tq)))
        for name in ("quadrature", "predict"):
            print("  device time by class, %-10s %s" % (name, "  ".join("%s %d x %.3f" % (k, n, ms) for k, (n, ms) in sorted(prof[name].items()))))
        g = lambda p, k: p.get(k, (0, 0.0))[1]               # noqa: E731
        print("  node build (gram class difference) %.3f   mixture reduce (reduce class difference) %.3f   solve (gemm classes, quadrature) %.3f"
              % (g(prof["quadrature"], "gram") - g(prof["predict"], "gram"), g(prof["quadrature"], "predict_reduce") - g(prof["predict"], "predict_reduce"),
                 sum(ms for k, (n, ms) in prof["quadrature"].items() if k.startswith("gemm"))))
        print("  against NumPy sums of gpx_predict's rows: max |dmean| %.2e  max |dvar| %.2e" % (np.abs(mom[0] - m).max(), np.abs(mom[1] - var).max()))


if __name__ == "__main__":
    main()
