#!/usr/bin/env python3
"""Timing of the MaternCovariance path next to the Gaussian AND the periodic one on the same box, runs interleaved.

    python tools/probe_matern.py [--n 16384] [--d 8] [--m 16384] [--b 4096] [--reps 5]

Per repetition, the kinds alternating (gauss, per, mat5 = Matern 5/2, mat3 = Matern 3/2): the fit (wall clock around the C call, and the
Gram's own time and bytes/s from the handle's event profiler, GPX_K_GRAM), estimate_many on m queries, one likelihood + gradient
evaluation (fit + gpx_nll + gradient); and for gauss and mat5 the batched propagation calls behind propagate_GA_many
(gpx_*propagate_approx_many) and get_best_solution_many (gpx_*propagate_dvh_many) on the same b inputs.  Prints the median of each and
the ratios."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scikit-gpuppy_amd"))
try:
    import torch  # noqa: F401  (one libamdhip64 for both)
except Exception:
    pass
from skgpuppy_amd import _gpx  # noqa: E402

KINDS = ("gauss", "per", "mat5", "mat3")
lib = _gpx.lib


def fit(kind, x, t, theta, profile=0):
    h = ctypes.c_void_p()
    if profile:
        os.environ["GPX_PROFILE"] = "2"
    args = (_gpx.ptr(x), _gpx.ptr(t), x.shape[0], x.shape[1], _gpx.ptr(theta))
    t0 = time.perf_counter()
    if kind == "gauss":
        st = lib.gpx_fit(*args, None, ctypes.byref(h))
    elif kind == "per":
        st = lib.gpx_periodic_fit(*args, None, ctypes.byref(h))
    else:
        st = lib.gpx_matern_fit(*args, int(kind[3]), None, ctypes.byref(h))
    _gpx.check(st, kind + " fit")
    dt = time.perf_counter() - t0
    os.environ.pop("GPX_PROFILE", None)
    return h, dt * 1e3


def gram_profile(h):
    launches, ms, work = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    _gpx.check(lib.gpx_profile_read(h, _gpx.K_GRAM, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work)), "profile_read")
    return ms.value, work.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--b", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.RandomState(1)
    N, d, M, B = a.n, a.d, a.m, a.b
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    t -= t.mean()
    xs = rng.uniform(0, 10, (M, d))
    U = rng.uniform(0, 10, (B, d))
    A = rng.uniform(-0.1, 0.1, (d, d))
    Sigma = np.ascontiguousarray(A.dot(A.T) + 0.005 * np.eye(d))
    w = rng.uniform(0.02, 0.2, d) / d
    theta = {"gauss": np.log(np.concatenate([[2.0, 0.01], w + 1.0 / d])),            # (tools/probe_periodic.py's two models)
             "per": np.log(np.concatenate([[2.0, 0.01], w, rng.uniform(1.5, 4, d), rng.uniform(0.5, 3, d) / d])),
             "mat5": np.log(np.concatenate([[2.0, 0.01], w])), "mat3": np.log(np.concatenate([[2.0, 0.01], w]))}
    predict = {"gauss": lib.gpx_predict, "per": lib.gpx_periodic_predict, "mat5": lib.gpx_matern_predict, "mat3": lib.gpx_matern_predict}
    grad = {"gauss": lib.gpx_nll_grad, "per": lib.gpx_periodic_nll_grad, "mat5": lib.gpx_matern_nll_grad, "mat3": lib.gpx_matern_nll_grad}
    approx = {"gauss": lib.gpx_propagate_approx_many, "mat5": lib.gpx_matern_propagate_approx_many}
    dvh = {"gauss": lib.gpx_propagate_dvh_many, "mat5": lib.gpx_matern_propagate_dvh_many}
    res = {}
    mean, var = np.empty(M), np.empty(M)
    out4 = [np.empty(B) for _ in range(4)]
    dv, s2 = np.empty((B, d)), np.empty(B)
    gbytes = 0.0
    for rep in range(a.reps + 1):                                        # repetition 0 warms up (allocator, stream probe)
        row = {}
        for kind in KINDS:
            th = theta[kind]
            h, _ms = fit(kind, x, t, th, profile=1)                    # (profiled: the Gram's own time only)
            row["gram_" + kind], gbytes = gram_profile(h)
            lib.gpx_profile_enable(h, 0)
            t0 = time.perf_counter()
            _gpx.check(predict[kind](h, _gpx.ptr(xs), M, _gpx.ptr(mean), _gpx.ptr(var)), "predict")
            row["pred_" + kind] = (time.perf_counter() - t0) * 1e3
            if kind in approx:
                t0 = time.perf_counter()
                _gpx.check(approx[kind](h, _gpx.ptr(U), _gpx.ptr(Sigma), 1, B, *[_gpx.ptr(o) for o in out4]), "approx_many")
                row["ga_many_" + kind] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                _gpx.check(dvh[kind](h, _gpx.ptr(U), B, _gpx.ptr(dv), _gpx.ptr(s2)), "dvh_many")
                row["dvh_many_" + kind] = (time.perf_counter() - t0) * 1e3
            jit = ctypes.c_double()
            lib.gpx_jitter_used(h, ctypes.byref(jit))
            if jit.value:
                print("  (%s: the fit used jitter %g)" % (kind, jit.value))
            lib.gpx_free(h)
            # likelihood + gradient at a fresh theta: fit, nll, gradient
            g = np.empty(len(th))
            nll = ctypes.c_double()
            t0 = time.perf_counter()
            h, row["fit_" + kind] = fit(kind, x, t, th)                # (unprofiled: the fit's wall clock)
            _gpx.check(lib.gpx_nll(h, ctypes.byref(nll)), "nll")
            _gpx.check(grad[kind](h, _gpx.ptr(g)), "grad")
            row["lik_" + kind] = (time.perf_counter() - t0) * 1e3
            lib.gpx_free(h)
        if rep:
            for key, val in row.items():
                res.setdefault(key, []).append(val)
        print("rep %d: " % rep + "  ".join("%s %.2f" % kv for kv in sorted(row.items())), flush=True)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print("N=%d d=%d M=%d B=%d medians over %d reps (ms):" % (N, d, M, B, a.reps))
    for k in sorted(med):
        print("  %-16s %9.3f" % (k, med[k]))
    print("  Gram (%.0f bytes stored): " % gbytes + ", ".join("%s %.3f ms = %.2f TB/s" % (k, med["gram_" + k], gbytes / med["gram_" + k] / 1e9) for k in KINDS))
    for k in ("mat5", "mat3"):
        for base in ("gauss", "per"):
            print("  ratios %s / %s: fit %.3f  predict %.3f  likelihood+gradient %.3f  Gram %.2f" % (
                k, base, med["fit_" + k] / med["fit_" + base], med["pred_" + k] / med["pred_" + base], med["lik_" + k] / med["lik_" + base],
                med["gram_" + k] / med["gram_" + base]))
    print("  ratios mat5 / gauss on the same %d inputs: propagate_GA_many %.3f  get_best_solution_many (dvh) %.3f" % (
        B, med["ga_many_mat5"] / med["ga_many_gauss"], med["dvh_many_mat5"] / med["dvh_many_gauss"]))


if __name__ == "__main__":
    main()
