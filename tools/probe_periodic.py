#!/usr/bin/env python3
"""Timing of the PeriodicCovariance path next to the Gaussian one on the same box, runs interleaved.

    python tools/probe_periodic.py [--n 16384] [--d 8] [--m 16384] [--reps 5]

Per repetition, Gaussian and periodic alternating: the fit (wall clock around the C call, and the Gram's own time and bytes/s from the
handle's event profiler, GPX_K_GRAM), estimate_many on m queries (gpx_predict / gpx_periodic_predict, and gpx_predict_kv on the periodic
handle with the same rows precomputed by gpx_periodic_gram), one likelihood + gradient evaluation (fit + gpx_nll + gradient).  Prints the
median of each and the ratios."""
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


def fit(kind, x, t, theta, profile=0):
    h = ctypes.c_void_p()
    f = _gpx.lib.gpx_fit if kind == "gauss" else _gpx.lib.gpx_periodic_fit
    if profile:
        os.environ["GPX_PROFILE"] = "2"
    t0 = time.perf_counter()
    _gpx.check(f(_gpx.ptr(x), _gpx.ptr(t), x.shape[0], x.shape[1], _gpx.ptr(theta), None, ctypes.byref(h)), kind + " fit")
    dt = time.perf_counter() - t0
    os.environ.pop("GPX_PROFILE", None)
    return h, dt * 1e3


def gram_profile(h):
    launches, ms, work = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_profile_read(h, _gpx.K_GRAM, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work)), "profile_read")
    return ms.value, work.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.RandomState(1)
    N, d, M = a.n, a.d, a.m
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    t -= t.mean()
    xs = rng.uniform(0, 10, (M, d))
    w = rng.uniform(0.02, 0.2, d) / d
    th_g = np.log(np.concatenate([[2.0, 0.01], w + 1.0 / d]))            # (a Gaussian K as well conditioned as the periodic one)
    th_p = np.log(np.concatenate([[2.0, 0.01], w, rng.uniform(1.5, 4, d), rng.uniform(0.5, 3, d) / d]))
    res = {k: [] for k in ("fit_g", "fit_p", "gram_g", "gram_p", "pred_g", "pred_p", "pred_kv", "lik_g", "lik_p")}
    mean, var = np.empty(M), np.empty(M)
    gbytes = 0.0
    for rep in range(a.reps + 1):                                        # repetition 0 warms up (allocator, stream probe)
        row = {}
        for kind, th in (("gauss", th_g), ("per", th_p)):
            k = kind[0]
            h, _ms = fit(kind, x, t, th, profile=1)                    # (profiled: the Gram's own time only)
            g_ms, gbytes = gram_profile(h)
            row["gram_" + k] = g_ms
            _gpx.lib.gpx_profile_enable(h, 0)
            f = _gpx.lib.gpx_predict if kind == "gauss" else _gpx.lib.gpx_periodic_predict
            t0 = time.perf_counter()
            _gpx.check(f(h, _gpx.ptr(xs), M, _gpx.ptr(mean), _gpx.ptr(var)), "predict")
            row["pred_" + k] = (time.perf_counter() - t0) * 1e3
            _gpx.lib.gpx_free(h)
            # likelihood + gradient at a fresh theta: fit, nll, gradient
            g = np.empty(len(th))
            nll = ctypes.c_double()
            t0 = time.perf_counter()
            h, row["fit_" + k] = fit(kind, x, t, th)                  # (unprofiled: the fit's wall clock)
            _gpx.check(_gpx.lib.gpx_nll(h, ctypes.byref(nll)), "nll")
            fg = _gpx.lib.gpx_nll_grad if kind == "gauss" else _gpx.lib.gpx_periodic_nll_grad
            _gpx.check(fg(h, _gpx.ptr(g)), "grad")
            row["lik_" + k] = (time.perf_counter() - t0) * 1e3
            if kind == "per" and rep in (0, a.reps) and M * N * 8 <= 4 << 30:
                # gpx_predict_kv on the same rows (host matrix: its transfer is part of that route)
                kv = np.empty((M, N))
                _gpx.check(_gpx.lib.gpx_periodic_gram(_gpx.ptr(xs), M, _gpx.ptr(x), N, d, _gpx.ptr(th), -1, _gpx.ptr(kv)), "gram")
                kd = np.full(M, 2.01)
                t0 = time.perf_counter()
                _gpx.check(_gpx.lib.gpx_predict_kv(h, _gpx.ptr(kv), M, _gpx.ptr(kd), _gpx.ptr(mean), _gpx.ptr(var)), "predict_kv")
                row["pred_kv"] = (time.perf_counter() - t0) * 1e3
            _gpx.lib.gpx_free(h)
        if rep:
            for key, val in row.items():
                res[key].append(val)
        print("rep %d: " % rep + "  ".join("%s %.2f" % kv for kv in sorted(row.items())), flush=True)
    med = {k: float(np.median(v)) for k, v in res.items() if v}
    print("N=%d d=%d M=%d medians over %d reps (ms):" % (N, d, M, a.reps))
    for k in sorted(med):
        print("  %-8s %9.3f" % (k, med[k]))
    print("  Gram: gaussian %.3f ms = %.2f TB/s, periodic %.3f ms = %.2f TB/s (%.0f bytes stored)" % (
        med["gram_g"], gbytes / med["gram_g"] / 1e9, med["gram_p"], gbytes / med["gram_p"] / 1e9, gbytes))
    print("  ratios periodic / gaussian: fit %.3f  predict %.3f  likelihood+gradient %.3f  Gram %.2f" % (
        med["fit_p"] / med["fit_g"], med["pred_p"] / med["pred_g"], med["lik_p"] / med["lik_g"], med["gram_p"] / med["gram_g"]))
    if "pred_kv" in med:
        print("  gpx_periodic_predict / gpx_predict_kv (host kv): %.3f" % (med["pred_p"] / med["pred_kv"]))


if __name__ == "__main__":
    main()
