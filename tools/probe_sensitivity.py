#!/usr/bin/env python
"""Timing of the variance decomposition of the predictor mean (gpx_sensitivity_many) on bench.py's recipe at N = 16384.  Needs an MI355X;
no fallback.  One leg per process; run each under its own time limit and chain them:

    timeout -k 10 400 python tools/probe_sensitivity.py d8  --out profiles/r24_sensitivity.txt && \\
    timeout -k 10 300 python tools/probe_sensitivity.py d2  --out profiles/r24_sensitivity.txt && \\
    timeout -k 10 300 python tools/probe_sensitivity.py d16 --out profiles/r24_sensitivity.txt

  d8   1, 64 and 1024 inputs, each with and without the total-effect sums; against them, interleaved in the same process, ONE
       gpx_propagate_exact call with K^-1 resident and gpx_propagate_exact_many on the same inputs (one shared diagonal Sigma)
  d2   64 inputs
  d16  64 inputs

Per shape, after one warm call: the wall time of the call on the host clock (best and median of REPS; the call ends in its own
synchronisation) and, from one profiled call (gpx_profile_enable level 2: device events), the build kernel (class approx_quad) and the pair
pass (class exact_sum) apart.  Alongside: pairs x slots exponentials per second of the pair pass, and the pass against its issue floor --
the vector instructions per pair counted in the compiled inner loops (VALU_OUT per pair and slot outside the sweep, VALU_OWN per pair and
own slot, VALU_ROW per pair and sweep with the total-effect sums, from the disassembly of sens_pair_kernel<true>) x N^2 / 2 pairs / 64 lanes x 4 cycles per wave instruction
(profiles/r03_probe_fp64_instruction_latency.txt: 3.3 - 4.6) on 1024 SIMDs at --clock-ghz.  Records, not thresholds."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

try:
    import torch  # noqa: F401  (its HIP runtime first: one libamdhip64 in the process)
except Exception:
    pass
from skgpuppy_amd import _gpx  # noqa: E402
from skgpuppy_amd.GaussianProcess import _DeviceModel  # noqa: E402

REPS = 5
KC = 8                 # SEN_KC of sensitivity.hip
VALU_OUT = 26.25       # 210 vector instructions for 8 rows x 1 slot in the loop over the slots outside the sweep
VALU_OWN = 43.0        # per own slot (argument, exponential, E - m, the first-order accumulation)
VALU_ROW = 85.0        # per pair and sweep: the prefix / suffix products of the own E and the total-effect and V accumulations


def recipe(N, d, b):
    """bench.py's data law; the inputs inside the data"""
    rng = np.random.RandomState(20240 + N + d)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.array([2.0, 0.01] + [0.04] * d))
    U = rng.uniform(1, 9, (b, d))
    s = rng.uniform(0.05, 0.5, d)
    return _gpx.f64(x), _gpx.f64(t - t.mean()), _gpx.f64(theta), _gpx.f64(U), _gpx.f64(s)


def sens(h, U, s, total):
    b, d = U.shape
    mean, V, first = np.empty(b), np.empty(b), np.empty((b, d))
    tot = np.empty((b, d)) if total else None
    _gpx.check(_gpx.lib.gpx_sensitivity_many(h, _gpx.ptr(U), _gpx.ptr(s), 1, b, _gpx.ptr(mean), _gpx.ptr(V), _gpx.ptr(first),
                                             _gpx.ptr(tot) if total else None), "gpx_sensitivity_many")
    return mean, V, first, tot


def exact_many(h, U, S):
    mean, var = np.empty(len(U)), np.empty(len(U))
    _gpx.check(_gpx.lib.gpx_propagate_exact_many(h, _gpx.ptr(U), _gpx.ptr(S), 1, len(U), _gpx.ptr(mean), _gpx.ptr(var)), "gpx_propagate_exact_many")
    return mean, var


def exact_one(h, u, S):
    m, v = ctypes.c_double(), ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_propagate_exact(h, _gpx.ptr(u), _gpx.ptr(S), ctypes.byref(m), ctypes.byref(v)), "gpx_propagate_exact")
    return m.value, v.value


def interleaved(fns, reps=REPS):
    """{name: (best ms, median ms)} of the calls run in turn, after one warm round"""
    ts = {k: [] for k in fns}
    for rep in range(reps + 1):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (min(v), float(np.median(v))) for k, v in ts.items()}


def profiled(h, fn):
    """(build ms, pair ms) of one call from device events"""
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 2), "gpx_profile_enable")
    _gpx.check(_gpx.lib.gpx_profile_reset(h), "gpx_profile_reset")
    fn()
    out = []
    for cls in (_gpx.K_QUAD, _gpx.K_EXACT):
        n, ms, w = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_profile_read(h, cls, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w)), "gpx_profile_read")
        out.append(ms.value)
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 0), "gpx_profile_enable")
    return out


def floor_ms(N, d, b, ghz):
    sweeps = (d + KC - 1) // KC
    per_pair = sum(VALU_OUT * (d - min(KC, d - y * KC)) + VALU_OWN * min(KC, d - y * KC) + VALU_ROW for y in range(sweeps))
    return per_pair * 0.5 * N * N * b / 64.0 * 4.0 / (1024.0 * ghz * 1e9) * 1e3, per_pair   # 64 pairs a wave instruction


def shape(say, model, N, d, U, s, ghz, against_exact):
    h, b = model.handle, len(U)
    fns = {"with total": lambda: sens(h, U, s, True), "without total": lambda: sens(h, U, s, False)}
    if against_exact:
        S = _gpx.f64(np.diag(s))
        exact_many(h, U[:1], S)                                     # builds K^-1
        fns["gpx_propagate_exact_many"] = lambda: exact_many(h, U, S)
        fns["one gpx_propagate_exact"] = lambda: exact_one(h, U[0], S)
    wall = interleaved(fns, REPS if b < 1024 else 3)
    sweeps = (d + KC - 1) // KC
    for name, total in (("with total", True), ("without total", False)):
        build, pair = profiled(h, lambda: sens(h, U, s, total))
        line = ("N=%d d=%d b=%d %-13s: call best %.3f ms median %.3f ms = %.1f us an input | build %.3f ms, pair pass %.3f ms = %.3g pair-slot "
                "exponentials/s" % (N, d, b, name, wall[name][0], wall[name][1], 1e3 * wall[name][0] / b, build, pair,
                                     0.5 * N * N * b * d * sweeps / max(pair, 1e-9) * 1e3))
        if total:
            fl, per_pair = floor_ms(N, d, b, ghz)
            line += " | issue floor %.3f ms (%.0f vector instructions a pair at %.2f GHz): the pass takes %.2fx of it" % (fl, per_pair, ghz, pair / fl)
        say(line)
    if against_exact:
        say("N=%d d=%d b=%d on the same box, interleaved: gpx_propagate_exact_many best %.3f ms median %.3f ms; one gpx_propagate_exact (K^-1 "
            "resident) best %.3f ms median %.3f ms" % ((N, d, b) + wall["gpx_propagate_exact_many"] + wall["one gpx_propagate_exact"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["d8", "d2", "d16"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="the clock the issue floor is computed at")
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("probe_sensitivity: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    d = {"d8": 8, "d2": 2, "d16": 16}[a.leg]
    x, t, theta, U, s = recipe(a.n, d, 1024 if a.leg == "d8" else 64)
    model = _DeviceModel(x, t, theta)
    out = sens(model.handle, U[:4], s, True)
    say("N=%d d=%d sanity: 4 inputs finite %s, V %s, sum first / V %s, sum total / V %s"
        % (a.n, d, bool(all(np.all(np.isfinite(o)) for o in out)), np.array2string(out[1], precision=4),
           np.array2string(out[2].sum(1) / out[1], precision=4), np.array2string(out[3].sum(1) / out[1], precision=4)))
    for b in ((1, 64, 1024) if a.leg == "d8" else (64,)):
        shape(say, model, a.n, d, U[:b], s, a.clock_ghz, a.leg == "d8")
    model.close()


if __name__ == "__main__":
    main()
