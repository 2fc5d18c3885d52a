#!/usr/bin/env python
"""Timing of the second-order Sobol terms (gpx_sensitivity_second_many) on bench.py's recipe at N = 16384, interleaved in one process with
gpx_sensitivity_many (total-effect sums on) at the same arguments.  Needs an MI355X; no fallback.  One leg per process, each under its
own time limit:

    timeout -k 10 400 python tools/probe_sensitivity_second.py d8  --out profiles/r29_sensitivity_second.txt && \\
    timeout -k 10 400 python tools/probe_sensitivity_second.py d16 --out profiles/r29_sensitivity_second.txt

Per leg, for 1 and 64 inputs after one warm round: the wall time of either call on the host clock (best and median of REPS; each call ends
in its own synchronisation), their ratio, and from one profiled call (gpx_profile_enable level 2: device events) the build kernel (class
approx_quad) and the pair pass (class exact_sum) of the new call apart, the remainder being the column sums, copies and the host scatter;
alongside, (pair, slot) exponentials per second of the new pair pass.  Records, not thresholds."""
import argparse
import time

import numpy as np

from probe_sensitivity import _DeviceModel, _gpx, profiled, recipe, sens

REPS = 5


def second(h, U, s):
    b, d = U.shape
    out = np.empty((b, d, d))
    _gpx.check(_gpx.lib.gpx_sensitivity_second_many(h, _gpx.ptr(U), _gpx.ptr(s), 1, b, _gpx.ptr(out)), "gpx_sensitivity_second_many")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["d8", "d16"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("probe_sensitivity_second: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    d = {"d8": 8, "d16": 16}[a.leg]
    x, t, theta, U, s = recipe(a.n, d, 64)
    model = _DeviceModel(x, t, theta)
    h = model.handle
    one, ref = second(h, U[:1], s)[0], sens(h, U[:1], s, True)
    iu = np.triu_indices(d, 1)
    say("N=%d d=%d sanity: finite %s, symmetric %s, (sum first + sum_{k<l} second) / V = %.6f <= 1, min_k (total_k - first_k - sum_l second_kl) / V = %.3e"
        % (a.n, d, bool(np.all(np.isfinite(one))), bool(np.array_equal(one, one.T)), (ref[2][0].sum() + one[iu].sum()) / ref[1][0],
           float((ref[3][0] - ref[2][0] - one.sum(1)).min() / ref[1][0])))
    for b in (1, 64):
        fns = {"second": lambda: second(h, U[:b], s), "first+total": lambda: sens(h, U[:b], s, True)}
        ts = {k: [] for k in fns}
        for rep in range(REPS + 1):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        build, pair = profiled(h, fns["second"])
        best = {k: min(v) for k, v in ts.items()}
        say("N=%d d=%d b=%d: gpx_sensitivity_second_many best %.3f ms median %.3f ms | gpx_sensitivity_many (total on) best %.3f ms median %.3f ms | "
            "ratio %.3f | second: build %.3f ms, pair pass %.3f ms, rest %.3f ms = %.3g pair-slot exponentials/s"
            % (a.n, d, b, best["second"], float(np.median(ts["second"])), best["first+total"], float(np.median(ts["first+total"])),
               best["second"] / best["first+total"], build, pair, best["second"] - build - pair, 0.5 * a.n * a.n * b * d / max(pair, 1e-9) * 1e3))
    model.close()


if __name__ == "__main__":
    main()
