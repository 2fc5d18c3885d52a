#!/usr/bin/env python
"""Timing of the full ANOVA decomposition (gpx_sensitivity_anova_many) on bench.py's recipe at N = 16384, interleaved in one process with
gpx_sensitivity_second_many and gpx_sensitivity_many (total-effect sums on) at the same arguments.  Needs an MI355X; no fallback.  One leg
per process, each under its own time limit:

    timeout -k 10 400 python tools/probe_sensitivity_anova.py d8  --out profiles/r34_sensitivity_anova.txt && \\
    timeout -k 10 400 python tools/probe_sensitivity_anova.py d10 --out profiles/r34_sensitivity_anova.txt && \\
    timeout -k 10 400 python tools/probe_sensitivity_anova.py d9  --out profiles/r34_sensitivity_anova.txt

Per leg, for 1 and 64 inputs after one warm round: the wall time of the three calls on the host clock (best and median of REPS; each call
ends in its own synchronisation), the ratios, and from one profiled call (gpx_profile_enable level 2: device events) the build kernel
(class approx_quad) and the pair pass (class exact_sum) of the new call apart, the remainder being the column sums, copies and the host
scatter; alongside, (pair, slot) exponentials per second of the new pair pass.  Records, not thresholds."""
import argparse
import time

import numpy as np

from probe_sensitivity import _DeviceModel, _gpx, profiled, recipe, sens
from probe_sensitivity_second import second

REPS = 5


def anova(h, U, s):
    b, d = U.shape
    out = np.empty((b, 1 << d))
    _gpx.check(_gpx.lib.gpx_sensitivity_anova_many(h, _gpx.ptr(U), _gpx.ptr(s), 1, b, _gpx.ptr(out), 1 << d), "gpx_sensitivity_anova_many")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["d8", "d9", "d10"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("probe_sensitivity_anova: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    d = int(a.leg[1:])
    x, t, theta, U, s = recipe(a.n, d, 64)
    model = _DeviceModel(x, t, theta)
    h = model.handle
    one, ref, sec = anova(h, U[:1], s)[0], sens(h, U[:1], s, True), second(h, U[:1], s)[0]
    V, masks = ref[1][0], np.arange(1 << d)
    order = np.array([bin(m).count("1") for m in masks])
    tot = np.array([one[(masks >> k & 1) == 1].sum() for k in range(d)])
    say("N=%d d=%d sanity: finite %s, sum D_S / V - 1 = %.3e, max_k |D_k - first_k| / V = %.3e, max_kl |D_kl - second_kl| / V = %.3e, "
        "max_k |sum_{S has k} D_S - total_k| / V = %.3e; share of V by order 1..%d: %s"
        % (a.n, d, bool(np.all(np.isfinite(one))), one.sum() / V - 1, float(np.abs(one[1 << np.arange(d)] - ref[2][0]).max() / V),
           max(abs(one[1 << k | 1 << l] - sec[k, l]) for k in range(d) for l in range(k)) / V, float(np.abs(tot - ref[3][0]).max() / V), d,
           " ".join("%.3e" % (one[order == o].sum() / V) for o in range(1, d + 1))))
    for b in (1, 64):
        fns = {"anova": lambda: anova(h, U[:b], s), "second": lambda: second(h, U[:b], s), "first+total": lambda: sens(h, U[:b], s, True)}
        ts = {k: [] for k in fns}
        for rep in range(REPS + 1):
            for k, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
        build, pair = profiled(h, fns["anova"])
        best = {k: min(v) for k, v in ts.items()}
        say("N=%d d=%d b=%d: gpx_sensitivity_anova_many best %.3f ms median %.3f ms | gpx_sensitivity_second_many best %.3f ms median %.3f ms | "
            "gpx_sensitivity_many (total on) best %.3f ms median %.3f ms | anova / second %.3f, anova / first+total %.3f | anova: build %.3f ms, "
            "pair pass %.3f ms, rest %.3f ms = %.3g pair-slot exponentials/s"
            % (a.n, d, b, best["anova"], float(np.median(ts["anova"])), best["second"], float(np.median(ts["second"])), best["first+total"],
               float(np.median(ts["first+total"])), best["anova"] / best["second"], best["anova"] / best["first+total"], build, pair,
               best["anova"] - build - pair, 0.5 * a.n * a.n * b * d / max(pair, 1e-9) * 1e3))
    model.close()


if __name__ == "__main__":
    main()
