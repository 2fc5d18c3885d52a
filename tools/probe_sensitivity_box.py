#!/usr/bin/env python
"""Timing of the variance decomposition under uniform inputs (gpx_sensitivity_box_many) next to the Gaussian call (gpx_sensitivity_many) on
bench.py's recipe at N = 16384, d = 8.  Needs an MI355X; no fallback.  One process, under its own time limit:

    timeout -k 10 500 python tools/probe_sensitivity_box.py --out profiles/r28_sensitivity_box.txt

For b = 1 and 64 inputs, interleaved in the same process after one warm round, 3 runs each: the box call with and without the total-effect
sums and with and without quad, and the Gaussian call with and without total, on inputs of the same centre and variance (lo, hi = u -+
sqrt(3 s)): the wall time of the call on the host clock (the call ends in its own synchronisation) and, from one profiled call
(gpx_profile_enable level 2: device events), the build kernel and the pair pass apart.  The pair pass against the issue time of the vector
instructions in the compiled loops of box_pair_kernel<true, true>: --valu-slot in the rolled slot loop, summed over ALL THREE branches of
the erf difference, --valu-row per pair and sweep, x N^2 / 2 pairs / 64 lanes x 4 cycles per wave instruction on 1024 SIMDs at
--clock-ghz.  That is NOT a floor: a wave executes a branch only when one of its lanes takes it, and a pass whose pairs sit in one branch
runs below it; the count of each branch alone has not been separated.  The two counts are read off the gfx950 ISA
(hipcc --save-temps) and belong to a revision of the kernel: recount them after an edit and pass them in.  Records, not thresholds."""
import argparse

import numpy as np

import probe_sensitivity as ps
from probe_sensitivity import _DeviceModel, _gpx

REPS = 3
GAUSS_FLOOR_RATIO = 1.47   # the Gaussian pair pass against its own floor at d = 8, b = 64 (profiles/r24_sensitivity.txt)


def box(h, lo, hi, total, quad):
    b, d = lo.shape
    mean, V, first = np.empty(b), np.empty(b), np.empty((b, d))
    tot, q = (np.empty((b, d)) if total else None), (np.empty(b) if quad else None)
    _gpx.check(_gpx.lib.gpx_sensitivity_box_many(h, _gpx.ptr(lo), _gpx.ptr(hi), 0, b, _gpx.ptr(mean), _gpx.ptr(V), _gpx.ptr(first),
                                                 _gpx.ptr(tot) if total else None, _gpx.ptr(q) if quad else None), "gpx_sensitivity_box_many")
    return mean, V, first, tot, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="the clock the issue floor is computed at")
    ap.add_argument("--valu-slot", type=float, default=582.0, help="vector instructions of the slot loop, all branches of erf_diff")
    ap.add_argument("--valu-row", type=float, default=177.0, help="vector instructions per pair and sweep outside the slot loop")
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("probe_sensitivity_box: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    N, d = a.n, a.d
    x, t, theta, U, s = ps.recipe(N, d, 64)
    model = _DeviceModel(x, t, theta)
    h = model.handle
    half = np.sqrt(3.0 * s)
    LO, HI = _gpx.f64(U - half), _gpx.f64(U + half)
    out = box(h, LO[:4], HI[:4], True, True)                         # builds K^-1 as well
    say("N=%d d=%d sanity: 4 inputs finite %s, V %s, sum first / V %s, sum total / V %s, quad %s"
        % (N, d, bool(all(np.all(np.isfinite(o)) for o in out)), np.array2string(out[1], precision=4),
           np.array2string(out[2].sum(1) / out[1], precision=4), np.array2string(out[3].sum(1) / out[1], precision=4),
           np.array2string(out[4], precision=6)))
    for b in (1, 64):
        lo, hi, u = LO[:b], HI[:b], U[:b]
        fns = {"box total quad": lambda: box(h, lo, hi, True, True), "box total": lambda: box(h, lo, hi, True, False),
               "box quad": lambda: box(h, lo, hi, False, True), "box": lambda: box(h, lo, hi, False, False),
               "gaussian total": lambda: ps.sens(h, u, s, True), "gaussian": lambda: ps.sens(h, u, s, False)}
        wall = ps.interleaved(fns, REPS)
        per_pair = a.valu_slot * d + a.valu_row
        floor = per_pair * 0.5 * N * N * b / 64.0 * 4.0 / (1024.0 * a.clock_ghz * 1e9) * 1e3
        for name, fn in fns.items():
            build, pair = ps.profiled(h, fn)
            line = "N=%d d=%d b=%d %-15s: call best %.3f ms median %.3f ms | build %.3f ms, pair pass %.3f ms" % ((N, d, b, name) + wall[name] + (build, pair))
            if name == "box total quad":
                line += (" | all-branches issue time %.3f ms (%.0f vector instructions a pair at %.2f GHz; not a floor): the pass takes %.2fx of it "
                         "(the Gaussian pass: %.2fx of its one-branch floor)" % (floor, per_pair, a.clock_ghz, pair / floor, GAUSS_FLOOR_RATIO))
            say(line)
        say("N=%d d=%d b=%d: box / gaussian, both with total, best wall %.2fx" % (N, d, b, wall["box total"][0] / wall["gaussian total"][0]))
    model.close()


if __name__ == "__main__":
    main()
