#!/usr/bin/env python
"""Timing of the second-order Sobol terms over a box (gpx_sensitivity_box_second_many) on bench.py's recipe at N = 16384, interleaved in one
process with its two yardsticks on inputs of the same centre and variance (lo, hi = u -+ sqrt(3 s)): gpx_sensitivity_box_many (total on,
quad off), the same erf-bound pair pass, and gpx_sensitivity_second_many, the same Gram frame with a plain exponential in the cell.
Needs an MI355X; no fallback.  One leg per process, each under its own time limit:

    timeout -k 10 400 python tools/probe_sensitivity_box_second.py d8  --out profiles/r30_sensitivity_box_second.txt && \\
    timeout -k 10 500 python tools/probe_sensitivity_box_second.py d16 --out profiles/r30_sensitivity_box_second.txt

Per leg, for 1 and 64 inputs after one warm round: the wall time of each call on the host clock (best and median of REPS; each call ends
in its own synchronisation), the ratio of the medians to either yardstick, and from one profiled call (gpx_profile_enable level 2: device
events) the build kernel (class approx_quad) and the pair pass (class exact_sum) of the new call apart; alongside, (pair, slot) cells per
second of the new pair pass.  Records, not thresholds."""
import argparse

import numpy as np

import probe_sensitivity as ps
from probe_sensitivity import _DeviceModel, _gpx
from probe_sensitivity_box import box
from probe_sensitivity_second import second

REPS = 5


def box_second(h, lo, hi):
    b, d = lo.shape
    out = np.empty((b, d, d))
    _gpx.check(_gpx.lib.gpx_sensitivity_box_second_many(h, _gpx.ptr(lo), _gpx.ptr(hi), 0, b, _gpx.ptr(out)), "gpx_sensitivity_box_second_many")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["d8", "d16"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("probe_sensitivity_box_second: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    d = {"d8": 8, "d16": 16}[a.leg]
    x, t, theta, U, s = ps.recipe(a.n, d, 64)
    model = _DeviceModel(x, t, theta)
    h = model.handle
    half = np.sqrt(3.0 * s)
    LO, HI = _gpx.f64(U - half), _gpx.f64(U + half)
    one, ref = box_second(h, LO[:1], HI[:1])[0], box(h, LO[:1], HI[:1], True, False)
    iu = np.triu_indices(d, 1)
    say("N=%d d=%d sanity: finite %s, symmetric %s, (sum first + sum_{k<l} second) / V = %.6f <= 1, min_k (total_k - first_k - sum_l second_kl) / V = %.3e"
        % (a.n, d, bool(np.all(np.isfinite(one))), bool(np.array_equal(one, one.T)), (ref[2][0].sum() + one[iu].sum()) / ref[1][0],
           float((ref[3][0] - ref[2][0] - one.sum(1)).min() / ref[1][0])))
    for b in (1, 64):
        lo, hi, u = LO[:b], HI[:b], U[:b]
        fns = {"box second": lambda: box_second(h, lo, hi), "box first+total": lambda: box(h, lo, hi, True, False),
               "gaussian second": lambda: second(h, u, s)}
        wall = ps.interleaved(fns, REPS)
        build, pair = ps.profiled(h, fns["box second"])
        med = {k: v[1] for k, v in wall.items()}
        say("N=%d d=%d b=%d: gpx_sensitivity_box_second_many best %.3f ms median %.3f ms | gpx_sensitivity_box_many (total on, quad off) best %.3f ms "
            "median %.3f ms: ratio of medians %.3f | gpx_sensitivity_second_many best %.3f ms median %.3f ms: ratio of medians %.2f | box second: "
            "build %.3f ms, pair pass %.3f ms, rest %.3f ms = %.3g pair-slot cells/s"
            % ((a.n, d, b) + wall["box second"] + wall["box first+total"] + (med["box second"] / med["box first+total"],) + wall["gaussian second"]
               + (med["box second"] / med["gaussian second"], build, pair, med["box second"] - build - pair,
                  0.5 * a.n * a.n * b * d / max(pair, 1e-9) * 1e3)))
    model.close()


if __name__ == "__main__":
    main()
