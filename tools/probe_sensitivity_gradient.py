#!/usr/bin/env python
"""Timing of the active-subspace sums (gpx_sensitivity_gradient_many) on bench.py's recipe at N = 16384, with and without cpost, interleaved
in one process with gpx_sensitivity_second_many at the same arguments.  Needs an MI355X; no fallback.  One leg per process, each under its
own time limit:

    timeout -k 10 400 python tools/probe_sensitivity_gradient.py d8  --out profiles/r32_sensitivity_gradient.txt && \\
    timeout -k 10 400 python tools/probe_sensitivity_gradient.py d16 --out profiles/r32_sensitivity_gradient.txt

Per leg, for 1 and 64 inputs after one warm round (K^-1 is built by the sanity call, outside every timed window): the wall time of each
call on the host clock (best and median of REPS; each call ends in its own synchronisation), and from one profiled call each (gpx_profile_enable
level 2: device events) the build kernel (class approx_quad) and the pair pass (class exact_sum) apart; alongside, pairs per second of the
pair pass.  Records, not thresholds."""
import argparse

import numpy as np

from probe_sensitivity import _DeviceModel, _gpx, interleaved, profiled, recipe
from probe_sensitivity_second import second


def gradient(h, U, s, post):
    b, d = U.shape
    g, c = np.empty((b, d)), np.empty((b, d, d))
    p = np.empty((b, d, d)) if post else None
    _gpx.check(_gpx.lib.gpx_sensitivity_gradient_many(h, _gpx.ptr(U), _gpx.ptr(s), 1, b, _gpx.ptr(g), _gpx.ptr(c), _gpx.ptr(p) if post else None),
               "gpx_sensitivity_gradient_many")
    return g, c, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["d8", "d16"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("probe_sensitivity_gradient: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    d = {"d8": 8, "d16": 16}[a.leg]
    x, t, theta, U, s = recipe(a.n, d, 64)
    model = _DeviceModel(x, t, theta)
    h = model.handle
    g, c, p = (o[0] for o in gradient(h, U[:1], s, True))
    lam = np.linalg.eigvalsh(c + p)[::-1]
    say("N=%d d=%d sanity: finite %s, symmetric %s, cov(grad mu) = cmean - gmean gmean^T min eigenvalue / max %.3e, cpost min eigenvalue / max %.3e, "
        "the leading 2 eigenvalues of cmean + cpost carry %.4f of its trace"
        % (a.n, d, bool(np.all(np.isfinite(c)) and np.all(np.isfinite(p))), bool(np.array_equal(c, c.T) and np.array_equal(p, p.T)),
           float(np.linalg.eigvalsh(c - np.outer(g, g))[0] / lam[0]), float(np.linalg.eigvalsh(p)[0] / lam[0]), float(lam[:2].sum() / lam.sum())))
    for b in (1, 64):
        fns = {"gradient": lambda: gradient(h, U[:b], s, False), "gradient+cpost": lambda: gradient(h, U[:b], s, True),
               "second": lambda: second(h, U[:b], s)}
        wall = interleaved(fns)
        line = "N=%d d=%d b=%d:" % (a.n, d, b)
        for k, fn in fns.items():
            build, pair = profiled(h, fn)
            line += (" %s best %.3f ms median %.3f ms (build %.3f ms, pair pass %.3f ms = %.3g pairs/s) |"
                     % (k, wall[k][0], wall[k][1], build, pair, 0.5 * a.n * a.n * b / max(pair, 1e-9) * 1e3))
        say(line + " gradient / second %.3f, cpost on / off %.3f (ratios of the best)"
            % (wall["gradient"][0] / wall["second"][0], wall["gradient+cpost"][0] / wall["gradient"][0]))
    model.close()


if __name__ == "__main__":
    main()
