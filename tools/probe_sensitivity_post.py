#!/usr/bin/env python
"""Timing of the posterior parts of the variance decomposition (gpx_sensitivity_post_many) on bench.py's recipe at N = 16384, interleaved in
one process with gpx_sensitivity_many with totals at the same arguments -- the yardstick: two separate passes would cost 2x of it plus the
reads of K^-1.  Needs an MI355X; no fallback.  One leg per process, each under its own time limit:

    timeout -k 10 400 python tools/probe_sensitivity_post.py d8  --out profiles/r33_sensitivity_post.txt && \\
    timeout -k 10 400 python tools/probe_sensitivity_post.py d16 --out profiles/r33_sensitivity_post.txt

Per leg: the first call (which builds K^-1) against the second, then for 1 and 64 inputs after one warm round the wall time of each call on
the host clock (best and median of REPS; each call ends in its own synchronisation), and from one profiled call each (gpx_profile_enable
level 2: device events) the build kernel (class approx_quad) and the pair pass (class exact_sum) apart.  Records, not thresholds."""
import argparse
import time

import numpy as np

from probe_sensitivity import _DeviceModel, _gpx, interleaved, profiled, recipe, sens


def post(h, U, s, total=True):
    b, d = U.shape
    o = [np.empty(b), np.empty(b), np.empty((b, d)), np.empty((b, d)) if total else None, np.empty(b), np.empty((b, d)), np.empty((b, d)) if total else None]
    _gpx.check(_gpx.lib.gpx_sensitivity_post_many(h, _gpx.ptr(U), _gpx.ptr(s), 1, b, *[None if a is None else _gpx.ptr(a) for a in o]),
               "gpx_sensitivity_post_many")
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["d8", "d16"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("probe_sensitivity_post: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    d = {"d8": 8, "d16": 16}[a.leg]
    x, t, theta, U, s = recipe(a.n, d, 64)
    model = _DeviceModel(x, t, theta)
    h = model.handle
    sens(h, U[:1], s, True)                                         # code objects and pools warm before the K^-1 build is timed
    t0 = time.perf_counter()
    o = post(h, U[:1], s)
    t1 = time.perf_counter()
    post(h, U[:1], s)
    t2 = time.perf_counter()
    base = sens(h, U[:1], s, True)
    V, vp = o[1][0], o[4][0]
    say("N=%d d=%d sanity: first call %.1f ms, second %.3f ms: the one-off K^-1 build %.1f ms | mean part bit-equal to gpx_sensitivity_many %s | "
        "V %.6g + var_post %.6g; sum first / V: mean %.4f, with the posterior part %.4f; sum total / V: %.4f, %.4f; smallest post term %.3e"
        % (a.n, d, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * ((t1 - t0) - (t2 - t1)), all(np.array_equal(p, q) for p, q in zip(o[:4], base)),
           V, vp, o[2].sum() / V, (o[2] + o[5]).sum() / (V + vp), o[3].sum() / V, (o[3] + o[6]).sum() / (V + vp), min(vp, o[5].min(), o[6].min())))
    for b in (1, 64):
        fns = {"mean part": lambda: sens(h, U[:b], s, True), "with the posterior part": lambda: post(h, U[:b], s),
               "posterior, no totals": lambda: post(h, U[:b], s, False)}
        wall = interleaved(fns)
        line = "N=%d d=%d b=%d:" % (a.n, d, b)
        for k, fn in fns.items():
            build, pair = profiled(h, fn)
            line += " %s best %.3f ms median %.3f ms (build %.3f ms, pair pass %.3f ms) |" % (k, wall[k][0], wall[k][1], build, pair)
        say(line + " posterior / mean part %.3f of the best, %.3f of the medians (two passes: 2 plus the reads of K^-1)"
            % (wall["with the posterior part"][0] / wall["mean part"][0], wall["with the posterior part"][1] / wall["mean part"][1]))
    model.close()


if __name__ == "__main__":
    main()
