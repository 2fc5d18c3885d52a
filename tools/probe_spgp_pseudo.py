#!/usr/bin/env python
"""Timing of uncertainty propagation over the pseudo-inputs of an SPGP model (GaussianProcess.pseudo_gp(), gpx_spgp_pseudo_handle).
Needs an MI355X; no fallback.  Two legs, each a process of its own; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/probe_spgp_pseudo.py c5    --out profiles/r23_spgp_pseudo.txt && \\
    timeout -k 10 300 python tools/probe_spgp_pseudo.py small --out profiles/r23_spgp_pseudo.txt

  c5     BASELINE config 5 (N = 262144, m = 2048, d = 8; bench.py's data): the SPGP fit and, in the same run, the build of the pseudo-input
         handle; one Exact propagate_GA; propagate_GA_many of 4096 inputs with one shared Sigma for Exact, Approx and Linear;
         estimate_many_gradient of 4096 queries.
  small  N = 4096, m = 512, d = 8: the same calls, and for the same inputs the routes an SPGP GaussianProcess had before: the dense
         UncertaintyPropagationExact (N x N Woodbury inverse, C_ux from N calls of the scalar kernel) per call, and estimate_many_gradient /
         UncertaintyPropagationLinear by central differences.

Wall time of the call on the host clock (every call ends in its own synchronisation), best and median of REPS after one warm call; the first
call of a kind is reported apart where it builds something (the handle, the dense inverse).  These are records, not thresholds."""
import argparse
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
import skgpuppy_amd as sk  # noqa: E402

REPS = 5
B = 4096


def data(n, m, d, b):
    rng = np.random.RandomState(20240 + n + d)
    x = rng.uniform(0, 10, (n, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(n)
    U = rng.uniform(1, 9, (b, d))
    xb = x[rng.choice(n, m, replace=False)].copy()
    theta = np.concatenate([np.log(np.array([2.0, 0.01] + [0.04] * d)), xb.ravel()])
    A = rng.uniform(-0.3, 0.3, (d, d))
    return x, t, theta, U, A.dot(A.T) + 0.05 * np.eye(d)


def timed(fn, reps=REPS, warm=1):
    """(first call ms, best ms, median ms)"""
    t0 = time.perf_counter()
    fn()
    first = (time.perf_counter() - t0) * 1e3
    for _ in range(max(0, warm - 1)):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return first, min(ts), float(np.median(ts))


def line(out, what, first, best, med, per=None):
    s = "  %-58s first %10.3f ms   best %10.3f ms   median %10.3f ms" % (what, first, best, med)
    if per:
        s += "   (%.2f us an input)" % (best * 1e3 / per)
    print(s)
    out.append(s)


def pseudo_calls(out, gp, pgp, U, S):
    ex, ap, li = sk.UncertaintyPropagationExact(pgp), sk.UncertaintyPropagationApprox(pgp), sk.UncertaintyPropagationLinear(pgp)
    line(out, "Exact propagate_GA, one input", *timed(lambda: ex.propagate_GA(U[0], S)))
    line(out, "Approx propagate_GA, one input (a new u each call)", *timed(lambda c=[0]: (c.__setitem__(0, c[0] + 1), ap.propagate_GA(U[c[0]], S))))
    line(out, "Exact propagate_GA_many, %d inputs, one Sigma" % len(U), *timed(lambda: ex.propagate_GA_many(U, S)), per=len(U))
    line(out, "Approx propagate_GA_many, %d inputs, one Sigma" % len(U), *timed(lambda: ap.propagate_GA_many(U, S)), per=len(U))
    line(out, "Linear propagate_GA_many, %d inputs, one Sigma" % len(U), *timed(lambda: li.propagate_GA_many(U, S)), per=len(U))
    line(out, "estimate_many_gradient, %d queries" % len(U), *timed(lambda: pgp.estimate_many_gradient(U)), per=len(U))
    line(out, "estimate_many_gradient(variance=False), %d queries" % len(U), *timed(lambda: pgp.estimate_many_gradient(U, variance=False)), per=len(U))
    mu, var = ex.propagate_GA_many(U[:64], S)
    pm, pv = gp.estimate_many(U[:64])
    out.append("  sanity: Exact moments of 64 inputs finite %s; mean within %.3g of the predictor's at u, variance above it by %.3g .. %.3g" %
               (bool(np.all(np.isfinite(mu)) and np.all(np.isfinite(var))), np.abs(mu - pm).max(), (var - pv).min(), (var - pv).max()))
    print(out[-1])


def leg_c5(out):
    n, m, d = 262144, 2048, 8
    x, t, theta, U, S = data(n, m, d, B)
    out.append("config 5: SPGP N = %d, m = %d, d = %d; %d inputs, one shared full Sigma" % (n, m, d, B))
    fits, builds = [], []
    gp = pgp = None
    for r in range(3):
        if gp is not None:
            pgp.close()
            gp._dev().close()
        t0 = time.perf_counter()
        gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), theta)
        t1 = time.perf_counter()
        pgp = gp.pseudo_gp()
        pgp._dev()
        t2 = time.perf_counter()
        fits.append((t1 - t0) * 1e3)
        builds.append((t2 - t1) * 1e3)
    out.append("  SPGP fit (GaussianProcess constructor)                      first %10.3f ms   best %10.3f ms" % (fits[0], min(fits[1:])))
    out.append("  pseudo-input handle build, right after that fit            first %10.3f ms   best %10.3f ms   (P = %.0f MB)" %
               (builds[0], min(builds[1:]), 8.0 * m * m / 1e6))
    print("\n".join(out[-2:]))
    pseudo_calls(out, gp, pgp, U, S)


def leg_small(out):
    n, m, d = 4096, 512, 8
    x, t, theta, U, S = data(n, m, d, B)
    out.append("N = %d, m = %d, d = %d; %d inputs, one shared full Sigma" % (n, m, d, B))
    gp = sk.GaussianProcess(x, t, sk.SPGPCovariance(m), theta)
    pgp = gp.pseudo_gp()
    line(out, "pseudo-input handle build", *timed(lambda: (pgp.close(), pgp._dev())))
    pseudo_calls(out, gp, pgp, U, S)
    out.append("  the routes of the SPGP GaussianProcess itself (unchanged), same inputs:")
    dex = sk.UncertaintyPropagationExact(gp)
    line(out, "dense Exact propagate_GA, one input (first: builds N x N Kinv)", *timed(lambda c=[0]: (c.__setitem__(0, c[0] + 1), dex.propagate_GA(U[c[0]], S)),
                                                                                      reps=3))
    line(out, "estimate_many_gradient by central differences, %d queries" % len(U), *timed(lambda: gp.estimate_many_gradient(U), reps=3), per=len(U))
    dli = sk.UncertaintyPropagationLinear(gp)
    line(out, "Linear propagate_GA_many by central differences, %d inputs" % len(U), *timed(lambda: dli.propagate_GA_many(U, S), reps=3), per=len(U))
    m0, v0 = dex.propagate_GA(U[0], S)
    m1, v1 = sk.UncertaintyPropagationExact(pgp).propagate_GA(U[0], S)
    out.append("  the two Exact routes answer different questions (the dense one corrects the low-rank kernel Q(u, x_i)): input 0 dense (%.6f, %.6f), "
               "pseudo (%.6f, %.6f)" % (m0, v0, m1, v1))
    print(out[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["c5", "small"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    {"c5": leg_c5, "small": leg_small}[a.leg](out)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(out) + "\n\n")


if __name__ == "__main__":
    main()
