#!/usr/bin/env python
"""Timing of the Exact moments' closed-form gradients (gpx_propagate_exact_grad_many) at N = 16384, d = 8, one Sigma, against the same
gradients by central differences through gpx_propagate_exact_many.  Needs an MI355X; no fallback.

Two legs, each a process of its own that fits the model, builds K^-1 and warms every shape it times.  Run each under its own time limit
and chain them, so that a leg that fails or hangs ends the run:

    timeout -k 10 400 python tools/bench_exact_grad.py call    --out FILE && \\
    timeout -k 10 400 python tools/bench_exact_grad.py inverse --out FILE

  call     b = 4096 and b = 1.  The new call and the difference composition alternate, RUNS times each (host clock around the calls, each of
           which ends in its one synchronisation).  The composition is what a caller without the gradient runs: ONE
           gpx_propagate_exact_many call on the b inputs and their 2 d b shifts along each coordinate under Sigma, then 2 d calls on the b
           inputs under Sigma -+ step e_k e_k^T, each of which pays its own weight pass: 4 d + 1 Exact evaluations per input.  Then one
           profiled call of the new entry point (gpx_profile_enable level 2; wall figures are taken with the profiler off): the Exact class
           (weight pass + build + finish) and the product's class.  The weight pass does not depend on b: the b = 1 call gives it; build +
           finish of b = 4096 is that call's Exact time minus the weight pass (the profiler keeps classes, not kernels: the two are not
           separated).  The product's rate is counted on its (2 d + 1) b rows: rows N^2 (1 + 128 / N) flops, as tools/bench_exact_many.py.
           The last lines compare the closed form with differences on the first 8 inputs, at the timed step and at a larger one: the variance
           is a difference of O(1) numbers on sums of far larger terms, so at N = 16384 its differences of step 1e-5 are rounding noise.
  inverse  InverseUncertaintyPropagationNumerical.get_best_solution at one operating point, method="slsqp" against "cobyla", both started at
           the log of InverseUncertaintyPropagationApprox's solution: propagation calls, wall time, both final costs and constraint values."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scikit-gpuppy_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

try:
    import torch  # noqa: F401  (its HIP runtime first: one libamdhip64 in the process)
except Exception:
    pass
import skgpuppy_amd as sk  # noqa: E402
from skgpuppy_amd import _gpx  # noqa: E402
from bench_exact_many import case, fit, inputs, many, profile  # noqa: E402

RUNS = 3
STEP = 1e-5
CHECK_STEP = 2.0 ** -7       # a step at which the variance's differences rise above their rounding noise (truncation ~ (step / length scale)^2)
NAMES = ("mean", "var", "dmean_du", "dvar_du", "dmean_ds", "dvar_ds")


def grad_many(model, U, S):
    b, d = U.shape
    out = [np.empty(b), np.empty(b)] + [np.empty((b, d)) for _ in range(4)]
    _gpx.check(_gpx.lib.gpx_propagate_exact_grad_many(model.handle, _gpx.ptr(U), _gpx.ptr(S), 1, b, *[_gpx.ptr(o) for o in out]),
               "gpx_propagate_exact_grad_many")
    return dict(zip(NAMES, out))


def by_differences(model, U, S, h=STEP):
    """the six outputs through gpx_propagate_exact_many alone (module docstring)"""
    b, d = U.shape
    pts = _gpx.f64(np.concatenate([U[None]] + [U[None] + s * h * np.eye(d)[k] for k in range(d) for s in (-1.0, 1.0)]).reshape(-1, d))
    mu, var = many(model, pts, S, True)
    mu, var = mu.reshape(2 * d + 1, b), var.reshape(2 * d + 1, b)
    out = {"mean": mu[0], "var": var[0], "dmean_du": ((mu[2::2] - mu[1::2]) / (2 * h)).T, "dvar_du": ((var[2::2] - var[1::2]) / (2 * h)).T,
           "dmean_ds": np.empty((b, d)), "dvar_ds": np.empty((b, d))}
    for k in range(d):
        step = h * S[k, k]
        side = []
        for s in (-1.0, 1.0):
            Sk = S.copy()
            Sk[k, k] += s * step
            side.append(many(model, U, _gpx.f64(Sk), True))
        out["dmean_ds"][:, k] = (side[1][0] - side[0][0]) / (2 * step)
        out["dvar_ds"][:, k] = (side[1][1] - side[0][1]) / (2 * step)
    return out


def leg_call(N, d, say):
    model, x, S = fit(N, d)
    weight_ms = None
    for b in (1, 4096):
        U = inputs(x, b)
        got, ref = grad_many(model, U, S), by_differences(model, U, S)          # warm both
        tn, td = [], []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            grad_many(model, U, S)
            t1 = time.perf_counter()
            by_differences(model, U, S)
            t2 = time.perf_counter()
            tn.append((t1 - t0) * 1e3)
            td.append((t2 - t1) * 1e3)
        prof = profile(model, lambda: grad_many(model, U, S))
        ex, gm = prof["exact"], (prof["gemm"] if prof["gemm"][0] else prof["gemm_small"])
        if weight_ms is None:
            weight_ms = ex[1]
        rows = (2 * d + 1) * b
        say("call N=%d d=%d b=%d: gradient call %s ms | difference composition (%d Exact evaluations per input) %s ms | ratio of the best %.2fx"
            % (N, d, b, " ".join("%.3f" % t for t in tn), 4 * d + 1, " ".join("%.3f" % t for t in td), min(td) / min(tn)))
        say("     profiled: Exact class %d launches %.3f ms (weight pass ~%.3f ms, build + finish ~%.3f ms) | product %d launches %.3f ms on %d rows"
            " = %.1f TFLOP/s counted as rows N^2 (1 + 128 / N) (%s)"
            % (ex[0], ex[1], weight_ms, max(ex[1] - weight_ms, 0.0), gm[0], gm[1], rows, rows * float(N) * N * (1 + 128.0 / N) / max(gm[1], 1e-9) / 1e9,
               "128x128 tiles" if prof["gemm"][0] else "small tiles"))
        nb = min(b, 8)
        for h in (STEP, CHECK_STEP):
            chk = by_differences(model, U[:nb], S, h)
            say("     first %d inputs, closed form against differences of step %g (relative to the largest entry of each output): %s"
                % (nb, h, " ".join("%s %.2e" % (k, np.abs(got[k][:nb] - chk[k]).max() / np.abs(got[k][:nb]).max()) for k in NAMES)))
    model.close()


def leg_inverse(N, d, say):
    x, t, theta, _S = case(N, d)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    u = _gpx.f64(x[0] + 0.25)
    rng = np.random.RandomState(5)
    c, I = rng.uniform(1, 3, d), rng.uniform(1, 2, d)
    up = sk.UncertaintyPropagationExact(gp)
    target = up.propagate_GA(u, np.diag(rng.uniform(0.1, 0.4, d)))[1]
    start = np.log(sk.InverseUncertaintyPropagationApprox(target, gp, u, c, I).get_best_solution())
    calls = {"n": 0}

    class Counted(sk.UncertaintyPropagationExact):
        def propagate_GA(self, uu, Sx):
            calls["n"] += 1
            return sk.UncertaintyPropagationExact.propagate_GA(self, uu, Sx)

        def propagate_GA_gradient(self, uu, Sx, h=1e-5):
            calls["n"] += 1
            return sk.UncertaintyPropagationExact.propagate_GA_gradient(self, uu, Sx, h)

    inv = sk.InverseUncertaintyPropagationNumerical(target, gp, u, c, I, upga_class=Counted)
    up.propagate_GA_gradient(u, np.diag(np.exp(start)))                      # warm both shapes
    for method in ("cobyla", "slsqp", "cobyla", "slsqp"):
        calls["n"] = 0
        t0 = time.perf_counter()
        v = inv.get_best_solution(start.copy(), method=method)
        ms = (time.perf_counter() - t0) * 1e3
        say("inverse N=%d d=%d %-6s: %4d propagation calls, %.1f ms, cost %.10g, var - target %.3e"
            % (N, d, method, calls["n"], ms, float(np.sum(c / v / I)), up.propagate_GA(u, np.diag(v))[1] - target))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["call", "inverse"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("bench_exact_grad: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.leg == "call":
        leg_call(a.n, a.d, say)
    else:
        leg_inverse(a.n, a.d, say)


if __name__ == "__main__":
    main()
