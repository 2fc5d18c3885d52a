#!/usr/bin/env python
"""Timing of the predictor's input gradients (gpx_predict_mean_grad, gpx_predict_grad, UncertaintyPropagationLinear) at N = 16384, d = 8,
4096 queries.  Needs an MI355X; no fallback.

Two legs, each a process of its own that fits its models and warms every shape it times; within a leg the calls that are compared run
interleaved, round by round, on the same box.  Run each under its own time limit and chain them, so that a leg that fails or hangs ends
the run:

    timeout -k 10 400 python tools/bench_predict_grad.py gaussian --out FILE && \\
    timeout -k 10 400 python tools/bench_predict_grad.py matern   --out FILE

  gaussian  (a) gpx_predict_mean_grad for the queries (wall time of the call, and its kernels by the profiler: the pass in the Gram class, the
                sum of the S partials in the reduce class) next to ONE gpx_dev_gram launch of the same queries x N shape (device buffers,
                host clock around launch + synchronise)
            (b) gpx_predict_grad for the queries ((d + 1) solved rows each) next to gpx_predict on as many ROWS and
                gpx_propagate_approx_many on the queries ((d + 2) rows each)
            (c) UncertaintyPropagationLinear.propagate_GA_many against UncertaintyPropagationApprox.propagate_GA_many, the same inputs
  matern    (d) (a) and (b) on a Gaussian, a Matern 5/2 and a Matern 3/2 model of the same data

Wall times are the host clock around a call that ends in its own synchronisation: best and median of REPS rounds."""
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
    torch = None
import skgpuppy_amd as sk  # noqa: E402
from skgpuppy_amd import _gpx  # noqa: E402

REPS = 7


def case(N, d, seed=1):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.array([2.0, 0.01] + [0.04 * 3.0 / d] * d))
    A = rng.uniform(-0.1, 0.1, (d, d))
    return x, t, theta, A.dot(A.T) + 0.005 * np.eye(d)


def interleaved(fns, reps=REPS):
    """{name: (best ms, median ms)} of the calls, one of each per round (the first round warms and is dropped)"""
    ts = {k: [] for k in fns}
    for r in range(reps + 1):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            if r:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (min(v), float(np.median(v))) for k, v in ts.items()}


def profile(h, fn, classes):
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 2), "gpx_profile_enable")
    _gpx.check(_gpx.lib.gpx_profile_reset(h), "gpx_profile_reset")
    fn()
    out = {}
    for cls in classes:
        n, ms, w = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_profile_read(h, cls, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w)), "gpx_profile_read")
        out[cls] = (n.value, ms.value)
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 0), "gpx_profile_enable")
    return out


def calls(gp, U, S):
    """the timed calls on one model: name -> callable"""
    h = gp._dev().handle
    m, d = U.shape
    mean, var, dm, dv = np.empty(m), np.empty(m), np.empty((m, d)), np.empty((m, d))
    rows = _gpx.f64(np.tile(U, (d + 1, 1)))
    rmean, rvar = np.empty(len(rows)), np.empty(len(rows))

    def mean_grad():
        _gpx.check(_gpx.lib.gpx_predict_mean_grad(h, _gpx.ptr(U), m, _gpx.ptr(mean), _gpx.ptr(dm)), "gpx_predict_mean_grad")

    def grad():
        _gpx.check(_gpx.lib.gpx_predict_grad(h, _gpx.ptr(U), m, _gpx.ptr(mean), _gpx.ptr(var), _gpx.ptr(dm), _gpx.ptr(dv)), "gpx_predict_grad")

    def predict_rows():
        rmean[:], rvar[:] = gp._dev().predict(rows)

    return {"mean_grad": mean_grad, "grad": grad, "predict_rows": predict_rows}, len(rows)


def leg_gaussian(N, d, b, say):
    x, t, theta, S = case(N, d)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    h = gp._dev().handle
    U = _gpx.f64(np.random.RandomState(3).uniform(1, 9, (b, d)))
    fns, nrows = calls(gp, U, S)
    # (a)
    xd, ud = torch.from_numpy(_gpx.f64(x)).cuda(), torch.from_numpy(U).cuda()
    out = torch.empty((b, N), dtype=torch.float64, device="cuda")
    vp = ctypes.c_void_p

    def gram():
        _gpx.check(_gpx.lib.gpx_dev_gram(vp(ud.data_ptr()), b, vp(xd.data_ptr()), N, d, _gpx.ptr(theta), 0.0, 0, 0, vp(out.data_ptr()), N, b, N, None),
                   "gpx_dev_gram")
        torch.cuda.synchronize()

    r = interleaved({"mean_grad": fns["mean_grad"], "gram": gram})
    pr = profile(h, fns["mean_grad"], (_gpx.K_GRAM, _gpx.K_REDUCE))
    say("(a) N=%d d=%d queries=%d: gpx_predict_mean_grad best %.3f ms median %.3f ms (kernels: pass %d launch %.3f ms, sum of partials %d launch %.3f ms)"
        " | one gpx_dev_gram launch %d x %d best %.3f ms median %.3f ms | call / Gram %.2fx, pass / Gram %.2fx"
        % (N, d, b, r["mean_grad"][0], r["mean_grad"][1], pr[_gpx.K_GRAM][0], pr[_gpx.K_GRAM][1], pr[_gpx.K_REDUCE][0], pr[_gpx.K_REDUCE][1], b, N,
           r["gram"][0], r["gram"][1], r["mean_grad"][0] / r["gram"][0], pr[_gpx.K_GRAM][1] / r["gram"][0]))
    del out
    # (b)
    o4 = [np.empty(b) for _ in range(4)]

    def approx():
        _gpx.check(_gpx.lib.gpx_propagate_approx_many(h, _gpx.ptr(U), _gpx.ptr(S), 1, b, *[_gpx.ptr(o) for o in o4]), "gpx_propagate_approx_many")

    r = interleaved({"grad": fns["grad"], "predict_rows": fns["predict_rows"], "approx": approx})
    say("(b) N=%d d=%d queries=%d: gpx_predict_grad (%d rows) best %.2f ms median %.2f ms | gpx_predict on %d rows best %.2f ms median %.2f ms: %.3fx"
        " | gpx_propagate_approx_many (%d rows) best %.2f ms median %.2f ms: per row %.3fx"
        % (N, d, b, nrows, r["grad"][0], r["grad"][1], nrows, r["predict_rows"][0], r["predict_rows"][1], r["grad"][0] / r["predict_rows"][0],
           b * (d + 2), r["approx"][0], r["approx"][1], (r["grad"][0] / nrows) / (r["approx"][0] / (b * (d + 2)))))
    # (c)
    lin, apx = sk.UncertaintyPropagationLinear(gp), sk.UncertaintyPropagationApprox(gp)
    r = interleaved({"linear": lambda: lin.propagate_GA_many(U, S), "approx": lambda: apx.propagate_GA_many(U, S)})
    say("(c) N=%d d=%d inputs=%d: UncertaintyPropagationLinear.propagate_GA_many best %.3f ms median %.3f ms | UncertaintyPropagationApprox.propagate_GA_many"
        " best %.2f ms median %.2f ms: %.1fx" % (N, d, b, r["linear"][0], r["linear"][1], r["approx"][0], r["approx"][1], r["approx"][0] / r["linear"][0]))


def leg_matern(N, d, b, say):
    x, t, theta, S = case(N, d)
    U = _gpx.f64(np.random.RandomState(3).uniform(1, 9, (b, d)))
    models = {"Gaussian": sk.GaussianCovariance(), "Matern 5/2": sk.MaternCovariance(2.5), "Matern 3/2": sk.MaternCovariance(1.5)}
    fns = {}
    gps = []
    for name, cov in models.items():
        gp = sk.GaussianProcess(x, t, cov, theta.copy())
        gps.append(gp)
        f, _ = calls(gp, U, S)
        fns[name + " mean_grad"], fns[name + " grad"] = f["mean_grad"], f["grad"]
    r = interleaved(fns)
    for name in models:
        say("(d) N=%d d=%d queries=%d %-10s: gpx_predict_mean_grad best %.3f ms median %.3f ms | gpx_predict_grad best %.2f ms median %.2f ms"
            % (N, d, b, name, r[name + " mean_grad"][0], r[name + " mean_grad"][1], r[name + " grad"][0], r[name + " grad"][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["gaussian", "matern"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--b", type=int, default=4096)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1 or torch is None:
        raise SystemExit("bench_predict_grad: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    (leg_gaussian if a.leg == "gaussian" else leg_matern)(a.n, a.d, a.b, say)


if __name__ == "__main__":
    main()
