#!/usr/bin/env python
"""Timing of the batched Exact propagation (gpx_propagate_exact_many) at N = 16384, d = 8, one Sigma.  Needs an MI355X; no fallback.

Three legs, each a process of its own that fits the model, builds K^-1 and warms every shape it times.  Run each under its own time
limit and chain them, so that a leg that fails or hangs ends the run:

    timeout -k 10 300 python tools/bench_exact_many.py call   --out FILE && \\
    timeout -k 10 300 python tools/bench_exact_many.py loop   --out FILE && \\
    timeout -k 10 400 python tools/bench_exact_many.py minrun --out FILE

  call    b = 8, 128, 4096: wall time of the call (host clock around the call, which ends in its one synchronisation; best and median of
          REPS), then one profiled call (gpx_profile_enable level 2; end-to-end figures are taken with the profiler off): the Exact class
          (weight pass + build + finish) and the product's class, launches / ms / work.  The weight pass does not depend on b: the b = 8 call,
          where build and finish touch 8 x N entries, gives it; build + finish of a larger b is that call's Exact time minus the weight pass.
  loop    a loop of gpx_propagate_exact over the same inputs with K^-1 resident (b = 4096: the first 512, scaled)
  minrun  the matrix path against the pair path on the same inputs, per-input Sigma repeated (one run), run lengths 1 .. 16, at N = 2048 and
          N = 16384: GPX_EXACT_MANY_MIN_RUN=1 (matrix) against =1000000 (pair), alternating; the smallest run length from which the matrix
          path stays faster is the measured MIN_RUN.

Work counted (algorithmic, from the shapes): weight pass N^2 / 2 pairs x (2 d + 25) flops and 8 N^2 bytes (4 N^2 read, 4 N^2 written);
product b N^2 (1 + 128 / N) flops; build b N (7 d + 65) flops, 8 b N bytes written; finish 2 b N flops, 16 b N bytes read."""
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
CLASSES = {"exact": _gpx.K_EXACT, "gemm": _gpx.K_GEMM, "gemm_small": _gpx.K_GEMM_SMALL}


def case(N, d, seed=1):
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    theta = np.log(np.array([2.0, 0.01] + [0.04 * 3.0 / d] * d))
    A = rng.uniform(-0.3, 0.3, (d, d))
    return x, t - t.mean(), theta, A.dot(A.T) + 0.05 * np.eye(d)


def fit(N, d):
    x, t, theta, S = case(N, d)
    model = _DeviceModel(_gpx.f64(x), _gpx.f64(t), _gpx.f64(theta))
    u0, S = _gpx.f64(x[:1] + 0.25), _gpx.f64(S)
    many(model, u0, S, True)                       # builds K^-1
    return model, x, S


def many(model, U, S, shared):
    mean, var = np.empty(len(U)), np.empty(len(U))
    _gpx.check(_gpx.lib.gpx_propagate_exact_many(model.handle, _gpx.ptr(U), _gpx.ptr(S), int(shared), len(U), _gpx.ptr(mean), _gpx.ptr(var)),
               "gpx_propagate_exact_many")
    return mean, var


def single_loop(model, U, S):
    m, v = ctypes.c_double(), ctypes.c_double()
    out = np.empty((len(U), 2))
    for i in range(len(U)):
        _gpx.check(_gpx.lib.gpx_propagate_exact(model.handle, _gpx.ptr(U[i]), _gpx.ptr(S), ctypes.byref(m), ctypes.byref(v)), "gpx_propagate_exact")
        out[i] = m.value, v.value
    return out


def abs_scales(x, theta, Kinv, beta, U, S, rows=128):
    """(scale of the mean [B], scale of the variance [B]): the sums of the absolute values of the terms that gpx_propagate_exact adds up, in
    float64 numpy from the factored form -- sum_i |beta_i| l_i, and (v + vt) + nc2 h^T ((|Kinv| + |beta| |beta|^T) o E) h + that squared --:
    what a difference between two evaluations of the same moments is measured against (tests/_dense_ld.py)"""
    N, d = x.shape
    v, vt, w = np.exp(theta[0]), np.exp(theta[1]), np.exp(theta[2:2 + d])
    Ainv = np.linalg.inv(S + np.diag(0.5 / w))
    Ls = 2 * np.diag(w) - Ainv
    Ls = (Ls + Ls.T) / 2
    sk = np.diag(S)
    dd, nc1, nc2 = w - w / (1 + w * sk), 1 / np.sqrt(np.prod(1 + w * sk)), 1 / np.sqrt(np.prod(1 + 2 * w * sk))
    a = U[:, None, :] - x[None, :, :]
    h = v * np.exp(-0.25 * (a.dot(Ainv) * a).sum(-1))
    ms = (v * np.exp(-0.5 * (w * a * a).sum(-1)) * nc1 * np.exp(0.5 * (dd * a * a).sum(-1))).dot(np.abs(beta))
    acc = np.zeros(len(U))
    for i0 in range(0, N, rows):
        D = x[i0:i0 + rows, None, :] - x[None, :, :]
        E = np.exp(-0.125 * (D.reshape(-1, d).dot(Ls).reshape(D.shape) * D).sum(-1))
        G = (np.abs(Kinv[i0:i0 + rows]) + np.outer(np.abs(beta[i0:i0 + rows]), np.abs(beta))) * E
        acc += (h[:, i0:i0 + rows] * G.dot(h.T).T).sum(1)
    return ms, (v + vt) + nc2 * acc + ms * ms


def timed(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts))


def profile(model, fn):
    h = model.handle
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 2), "gpx_profile_enable")
    _gpx.check(_gpx.lib.gpx_profile_reset(h), "gpx_profile_reset")
    fn()
    out = {}
    for name, cls in CLASSES.items():
        n, ms, w = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _gpx.check(_gpx.lib.gpx_profile_read(h, cls, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w)), "gpx_profile_read")
        out[name] = (n.value, ms.value, w.value)
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 0), "gpx_profile_enable")
    return out


def inputs(x, b, seed=3):
    rng = np.random.RandomState(seed)
    return _gpx.f64(rng.uniform(1, 9, (b, x.shape[1])))


def leg_call(N, d, say):
    model, x, S = fit(N, d)
    weight_ms = None
    for b in (8, 128, 4096):
        U = inputs(x, b)
        many(model, U, S, True)                    # warm this shape
        best, med = timed(lambda: many(model, U, S, True))
        prof = profile(model, lambda: many(model, U, S, True))
        ex, gm = prof["exact"], (prof["gemm"] if prof["gemm"][0] else prof["gemm_small"])
        if weight_ms is None:
            weight_ms = ex[1]
        say("call N=%d d=%d b=%d: best %.3f ms median %.3f ms = %.2f us per input | Exact class %d launches %.3f ms (weight pass ~%.3f ms, "
            "build + finish ~%.3f ms) | product %d launch %.3f ms = %.1f TFLOP/s (%s)"
            % (N, d, b, best, med, 1e3 * best / b, ex[0], ex[1], weight_ms, max(ex[1] - weight_ms, 0.0), gm[0], gm[1],
               gm[2] / max(gm[1], 1e-9) / 1e9, "128x128 tiles" if prof["gemm"][0] else "small tiles"))
        say("     weight pass: %.1f GB/s of 8 N^2 bytes, %.2f TFLOP/s of N^2 / 2 (2 d + 25)"
            % (8.0 * N * N / weight_ms / 1e6, 0.5 * N * N * (2 * d + 25) / weight_ms / 1e9))
    model.close()


def leg_loop(N, d, say):
    model, x, S = fit(N, d)
    for b in (8, 128, 4096):
        U = inputs(x, b)
        nb = min(b, 512)
        single_loop(model, U[:8], S)
        best, med = timed(lambda: single_loop(model, U[:nb], S), reps=3)
        mb, _ = timed(lambda: many(model, U, S, True))
        say("loop N=%d d=%d b=%d: %d single calls best %.2f ms = %.1f us per input (%.0f calls/s)%s; the many call %.3f ms: %.1fx"
            % (N, d, b, nb, best, 1e3 * best / nb, nb / best * 1e3, "" if nb == b else ", scaled to b: %.1f ms" % (best * b / nb), mb,
               best * b / nb / mb))
        if b == 4096:
            got = many(model, U[:64], S, True)
            ref = single_loop(model, U[:64], S)
            _x, _t, theta, _S = case(N, d)
            ms, vs = abs_scales(x, theta, model.kinv(), model.alpha(), U[:64], S)
            say("     first 64 inputs, many call against the loop: worst |dmean| %.3e |dvar| %.3e; on the scale of the sums' absolute terms "
                "(mean %.3e, variance %.3e at the worst input): %.3e / %.3e"
                % (np.abs(got[0] - ref[:, 0]).max(), np.abs(got[1] - ref[:, 1]).max(), ms[np.argmax(np.abs(got[0] - ref[:, 0]) / ms)],
                   vs[np.argmax(np.abs(got[1] - ref[:, 1]) / vs)], (np.abs(got[0] - ref[:, 0]) / ms).max(), (np.abs(got[1] - ref[:, 1]) / vs).max()))
    model.close()


def leg_minrun(d, say):
    for N in (2048, 16384):
        model, x, S = fit(N, d)
        first = None
        rows = []
        for r in (1, 2, 3, 4, 5, 6, 8, 12, 16):
            U = inputs(x, r)
            Sr = _gpx.f64(np.repeat(S[None], r, 0))
            t = {}
            for rep in range(REPS + 1):                # the first round warms both
                for setting in ("1", "1000000"):
                    os.environ["GPX_EXACT_MANY_MIN_RUN"] = setting
                    t0 = time.perf_counter()
                    many(model, U, Sr, False)
                    if rep:
                        t.setdefault(setting, []).append((time.perf_counter() - t0) * 1e3)
            os.environ.pop("GPX_EXACT_MANY_MIN_RUN", None)
            mt, pr = min(t["1"]), min(t["1000000"])
            rows.append((r, mt, pr))
            say("minrun N=%d d=%d run %2d: matrix path %.3f ms, pair path %.3f ms (%.2fx)" % (N, d, r, mt, pr, pr / mt))
        for r, mt, pr in reversed(rows):
            if mt < pr:
                first = r
            else:
                break
        say("minrun N=%d: the matrix path stays faster from a run of %s" % (N, first))
        model.close()
        _gpx.lib.gpx_pool_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["call", "loop", "minrun"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    a = ap.parse_args()
    if _gpx.device_count() < 1:
        raise SystemExit("bench_exact_many: no gfx950 device (there is no CPU path to time)")

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.leg == "call":
        leg_call(a.n, a.d, say)
    elif a.leg == "loop":
        leg_loop(a.n, a.d, say)
    else:
        leg_minrun(a.d, say)


if __name__ == "__main__":
    main()
