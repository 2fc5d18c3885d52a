"""The factorisation with its far columns updated by group on the int8 path (csrc/chol.hip, Lookahead::group_boundary; DESIGN.md
section 5.1), at sizes where the knobs put one boundary (N = 2200: three panels, ragged last, groups of one), two (N = 3300) and two
with groups of two panels (N = 5200), each in a child process: the knobs are read once per process.

Held to what tests/test_backward_error.py holds the fp64 schedules to: the factor's backward error against the device Gram
<= 16 x max(LAPACK's, u) and <= N u (section A there), estimate_many within MEAN_ATOL_V / VAR_ATOL_V (section F) of the GPX_FIT_EMU=0 run
of the same problem.  alpha has no tolerance of its own in that file; here its two values are compared through K: both solve
K alpha = t with a residual of at most N u |K| |alpha| each (the factor bound above), so |K (alpha_1 - alpha_0)| <= 2 N u |K| |alpha| in
the infinity norms.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import torch  # noqa: F401

import skgpuppy_amd as sk

import _accuracy as acc
from test_backward_error import MEAN_ATOL_V, VAR_ATOL_V

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "_fit_emulated_worker.py")
KNOBS = ("GPX_FIT_EMU", "GPX_FIT_EMU_GROUP", "GPX_EMU_MIN_K", "GPX_CONCURRENT_STREAMS", "GPX_SQK_FROM", "GPX_TRAP")

G1 = {"GPX_FIT_EMU": "1", "GPX_FIT_EMU_GROUP": "1", "GPX_EMU_MIN_K": "1024"}
G2 = {"GPX_FIT_EMU": "1", "GPX_FIT_EMU_GROUP": "2", "GPX_EMU_MIN_K": "2048"}
D_OF = {2200: 3, 3300: 4, 5200: 5}
CASES = [
    ("groups of one", 2200, G1),
    ("groups of one", 3300, G1),
    ("groups of two", 5200, G2),
    ("groups of two, serialised streams", 5200, dict(G2, GPX_CONCURRENT_STREAMS="0")),
    ("groups of two, no square launches", 5200, dict(G2, GPX_SQK_FROM="-1")),
    ("groups of two, narrow and bulk as two launches", 5200, dict(G2, GPX_TRAP="0")),
]

_RUNS = {}


def _child(args, extra, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(extra)
    r = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (args, extra, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _fit(tmp, N, extra):
    """one child per (N, knobs) and test session: its JSON line and its arrays"""
    key = (N, tuple(sorted(extra.items())))
    if key not in _RUNS:
        path = os.path.join(str(tmp), "fit_%d_%d.npz" % (N, len(_RUNS)))
        res = _child(["fit", N, D_OF[N], path], extra)
        _RUNS[key] = (res, dict(np.load(path)))
    return _RUNS[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("fit_emulated")


_BASE = {}


def _baseline(N):
    if N not in _BASE:
        x, _t, _xs, theta = acc.recipe(N, D_OF[N])
        K = sk.GaussianCovariance().cov_matrix(x, theta)
        _BASE[N] = (acc.chol_backward_error(acc.lapack_chol(K), K), K)
    return _BASE[N]


@pytest.mark.parametrize("name,N,knobs", CASES, ids=[c[0] + " N=%d" % c[1] for c in CASES])
def test_factor_alpha_and_predictions(tmp, name, N, knobs):
    res, arr = _fit(tmp, N, knobs)
    off, ref = _fit(tmp, N, {"GPX_FIT_EMU": "0"})
    base, K = _baseline(N)
    print("FIT-EMU | %s N=%d | offdiag %.3e diag %.3e | LAPACK %.3e %.3e | N u %.3e | GPX_FIT_EMU=0 %.3e %.3e | same bytes: %s"
          % (name, N, res["offdiag"], res["diag"], base[0], base[1], N * acc.U, off["offdiag"], off["diag"], res["hash"] == off["hash"]))
    assert res["jitter"] == 0.0 and off["jitter"] == 0.0
    assert res["hash"] != off["hash"], "the knobs did not reach the schedule: the factor is the fp64 schedule's, bit for bit"
    assert res["offdiag"] <= acc.bound(base[0]) and res["diag"] <= acc.bound(base[1]), (res, base)
    assert res["offdiag"] <= N * acc.U, (res["offdiag"], N * acc.U)
    v = 2.0
    em, ev = float(np.abs(arr["mean"] - ref["mean"]).max()) / v, float(np.abs(arr["var"] - ref["var"]).max()) / v
    with acc.blas_threads():
        Kf = np.tril(K) + np.tril(K, -1).T
        da = float(np.abs(Kf.dot(arr["beta"] - ref["beta"])).max()) / (float(np.abs(Kf).sum(1).max()) * float(np.abs(ref["beta"]).max()))
    print("FIT-EMU | %s N=%d | mean %.3e (<= %.1e) var %.3e (<= %.1e) |K dalpha| %.3e (<= %.3e)" % (name, N, em, MEAN_ATOL_V, ev, VAR_ATOL_V, da, 2 * N * acc.U))
    assert em <= MEAN_ATOL_V and ev <= VAR_ATOL_V, (em, ev)
    assert da <= 2 * N * acc.U, da


@pytest.mark.parametrize("name,N,knobs", CASES[:3], ids=[c[0] + " N=%d" % c[1] for c in CASES[:3]])
def test_two_fits_in_one_process_agree_to_the_bit(tmp, name, N, knobs):
    res, _ = _fit(tmp, N, knobs)
    assert res["hash"] == res["hash2"], res


@pytest.mark.parametrize("N", [2200, 3300, 5200])
def test_switched_off_is_the_schedule_of_a_process_where_size_rules_it_out(tmp, N):
    """GPX_FIT_EMU=0 against the default environment, where these sizes have a single group of panels at the default depth: same bytes"""
    _, a = _fit(tmp, N, {"GPX_FIT_EMU": "0"})
    _, b = _fit(tmp, N, {})
    assert np.array_equal(a["L"], b["L"])


@pytest.mark.parametrize("at,where", [(700, "in the first group"), (2600, "behind the first boundary")])
def test_non_positive_pivot_ends_in_the_jitter_retry(at, where):
    """150 numerically identical rows and vt = 0 (the recipe of the multi-device test): the pivot fails in panel at // 1024, the rest of the
    schedule -- the boundaries' updates of NaN rows included -- runs to its end, the status word is read and the fit repeated with jitter"""
    on = _child(["dup", 5200, 5, at], G2)
    off = _child(["dup", 5200, 5, at], {"GPX_FIT_EMU": "0"})
    print("FIT-EMU | pivot %s | jitter %g / %g" % (where, on["jitter"], off["jitter"]))
    assert on["jitter"] == off["jitter"] == 1e-5, (on, off)
    assert on["finite"] and off["finite"]
