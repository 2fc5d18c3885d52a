"""Child process of tests/test_propagate_many.py: the batched Approx propagation at full size (N = 16384, d = 8) against the single-input
call, in a process of its own because GPX_EMU_F64 is read once per process and the buffers are gigabytes.

  compare N d B NSINGLE   fit the recipe problem, ONE propagate_GA_many over B inputs (per-input full Sigma), then NSINGLE inputs drawn from
                          the batch through propagate_GA one by one: worst |mean difference| and |variance difference| as one JSON line
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "scikit-gpuppy_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
try:
    import torch  # noqa: F401,E402  (HIP runtime of torch first, as in the rest of the suite)
except Exception:
    pass
import skgpuppy_amd as sk  # noqa: E402

import _accuracy as acc  # noqa: E402


def inputs(x, B, d, seed):
    """B inputs in the data's box, every 37th one a copy of a training row (the +vt-on-equality quirk), and a full SPD Sigma for each"""
    rng = np.random.RandomState(seed)
    U = rng.uniform(0, 10, (B, d))
    U[::37] = x[rng.randint(0, len(x), len(U[::37]))]
    A = rng.uniform(-0.1, 0.1, (B, d, d))
    S = np.einsum("bij,bkj->bik", A, A) + 0.005 * np.eye(d)
    return U, S


def main():
    mode, N, d, B, ns = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    assert mode == "compare"
    x, t, _xs, theta = acc.recipe(N, d)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    up = sk.UncertaintyPropagationApprox(gp)
    U, S = inputs(x, B, d, 5 + N + B)
    mean, var = up.propagate_GA_many(U, S)
    fixed = [0, 37, B - 1]                      # 37: a copy of a training row
    pick = fixed + [int(c) for c in np.random.RandomState(3).permutation(B) if c not in fixed][:ns - len(fixed)]
    dm, dv = 0.0, 0.0
    for i in pick:
        m1, v1 = sk.UncertaintyPropagationApprox(gp).propagate_GA(U[i], S[i])
        dm, dv = max(dm, abs(m1 - mean[i])), max(dv, abs(v1 - var[i]))
    out = {"N": N, "d": d, "B": B, "singles": int(len(pick)), "emu": os.environ.get("GPX_EMU_F64", "1"), "dmean": float(dm), "dvar": float(dv),
           "finite": bool(np.isfinite(mean).all() and np.isfinite(var).all())}
    gp._dev().close()
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
