"""A long-double model of the variance decomposition of the predictor mean under independent Gaussian inputs (gpx_sensitivity_many;
scikit-gpuppy_amd/csrc/sensitivity.hip), the tensor Gauss-Hermite evaluation of its definitions, and the inputs of
tests/test_sensitivity.py.  Host only.

x_k ~ N(u_k, s_k) independent, mu(x) = sum_i beta_i c_i(x), c_i the plain kernel v exp(-1/2 sum_k w_k (x_k - x_ik)^2).  Per coordinate,
with a_i = u_k - x_ik, om = w_k, sg = s_k, restated as include/gpx.h states them (NOT as the device evaluates them: the device completes
the square in lE and takes the m side from per-point products):
    lm_ik      = -1/2 log1p(om sg) - 1/2 om a_i^2 / (1 + om sg)
    lE_k(i,j)  = -1/2 log1p(2 om sg) - 1/2 om (1 + om sg) / (1 + 2 om sg) (a_i^2 + a_j^2) + om^2 sg / (1 + 2 om sg) a_i a_j
    m_k = exp(lm_ik) exp(lm_jk),  E_k = exp(lE_k),  b_ij = v^2 beta_i beta_j
    mean = v sum_i beta_i exp(sum_k lm_ik),   V = sum_ij b_ij (prod E - prod m),
    first_k = sum_ij b_ij (prod_{l != k} m_l) (E_k - m_k),   total_k = sum_ij b_ij (prod_{l != k} E_l) (E_k - m_k)
over the pairs j <= i with weight 2 below the diagonal and 1 on it.

`sums` takes `dt`: np.longdouble is the model, np.float64 the plain numpy evaluation of the same case that rho_ref is measured on.  Each
sum comes as (values, scales): the scale is the sum of the absolute terms with the difference taken apart -- |b_ij| (prod E + prod m) for
V, |b_ij| prod_{l != k}(.) (E_k + m_k) for first and total, v sum |beta_i| prod m for the mean.  The rule (distances, MARGIN, FLOOR, bound)
is the project's one rule of tests/_spgp_ld.py through tests/_dense_ld.py: imported, not copied.

`defect=` plants one of the seeded defects of tests/test_sensitivity_model.py (meant for dt = np.float64): "pair" drops one pair,
"offdiag1" gives the pairs below the diagonal weight 1 instead of 2, "allprod" takes the products over all l instead of l != k."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _dense_ld as dl
from _spgp_ld import FLOOR, LD, MARGIN, bound  # noqa: F401  (the project's one rule: imported, not copied)

ROWS = 64
TEMP = 1 << 20            # entries of a temporary [d, rows, N] (16 MiB in long double): large enough that a thread spends its time inside numpy
THREADS = 8
KEYS = ("mean", "V", "first", "total")


def _suffix(F):
    """[d, ...] -> suf with suf[k] = prod of F[k + 1:] over the first axis"""
    suf = np.ones_like(F)
    for k in range(F.shape[0] - 2, -1, -1):
        suf[k] = suf[k + 1] * F[k + 1]
    return suf


def sums(x, theta, beta, u, s, dt=LD, defect=None):
    """{"mean": ([1], [1]), "V": ([1], [1]), "first": ([d], [d]), "total": ([d], [d])}, each (values, scales)"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, _vt, w = dl.params(theta, d, dt)
    sg = np.asarray(s, dtype=np.float64).astype(dt)
    a = np.asarray(u, dtype=np.float64).astype(dt) - xr.astype(dt)
    be = np.asarray(beta, dtype=np.float64).astype(dt)
    ws = w * sg
    lm = -np.log1p(ws) / 2 - w * a * a / (1 + ws) / 2
    c0 = -np.log1p(2 * ws) / 2
    A = w * (1 + ws) / (1 + 2 * ws) / 2
    B = w * w * sg / (1 + 2 * ws)
    m = np.exp(lm)                                           # [N, d]
    g = np.exp(lm.sum(1))
    pa = -A * a * a                                          # lE_k(i, j) = (c0 + pa_ik) + pa_jk + (B a_ik) a_jk
    pc, Ba = c0 + pa, B * a
    out = {"mean": (np.array([v * (be * g).sum()], dt), np.array([v * (np.abs(be) * g).sum()], dt))}
    pair = dl._pair_of(xr, np.asarray(w, dtype=np.float64)) if defect == "pair" else None
    cols = np.arange(N)
    rows = max(4, min(ROWS, TEMP // (d * N)))                # every temporary within TEMP entries

    def block(i0):
        """(V, aV, F, aF, T, aT) of the rows [i0, i0 + rows)"""
        V, aV = dt(0), dt(0)
        F, aF, T, aT = (np.zeros(d, dt) for _ in range(4))
        i1 = min(N, i0 + rows)
        E = np.empty((d, i1 - i0, i1), dt)
        M = np.empty((d, i1 - i0, i1), dt)
        for k in range(d):
            E[k] = np.outer(Ba[i0:i1, k], a[:i1, k])
            E[k] += pc[i0:i1, k][:, None]
            E[k] += pa[:i1, k][None, :]
            np.exp(E[k], out=E[k])
            M[k] = np.outer(m[i0:i1, k], m[:i1, k])
        ii = np.arange(i0, i1)[:, None]
        jj = cols[None, :i1]
        wgt = np.where(jj < ii, 1.0 if defect == "offdiag1" else 2.0, np.where(jj == ii, 1.0, 0.0))
        if pair is not None:
            lo, hi = min(pair), max(pair)
            if i0 <= hi < i1:
                wgt[hi - i0, lo] = 0.0
        b = (v * v) * np.outer(be[i0:i1], be[:i1]) * wgt.astype(dt)
        ab = np.abs(b)
        sufE, sufM = _suffix(E), _suffix(M)
        preE, preM = np.ones_like(b), np.ones_like(b)        # the products of the coordinates before k
        if defect == "allprod":
            allE, allM = sufE[0] * E[0], sufM[0] * M[0]
        for k in range(d):
            D, S = E[k] - M[k], E[k] + M[k]
            looM = allM if defect == "allprod" else preM * sufM[k]
            looE = allE if defect == "allprod" else preE * sufE[k]
            F[k] += np.einsum("ij,ij,ij->", b, looM, D)
            aF[k] += np.einsum("ij,ij,ij->", ab, looM, S)
            T[k] += np.einsum("ij,ij,ij->", b, looE, D)
            aT[k] += np.einsum("ij,ij,ij->", ab, looE, S)
            preE, preM = preE * E[k], preM * M[k]
        V += (b * (preE - preM)).sum()
        aV += (ab * (preE + preM)).sum()
        return V, aV, F, aF, T, aT

    # the row blocks on a few threads (numpy's loops release the interpreter lock); their sums are added in block order
    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        parts = list(pool.map(block, range(0, N, rows)))
    V, aV, F, aF, T, aT = (sum((p[q] for p in parts[1:]), parts[0][q]) for q in range(6))
    out["V"] = (np.array([V], dt), np.array([aV], dt))
    out["first"] = (F, aF)
    out["total"] = (T, aT)
    return out


def both(x, theta, beta, u, s):
    return sums(x, theta, beta, u, s), sums(x, theta, beta, u, s, dt=np.float64)


def ref_distances(want, ref):
    return {k: dl.distances(ref[k][0], want[k][0], want[k][1]) for k in KEYS}


# ------------------------------------------------------------------------------------------------
# the definitions by tensor Gauss-Hermite quadrature (d <= 3)
# ------------------------------------------------------------------------------------------------
def quadrature(x, theta, beta, u, s, order=60):
    """(mean, V, first [d], total [d]) in long double: mu on the tensor grid of `order` nodes per coordinate, then
    first_k = Var_{x_k}(E[mu | x_k]) and total_k = E[Var_{x_k}(mu | x_~k)] = E[mu^2] - E_{x_~k}[(E_{x_k} mu)^2] by contraction"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, _vt, w = dl.params(theta, d, LD)
    z, q = np.polynomial.hermite_e.hermegauss(order)
    z, q = z.astype(LD), q.astype(LD)
    q = q / q.sum()
    be = np.asarray(beta, dtype=np.float64).astype(LD)
    fac = []                                                  # per coordinate [N, order]: the kernel factor at the nodes
    for k in range(d):
        node = LD(u[k]) + np.sqrt(LD(s[k])) * z
        fac.append(np.exp(-w[k] * (node[None, :] - xr[:, k].astype(LD)[:, None]) ** 2 / 2))
    mu = v * be
    letters = "abc"[:d]
    mu = np.einsum("i," + ",".join("i" + c for c in letters) + "->" + letters, mu, *fac)        # [order] * d
    wts = [q] * d
    full = lambda T: np.einsum(letters + "," + ",".join(letters) + "->", T, *wts)              # noqa: E731
    mean = full(mu)
    e2 = full(mu * mu)
    first, total = np.empty(d, LD), np.empty(d, LD)
    for k in range(d):
        others = [c for c in letters if c != letters[k]]
        # E[mu | x_k]: contract the other axes
        cond = np.einsum(letters + ("," + ",".join(others) if others else "") + "->" + letters[k], mu, *[q for _ in others])
        first[k] = (q * cond * cond).sum() - mean * mean
        # E_{x_k}[mu | x_~k]: contract axis k
        rest = np.einsum(letters + "," + letters[k] + "->" + "".join(others), mu, q)
        inner = np.einsum("".join(others) + ("," + ",".join(others) if others else "") + "->", rest * rest, *[q for _ in others])
        total[k] = e2 - inner
    return mean, e2 - mean * mean, first, total


# ------------------------------------------------------------------------------------------------
# the inputs of tests/test_sensitivity.py
# ------------------------------------------------------------------------------------------------
def variances(d, seed):
    """the s of a case: drawn in [0.01, 4]; the same with zeros in some coordinates (every other one, and at least one); 1e-10 everywhere
    (cancellation: E_k - m_k ~ 1e-10 of its terms); 100"""
    rng = np.random.RandomState(seed + 23)
    drawn = rng.uniform(0.01, 4.0, d)
    zeros = drawn.copy()
    zeros[::2] = 0.0
    return {"drawn": drawn, "zeros": zeros, "tiny": np.full(d, 1e-10), "large": np.full(d, 100.0)}


def combos(x, theta, seed):
    """[(name, u, s)]: the three inputs of _dense_ld.inputs_u under the drawn s, the input between the points under the other three"""
    d = x.shape[1]
    us, ss = dl.inputs_u(x, theta, seed), variances(d, seed)
    out = [("%s/drawn" % un, u, ss["drawn"]) for un, u in us.items()]
    out += [("between/%s" % sn, us["between"], ss[sn]) for sn in ("zeros", "tiny", "large")]
    return out
