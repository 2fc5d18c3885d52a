"""A long-double model of MaternCovariance (scikit-gpuppy_amd/csrc/matern.hip): the kernel for nu = 3/2 and 5/2, its theta and input
derivatives and the d + 2 sums of the likelihood gradient in np.longdouble (x87, eps 1.08e-19) from DIRECT differences of the raw inputs,
the seeded cases of tests/test_matern.py, and the rules those tests compare by.  Host only.

  theta = (log v, log vt, log w_1..d);  delta = xi - xj,  q = sum_k w_k delta_k^2,  s = sqrt(2 nu q),  nu2 = 2 nu
  nu2 = 5: Kf = v (1 + s + s^2 / 3) exp(-s),  G = (5/3) v (1 + s) exp(-s)        nu2 = 3: Kf = v (1 + s) exp(-s),  G = 3 v exp(-s)
  K = Kf + (vt iff delta == 0 in every component)
  dK/dtheta: Kf | vt on equality | -1/2 w_k delta_k^2 G
  nu2 = 5, diff = xi - u:  J_k = -diff_k w_k G,  H_kl = (5/3) v exp(-s) [5 (w_k diff_k)(w_l diff_l) - [k == l] w_k (1 + s)]
  gradient sums over all (i, j), M = Kinv - alpha alpha^T:  S_0 = sum M Kf,  A_k = sum M G delta_k^2,  T = sum over the pairs with
  x_i == x_j of M;  g_0 = S_0 / 2, g_1 = vt T / 2, g_{2+k} = -w_k A_k / 4.

The parameters are exp(theta) in float64 -- what the device holds -- then widened.  dt = np.float64 evaluates the same formulas in plain
numpy: rho_K and rho_ref are measured on that evaluation, never on a device result.

Rules.
  Gram: |K - K_ld| in units of u K_ld (1 + s), u = 2^-53 (the exponent s carries a relative rounding error, exp(-s) one of s times it);
    the device passes within GRAM_MARGIN * max(rho_K, GRAM_FLOOR).
  Derivatives: the same bound times the derivative's factor: Kf, (exact), 1/2 w_k delta_k^2 G.
  Gradient: tests/_dense_ld.py's rule (distance = |got - model| / sum of the absolute terms, MARGIN * max(rho_ref, FLOOR)).

`defect=` plants one of the seeded defects of tests/test_matern_model.py in an evaluation (meant for dt = np.float64)."""
import numpy as np

from _dense_ld import FLOOR, LD, MARGIN, ROWS, _grid, assert_within, bound, distances  # noqa: F401  (the project's one rule: imported)

U = 2.0 ** -53
GRAM_MARGIN, GRAM_FLOOR = 8.0, 4.0
NU2_ALL = (3, 5)
D_ALL = (1, 2, 3, 8, 9, 16, 17, 64)            # 8 | 9 and 16 | 17: on each side of a sweep boundary of the gradient pass (8 coordinates a sweep)
GRAM_SHAPES = ((130, 257), (257, 130), (1, 1), (128, 128), (64, 129))
GRAD_N = (130, 257, 700)
FIT_CASES = ((130, 1), (203, 3), (257, 8), (130, 64))
DEFECTS = ("poly32", "nos2", "novt", "diagvt", "exp32", "sign")


def gram_bound(rho_K):
    return GRAM_MARGIN * max(rho_K, GRAM_FLOOR)


def make_theta(d, rng):
    """v = 2, vt = 0.01, w_k in [0.02, 0.2] / d"""
    return np.log(np.concatenate([[2.0, 0.01], rng.uniform(0.02, 0.2, d) / d]))


def seed_of(N, d):
    return 7000 + 1000 * d + N


def make_case(N, d, seed=None):
    """(x, t centred, theta): x uniform in [0, 10]^d on the 2^-20 grid"""
    rng = np.random.RandomState(seed_of(N, d) if seed is None else seed)
    x = _grid(rng.uniform(0, 10, (N, d)))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    return x, t - t.mean(), make_theta(d, rng)


def make_gram_case(n1, n2, d):
    """(xi, xj, theta); from the fourth row on every seventh row of xi equals a row of xj (the +vt off the diagonal)"""
    rng = np.random.RandomState(90000 + 1000 * d + 7 * n1 + n2)
    xi, xj = _grid(rng.uniform(0, 10, (n1, d))), _grid(rng.uniform(0, 10, (n2, d)))
    for i in range(3, n1, 7):
        xi[i] = xj[(5 * i) % n2]
    return xi, xj, make_theta(d, rng)


def make_queries(x, m, seed):
    """m queries in [0, 10]^d, query 3 bit-equal to training row 5"""
    rng = np.random.RandomState(seed)
    xs = _grid(rng.uniform(0, 10, (m, x.shape[1])))
    if m > 3:
        xs[3] = x[5 % len(x)]
    return xs


def params(theta, d, dt=LD):
    """(v, vt, w): exp(theta) in float64 -- the parameters the device holds -- then widened"""
    th = np.asarray(theta, dtype=np.float64)
    if th.shape != (2 + d,):
        raise ValueError("theta must have 2 + d = %d entries" % (2 + d))
    with np.errstate(divide="ignore"):
        e = np.exp(th)
    return dt(e[0]), dt(e[1]), e[2:2 + d].astype(dt)


def radial(q, v, nu2, dt=LD, defect=None):
    """(s, Kf, G, e = v exp(-s)) at q"""
    s = np.sqrt(dt(nu2) * q)
    ex = np.exp(-s.astype(np.float32)).astype(dt) if defect == "exp32" else np.exp(-s)
    e = v * ex
    if nu2 == 5 and defect != "poly32":
        Kf = e * (1 + s + (0 if defect == "nos2" else s * s / 3))
        G = dt(5) / 3 * e * (1 + s)
    else:
        Kf, G = e * (1 + s), 3 * e
    return s, Kf, G, e


def kernel_parts(xi, xj, theta, nu2, dt=LD, defect=None, keep=False):
    """{"K", "Kf", "G", "e", "q", "s", "eq"} [n1, n2] and, with keep, "delta" [d, n1, n2]"""
    a, b = np.asarray(xi, dtype=np.float64), np.asarray(xj, dtype=np.float64)
    d = a.shape[1]
    v, vt, w = params(theta, d, dt)
    q = np.zeros((a.shape[0], b.shape[0]), dt)
    eq = np.ones(q.shape, bool)
    D = []
    for k in range(d):
        delta = a[:, k].astype(dt)[:, None] - b[:, k].astype(dt)[None, :]
        q += w[k] * delta * delta
        eq &= (a[:, k][:, None] == b[:, k][None, :])
        if keep:
            D.append(delta)
    s, Kf, G, e = radial(q, v, nu2, dt, defect)
    where_vt = eq
    if defect == "novt":
        where_vt = np.zeros(q.shape, bool)
    elif defect == "diagvt":
        where_vt = np.eye(*q.shape, dtype=bool)
    out = {"K": Kf + vt * where_vt.astype(dt), "Kf": Kf, "G": G, "e": e, "q": q, "s": s, "eq": eq}
    if keep:
        out["delta"] = np.array(D)
    return out


def gram_units(K, parts):
    """|K - K_ld| / (u K_ld (1 + s)) entry by entry (parts: the long-double kernel_parts)"""
    return (np.abs(np.asarray(K).astype(LD) - parts["K"]) / (LD(U) * parts["K"] * (1 + parts["s"]))).astype(np.float64)


def deriv(parts, theta, j, dt=LD, defect=None):
    """(d K / d theta_j, its scale for the rule above) from kernel_parts(..., keep=True) of the same dt"""
    d = parts["delta"].shape[0]
    _v, vt, w = params(theta, d, dt)
    if j == 0:
        return parts["Kf"], parts["Kf"]
    if j == 1:
        return vt * parts["eq"].astype(dt), vt * parts["eq"].astype(dt)      # (0 off the equal pairs: those entries must be exact zeros)
    delta = parts["delta"][j - 2]
    scale = (w[j - 2] / 2) * delta * delta * parts["G"]
    return (1 if defect == "sign" else -1) * scale, scale


def deriv_units(dK, parts, theta, j):
    """|dK - dK_ld| in units of u (1 + s) scale_j; where the scale is 0 the entry must be exact: inf unless equal"""
    want, scale = deriv(parts, theta, j)
    diff = np.abs(np.asarray(dK).astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = diff / (LD(U) * (1 + parts["s"]) * scale)
    return np.where(diff == 0, LD(0), r).astype(np.float64)


def jacobian_hessian(u, x, theta, dt=LD):
    """nu = 5/2: (J [n, d], H [n, d, d]) of the noise-free kernel at the rows of x, diff = x_i - u"""
    xr = np.asarray(x, dtype=np.float64)
    d = xr.shape[1]
    v, _vt, w = params(theta, d, dt)
    diff = xr.astype(dt) - np.asarray(u, dtype=np.float64).astype(dt)[None, :]
    wd = diff * w[None, :]
    s, _Kf, G, e = radial((wd * diff).sum(1), v, 5, dt)
    J = -wd * G[:, None]
    H = (dt(5) / 3 * e)[:, None, None] * (5 * wd[:, :, None] * wd[:, None, :] - (1 + s)[:, None, None] * np.diag(w)[None])
    return J, H


# ------------------------------------------------------------------------------------------------
# the gradient
# ------------------------------------------------------------------------------------------------
def grad_sums(x, theta, nu2, Kinv, alpha, dt=LD, defect=None):
    """([S_0, A_1..d, T], their scales): every sum over ALL ordered pairs, taken from the j <= i half with weight 2 below the diagonal
    (each term is even in delta)"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    Ki, al = np.asarray(Kinv).astype(dt), np.asarray(alpha).astype(dt)
    S, A = np.zeros(d + 2, dt), np.zeros(d + 2, dt)
    for i0 in range(0, N, ROWS):
        i1 = min(N, i0 + ROWS)
        pr = kernel_parts(xr[i0:i1], xr[:i1], theta, nu2, dt, defect, keep=True)
        cols, rows = np.arange(i1)[None, :], np.arange(i0, i1)[:, None]
        wgt = np.where(cols < rows, 2.0, np.where(cols == rows, 1.0, 0.0)).astype(dt)
        M = (Ki[i0:i1, :i1] - np.outer(al[i0:i1], al[:i1])) * wgt
        Ma = (np.abs(Ki[i0:i1, :i1]) + np.outer(np.abs(al[i0:i1]), np.abs(al[:i1]))) * wgt
        S[0] += (M * pr["Kf"]).sum()
        A[0] += (Ma * pr["Kf"]).sum()
        S[d + 1] += (M * pr["eq"]).sum()
        A[d + 1] += (Ma * pr["eq"]).sum()
        MG, AG = M * pr["G"], Ma * pr["G"]
        for k in range(d):
            de = pr["delta"][k]
            S[1 + k] += (-1 if defect == "sign" else 1) * (MG * de * de).sum()
            A[1 + k] += (AG * de * de).sum()
    return S, A


def grad_from_sums(S, A, theta):
    """(gradient [2 + d], scales) as gpx_matern_nll_grad combines the sums"""
    d = len(S) - 2
    dt = S.dtype.type
    _v, vt, w = params(theta, d, dt)
    g, s = np.empty_like(S), np.empty_like(A)
    g[0], s[0] = S[0] / 2, A[0] / 2
    g[1], s[1] = vt * S[d + 1] / 2, vt * A[d + 1] / 2
    g[2:], s[2:] = -w * S[1:1 + d] / 4, w * A[1:1 + d] / 4
    return g, s


def grad(x, theta, nu2, Kinv, alpha, dt=LD, defect=None):
    return grad_from_sums(*grad_sums(x, theta, nu2, Kinv, alpha, dt, defect), theta=theta)


def nll(K, t):
    """N/2 log 2 pi + 1/2 log det K + 1/2 t^T K^-1 t in float64 (numpy's Cholesky)"""
    L = np.linalg.cholesky(K)
    y = np.linalg.solve(L, t)
    return 0.5 * len(t) * np.log(2 * np.pi) + np.log(np.diag(L)).sum() + 0.5 * y.dot(y)
