"""A long-double model of PeriodicCovariance (scikit-gpuppy_amd/csrc/periodic.hip): the kernel, its theta derivatives and the 3 d + 2
sums of the likelihood gradient in np.longdouble (x87, eps 1.08e-19) from DIRECT differences of the raw inputs, the seeded cases of
tests/test_periodic.py, and the rules those tests compare by.  Host only.

  theta = (log v, log vt, log w_1..d, log p_1..d, log w2_1..d);  delta = xi - xj
  q = 1/2 sum_k [ w_k delta_k^2 + w2_k sin^2(pi delta_k / p_k) ],  Kf = v exp(-q),  K = Kf + (vt iff delta == 0 in every component)
  dK/dtheta: Kf | vt on equality | -1/2 w_k delta_k^2 Kf | (pi delta_k w2_k / p_k) sin cos Kf | -1/2 w2_k sin^2 Kf        (reference :399-433)
  gradient sums over all (i, j), M = Kinv - alpha alpha^T:  S_0 = sum M Kf,  A_k = sum M Kf delta_k^2,  B_k = sum M Kf delta_k sin cos,
  C_k = sum M Kf sin^2,  T = sum over the pairs with x_i == x_j of M;  g_0 = S_0 / 2, g_1 = vt T / 2, g_w = -w A / 4,
  g_p = (pi w2 / p) B / 2, g_w2 = -w2 C / 4.

The parameters are exp(theta) in float64 -- what the device holds -- then widened.  dt = np.float64 evaluates the same formulas the way
the reference writes them (np.sin(np.pi / p * diff)): rho_K and rho_ref are measured on that evaluation, never on a device result.

Rules.
  Gram: |K - K_ld| in units of u K_ld (1 + q), u = 2^-53; the device passes within GRAM_MARGIN * max(rho_K, GRAM_FLOOR).
  Derivatives: the same bound times the derivative's factor with its oscillating part at its maximum -- 1, (exact), 1/2 w delta^2,
    1/2 pi |delta| w2 / p, 1/2 w2.  (sin^2 and sin cos are functions of t = delta / p whose rounding moves them by pi u |t| ABSOLUTELY, however
    small they are: near their zeros no evaluation that rounds delta / p is relatively accurate, the float64 one included.)
  Gradient: tests/_dense_ld.py's rule (distance = |got - model| / sum of the absolute terms, MARGIN * max(rho_ref, FLOOR)).

`defect=` plants one of the seeded defects of tests/test_periodic_model.py in an evaluation (meant for dt = np.float64)."""
import numpy as np

from _dense_ld import FLOOR, LD, MARGIN, ROWS, _grid, assert_within, bound, distances  # noqa: F401  (the project's one rule: imported)

U = 2.0 ** -53
PI_LD = LD("3.14159265358979323846264338327950288")
GRAM_MARGIN, GRAM_FLOOR = 8.0, 4.0
D_ALL = (1, 2, 3, 8, 9, 16, 17, 64)            # 8 | 9 and 16 | 17: on each side of a sweep boundary of the gradient pass (8 coordinates a sweep)
GRAM_SHAPES = ((130, 257), (257, 130), (1, 1), (128, 128), (64, 129))
GRAD_N = (130, 257, 700)
FIT_CASES = ((130, 1), (203, 3), (257, 8), (130, 64))
GOLDEN_CASES = ((130, 1), (203, 3))
DEFECTS = ("sin32", "novt", "swap", "sign", "unreduced")


def gram_bound(rho_K):
    return GRAM_MARGIN * max(rho_K, GRAM_FLOOR)


def make_theta(d, rng):
    """v = 2, vt = 0.01, w_k in [0.02, 0.2] / d, p_k in [1.5, 4], w2_k in [0.5, 3] / d"""
    w = rng.uniform(0.02, 0.2, d) / d
    p = rng.uniform(1.5, 4.0, d)
    w2 = rng.uniform(0.5, 3.0, d) / d
    return np.log(np.concatenate([[2.0, 0.01], w, p, w2]))


def seed_of(N, d):
    return 7000 + 1000 * d + N


def make_case(N, d, seed=None):
    """(x, t centred, theta): x uniform in [0, 10]^d on the 2^-20 grid"""
    rng = np.random.RandomState(seed_of(N, d) if seed is None else seed)
    x = _grid(rng.uniform(0, 10, (N, d)))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    return x, t - t.mean(), make_theta(d, rng)


def make_gram_case(n1, n2, d):
    """(xi, xj, theta); from the fourth row on every seventh row of xi equals a row of xj (the +vt quirk off the diagonal)"""
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
    th = np.asarray(theta, dtype=np.float64)
    with np.errstate(divide="ignore"):
        e = np.exp(th)
    return dt(e[0]), dt(e[1]), e[2:2 + d].astype(dt), e[2 + d:2 + 2 * d].astype(dt), e[2 + 2 * d:2 + 3 * d].astype(dt)


def _taylor_sin(t):
    """the degree-23 Taylor polynomial of sin(pi t) -- good on |t| <= 1/2 only (the 'unreduced' defect applies it to t itself)"""
    out, term, x = np.zeros_like(t), np.pi * t, np.pi * t
    for k in range(12):
        out = out + term
        term = -term * x * x / ((2 * k + 2) * (2 * k + 3))
    return out


def sincos(delta, pk, dt, defect=None):
    """(sin, cos) of pi delta / p_k: in long double from the quotient; in float64 as the reference forms it, np.pi / p * diff"""
    if dt is LD:
        a = PI_LD * (delta / pk)
        return np.sin(a), np.cos(a)
    a = np.pi / pk * delta
    if defect == "sin32":
        return np.sin(a.astype(np.float32)).astype(dt), np.cos(a.astype(np.float32)).astype(dt)
    if defect == "unreduced":
        return _taylor_sin(delta / pk), np.cos(a)
    return np.sin(a), np.cos(a)


def kernel_parts(xi, xj, theta, dt=LD, defect=None, keep=False):
    """{"K", "Kf", "q", "eq"} [n1, n2] and, with keep, "delta", "sin", "cos" [d, n1, n2]"""
    a, b = np.asarray(xi, dtype=np.float64), np.asarray(xj, dtype=np.float64)
    d = a.shape[1]
    v, vt, w, p, w2 = params(theta, d, dt)
    if defect == "swap":
        p, w2 = w2, p
    q = np.zeros((a.shape[0], b.shape[0]), dt)
    eq = np.ones(q.shape, bool)
    D, S, C = [], [], []
    for k in range(d):
        delta = a[:, k].astype(dt)[:, None] - b[:, k].astype(dt)[None, :]
        sn, cs = sincos(delta, p[k], dt, defect)
        q += w[k] * delta * delta + w2[k] * sn * sn
        eq &= (a[:, k][:, None] == b[:, k][None, :])
        if keep:
            D.append(delta), S.append(sn), C.append(cs)
    q = q / 2
    Kf = v * np.exp(-q)
    out = {"K": Kf + (0 if defect == "novt" else vt) * eq.astype(dt), "Kf": Kf, "q": q, "eq": eq}
    if keep:
        out.update(delta=np.array(D), sin=np.array(S), cos=np.array(C))
    return out


def gram_units(K, parts):
    """|K - K_ld| / (u K_ld (1 + q)) entry by entry (parts: the long-double kernel_parts)"""
    return (np.abs(np.asarray(K).astype(LD) - parts["K"]) / (LD(U) * parts["K"] * (1 + parts["q"]))).astype(np.float64)


def deriv(parts, theta, j, dt=LD, defect=None):
    """(d K / d theta_j, its scale for the rule above) from kernel_parts(..., keep=True) of the same dt"""
    d = parts["delta"].shape[0]
    v, vt, w, p, w2 = params(theta, d, dt)
    Kf = parts["Kf"]
    if j == 0:
        return Kf, Kf
    if j == 1:
        return vt * parts["eq"].astype(dt), vt * parts["eq"].astype(dt)      # (0 off the equal pairs: those entries must be exact zeros)
    kind, k = (j - 2) // d, (j - 2) % d
    delta, sn, cs = parts["delta"][k], parts["sin"][k], parts["cos"][k]
    pi = PI_LD if dt is LD else dt(np.pi)
    if kind == 0:
        return -(w[k] / 2) * delta * delta * Kf, (w[k] / 2) * delta * delta * Kf
    if kind == 1:
        sgn = -1 if defect == "sign" else 1
        return sgn * (pi * delta * w2[k] / p[k]) * sn * cs * Kf, (pi * np.abs(delta) * w2[k] / p[k]) / 2 * Kf
    return -(w2[k] / 2) * sn * sn * Kf, (w2[k] / 2) * Kf


def deriv_units(dK, parts, theta, j):
    """|dK - dK_ld| in units of u (1 + q) scale_j; where the scale is 0 (j = 1 off the equal pairs) the entry must be exact: inf unless equal"""
    want, scale = deriv(parts, theta, j)
    diff = np.abs(np.asarray(dK).astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = diff / (LD(U) * (1 + parts["q"]) * scale)
    return np.where(diff == 0, LD(0), r).astype(np.float64)


# ------------------------------------------------------------------------------------------------
# the gradient
# ------------------------------------------------------------------------------------------------
def grad_sums(x, theta, Kinv, alpha, dt=LD, defect=None):
    """([S_0, A_1..d, B_1..d, C_1..d, T], their scales): every sum over ALL ordered pairs, taken from the j <= i half with weight 2 below
    the diagonal (each term is even in delta)"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    Ki, al = np.asarray(Kinv).astype(dt), np.asarray(alpha).astype(dt)
    S, A = np.zeros(3 * d + 2, dt), np.zeros(3 * d + 2, dt)
    for i0 in range(0, N, ROWS):
        i1 = min(N, i0 + ROWS)
        pr = kernel_parts(xr[i0:i1], xr[:i1], theta, dt, defect, keep=True)
        wgt = np.where(np.arange(i1)[None, :] < np.arange(i0, i1)[:, None], 2.0, np.where(np.arange(i1)[None, :] == np.arange(i0, i1)[:, None], 1.0, 0.0)).astype(dt)
        M = (Ki[i0:i1, :i1] - np.outer(al[i0:i1], al[:i1])) * wgt
        Ma = (np.abs(Ki[i0:i1, :i1]) + np.outer(np.abs(al[i0:i1]), np.abs(al[:i1]))) * wgt
        MK, AK = M * pr["Kf"], Ma * pr["Kf"]
        S[0] += MK.sum()
        A[0] += AK.sum()
        S[3 * d + 1] += (M * pr["eq"]).sum()
        A[3 * d + 1] += (Ma * pr["eq"]).sum()
        sgn = -1 if defect == "sign" else 1
        for k in range(d):
            de, sn, cs = pr["delta"][k], pr["sin"][k], pr["cos"][k]
            S[1 + k] += (MK * de * de).sum()
            A[1 + k] += (AK * de * de).sum()
            S[1 + d + k] += sgn * (MK * de * sn * cs).sum()
            A[1 + d + k] += (AK * np.abs(de * sn * cs)).sum()
            S[1 + 2 * d + k] += (MK * sn * sn).sum()
            A[1 + 2 * d + k] += (AK * sn * sn).sum()
    return S, A


def grad_from_sums(S, A, theta):
    """(gradient [2 + 3 d], scales) as gpx_periodic_nll_grad combines the sums"""
    d = (len(S) - 2) // 3
    dt = S.dtype.type
    _v, vt, w, p, w2 = params(theta, d, dt)
    pi = PI_LD if dt is LD else dt(np.pi)
    g, s = np.empty_like(S), np.empty_like(A)
    g[0], s[0] = S[0] / 2, A[0] / 2
    g[1], s[1] = vt * S[3 * d + 1] / 2, vt * A[3 * d + 1] / 2
    g[2:2 + d], s[2:2 + d] = -w * S[1:1 + d] / 4, w * A[1:1 + d] / 4
    g[2 + d:2 + 2 * d], s[2 + d:2 + 2 * d] = (pi * w2 / p) * S[1 + d:1 + 2 * d] / 2, (pi * w2 / p) * A[1 + d:1 + 2 * d] / 2
    g[2 + 2 * d:], s[2 + 2 * d:] = -w2 * S[1 + 2 * d:1 + 3 * d] / 4, w2 * A[1 + 2 * d:1 + 3 * d] / 4
    return g, s


def grad(x, theta, Kinv, alpha, dt=LD, defect=None):
    return grad_from_sums(*grad_sums(x, theta, Kinv, alpha, dt, defect), theta=theta)


def nll(K, t):
    """N/2 log 2 pi + 1/2 log det K + 1/2 t^T K^-1 t in float64 (numpy's Cholesky)"""
    L = np.linalg.cholesky(K)
    y = np.linalg.solve(L, t)
    return 0.5 * len(t) * np.log(2 * np.pi) + np.log(np.diag(L)).sum() + 0.5 * y.dot(y)
