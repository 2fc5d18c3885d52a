"""A long-double model of the two kernel stages at the ends of the batched calls (gpx_propagate_approx_many, gpx_propagate_dvh_many,
gpx_predict_grad, gpx_matern_propagate_*_many): the right-hand-side rows that the build kernels write (scikit-gpuppy_amd/csrc/propagate.hip,
matern.hip) and the row reductions (propagate.hip, predict_grad.hip), the seeded inputs of tests/test_rows.py and the two rules those tests
compare by.  Host only.  The device side is reached through gpx_rows_build / gpx_rows_reduce (include/gpx.h, test / tool access).

Rows.  With delta = x_i - u (DIRECT differences of the raw inputs), a = w delta, q = sum_k w_k delta_k^2 and the radial factors of the kind
  kind 0 (Gaussian): c = g = v exp(-q / 2)                                                    (_predict_grad_model.radial)
  kind 5 (Matern 5/2): s = sqrt(5 q), c = v (1 + s + s^2 / 3) exp(-s), g = (5/3) v (1 + s) exp(-s), f = (5/3) v exp(-s)   (_matern_ld.radial)
  kind 3 (Matern 3/2): s = sqrt(3 q), c = v (1 + s) exp(-s), g = 3 v exp(-s)                  (GRAD alone: no Hessian at the origin)
the rows of an input are
  C      c (+ vt iff x_i == u elementwise: Gaussian APPROX and DVH, Matern every layout; a Gaussian GRAD row carries none, it is gpx_predict's)
  J_k    -a_k g
  H_kk   Gaussian (a_k^2 - w_k) c                        Matern f (5 a_k^2 - w_k (1 + s))
  tr     Gaussian c (a^T Sigma a - sum_k w_k Sigma_kk)   Matern f (5 a^T Sigma a - (1 + s) sum_k w_k Sigma_kk)      (= tracedot(H, Sigma), full Sigma)
in the layouts APPROX [C, tr, J_1..J_d], DVH [C, J_1..J_d, H_11..H_dd], GRAD [C, J_1..J_d], input b at rows b nrow .., in a block of
round_up(B nrow, 128) rows and npad = round_up(N, 128) columns.  rows() returns (values, scales, q) of the whole block; an entry's scale is the
sum of the absolute values of its terms,
  C: c (+ vt)     J_k: |a_k| g     H_kk: (a_k^2 + w_k) c resp. f (5 a_k^2 + w_k (1 + s))
  tr: c (|a|^T |Sigma| |a| + sum_k w_k |Sigma_kk|) resp. f (5 |a|^T |Sigma| |a| + (1 + s) sum_k w_k |Sigma_kk|)
and 0 in the padded columns, in the rows of the last tile past B nrow and at J where delta_k = 0.

Rule for rows: the Gram rule of tests/_gauss_ld.py without its prescale term (these kernels difference the raw inputs):
    distance = |got - model| / (u scale (1 + q)),  u = 2^-53;  where the scale is 0 the entry must be exactly 0 (distance inf otherwise)
and the device passes when every entry is within gram_bound(rho) = GRAM_MARGIN * max(rho, GRAM_FLOOR) (tests/_periodic_ld.py's constants,
imported), rho the worst distance of the float64 evaluation (dt = np.float64: the same formulas in plain numpy) over every case of
all_cases().  Nothing is fitted to a device result.  The q term: the rounding of the exponent's argument and of each step of the sum that forms
q costs a relative error of order q u in exp(-q / 2); for Matern the argument is s = sqrt(nu2 q) <= 1 + q, so the same term covers it.

Reductions.  reduce_model() evaluates the three reduce formulas on given solved rows Zs, y and Sigma
  APPROX  mean = z_C.y + 1/2 z_tr.y   sigma2 = (v + vt) - |z_C|^2   rest = -sum_k Sigma_kk (|z_Jk|^2 - (z_Jk.y)^2) - z_C.z_tr   var = sigma2 + rest
  DVH     dvh_k = -(|z_Jk|^2 - (z_Jk.y)^2) - z_C.z_Hkk   sigma2 as above
  GRAD    mean = z_C.y   var = (v + vt) - |z_C|^2   dmean_k = -z_Jk.y   dvar_k = 2 z_C.z_Jk
as {name: (values, scales)}: each sum on the scale of its absolute terms, a combined output on the same combination of its parts' scales
(dvh_k: |z_Jk|^2 + (|z_Jk|.|y|)^2 + |z_C|.|z_Hkk|).  The rule is tests/_dense_ld.py's (distances, rho_of, assert_within: imported), rho_ref the
float64 evaluation's of the same case.

Seeded inputs (make_case): the 2^-20 grid and the laws of _dense_ld.make_case for every kind; eight inputs a case -- _dense_ld.inputs_u's three
(between, bit-equal to training row 5, far: q about 600 to 760), a training row with its last coordinate moved, a training row with its first
coordinate moved, u = 0 exactly (the padded columns of x are 0: the input that would put +vt there without the kernels' column guard), two
random ones -- and pairwise distinct Sigmas, full SPD from d = 2 on, diagonal at d = 1.

`defect=` plants one of ROW_DEFECTS / REDUCE_DEFECTS in an evaluation (meant for dt = np.float64; tests/test_rows_model.py)."""
import functools
import os

import numpy as np

import _dense_ld as dl
import _matern_ld as ml
import _predict_grad_model as pg
from _dense_ld import LD, _grid, assert_within, distances, rho_of  # noqa: F401  (the project's one rule for sums: imported, not copied)
from _periodic_ld import GRAM_FLOOR, GRAM_MARGIN, gram_bound  # noqa: F401  (the project's constants for entries: imported, not copied)

U = 2.0 ** -53
APPROX, DVH, GRAD = 0, 1, 2                      # GPX_ROWS_* of include/gpx.h
LAYOUT_NAMES = {APPROX: "approx", DVH: "dvh", GRAD: "grad"}
KINDS = pg.KINDS                                 # nu2: 0 = the Gaussian kernel, 3, 5
KIND_NAMES = {0: "gauss", 3: "matern32", 5: "matern52"}
LAYOUTS_OF = {0: (APPROX, DVH, GRAD), 5: (APPROX, DVH, GRAD), 3: (GRAD,)}
D_ALL = (1, 3, 8, 9, 17, 64)                     # 1, 3, 8: DR = 8 (k < d live at 1 and 3); 9, 17, 64: DR = 0
N_SMALL = (128, 129, 200)                        # no padding | 127 padded columns, in0 true and in1 false in the last pair | a partial tile
CASES = [(N, d) for d in D_ALL for N in N_SMALL] + [(700, 3), (700, 9)]
NB = 8                                           # inputs a case
INPUT_NAMES = ("between", "equal", "far", "but_last", "but_first", "zero", "random0", "random1")
ROW_DEFECTS = ("jsign", "h_now", "h_nos", "tr_diag", "tr_sigma0", "flag0", "vt_pad", "vt_grad", "exp32", "coord")
REDUCE_DEFECTS = ("tail512", "quarter", "nosquare", "sigma0", "dvar1", "trhalf")
REDUCE_NPAD = (128, 256, 768, 1024)              # fewer than one stride of 512 | half a stride | one and a half | two
REDUCE_D = (1, 8, 9, 64)
REDUCE_B = 5


def round_up(a, b):
    return (a + b - 1) // b * b


def nrow_of(layout, d):
    return {APPROX: d + 2, DVH: 2 * d + 1, GRAD: d + 1}[layout]


def has_vt(kind, layout):
    """does the C row carry +vt on equality: the kind's own convention (tests/test_predict_grad.py's docstring)"""
    return kind != 0 or layout != GRAD


# ------------------------------------------------------------------------------------------------
# seeded inputs
# ------------------------------------------------------------------------------------------------
def make_case(N, d):
    """(x [N, d], t centred, theta, U [NB, d], Sigma [NB, d, d])"""
    seed = dl.seed_of(N, d)
    x, t, theta = dl.make_case(N, d, seed)
    ins = dl.inputs_u(x, theta, seed)
    rng = np.random.RandomState(seed + 29)
    but_last, but_first = x[7].copy(), x[9].copy()
    but_last[d - 1] += 0.5
    but_first[0] += 0.5
    Uin = np.vstack([ins["between"], ins["equal"], ins["far"], but_last, but_first, np.zeros(d), _grid(rng.uniform(0, 10, (2, d)))])
    Sig = np.array([dl.sigmas(d, seed + 100 * i)["full" if d >= 2 else "diag"] for i in range(NB)])
    return x, t, theta, Uin, Sig


def all_cases():
    """every (N, d, kind, layout) that tests/test_rows.py holds gpx_rows_build to the model on; rho is taken over these"""
    return [(N, d, kind, layout) for N, d in CASES for kind in KINDS for layout in LAYOUTS_OF[kind]]


# ------------------------------------------------------------------------------------------------
# the rows
# ------------------------------------------------------------------------------------------------
def parts(x, theta, Uin, kind, dt=LD, defect=None):
    """{"v", "vt", "w", "a" [B, N, d] = w delta, "q", "c", "g" [B, N], "same" [B, N] and for a Matern kind "s", "f"}"""
    xr, ur = np.asarray(x, dtype=np.float64), np.atleast_2d(np.asarray(Uin, dtype=np.float64))
    d = xr.shape[1]
    v, vt, w = pg.params(theta, d, dt)
    delta = xr.astype(dt)[None, :, :] - ur.astype(dt)[:, None, :]
    a = w * delta
    qk = a * delta
    q = qk[:, :, :d - 1].sum(2) if defect == "coord" else qk.sum(2)
    out = {"v": v, "vt": vt, "w": w, "a": a, "q": q}
    if kind == 0:
        if defect == "exp32":
            out["c"] = out["g"] = v * np.exp((-q / 2).astype(np.float32)).astype(dt)
        else:
            out["c"], out["g"] = pg.radial(q, v, 0, dt)
    else:
        s, c, g, e = ml.radial(q, v, kind, dt, "exp32" if defect == "exp32" else None)
        out.update(s=s, c=c, g=g, f=dt(5) / 3 * e)
    eq = xr[None, :, :] == ur[:, None, :]
    out["same"] = eq[:, :, 0] if defect == "flag0" else eq.all(2)
    return out


def rows(x, theta, Uin, Sigma, kind, layout, dt=LD, defect=None):
    """(values, scales, q), each [round_up(B nrow, 128), round_up(N, 128)]; Sigma [B, d, d] or one [d, d], read for APPROX alone"""
    if layout not in LAYOUTS_OF[kind]:
        raise ValueError("kind %d has no layout %d" % (kind, layout))
    xr, ur = np.asarray(x, dtype=np.float64), np.atleast_2d(np.asarray(Uin, dtype=np.float64))
    N, d = xr.shape
    B = len(ur)
    p = parts(xr, theta, ur, kind, dt, defect)
    a, c, g, w = p["a"], p["c"], p["g"], p["w"]
    nrow, npad = nrow_of(layout, d), round_up(N, 128)
    mp = round_up(B * nrow, 128)
    val, sca = np.zeros((B, nrow, npad), dt), np.zeros((B, nrow, npad), dt)
    vt_here = has_vt(kind, layout) != (defect == "vt_grad" and kind == 0 and layout == GRAD)
    C = c + (p["vt"] * p["same"].astype(dt) if vt_here else 0)
    val[:, 0, :N] = sca[:, 0, :N] = C
    if defect == "vt_pad" and vt_here:
        val[(ur == 0).all(1), 0, N:] = p["vt"]
    j0 = 2 if layout == APPROX else 1
    J = -a * g[:, :, None]
    val[:, j0:j0 + d, :N] = np.transpose(-J if defect == "jsign" else J, (0, 2, 1))
    sca[:, j0:j0 + d, :N] = np.transpose(np.abs(J), (0, 2, 1))
    if kind == 0:
        lead, five, one_s = c, dt(1), np.ones_like(c)            # H = lead (five a a^T - diag(w) one_s)
    else:
        lead, five, one_s = p["f"], dt(5), 1 + p["s"]
    if layout == DVH:
        ws = w[None, None, :] * one_s[:, :, None]                # diag(w) resp. diag(w) (1 + s)
        if defect == "h_now" and kind == 0:
            ws_got = 0 * ws
        elif defect == "h_nos" and kind != 0:
            ws_got = w[None, None, :] + 0 * ws
        else:
            ws_got = ws
        H = lead[:, :, None] * (five * a * a - ws_got)
        Habs = lead[:, :, None] * (five * a * a + ws)
        val[:, 1 + d:, :N], sca[:, 1 + d:, :N] = np.transpose(H, (0, 2, 1)), np.transpose(Habs, (0, 2, 1))
    if layout == APPROX:
        S = np.broadcast_to(np.asarray(Sigma, dtype=np.float64), (B, d, d)).astype(dt)
        if defect == "tr_sigma0":
            S = np.broadcast_to(S[0], (B, d, d))
        if defect == "tr_diag":
            S = S * np.eye(d, dtype=dt)
        aa = np.abs(a)
        quad = (np.matmul(a, np.transpose(S, (0, 2, 1))) * a).sum(2)
        aquad = (np.matmul(aa, np.transpose(np.abs(S), (0, 2, 1))) * aa).sum(2)
        dg = np.diagonal(S, axis1=1, axis2=2)
        wdiag, awdiag = (w * dg).sum(1)[:, None], (w * np.abs(dg)).sum(1)[:, None]
        val[:, 1, :N] = lead * (five * quad - one_s * wdiag)
        sca[:, 1, :N] = lead * (five * aquad + one_s * awdiag)
    Q = np.zeros((B, nrow, npad), dt)
    Q[:, :, :N] = p["q"][:, None, :]
    pad = lambda A: np.concatenate([A.reshape(B * nrow, npad), np.zeros((mp - B * nrow, npad), dt)])  # noqa: E731
    return pad(val), pad(sca), pad(Q)


def row_kinds(layout, d, B):
    """the name of every row of the block: "C", "tr", "J", "H" and "tile" for the rows of the last tile past B nrow"""
    one = {APPROX: ["C", "tr"] + ["J"] * d, DVH: ["C"] + ["J"] * d + ["H"] * d, GRAD: ["C"] + ["J"] * d}[layout]
    return np.array(one * B + ["tile"] * (round_up(B * len(one), 128) - B * len(one)))


def units(got, model):
    """an entry's distance |got - model| / (u scale (1 + q)); scale 0: 0 iff the entry is exactly the model's 0, inf otherwise"""
    want, scale, q = model
    g = np.asarray(got, dtype=np.float64)
    if g.shape != want.shape:
        raise ValueError("shape %r against %r" % (g.shape, want.shape))
    diff = np.abs(g.astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = (diff / (LD(U) * scale * (1 + q))).astype(np.float64)
    r = np.where(scale == 0, np.where(diff == 0, 0.0, np.inf), r)
    return np.where(np.isfinite(g), r, np.inf)


def worst_by_kind(dist, layout, d, B, N):
    """{row kind: the worst distance of its live columns} plus "padding": the padded columns of every row and the rows past B nrow"""
    names = row_kinds(layout, d, B)
    out = {k: float(dist[names == k][:, :N].max()) for k in ("C", "tr", "J", "H") if (names == k).any()}
    rest = [dist[:, N:].ravel(), dist[names == "tile"].ravel()]
    out["padding"] = float(max([r.max() for r in rest if r.size] + [0.0]))
    return out


@functools.lru_cache(maxsize=None)
def rho_all():
    """(rho, {case: the float64 evaluation's worst distance}) over all_cases()"""
    per = {}
    for N, d in CASES:
        x, _t, theta, Uin, Sig = make_case(N, d)
        for kind in KINDS:
            for layout in LAYOUTS_OF[kind]:
                f64 = rows(x, theta, Uin, Sig, kind, layout, dt=np.float64)[0]
                per[(N, d, kind, layout)] = float(units(f64, rows(x, theta, Uin, Sig, kind, layout)).max())
    return max(per.values()), per


def bound():
    return gram_bound(rho_all()[0])


# ------------------------------------------------------------------------------------------------
# the reductions
# ------------------------------------------------------------------------------------------------
def reduce_model(layout, d, Zs, y, Sigma, vplusvt, dt=LD, defect=None):
    """{name: (values, scales)} of B inputs; Zs [B nrow, npad], y [npad], Sigma [B, d, d] or one [d, d] (APPROX alone)"""
    nrow = nrow_of(layout, d)
    Z = np.asarray(Zs, dtype=np.float64)
    npad = Z.shape[1]
    B = Z.shape[0] // nrow
    Z, yy = Z.reshape(B, nrow, npad).astype(dt), np.asarray(y, dtype=np.float64).astype(dt)
    cols = np.arange(npad)
    if defect == "tail512":
        Z = Z * (cols < 512)
    elif defect == "quarter":                                       # wave 1 of 4: columns [128, 256) of every stride of 512
        Z = Z * ((cols % 512) // 128 != 1)
    aZ, ay = np.abs(Z), np.abs(yy)
    sq, zy, azy = (Z * Z).sum(2), Z.dot(yy), aZ.dot(ay)             # [B, nrow]
    kuu = dt(vplusvt)
    s2, as2 = kuu - sq[:, 0], np.abs(kuu) + sq[:, 0]
    j0 = 2 if layout == APPROX else 1
    sqJ, zyJ, azyJ = sq[:, j0:j0 + d], zy[:, j0:j0 + d], azy[:, j0:j0 + d]
    quadJ = sqJ - (zyJ if defect == "nosquare" else zyJ * zyJ)
    aquadJ = sqJ + azyJ * azyJ
    if layout == APPROX:
        S = np.broadcast_to(np.asarray(Sigma, dtype=np.float64), (B, d, d)).astype(dt)
        sd = np.diagonal(S[:1] if defect == "sigma0" else S, axis1=1, axis2=2)
        half = dt(1) if defect == "trhalf" else dt(1) / 2
        mean, amean = zy[:, 0] + half * zy[:, 1], azy[:, 0] + azy[:, 1] / 2
        ctr, actr = (Z[:, 0] * Z[:, 1]).sum(1), (aZ[:, 0] * aZ[:, 1]).sum(1)
        rest, arest = -(sd * quadJ).sum(1) - ctr, (np.abs(sd) * aquadJ).sum(1) + actr
        return {"mean": (mean, amean), "var": (s2 + rest, as2 + arest), "sigma2": (s2, as2), "rest": (rest, arest)}
    if layout == DVH:
        ch, ach = (Z[:, :1] * Z[:, 1 + d:]).sum(2), (aZ[:, :1] * aZ[:, 1 + d:]).sum(2)
        return {"dvh": (-quadJ - ch, aquadJ + ach), "sigma2": (s2, as2)}
    two = dt(1) if defect == "dvar1" else dt(2)
    cj, acj = (Z[:, :1] * Z[:, 1:]).sum(2), (aZ[:, :1] * aZ[:, 1:]).sum(2)
    return {"mean": (zy[:, 0], azy[:, 0]), "var": (s2, as2), "dmean": (-zyJ, azyJ), "dvar": (two * cj, 2 * acj)}


def unpack(layout, d, B, out):
    """gpx_rows_reduce's out as {name: values}"""
    o = np.asarray(out, dtype=np.float64)
    if layout == APPROX:
        return {"mean": o[:B], "var": o[B:2 * B], "sigma2": o[2 * B:3 * B], "rest": o[3 * B:4 * B]}
    if layout == DVH:
        return {"dvh": o[:B * d].reshape(B, d), "sigma2": o[B * d:B * d + B]}
    return {"mean": o[:B], "var": o[B:2 * B], "dmean": o[2 * B:2 * B + B * d].reshape(B, d), "dvar": o[2 * B + B * d:2 * B + 2 * B * d].reshape(B, d)}


def out_len(layout, d, B):
    return {APPROX: 4 * B, DVH: B * (d + 1), GRAD: B * (2 + 2 * d)}[layout]


def reduce_case(layout, d, npad, family="random"):
    """(Zs [B nrow, npad], y [npad], Sigma [B, d, d], v + vt), B = REDUCE_B: seeded, non-zero in every column; input 4 is input 0 again.
    family "cancel": y of unit length and every J row a multiple of y, so that |z_J|^2 - (z_J.y)^2 cancels to rounding"""
    nrow, B = nrow_of(layout, d), REDUCE_B
    rng = np.random.RandomState(500000 + 10000 * layout + 100 * d + npad + (7 if family == "cancel" else 0))
    y = rng.randn(npad) * np.exp(rng.uniform(-2, 0, npad))
    if family == "cancel":
        y = y / np.sqrt((y * y).sum())
    Z = (rng.randn(B, nrow, npad) * np.exp(rng.uniform(-3, 0, (B, nrow, npad)))) / np.sqrt(npad)
    if family == "cancel":
        j0 = 2 if layout == APPROX else 1
        Z[:, j0:j0 + d] = rng.uniform(0.5, 2.0, (B, d))[:, :, None] * y[None, None, :]
    Sig = np.array([dl.sigmas(d, 900 + 10 * d + i)["full" if d >= 2 else "diag"] for i in range(B)])
    Z[4], Sig[4] = Z[0], Sig[0]
    assert (Z != 0).all() and (y != 0).all()
    return np.ascontiguousarray(Z.reshape(B * nrow, npad)), y, Sig, 2.01


def reduce_check(title, got, want, ref):
    """got {name: values} against want {name: (values, scales)} under the bound of ref, the float64 evaluation of the same case"""
    ref_dist = {k: distances(ref[k][0], want[k][0], want[k][1]) for k in got}
    rho = rho_of(ref_dist)
    dist = {k: distances(g, want[k][0], want[k][1]) for k, g in got.items()}
    lim = dl.bound(rho)
    record(["%s | rho_ref %.3e  bound %.3e (margin %g)" % (title, rho, lim, dl.MARGIN)]
           + ["    %-8s ref %.3e   got %.3e = %8.6f bound" % (k, float(np.max(ref_dist[k])), float(np.max(r)), float(np.max(r)) / lim) for k, r in dist.items()])
    return assert_within(dist, rho, what=title)


def record(lines):
    """print, and with GPX_ROWS_RECORD=<file> append"""
    text = "\n".join([lines] if isinstance(lines, str) else lines)
    print(text)
    path = os.environ.get("GPX_ROWS_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(text + "\n")
