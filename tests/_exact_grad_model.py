"""A model of the six outputs of gpx_propagate_exact_grad_many (scikit-gpuppy_amd/csrc/exact_grad.hip; include/gpx.h): Girard's exact mean
and variance of the built-in kernel and their derivatives in u_k and in s_k = Sigma_kk (every other entry of Sigma held fixed).  Host only.

`moments_grad(.., dt=)` evaluates the PAIR SUMS directly, in row blocks of 64 and in the style of tests/_dense_ld.exact_parts -- it does not
use the device's row factorisation.  With a_i = u - x_i, A = Sigma + W^-1 / 2, b_i = A^-1 a_i, g = (b_i + b_j) / 2 = A^-1 (a_i + a_j) / 2,
M = Ksym - beta beta^T, T_ij = C_i C_j exp(z^T Ls z / 2) (z = (a_i + a_j) / 2; the pair weight without nc2) and the j <= i weights of
exact_parts:
    P0 = sum_ij M_ij T_ij,    P1_k = sum_ij M_ij T_ij g_k,    P2_k = sum_ij M_ij T_ij g_k^2
The exponent of T_ij is -1/4 a_i^T A^-1 a_i - 1/4 a_j^T A^-1 a_j + (terms without u), so dT/du_k = -g_k T; in s_k, dA^-1/ds_k =
-A^-1 e_k e_k^T A^-1 gives dT/ds_k = 1/2 g_k^2 T.  nc1 = prod (1 + w_k s_k)^-1/2 and nc2 = prod (2 w_k s_k + 1)^-1/2 read the diagonal of
Sigma only (exact_constants; the reference's behaviour), D_k = w_k / (1 + w_k s_k), l_i = F_i nc1 exp(-1/2 sum_k D_k a_ik^2)
(F_i = v, or v + vt on exact equality; = C_i nc1 exp(+1/2 sum_k (w_k - D_k) a_ik^2), the form exact_parts evaluates):
    m       = sum_i beta_i l_i                                  var      = cuu - nc2 P0 - m^2
    dm/du_k = -sum_i beta_i l_i D_k a_ik                        dvar/du_k = nc2 P1_k - 2 m dm/du_k
    dm/ds_k = 1/2 sum_i beta_i l_i (D_k^2 a_ik^2 - D_k)         dvar/ds_k = -nc2 (P2_k / 2 - w_k / (2 w_k s_k + 1) P0) - 2 m dm/ds_k
C_i carries vt where x_i == u elementwise; it is a constant of the differentiation.  Each value comes with its absolute scale: M_ij taken apart
as |Ksym_ij| + |beta_i| |beta_j|, g_k as (|b_ik| + |b_jk|) / 2, D_k^2 a^2 - D_k as D_k^2 a^2 + D_k, a combined value as the same combination of
its parts' scales.  dt = np.longdouble is the model, dt = np.float64 the plain evaluation that rho_ref is measured on.

`route(..)` is a float64 numpy statement of the DEVICE's route, in the style of tests/_exact_many_model.py: b from the differences of the
eigen-transformed coordinates (b = 4 T^T (s o (uh - xh))), the 2 d + 1 rows h, p_k = h o b_k, c_k = h o b_k^2, Y = rows Lo^T, and
    S = 2 h.Y_h,   G_k = p_k.Y_h + h.Y_pk,   Q_k = 1/2 (c_k.Y_h + h.Y_ck) + p_k.Y_pk
    dvar/du_k = nc2 G_k - 2 m dm/du_k,   dvar/ds_k = -nc2 (Q_k / 2 - w_k / (2 w_k s_k + 1) S) - 2 m dm/ds_k.
`defect=` plants one seeded defect in it (tests/test_exact_grad_model.py): "no_2m" the -2 m dm term dropped from both variance gradients,
"no_nc2" the derivative of nc2 dropped, "q_half" Q's 1/2 put on p_k.Y_pk instead of on the c_k terms, "b_W" b formed with 2 W in place of
A^-1 (their common value at Sigma = 0), "diag_full" the diagonal of Lo not halved."""
import numpy as np

import _dense_ld as dl
import _exact_many_model as em

LD = dl.LD
ROWS = 64
OUTPUTS = ("mean", "var", "dmean_du", "dvar_du", "dmean_ds", "dvar_ds")


def moments_grad(x, theta, Kinv, alpha, u, Sigma, dt=LD, quirk=True):
    """{name: (values, scales)} for the six OUTPUTS at one input u; mean without meant.  quirk=False: C without vt on exact equality (a
    pseudo-input model, as tests/test_spgp_pseudo.py evaluates exact_builtin for it)"""
    xr = np.asarray(x, dtype=np.float64)
    N, d = xr.shape
    v, vt, w, _wd, _q, _c, C = dl._rows_of(xr, theta, u, dt, None if quirk else "quirk")
    S = np.asarray(Sigma).astype(dt)
    sk = np.diagonal(S)
    Ls, dd, nc1, nc2 = dl.exact_constants(w, S, dt)
    Ai = dl.small_inverse(S + np.diag(1 / (2 * w)))
    Ai = (Ai + Ai.T) / 2
    D = w / (1 + w * sk)
    nq = w / (2 * w * sk + 1)
    a = np.asarray(u, dtype=np.float64).astype(dt) - xr.astype(dt)
    be = np.asarray(alpha).astype(dt)
    abe = np.abs(be)
    # the mean and its gradients: N-fold sums
    lm = C * nc1 * np.exp((a * a * dd).sum(1) / 2)          # C_i holds exp(-1/2 a^T W a): dd = w - D, as exact_parts has it
    bl, abl = be * lm, abe * np.abs(lm)
    m, am = bl.sum(), abl.sum()
    Da = D * a
    dmu, admu = -(bl[:, None] * Da).sum(0), (abl[:, None] * np.abs(Da)).sum(0)
    dms, adms = (bl[:, None] * (Da * Da - D)).sum(0) / 2, (abl[:, None] * (Da * Da + D)).sum(0) / 2
    # the pair sums
    b = a.dot(Ai)
    ab = np.abs(b)
    aL = a.dot(Ls)
    ql = (aL * a).sum(1)
    P0, A0 = dt(0), dt(0)
    P1, A1, P2, A2 = (np.zeros(d, dt) for _ in range(4))
    cols = np.arange(N)
    for i0 in range(0, N, ROWS):
        i1 = min(N, i0 + ROWS)
        Ks = (np.asarray(Kinv[i0:i1]).astype(dt) + np.asarray(Kinv[:, i0:i1]).astype(dt).T) / 2
        E = (ql[i0:i1][:, None] + ql[None, :]) / 8 + aL[i0:i1].dot(a.T) / 4
        ii = np.arange(i0, i1)[:, None]
        wgt = np.where(cols[None, :] < ii, 2.0, np.where(cols[None, :] == ii, 1.0, 0.0)).astype(dt)
        T = np.outer(C[i0:i1], C) * np.exp(E) * wgt
        MT = (Ks - np.outer(be[i0:i1], be)) * T
        AT = (np.abs(Ks) + np.outer(abe[i0:i1], abe)) * np.abs(T)
        P0 += MT.sum()
        A0 += AT.sum()
        for k in range(d):
            g = (b[i0:i1, k][:, None] + b[None, :, k]) / 2
            ag = (ab[i0:i1, k][:, None] + ab[None, :, k]) / 2
            P1[k] += (MT * g).sum()
            A1[k] += (AT * ag).sum()
            P2[k] += (MT * g * g).sum()
            A2[k] += (AT * ag * ag).sum()
    cuu = v + vt
    one = lambda p, q: (np.array([p], dt), np.array([q], dt))  # noqa: E731
    return {"mean": one(m, am), "var": one(cuu - nc2 * P0 - m * m, np.abs(cuu) + nc2 * A0 + am * am),
            "dmean_du": (dmu, admu), "dvar_du": (nc2 * P1 - 2 * m * dmu, nc2 * A1 + 2 * am * admu),
            "dmean_ds": (dms, adms), "dvar_ds": (-nc2 * (P2 / 2 - nq * P0) - 2 * m * dms, nc2 * (A2 / 2 + nq * A0) + 2 * am * adms)}


def route(x, theta, Kinv, alpha, U, Sigma, defect=None):
    """{name: values [B] or [B, d]} of the inputs U [B, d] under one Sigma, float64, as the device runs it"""
    x, U = np.asarray(x, dtype=np.float64), np.atleast_2d(np.asarray(U, dtype=np.float64))
    N, d = x.shape
    B = len(U)
    v, vt, w = dl.params(theta, d, np.float64)
    S = np.asarray(Sigma, dtype=np.float64)
    sk = np.diagonal(S)
    Ls, dd, nc1, nc2 = dl.exact_constants(w, S, np.float64)
    Ainv = dl.small_inverse(S + np.diag(1 / (2 * w)))
    D, nq = w / (1 + w * sk), w / (2 * w * sk + 1)
    Kinv, beta = np.asarray(Kinv, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    Lo = em.weight_matrix(x, Kinv, beta, Ls, "diag_full" if defect == "diag_full" else None)
    T, s = em.square_transform(Ainv, 0.25)
    xh, uh = (x - x[0]).dot(T.T), (U - x[0]).dot(T.T)
    df = uh[:, None, :] - xh[None, :, :]                      # [B, N, d]
    qa = (s * df * df).sum(-1)
    same = (x[None, :, :] == U[:, None, :]).all(-1)
    h = np.where(same, v + vt, v) * np.exp(-qa)
    a = U[:, None, :] - x[None, :, :]
    bb = a * (2 * w) if defect == "b_W" else 4 * (df * s).dot(T)      # b_k = sum_m 4 T_mk s_m df_m
    qw, qd = (w * a * a).sum(-1), (dd * a * a).sum(-1)
    C = v * np.exp(-0.5 * qw) + vt * same
    bl = C * nc1 * np.exp(0.5 * qd) * beta
    mean = bl.sum(1)
    Da = D * a
    dmu = -(bl[:, :, None] * Da).sum(1)
    dms = 0.5 * (bl[:, :, None] * (Da * Da - D)).sum(1)
    out = {"mean": mean, "var": np.empty(B), "dmean_du": dmu, "dvar_du": np.empty((B, d)), "dmean_ds": dms, "dvar_ds": np.empty((B, d))}
    for i in range(B):
        R = np.concatenate([h[i][None], (h[i][:, None] * bb[i]).T, (h[i][:, None] * bb[i] ** 2).T])      # [2 d + 1, N]
        Y = R.dot(Lo.T)
        Ssum = 2 * R[0].dot(Y[0])
        p, c, Yp, Yc = R[1:d + 1], R[d + 1:], Y[1:d + 1], Y[d + 1:]
        G = p.dot(Y[0]) + Yp.dot(R[0])
        pYp = (p * Yp).sum(1)
        Q = 0.5 * (c.dot(Y[0]) + Yc.dot(R[0]) + pYp) if defect == "q_half" else 0.5 * (c.dot(Y[0]) + Yc.dot(R[0])) + pYp
        mm = 0.0 if defect == "no_2m" else mean[i]
        out["var"][i] = (v + vt) - nc2 * Ssum - mean[i] * mean[i]
        out["dvar_du"][i] = nc2 * G - 2 * mm * dmu[i]
        out["dvar_ds"][i] = -nc2 * (0.5 * Q - (0.0 if defect == "no_nc2" else nq) * Ssum) - 2 * mm * dms[i]
    return out


def distances(got, want):
    """{name: distances} of the outputs in got (values) against want ({name: (values, scales)})"""
    return {k: dl.distances(np.ravel(g), want[k][0], want[k][1]) for k, g in got.items()}
