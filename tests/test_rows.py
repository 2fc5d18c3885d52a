"""The two kernel stages at the ends of the batched calls, each alone and per entry: the right-hand-side rows that the build kernels write
(gpx_rows_build: the launch of gpx_propagate_approx_many, gpx_propagate_dvh_many, gpx_predict_grad and gpx_matern_propagate_*_many, from
their one dispatch, before any solve) and the row reductions (gpx_rows_reduce) against the long-double model of tests/_rows_ld.py, which
also holds the inputs and the two rules; tests/test_rows_model.py shows that the model is right and that the rules see seeded defects.

(a) every entry of every returned row -- the padded columns and the rows of the last tile past b nrow included -- within gram_bound(rho) units
    of u scale (1 + q), rho the float64 evaluation's own worst over every case; a zero scale demands an exact zero;
(b) batch geometry: an input's rows do not depend on the batch, a shared Sigma and the same Sigma repeated give the same bits, a short batch
    after a long one leaves the rest of its tile zero;
(c) the reductions on seeded solved rows by tests/_dense_ld.py's rule, a family whose |z_J|^2 - (z_J.y)^2 cancels, place independence, the
    nullable outputs;
(d) refusals leave the output untouched.

Which case reaches which instantiation of the build frame (csrc/rows_tile.h: rows_build_tile<DR, LAYOUT> with the GaussRows / MaternRows<NU2>
policy; launch_rows_build dispatches on kernel family, layout and d <= 8; a case = kind, layout, d; every N of its d):
  approx_build_many_kernel<8, false>          (a) gauss approx d = 1, 3, 8 (k < d live at 1 and 3)      <0, false>  d = 9, 17, 64
  approx_build_many_kernel<8, true>           (a) gauss grad d = 1, 3, 8                               <0, true>   d = 9, 17, 64
  dvh_build_many_kernel<8>                    (a) gauss dvh d = 1, 3, 8                                <0>         d = 9, 17, 64
  matern52_build_many_kernel<8, false>        (a) matern52 approx d = 1, 3, 8                          <0, false>  d = 9, 17, 64
  matern52_build_many_kernel<8, true>         (a) matern52 dvh d = 1, 3, 8                             <0, true>   d = 9, 17, 64
  matern_grad_build_many_kernel<8, 3>         (a) matern32 grad d = 1, 3, 8                            <0, 3>      d = 9, 17, 64
  matern_grad_build_many_kernel<8, 5>         (a) matern52 grad d = 1, 3, 8                            <0, 5>      d = 9, 17, 64
  (b) runs all fourteen again at N = 129 with d = 3 (<8, ..>) and d = 9 (<0, ..>)
  approx_reduce_many_kernel                   (c) approx at every d
  dvh_reduce_many_kernel<8>                   (c) dvh d = 1, 8                                         <0>         d = 9, 64
  grad_reduce_many_kernel<8>                  (c) grad d = 1, 8                                        <0>         d = 9, 64
Shapes of (a): N = 128 (no padding), 129 (127 padded columns; in0 true, in1 false in the last pair), 200 (a partial tile) at every d, N = 700
(six column tiles) at d = 3 and 9; eight inputs: one wave of a workgroup takes two inputs, the loop ends at b >= nb.  (b): B = 1, 3, 16, 17, 35
-- a wave with fewer than four inputs, the loop broken midway, a second and third blockIdx.y with one and three inputs.
(c): npad = 128 (most threads idle), 256, 768 (one and a half strides of 512), 1024 (two).

With GPX_ROWS_RECORD=<file> every comparison appends rho, the bound and the worst ratio per row kind or output
(profiles/r23_rows.txt is such a record)."""
import functools

import numpy as np
import pytest

from conftest import torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _rows_ld as rl

pytestmark = pytest.mark.gpu

SENTINEL = 7.25


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _cov(kind):
    return sk.GaussianCovariance() if kind == 0 else sk.MaternCovariance(kind / 2.0)


@functools.lru_cache(maxsize=None)
def _fit(N, d, kind):
    """(gp, x, theta, U [8, d], Sigma [8, d, d]) of a case; the handle lives as long as the module's cache"""
    x, t, theta, Uin, Sig = rl.make_case(N, d)
    return sk.GaussianProcess(x, t, _cov(kind), theta.copy()), x, theta, Uin, Sig


def build(h, layout, Uin, Sig, N, d, shared=False):
    """gpx_rows_build: [round_up(b nrow, 128), npad]; the array starts as SENTINEL"""
    Uin = _gpx.f64(Uin)
    b = len(Uin)
    out = np.full((rl.round_up(b * rl.nrow_of(layout, d), 128), rl.round_up(N, 128)), SENTINEL)
    S = None if Sig is None else _gpx.f64(Sig)
    _gpx.check(_gpx.lib.gpx_rows_build(h, layout, _gpx.ptr(Uin), None if S is None else _gpx.ptr(S), int(shared), b, _gpx.ptr(out)), "gpx_rows_build")
    return out


def reduce(layout, d, Zs, y, Sig, kuu, shared=False, skip=False):
    """gpx_rows_reduce: the flat out array (SENTINEL where the call wrote nothing)"""
    Zs, y = _gpx.f64(Zs), _gpx.f64(y)
    B = Zs.shape[0] // rl.nrow_of(layout, d)
    out = np.full(rl.out_len(layout, d, B), SENTINEL)
    S = None if Sig is None else _gpx.f64(Sig)
    st = _gpx.lib.gpx_rows_reduce(layout | (_gpx.ROWS_SKIP_NULLABLE if skip else 0), d, Zs.shape[1], _gpx.ptr(Zs), _gpx.ptr(y),
                                  None if S is None else _gpx.ptr(S), int(shared), B, kuu, _gpx.ptr(out))
    _gpx.check(st, "gpx_rows_reduce")
    return out


def hold_rows(title, got, model, layout, d, B, N):
    """every entry of the block within the bound; the worst ratio per row kind is recorded first"""
    rho, lim = rl.rho_all()[0], rl.bound()
    dist = rl.units(got, model)
    worst = rl.worst_by_kind(dist, layout, d, B, N)
    rl.record("%s | rho %.3f  bound %.1f | " % (title, rho, lim) + "  ".join("%s %.3f = %.4f bound" % (k, w, w / lim) for k, w in worst.items()))
    assert (dist <= lim).all(), "%s: %d entries beyond %.1f units, the worst %.3e at (row, column) %r" % (
        title, int((~(dist <= lim)).sum()), lim, float(dist.max()), np.unravel_index(int(np.argmax(dist)), dist.shape))


# ------------------------------------------------------------------------------------------------
# (a) rows against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rl.KINDS, ids=[rl.KIND_NAMES[k] for k in rl.KINDS])
@pytest.mark.parametrize("N,d", rl.CASES, ids=["n%d_d%d" % c for c in rl.CASES])
def test_rows_against_long_double(N, d, kind):
    gp, x, theta, Uin, Sig = _fit(N, d, kind)
    h = gp._dev().handle
    for layout in rl.LAYOUTS_OF[kind]:
        got = build(h, layout, Uin, Sig if layout == rl.APPROX else None, N, d)
        model = rl.rows(x, theta, Uin, Sig, kind, layout)
        hold_rows("a rows %s %s N=%d d=%d" % (rl.KIND_NAMES[kind], rl.LAYOUT_NAMES[layout], N, d), got, model, layout, d, len(Uin), N)


# ------------------------------------------------------------------------------------------------
# (b) batch geometry
# ------------------------------------------------------------------------------------------------
GEOMETRY_B = (1, 3, 16, 17, 35)


def _batch35(x, Uin, Sig, d):
    """35 inputs: the case's eight, then seeded ones on the grid in [0, 10]^d; Sigma i = Sigma (i mod 8) scaled by 1 + i / 64 (pairwise distinct)"""
    rng = np.random.RandomState(3500 + d)
    U35 = np.vstack([Uin, rl._grid(rng.uniform(0, 10, (35 - len(Uin), d)))])
    S35 = np.array([Sig[i % len(Sig)] * (1 + i / 64.0) for i in range(35)])
    return U35, S35


@pytest.mark.parametrize("kind", rl.KINDS, ids=[rl.KIND_NAMES[k] for k in rl.KINDS])
@pytest.mark.parametrize("d", [3, 9])
def test_batch_geometry(d, kind):
    N = 129
    gp, x, theta, Uin, Sig = _fit(N, d, kind)
    h = gp._dev().handle
    U35, S35 = _batch35(x, Uin, Sig, d)
    for layout in rl.LAYOUTS_OF[kind]:
        nrow = rl.nrow_of(layout, d)
        sig = (lambda S: S) if layout == rl.APPROX else (lambda S: None)
        name = "%s %s N=%d d=%d" % (rl.KIND_NAMES[kind], rl.LAYOUT_NAMES[layout], N, d)
        full = build(h, layout, U35, sig(S35), N, d)
        hold_rows("b rows B=35 " + name, full, rl.rows(x, theta, U35, S35, kind, layout), layout, d, 35, N)
        # every shorter batch: the bits of the long one, and the rest of its last tile zero
        for B in GEOMETRY_B[:-1]:
            part = build(h, layout, U35[:B], sig(S35[:B]), N, d)
            np.testing.assert_array_equal(part[:B * nrow], full[:B * nrow], err_msg="%s B=%d" % (name, B))
            assert (part[B * nrow:] == 0).all(), (name, B)
        # input i of the long batch has the bits of the same input built alone
        for i in range(35):
            alone = build(h, layout, U35[i:i + 1], sig(S35[i:i + 1]), N, d)
            np.testing.assert_array_equal(alone[:nrow], full[i * nrow:(i + 1) * nrow], err_msg="%s input %d" % (name, i))
        # a long build, then a short one on the same handle: the stale rows of the pool buffer do not show
        build(h, layout, U35, sig(S35), N, d)
        after = build(h, layout, U35[:1], sig(S35[:1]), N, d)
        assert after.shape[0] == 128 and (after[nrow:] == 0).all(), name
        # a shared Sigma and the same Sigma repeated per input
        if layout == rl.APPROX:
            for B in GEOMETRY_B:
                shared = build(h, layout, U35[:B], S35[2], N, d, shared=True)
                np.testing.assert_array_equal(shared, build(h, layout, U35[:B], np.repeat(S35[2:3], B, axis=0), N, d), err_msg="%s B=%d" % (name, B))


# ------------------------------------------------------------------------------------------------
# (c) the reductions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["random", "cancel"])
@pytest.mark.parametrize("npad", rl.REDUCE_NPAD)
@pytest.mark.parametrize("d", rl.REDUCE_D)
@pytest.mark.parametrize("layout", [rl.APPROX, rl.DVH, rl.GRAD], ids=[rl.LAYOUT_NAMES[k] for k in (rl.APPROX, rl.DVH, rl.GRAD)])
def test_reductions_against_long_double(layout, d, npad, family):
    Zs, y, Sig, kuu = rl.reduce_case(layout, d, npad, family)
    B = rl.REDUCE_B
    S = Sig if layout == rl.APPROX else None
    out = reduce(layout, d, Zs, y, S, kuu)
    assert np.isfinite(out).all() and not (out == SENTINEL).any()
    got = rl.unpack(layout, d, B, out)
    want, ref = rl.reduce_model(layout, d, Zs, y, Sig, kuu), rl.reduce_model(layout, d, Zs, y, Sig, kuu, dt=np.float64)
    rl.reduce_check("c reduce %s %s d=%d npad=%d" % (rl.LAYOUT_NAMES[layout], family, d, npad), got, want, ref)
    # input 4 is input 0 again: the same bits at both places
    for k, g in got.items():
        np.testing.assert_array_equal(g[4], g[0], err_msg=k)
    # the nullable output (sigma2 of DVH, dmean of GRAD) left out: its part of out is not written, its siblings keep their bits
    if layout != rl.APPROX:
        skipped = rl.unpack(layout, d, B, reduce(layout, d, Zs, y, S, kuu, skip=True))
        nullable = "sigma2" if layout == rl.DVH else "dmean"
        for k, g in got.items():
            if k == nullable:
                assert (skipped[k] == SENTINEL).all(), k
            else:
                np.testing.assert_array_equal(skipped[k], g, err_msg=k)
    else:                                                           # one Sigma for every input: the bits of the same Sigma repeated
        np.testing.assert_array_equal(reduce(layout, d, Zs, y, Sig[1], kuu, shared=True), reduce(layout, d, Zs, y, np.repeat(Sig[1:2], B, axis=0), kuu))


# ------------------------------------------------------------------------------------------------
# (d) refusals
# ------------------------------------------------------------------------------------------------
class PlainGaussian(sk.GaussianCovariance):
    """the built-in kernel behind the generic route (gpx_fit_matrix): an overridden matrix builder"""

    def cov_matrix_ij(self, xi, xj, theta):
        return sk.GaussianCovariance.cov_matrix_ij(self, xi, xj, theta)


def test_refusals_leave_the_output_untouched():
    N, d = 129, 3
    gp, x, theta, Uin, Sig = _fit(N, d, 0)
    t = np.sin(0.3 * x.sum(1))
    t = t - t.mean()
    gen = sk.GaussianProcess(x, t, PlainGaussian(), theta.copy())
    per = sk.GaussianProcess(x, t, sk.PeriodicCovariance(), np.concatenate([theta, np.log(np.full(d, 4.0)), np.log(np.full(d, 0.5))]))
    m32 = _fit(N, d, 3)[0]
    assert gen._route() == "generic" and per._route() == "periodic"
    P, lib = _gpx.ptr, _gpx.lib
    U, S = _gpx.f64(Uin), _gpx.f64(Sig)
    out = np.full((128, 256), SENTINEL)

    def refused(status, word, *args):
        st = lib.gpx_rows_build(*args)
        assert st == status and word in _gpx.last_error(), (st, _gpx.last_error())
        assert (out == SENTINEL).all()

    h = gp._dev().handle
    for layout in (rl.APPROX, rl.DVH, rl.GRAD):
        refused(_gpx.GPX_ERR_BAD_ARG, "null handle", None, layout, P(U), P(S), 0, 8, P(out))
        refused(_gpx.GPX_ERR_STATE, "PeriodicCovariance", per._dev().handle, layout, P(U), P(S), 0, 8, P(out))
        refused(_gpx.GPX_ERR_STATE, "gpx_fit_matrix", gen._dev().handle, layout, P(U), P(S), 0, 8, P(out))
        refused(_gpx.GPX_ERR_BAD_ARG, "gpx_rows_build", h, layout, None, P(S), 0, 8, P(out))
        refused(_gpx.GPX_ERR_BAD_ARG, "gpx_rows_build", h, layout, P(U), P(S), 0, -1, P(out))
        assert lib.gpx_rows_build(h, layout, P(U), P(S), 0, 8, None) == _gpx.GPX_ERR_BAD_ARG
    for layout in (rl.APPROX, rl.DVH):
        refused(_gpx.GPX_ERR_STATE, "3/2", m32._dev().handle, layout, P(U), P(S), 0, 8, P(out))
    refused(_gpx.GPX_ERR_BAD_ARG, "gpx_rows_build", h, rl.APPROX, P(U), None, 0, 8, P(out))
    refused(_gpx.GPX_ERR_BAD_ARG, "gpx_rows_build", h, 3, P(U), P(S), 0, 8, P(out))
    # a batch beyond one chunk (32768 rows at this npad): 8192 inputs of d + 1 = 4 rows fill it, one more is refused
    big = np.zeros((8193, d))
    refused(_gpx.GPX_ERR_BAD_ARG, "chunk", h, rl.GRAD, P(big), None, 0, 8193, P(out))
    assert lib.gpx_rows_build(h, rl.GRAD, P(U), None, 0, 0, P(out)) == 0 and (out == SENTINEL).all()          # b = 0: a no-op
    # the reduction: bad arguments before anything is written
    Zs, y, Sg, kuu = rl.reduce_case(rl.APPROX, d, 128)
    o = np.full(rl.out_len(rl.APPROX, d, rl.REDUCE_B), SENTINEL)
    for args in ((3, d, 128, P(Zs), P(y), P(Sg), 0, 5, kuu, P(o)), (rl.APPROX, 0, 128, P(Zs), P(y), P(Sg), 0, 5, kuu, P(o)),
                 (rl.APPROX, 65, 128, P(Zs), P(y), P(Sg), 0, 5, kuu, P(o)), (rl.APPROX, d, 130, P(Zs), P(y), P(Sg), 0, 5, kuu, P(o)),
                 (rl.APPROX, d, 128, None, P(y), P(Sg), 0, 5, kuu, P(o)), (rl.APPROX, d, 128, P(Zs), None, P(Sg), 0, 5, kuu, P(o)),
                 (rl.APPROX, d, 128, P(Zs), P(y), None, 0, 5, kuu, P(o)), (rl.APPROX, d, 128, P(Zs), P(y), P(Sg), 0, -1, kuu, P(o)),
                 (rl.APPROX, d, 128, P(Zs), P(y), P(Sg), 0, 5, kuu, None)):
        assert lib.gpx_rows_reduce(*args) == _gpx.GPX_ERR_BAD_ARG, args
    assert (o == SENTINEL).all()
