"""Batched Exact propagation: UncertaintyPropagationExact.propagate_GA_many / propagate_mean_many and gpx_propagate_exact_many.

For the inputs that share a Sigma the double sum of Girard's exact variance is the quadratic form h^T M h with M = (Kinv - beta beta^T) o E built
once (include/gpx.h; tests/_exact_many_model.py states the path in numpy, tests/test_exact_many_model.py holds that statement to the
long-double model).  Here the device path is held to the same long-double model of the UNFACTORED sum (tests/_dense_ld.exact_builtin) on
the device's own K^-1 and alpha, under the rule of tests/_dense_ld.py: distance on the sum's absolute scale within
MARGIN * max(rho_ref, FLOOR), rho_ref from the float64 numpy evaluation of the same unfactored sum.  Where the batched call is compared with
gpx_propagate_exact, two device paths that are each held to that bound may differ by twice it; rho_ref of these inputs is below FLOOR
(at most 2.6e-14 on the host that wrote the test), so the bound used is 2 * MARGIN * FLOOR, the smallest the rule can give.

The CPU cases need no device: the methods and the symbol exist, and a null handle is refused before anything is touched."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from conftest import load_golden, torch  # noqa: F401  (HIP runtime of torch first, as in the rest of the suite)

import skgpuppy_amd as sk
from skgpuppy_amd import _gpx

import _dense_ld as dl
from _operators import make_warped_gaussian
from test_dense_bounds import both, check, fit
from test_exact_many_model import negative_sigma

HERE = os.path.dirname(os.path.abspath(__file__))
GPX_K_GEMM, GPX_K_EXACT, GPX_K_GEMM_SMALL = 1, 6, 7      # include/gpx.h
FILL = 7.25
TWO_PATHS = 2 * dl.bound(0.0)                             # 2 * MARGIN * FLOOR (module docstring)


# ------------------------------------------------------------------------------------------------
# without a device
# ------------------------------------------------------------------------------------------------
def test_batched_methods_and_symbol_exist():
    assert callable(getattr(sk.UncertaintyPropagationExact, "propagate_GA_many"))
    assert callable(getattr(sk.UncertaintyPropagationExact, "propagate_mean_many"))
    assert callable(getattr(sk.UncertaintyPropagationGA, "_many_args"))
    assert "_many_args" not in vars(sk.UncertaintyPropagationApprox)        # one copy, on the common base class
    assert "gpx_propagate_exact_many" in _gpx.SIGNATURES
    assert hasattr(_gpx.lib, "gpx_propagate_exact_many")
    header = open(os.path.join(os.path.dirname(HERE), "include", "gpx.h")).read()
    assert "int gpx_propagate_exact_many(" in header
    assert _gpx.lib.gpx_abi_version() == 1      # additive


def test_null_handle_is_refused_and_no_output_touched():
    U, S = np.zeros((3, 2)), np.eye(2)
    out = [np.full(3, FILL) for _ in range(2)]
    st = _gpx.lib.gpx_propagate_exact_many(None, _gpx.ptr(U), _gpx.ptr(S), 1, 3, *[_gpx.ptr(o) for o in out])
    assert st == _gpx.GPX_ERR_BAD_ARG
    assert "null handle" in _gpx.last_error()
    for o in out:
        np.testing.assert_array_equal(o, np.full(3, FILL))


# ------------------------------------------------------------------------------------------------
# on the device
# ------------------------------------------------------------------------------------------------
def raw_many(h, U, S, shared=True, want_var=True, status=False):
    """gpx_propagate_exact_many itself: (mean without meant, var); the outputs enter holding FILL"""
    U, S = _gpx.f64(U), _gpx.f64(S)
    mean, var = np.full(len(U), FILL), np.full(len(U), FILL)
    st = _gpx.lib.gpx_propagate_exact_many(h, _gpx.ptr(U), _gpx.ptr(S), int(shared), len(U), _gpx.ptr(mean), _gpx.ptr(var) if want_var else None)
    if status:
        return st, mean, var
    _gpx.check(st, "gpx_propagate_exact_many")
    return mean, var


def single(h, u, S):
    u, S = _gpx.f64(u), _gpx.f64(S)
    m, v = ctypes.c_double(), ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_propagate_exact(h, _gpx.ptr(u), _gpx.ptr(S), ctypes.byref(m), ctypes.byref(v)), "gpx_propagate_exact")
    return m.value, v.value


def seeded(f, count, salt):
    rng = np.random.RandomState(f.seed + salt)
    return [dl._grid(rng.uniform(2, 8, f.d)) for _ in range(count)]


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def against_model(title, f, U, S, mean, var, refs=None):
    """every input's mean and variance under the rule; refs (optional) caches (want, ref) per input index"""
    for i, u in enumerate(U):
        want, ref = refs[i] if refs is not None else both(dl.exact_builtin, *f.args, u, S)
        check("%s input %d" % (title, i), f.name, {"mean": np.array([mean[i]]), "var": np.array([var[i]])}, want, ref)


def against_single(title, f, U, S, mean, var, idx):
    """inputs idx of a batch against gpx_propagate_exact on the absolute scale of the float64 evaluation, within TWO_PATHS"""
    worst = 0.0
    for i in idx:
        Si = S if np.ndim(S) == 2 else S[i]
        m1, v1 = single(f.h, U[i], Si)
        scale = dl.exact_builtin(*f.args, U[i], Si, dt=np.float64)
        dist = {"mean": dl.distances(mean[i], m1, scale["mean"][1]), "var": dl.distances(var[i], v1, scale["var"][1])}
        worst = max(worst, float(dist["mean"].max()), float(dist["var"].max()))
        for k, r in dist.items():
            assert np.all(r <= TWO_PATHS), (title, i, k, float(r.max()), TWO_PATHS)
    print("%s | %s: worst distance to the single call %.3e of %.3e" % (title, f.name, worst, TWO_PATHS))


RULE_CASES = [(700, d) for d in (1, 3, 8, 9, 17, 64)] + [(128, 3), (129, 8), (200, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,d", RULE_CASES, ids=["n%d_d%d" % c for c in RULE_CASES])
def test_rule_against_the_long_double_model(N, d):
    """(1) one shared Sigma, diagonal and full; B = 1 (each of the three inputs of dl.inputs_u alone) and B = 5 (the three and two seeded
    ones).  d = 1, 3, 8, 9, 17, 64 at N = 700 (npad 768: 68 padded rows and columns, 12 x 12 tiles of the weight pass), 128 (no padding),
    129 (127 padded), 200."""
    with fit(N, d) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        U = np.array([ins["between"], ins["equal"], ins["far"]] + seeded(f, 2, 23))
        for sn, S in dl.sigmas(d, f.seed).items():
            refs = [both(dl.exact_builtin, *f.args, u, S) for u in U]
            for pick in ([0], [1], [2], [0, 1, 2, 3, 4]):
                mean, var = raw_many(f.h, U[pick], S)
                against_model("many B=%d Sigma %s" % (len(pick), sn), f, U[pick], S, mean, var, [refs[i] for i in pick])


@pytest.mark.gpu
@pytest.mark.parametrize("N,d", [(700, 3), (200, 8)])
def test_sharp_cases(N, d):
    """(2) sharp length scales: E far from 1 and a heavy diagonal; the inputs between / equal and two seeded ones, both Sigma, and
    Sigma = diag(-0.1 / w_k), where Ls is negative definite and every s_k = -1"""
    with fit(N, d, sharp=True) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        U = np.array([ins["between"], ins["equal"]] + seeded(f, 2, 29))
        Ss = dict(dl.sigmas(d, f.seed))
        Ss["negative"] = negative_sigma(f.theta, d)
        for sn, S in Ss.items():
            mean, var = raw_many(f.h, U, S)
            against_model("many sharp Sigma %s" % sn, f, U, S, mean, var)


@pytest.mark.gpu
def test_larger_batch_every_input_against_the_single_call():
    """(3) B = 130 at N = 700, d = 8 (126 padded inputs, 68 padded rows): every input through the many call and through
    gpx_propagate_exact; eight of them also against the long-double model"""
    with fit(700, 8) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        U = np.array([ins["between"], ins["equal"], ins["far"]] + seeded(f, 127, 31))
        S = dl.sigmas(8, f.seed)["full"]
        mean, var = raw_many(f.h, U, S)
        assert np.isfinite(mean).all() and np.isfinite(var).all()
        against_single("many B=130", f, U, S, mean, var, range(130))
        pick = [0, 129, 127, 128, 1, 2, 50, 77]             # first, last, 127, 128, the quirk, the far one, two seeded
        against_model("many B=130", f, U[pick], S, mean[pick], var[pick])


def _launches(h, cls):
    n, ms, w = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    _gpx.check(_gpx.lib.gpx_profile_read(h, cls, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(w)), "gpx_profile_read")
    return n.value


@pytest.mark.gpu
@pytest.mark.parametrize("N,B,cls", [(2200, 1500, GPX_K_GEMM_SMALL), (4000, 2048, GPX_K_GEMM)])
def test_gemm_launch_forms(N, B, cls):
    """(4) the product's launch follows the tile count (thresholds in gpx.h): N = 2200, B = 1500 is 12 x 18 tiles, the 64 x 64 triangular
    form (192 .. 447 tiles; profiled with the small-tile class); N = 4000, B = 2048 is 16 x 32 tiles, a 128 x 128 triangular form (the
    dominant class).  Eight inputs of each against the single call."""
    d = 5
    with fit(N, d) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        U = np.array([ins["between"], ins["equal"], ins["far"]] + seeded(f, B - 3, 37))
        S = dl.sigmas(d, f.seed)["full"]
        _gpx.check(_gpx.lib.gpx_profile_enable(f.h, 2), "gpx_profile_enable")
        _gpx.check(_gpx.lib.gpx_profile_reset(f.h), "gpx_profile_reset")
        mean, var = raw_many(f.h, U, S)
        other = GPX_K_GEMM if cls == GPX_K_GEMM_SMALL else GPX_K_GEMM_SMALL
        assert _launches(f.h, cls) == 1 and _launches(f.h, other) == 0
        assert _launches(f.h, GPX_K_EXACT) == 3             # the weight pass, one slab's build and finish
        _gpx.check(_gpx.lib.gpx_profile_enable(f.h, 0), "gpx_profile_enable")
        assert np.isfinite(mean).all() and np.isfinite(var).all()
        against_single("many N=%d B=%d" % (N, B), f, U, S, mean, var, [0, 1, 2, 127, 128, B // 2, B - 2, B - 1])


@pytest.mark.gpu
def test_slab_boundary():
    """(4) GPX_EXACT_MANY_SLAB=256 with B = 300 at N = 700: two slabs, the second of 44 inputs; the inputs either side of the boundary, the
    ends and the quirk against the single call"""
    with fit(700, 5) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        U = np.array([ins["between"], ins["equal"], ins["far"]] + seeded(f, 297, 41))
        S = dl.sigmas(5, f.seed)["full"]
        with env(GPX_EXACT_MANY_SLAB=256):
            _gpx.check(_gpx.lib.gpx_profile_enable(f.h, 2), "gpx_profile_enable")
            _gpx.check(_gpx.lib.gpx_profile_reset(f.h), "gpx_profile_reset")
            mean, var = raw_many(f.h, U, S)
            assert _launches(f.h, GPX_K_EXACT) == 5         # the weight pass once, build and finish per slab
            _gpx.check(_gpx.lib.gpx_profile_enable(f.h, 0), "gpx_profile_enable")
        assert np.isfinite(mean).all() and np.isfinite(var).all()
        against_single("many slab 256 B=300", f, U, S, mean, var, [0, 1, 2, 127, 255, 256, 257, 299])


@pytest.mark.gpu
def test_routes_with_per_input_sigma():
    """(5) per-input Sigma in runs [S0 x 40, S1 x 1, S0 x 2, S2 x 37] at N = 700, d = 3: under the default MIN_RUN the runs of 40 and 37 take
    the matrix path and the two short ones the pair path; GPX_EXACT_MANY_MIN_RUN=1 sends every run to the matrix path, =1000000 to the
    pair path.  All three within the rule for every input (the inputs cycle through six distinct u, so that 18 long-double evaluations
    serve the 80); under 1000000 every input has the bits of gpx_propagate_exact."""
    with fit(700, 3) as f:
        ins = dl.inputs_u(f.x, f.theta, f.seed)
        pool = [ins["between"], ins["equal"], ins["far"]] + seeded(f, 3, 43)
        sig = dl.sigmas(3, f.seed)
        Ss = [sig["diag"], sig["full"], 0.5 * sig["full"]]
        which = [0] * 40 + [1] + [0] * 2 + [2] * 37
        U = np.array([pool[i % 6] for i in range(80)])
        S = np.array([Ss[k] for k in which])
        cache = {}

        def refs():
            out = []
            for i in range(80):
                key = (i % 6, which[i])
                if key not in cache:
                    cache[key] = both(dl.exact_builtin, *f.args, U[i], S[i])
                out.append(cache[key])
            return out

        for setting in (None, 1, 1000000):
            with env(**({} if setting is None else {"GPX_EXACT_MANY_MIN_RUN": setting})):
                mean, var = raw_many(f.h, U, S, shared=False)
            for i in range(80):
                want, ref = refs()[i]
                check("routes MIN_RUN=%s input %d" % (setting, i), f.name, {"mean": np.array([mean[i]]), "var": np.array([var[i]])}, want, ref)
            if setting == 1000000:
                for i in range(80):
                    assert (mean[i], var[i]) == single(f.h, U[i], S[i]), i
            if setting is None:                              # the short runs took the pair path: the single call's bits
                for i in (40, 41, 42):
                    assert (mean[i], var[i]) == single(f.h, U[i], S[i]), i


@pytest.mark.gpu
def test_independence_of_position_and_sigma_form():
    """(6) the batch reversed gives the reversed bits; one shared Sigma and the same Sigma repeated B times give the same bits; the (d, d)
    form of the Python call is the shared form"""
    x, t, theta = dl.make_case(700, 4, 99)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy())
    h = gp._dev().handle
    rng = np.random.RandomState(5)
    B, d = 130, 4
    U = dl._grid(rng.uniform(1, 9, (B, d)))
    U[17] = x[9]
    S = dl.sigmas(d, 3)["full"]
    one = raw_many(h, U, S)
    rev = raw_many(h, U[::-1], S)
    for a, b in zip(one, rev):
        np.testing.assert_array_equal(a, b[::-1])
    rep = raw_many(h, U, np.repeat(S[None], B, 0), shared=False)
    for a, b in zip(one, rep):
        np.testing.assert_array_equal(a, b)
    rrev = raw_many(h, U[::-1], np.repeat(S[None], B, 0), shared=False)
    for a, b in zip(one, rrev):
        np.testing.assert_array_equal(a, b[::-1])
    up = sk.UncertaintyPropagationExact(gp)
    ms, vs = up.propagate_GA_many(U, S)
    np.testing.assert_array_equal(ms, one[0] + gp.meant)
    np.testing.assert_array_equal(vs, one[1])
    np.testing.assert_array_equal(up.propagate_mean_many(U, S), raw_many(h, U, S, want_var=False)[0])


def _fresh_gp(N=700, d=5):
    x, t, theta = dl.make_case(N, d, 7 + N)
    return sk.GaussianProcess(x, t, sk.GaussianCovariance(), theta.copy()), x


@pytest.mark.gpu
def test_no_side_effects_on_the_single_input_path():
    """(7) after a fresh fit a means-only call launches nothing of the Exact class and no GEMM, and leaves K^-1 unbuilt on the Python
    object; a propagate_GA after a full many call returns the bits of a fresh fit's propagate_GA; the many calls leave the instance's
    attributes of the single-input path unset"""
    gp, x = _fresh_gp()
    d = gp.d
    rng = np.random.RandomState(11)
    U = dl._grid(rng.uniform(2, 8, (40, d)))
    S = dl.sigmas(d, 11)["full"]
    h = gp._dev().handle
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 2), "gpx_profile_enable")
    _gpx.check(_gpx.lib.gpx_profile_reset(h), "gpx_profile_reset")
    up = sk.UncertaintyPropagationExact(gp)
    means = up.propagate_mean_many(U, S)
    assert np.isfinite(means).all()
    assert _launches(h, GPX_K_EXACT) == 0 and _launches(h, GPX_K_GEMM) == 0 and _launches(h, GPX_K_GEMM_SMALL) == 0
    assert gp._Kinv is None
    _gpx.check(_gpx.lib.gpx_profile_enable(h, 0), "gpx_profile_enable")
    for i in (0, 39):                                        # the means-only call is the mean of the single call
        assert means[i] == pytest.approx(sk.UncertaintyPropagationExact(gp).propagate_mean(U[i], S), abs=1e-12)
    # a single call first (it stages u and Sigma on the handle), then the full many call, then the single call again
    before = up.propagate_GA(U[3], S)
    up2 = sk.UncertaintyPropagationExact(gp)
    mean, var = up2.propagate_GA_many(U, S)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    for name in ("Winv", "Sigma_x", "Deltainv", "LambdaInv", "normalize_C_corr", "normalize_C_corr2"):
        assert not hasattr(up2, name), name
    after = up.propagate_GA(U[3], S)
    gp2, _x = _fresh_gp()
    plain = sk.UncertaintyPropagationExact(gp2).propagate_GA(U[3], S)
    assert before == plain and after == plain                # bit for bit
    # and an Approx single call keeps its cached u across the many call
    ap = sk.UncertaintyPropagationApprox(gp)
    a1 = ap.propagate_GA(U[4], S)
    up2.propagate_GA_many(U, S)
    assert ap.propagate_GA(U[4], S) == a1 == sk.UncertaintyPropagationApprox(gp2).propagate_GA(U[4], S)


@pytest.mark.gpu
def test_edges():
    """(8) B = 0; the refusals, with the outputs still holding their fill value; shape errors; a generic-route GP equals its own loop"""
    gp, x = _fresh_gp()
    d = gp.d
    h = gp._dev().handle
    up = sk.UncertaintyPropagationExact(gp)
    m, var = up.propagate_GA_many(np.zeros((0, d)), np.eye(d))
    assert m.shape == var.shape == (0,)
    assert up.propagate_mean_many(np.zeros((0, d)), np.zeros((0, d, d))).shape == (0,)
    assert _gpx.lib.gpx_propagate_exact_many(h, None, None, 1, 0, None, None) == 0
    U, S = dl._grid(np.random.RandomState(2).uniform(2, 8, (12, d))), 0.1 * np.eye(d)

    def refused(status, text, *a, **kw):
        st, mean, var_ = raw_many(*a, status=True, **kw)
        assert st == status and text in _gpx.last_error(), (st, _gpx.last_error())
        np.testing.assert_array_equal(mean, np.full(len(mean), FILL))
        np.testing.assert_array_equal(var_, np.full(len(var_), FILL))

    mean, var_ = np.full(12, FILL), np.full(12, FILL)
    for args in ((None, _gpx.ptr(S), 1, 12, _gpx.ptr(mean), _gpx.ptr(var_)), (_gpx.ptr(U), None, 1, 12, _gpx.ptr(mean), _gpx.ptr(var_)),
                 (_gpx.ptr(U), _gpx.ptr(S), 1, 12, None, _gpx.ptr(var_)), (_gpx.ptr(U), _gpx.ptr(S), 1, -1, _gpx.ptr(mean), _gpx.ptr(var_))):
        assert _gpx.lib.gpx_propagate_exact_many(h, *args) == _gpx.GPX_ERR_BAD_ARG
    np.testing.assert_array_equal(mean, np.full(12, FILL))
    np.testing.assert_array_equal(var_, np.full(12, FILL))
    # a singular W/2 + Sigma anywhere in the batch: refused before the first launch, on both routes.  (1e300 in every entry absorbs the
    # diagonal W^-1 / 2 entirely: the matrix is exactly rank one in fp64 and the elimination meets an exact zero pivot.)
    sing = np.full((d, d), 1e300)
    refused(_gpx.GPX_ERR_BAD_ARG, "singular", h, U, sing)
    Sb = np.repeat(S[None], 12, 0)
    Sb[11] = sing
    refused(_gpx.GPX_ERR_BAD_ARG, "singular", h, U, Sb, shared=False)
    with env(GPX_EXACT_MANY_MIN_RUN=1):
        refused(_gpx.GPX_ERR_BAD_ARG, "singular", h, U, Sb, shared=False)
    for bad_U, bad_S in [(np.zeros(d), np.eye(d)), (np.zeros((3, d + 1)), np.eye(d)), (np.zeros((3, d)), np.eye(d + 1)),
                         (np.zeros((3, d)), np.zeros((2, d, d))), (np.zeros((3, d)), np.zeros(d)), (np.zeros((2, 3, d)), np.eye(d))]:
        with pytest.raises(ValueError):
            up.propagate_GA_many(bad_U, bad_S)
        with pytest.raises(ValueError):
            up.propagate_mean_many(bad_U, bad_S)
    # a handle built from a supplied matrix has no inputs / theta to evaluate the kernel on
    from skgpuppy_amd.Covariance import _MatrixModel
    mm = _MatrixModel(np.eye(4) * 2.0, np.arange(4.0))
    refused(_gpx.GPX_ERR_STATE, "gpx_fit_matrix", mm.handle, np.zeros((2, 1)), np.eye(1))
    mm.close()
    # generic route (an operator that overrides a matrix builder): the documented loop over the single-input path
    g = load_golden("generic_ops")
    ggp = sk.GaussianProcess(g["wg_x"], g["wg_t"], make_warped_gaussian(sk.GaussianCovariance)(), g["wg_theta"].copy())
    gd = ggp.d
    rng = np.random.RandomState(4)
    GU = rng.uniform(g["wg_x"].min(0), g["wg_x"].max(0), (5, gd))
    GS = np.array([np.diag(rng.uniform(0.005, 0.05, gd)) for _ in range(5)])
    gup = sk.UncertaintyPropagationExact(ggp)
    assert ggp._route() != "gaussian"
    gm, gv = gup.propagate_GA_many(GU, GS)
    gmo = gup.propagate_mean_many(GU, GS[0])
    for i in range(5):
        one = sk.UncertaintyPropagationExact(ggp)
        assert (gm[i], gv[i]) == one.propagate_GA(GU[i], GS[i])
        assert gmo[i] == one.propagate_mean(GU[i], GS[0])
    assert not hasattr(gup, "Winv") and not hasattr(gup, "Sigma_x")
