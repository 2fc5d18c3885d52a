"""SPGP on the device (scikit-gpuppy_amd/csrc/spgp.hip) against a long-double model of the same algebra, group by group, under a bound
measured on the float64 CPU evaluation of the same case (tests/_spgp_ld.py: the model, the inputs, the rule).

What the end-to-end tests of tests/test_gpu_parity.py do not reach, and these do:
  a. every group of the gradient on its own scale (there: 2e-7 of the largest entry, log vt's, which hides the pseudo-input block), the
     predictor, the dense forms, at m below / across / on a tile and N < m;
  b. the halves of the gradient's E-pass that need mpad > 512 (the second column pair) and mpad > 1024 (blockIdx.y = 1, two row blocks
     over Qbar), and two coordinate blocks beside them;
  c. the split-K product inside the fit, the likelihood and the gradient, with the chunk count asserted through gpx_spgp_split;
  d. inputs far from the origin: the gradient's expanded moments lose (|x| / |xb - x|)^2 digits unless the inputs are centred first;
  e. more than one 65536-query chunk of the predictor.
Well-conditioned inputs only (rho_ref 1e-13 .. 3e-11; one case of b excepted, see there): at the cond 8e7 of the older tests' recipe the float64 evaluation itself is 1e-8
from the long-double mean, and a bound measured on it would tell little.  Long-double values come from the model inside the test where that
takes about a second (m <= 130, N <= 1500) and from tests/golden/spgp_ld.npz (tools/gen_spgp_ld_golden.py) otherwise.

With GPX_SPGP_BOUNDS_RECORD=<file> every case appends its rho_ref, the chunk count and each group's ratio to rho_ref and to the bound
(profiles/r09_spgp_bounds.txt is such a record)."""
import functools
import os

import numpy as np
import pytest

from conftest import load_golden

import skgpuppy_amd as sk
from oracle import oracle as orc

import _spgp_ld as ld

pytestmark = pytest.mark.gpu

SOFT = (0.5, 2.0, 0.05)     # (wlo, whi, jit)
SHARP = (2.0, 8.0, 0.3)
WIDE = (0.05, 0.2, 0.3)
GOLDEN = {((300, 3, 520), SHARP): "n300_d3_m520", ((300, 9, 520), SHARP): "n300_d9_m520", ((300, 9, 520), WIDE): "n300_d9_m520_wide",
          ((200, 3, 1030), SHARP): "n200_d3_m1030", ((16384, 3, 130), SOFT): "n16384_d3_m130"}


class Case(object):
    """seeded inputs, their long-double values and rho_ref, built once per shape"""

    def __init__(self, shape, recipe):
        self.shape, self.recipe = shape, recipe
        self.N, self.d, self.m = shape
        self.x, self.t, self.theta, self.xs = ld.make_case(*shape, *recipe)
        self.vvt = ld.vvt_of(self.theta)
        if (shape, recipe) in GOLDEN:
            g = load_golden("spgp_ld")
            pre = GOLDEN[shape, recipe] + "__"
            assert str(g[pre + "sha256"]) == ld.input_hash(self.x, self.t, self.theta, self.xs), "the fixture was made from other inputs"
            self.want = {"nll": float(g[pre + "nll"]), "grad": g[pre + "grad"], "mean": g[pre + "mean"], "var": g[pre + "var"]}
        else:
            self.want = ld.evaluate(self.x, self.t, self.theta, self.m, self.xs)
        self.ref = ld.evaluate_f64(self.x, self.t, self.theta, self.m, self.xs)
        self.ref_dist = ld.distances(self.ref, self.want, self.d, self.vvt)
        self.rho = max(self.ref_dist.values())

    def shifted(self):
        x, t, theta, xs = ld.make_case(*self.shape, *self.recipe, shift=ld.SHIFT)
        np.testing.assert_array_equal(x - ld.SHIFT, self.x)                      # the translation is exact
        np.testing.assert_array_equal(theta[2 + self.d:] - ld.SHIFT, self.theta[2 + self.d:])
        return x, t, theta, xs

    def name(self):
        return "N=%d d=%d m=%d w=[%g,%g] jit=%g" % (self.shape + self.recipe)


@functools.lru_cache(maxsize=None)
def case(shape, recipe):
    return Case(shape, recipe)


def run_device(x, t, theta, m, xs):
    """fit on the device: ({nll, grad, mean, var}, chunk count, the device model)"""
    dev = sk.SPGPCovariance(m)._model(x, t, theta)
    chunks = dev.split()
    got = {"nll": dev.nll(), "grad": dev.nll_grad()}
    got["mean"], got["var"] = dev.predict(np.ascontiguousarray(xs))
    return got, chunks, dev


def record(title, c, rho, chunks, dist, ref_dist=None, margin=ld.MARGIN):
    path = os.environ.get("GPX_SPGP_BOUNDS_RECORD")
    if not path:
        return
    lim = ld.bound(rho, margin)
    ref_dist = c.ref_dist if ref_dist is None else ref_dist
    with open(path, "a") as f:
        f.write("%s | %s | rho_ref %.3e  bound %.3e (margin %g)  chunks %d\n" % (title, c.name(), rho, lim, margin, chunks))
        for k, r in dist.items():
            f.write("    %-10s ref %.3e   device %.3e = %8.3f rho_ref = %6.4f bound\n" % (k, ref_dist.get(k, float("nan")), r, r / rho, r / lim))


def check(title, c, got, chunks, keys=("nll", "grad", "mean", "var")):
    got = {k: got[k] for k in keys}
    dist = ld.distances(got, c.want, c.d, c.vvt)
    record(title, c, c.rho, chunks, dist)
    print(title, c.name(), "rho_ref %.3e" % c.rho, {k: "%.2e" % r for k, r in dist.items()})
    return ld.assert_within(got, c.want, c.rho, c.d, c.vvt, what=title + " " + c.name())


# ------------------------------------------------------------------------------------------------
# a. small shapes, long double in the test; the dense forms beside the low-rank ones
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,recipe", [((300, 2, 7), SOFT), ((1500, 3, 130), SOFT), ((256, 3, 128), SHARP), ((100, 3, 130), SHARP)],
                         ids=["m_below_a_tile", "m_across_a_tile", "no_padding", "n_below_m"])
def test_small_shapes(shape, recipe):
    c = case(shape, recipe)
    cov = sk.SPGPCovariance(c.m)
    got = {"nll": cov._negativeloglikelihood(c.x, c.t, c.theta), "grad": cov._d_nll_d_theta(c.x, c.t, c.theta)}
    chunks = cov._fit_model(c.x, c.t, c.theta).split()
    gp = sk.GaussianProcess(c.x, c.t, cov, c.theta.copy())
    mu, got["var"] = gp.estimate_many(c.xs)
    got["mean"] = mu - gp.meant
    assert chunks == 0
    check("a", c, got, chunks)
    # the dense forms: cov_matrix, inv_cov_matrix, cov_matrix_ij, each on its max-norm; rho_ref now measured over these groups as well
    p = ld.Predictor(c.x, c.t, c.theta, c.m)
    want = {"cov": p.cov(), "inv": p.inv(), "cross": p.cross(c.xs, c.x)}
    ref = {"cov": orc.spgp_cov_matrix(c.x, c.theta, c.m), "inv": orc.spgp_inv_cov_matrix(c.x, c.theta, c.m),
           "cross": orc.spgp_cov_matrix_ij(c.xs, c.x, c.theta, c.m)}
    gotd = {"cov": cov.cov_matrix(c.x, c.theta), "inv": cov.inv_cov_matrix(c.x, c.theta), "cross": cov.cov_matrix_ij(c.xs, c.x, c.theta)}
    ref_dist = ld.distances(ref, want, c.d, c.vvt)
    rho = max(c.rho, max(ref_dist.values()))
    dist = ld.distances(gotd, want, c.d, c.vvt)
    record("a dense", c, rho, chunks, dist, ref_dist)
    print("a dense", c.name(), "rho_ref %.3e" % rho, {k: "%.2e" % r for k, r in dist.items()})
    ld.assert_within(gotd, want, rho, c.d, c.vvt, what="a dense " + c.name())
    cov.clear_cache()


# ------------------------------------------------------------------------------------------------
# b. the E-pass beyond 512 and 1024 columns, long double from the fixture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,recipe", [((300, 3, 520), SHARP), ((300, 9, 520), SHARP), ((300, 9, 520), WIDE), ((200, 3, 1030), SHARP)],
                         ids=["second_column_pair", "two_coordinate_blocks", "two_coordinate_blocks_wide", "second_column_block"])
def test_epass_upper_halves(shape, recipe):
    """mpad = 640: the second column pair of the E-pass partly filled; the same with d = 9, two coordinate blocks; mpad = 1152: the second
    column block, and two row blocks over Qbar.  At d = 9 the sharp length scales (w in [2, 8]) leave a nearly diagonal kernel, gradients
    of 1e-8 in log w and the pseudo-inputs that are sums of cancelling terms, and rho_ref = 1e-7: that case holds the device to no more
    than 3e-6, so the same shape runs with w in [0.05, 0.2] as well, where rho_ref is 3e-13."""
    c = case(shape, recipe)
    got, chunks, _dev = run_device(c.x, c.t, c.theta, c.m, c.xs)
    assert chunks == 0
    check("b", c, got, chunks)


# ------------------------------------------------------------------------------------------------
# c. split-K inside the fit, the likelihood and the gradient
# ------------------------------------------------------------------------------------------------
def test_natural_split():
    """npad / 128 = 128, mpad = 256: three lower tiles never fill a round of the chip, so spgp_pick_split takes the divisor that fills the
    most of one -- the largest whose chunks are still 2048 long, 16384 / 2048 = 8"""
    c = case((16384, 3, 130), SOFT)
    got, chunks, _dev = run_device(c.x, c.t, c.theta, c.m, c.xs)
    assert chunks == 8
    check("c natural", c, got, chunks)


@pytest.mark.parametrize("split", [2, 4, 8])
def test_forced_split(split, monkeypatch):
    c = case((1000, 3, 130), SOFT)          # npad / 128 = 8
    monkeypatch.setenv("GPX_SPGP_SPLIT", str(split))
    got, chunks, _dev = run_device(c.x, c.t, c.theta, c.m, c.xs)
    assert chunks == split
    check("c forced", c, got, chunks)


def test_forced_split_not_a_divisor(monkeypatch):
    c = case((1000, 3, 130), SOFT)
    monkeypatch.delenv("GPX_SPGP_SPLIT", raising=False)
    plain, chunks0, _dev = run_device(c.x, c.t, c.theta, c.m, c.xs)
    monkeypatch.setenv("GPX_SPGP_SPLIT", "3")
    got, chunks, _dev = run_device(c.x, c.t, c.theta, c.m, c.xs)
    assert chunks0 == 0 and chunks == 0
    check("c unsplit", c, plain, chunks0)
    for k in plain:
        np.testing.assert_array_equal(got[k], plain[k])


# ------------------------------------------------------------------------------------------------
# d. the same problems 2^17 away from the origin
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,recipe", [((1500, 3, 130), SOFT), ((300, 3, 520), SHARP)], ids=["m130", "m520"])
def test_shifted_inputs(shape, recipe):
    """x, the pseudo-inputs and the queries moved by 2^17 in every coordinate, exactly: the unshifted case's long-double values and its
    rho_ref hold.  (The oracle is no reference here: it expands squares and is 6e-7 off in the likelihood at this shift.)  The device takes
    every input from the first training row, and the translated grid inputs leave the same differences from it: the same bits as well."""
    c = case(shape, recipe)
    x, t, theta, xs = c.shifted()
    got, chunks, dev = run_device(x, t, theta, c.m, xs)
    cross = dev.cross(np.ascontiguousarray(xs), x)
    del dev
    check("d shifted", c, got, chunks)
    plain, _chunks, dev = run_device(c.x, c.t, c.theta, c.m, c.xs)
    for k in plain:
        np.testing.assert_array_equal(got[k], plain[k])
    np.testing.assert_array_equal(cross, dev.cross(np.ascontiguousarray(c.xs), c.x))


# ------------------------------------------------------------------------------------------------
# e. two chunks of queries
# ------------------------------------------------------------------------------------------------
def test_two_prediction_chunks():
    c = case((300, 2, 7), SOFT)
    rng = np.random.RandomState(65536)
    ms = 65536 + ld.NQ
    xs = np.ascontiguousarray(np.concatenate([c.xs, np.round(rng.uniform(0, 10, (ms - ld.NQ, c.d)) * 2.0 ** 20) / 2.0 ** 20]))
    dev = sk.SPGPCovariance(c.m)._model(c.x, c.t, c.theta)
    mean, var = dev.predict(xs)
    assert mean.shape == var.shape == (ms,)
    ref = dict(zip(("mean", "var"), ld.woodbury_predict(c.x, c.t, c.theta, c.m, xs)))
    dist = ld.assert_within({"mean": mean, "var": var}, ref, c.rho, c.d, c.vvt, what="e against float64")
    record("e all %d queries against float64" % ms, c, c.rho, dev.split(), dist, {})
    check("e first chunk's head", c, {"mean": mean[:ld.NQ], "var": var[:ld.NQ]}, dev.split(), keys=("mean", "var"))
    for part in (slice(0, ld.NQ), slice(ms - ld.NQ, ms)):        # the second chunk holds the last 77 only: offsets of xs, mean_out, var_out
        m1, v1 = dev.predict(np.ascontiguousarray(xs[part]))
        np.testing.assert_allclose(mean[part], m1, rtol=0, atol=1e-12)
        np.testing.assert_allclose(var[part], v1, rtol=0, atol=1e-12)
