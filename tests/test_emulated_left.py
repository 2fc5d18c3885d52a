"""The left-looking emulated solve (csrc/tsolve.hip trsm_right_lt_slabs, csrc/emu.hip emu_left_plan / emu_left_update) on the GPU.

Entry point: gpx_emu_trsm_left at the smallest shapes that reach every branch -- npad = 5120 (one emulated slab, K = 4096), 6144 (the
residues of slabs 0 .. 3 read at two depths), 9216 (five depths), 300 rows (padded to 384), and 640 rows in row tiles of 256 through the
entry's test-only tile argument (emu_cap(4096, 16) = 32768 rows: no natural shape of test size has two tiles).  Every emulated update is
compared entry by entry with the error-free reference of tests/_exact_product.py, slab by slab: the call leaves Z_p minus its update in
Z, so  exact_sub(Z0_p, Zs[:, 0:K), L[p, 0:K))  is what slab p must hold, under the bound of tests/_emu_left_model.py (DESIGN.md section
6).  Largest observed share of the bound on an MI355X: 0.1759 (npad = 6144, slab 5); 0.1576 / 0.1601 / 0.1548 at npad = 5120 / 9216 /
three row tiles (the EMU-LEFT lines the test prints; profiles/r12_left_looking.txt).

Bound edge cases ride in every shape: a row whose largest entry equals its bound, a row 2^-30 below its bound, an all-zero row with
bound 0, a row with a NaN (NaN from the NaN's slab on, every other row bit-unchanged), and a row whose bound is too small by a factor of
8 (the status word is raised).  Call site: estimate_many and gpx_predict_kv at N = 5200 and 7300 against the oracle, in child processes
with GPX_EMU_LEFT = 1 and 0 (the switches are read once per process): with 300 queries (the row sums in a pass of their own), and at
N = 5200 with 3100 and 14400 queries, where the row sums ride with each slab's leaf (predict.hip: 3072 padded rows or more; below
14336 rows launch_slab_reduce, from there on the leaf product's own epilogue) -- the only form the benchmark's shape runs.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _emu_left_model as lm
import _exact_product as xp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 8
THETA = np.log(np.array([2.0, 0.01] + [0.04] * D))
V, VT = 2.0, 0.01
SHAPES = [(5120, 300, 0), (6144, 300, 0), (9216, 300, 0), (5120, 640, 256)]      # npad, rows, tile_rows
R_EQ, R_30, R_ZERO, R_NAN, R_BAD = 3, 5, 9, 11, 3                                # the special rows (R_BAD: in a run of its own)
CHECK_ROWS = 24                                                                  # rows per shape held against the exact reference
SITE_N = (5200, 7300)
SITE_M = 300
FUSED_M = (3100, 14400)                                                          # at SITE_N[0]: fused row sums, by slab pass / by leaf epilogue
SITE_CASES = [(N, SITE_M) for N in SITE_N] + [(SITE_N[0], M) for M in FUSED_M]


def _problem(N, M, d=D, seed=0):
    rng = np.random.RandomState(1000 + N + seed)
    x = rng.uniform(0, 10, (N, d))
    t = np.sin(0.3 * x.sum(1)) + 0.1 * rng.randn(N)
    xs = rng.uniform(0, 10, (M, d))
    xs[::7] = x[rng.randint(0, N, len(xs[::7]))] + 1e-3 * rng.randn(len(xs[::7]), d)      # queries next to training points: large |Zs|
    return x, t, xs


# ------------------------------------------------------------------------------------------------------------------------
# child processes
# ------------------------------------------------------------------------------------------------------------------------
def _load():
    import torch  # (HIP runtime of torch first, as in the rest of the suite)
    import skgpuppy_amd as sk
    from skgpuppy_amd import _gpx
    from oracle import oracle as orc
    return torch, sk, _gpx, orc


def run_entry(out):
    """every shape: run 1 (bounds sqrt(v), clean Z), run 2 (the edge rows), run 3 (one bound too small) -> one .npz"""
    torch, sk, _gpx, orc = _load()
    res = {}
    for npad, rows, tile in SHAPES:
        x, t, xs = _problem(npad, rows)
        theta = THETA.copy()
        h = ctypes.c_void_p()
        tc = np.ascontiguousarray(t - t.mean())
        _gpx.check(_gpx.lib.gpx_fit(_gpx.ptr(_gpx.f64(x)), _gpx.ptr(tc), npad, D, _gpx.ptr(_gpx.f64(theta)), None, ctypes.byref(h)), "gpx_fit")
        Lf = np.empty((npad, npad))
        _gpx.check(_gpx.lib.gpx_chol(h, _gpx.ptr(Lf)), "gpx_chol")
        rp = -(-rows // 128) * 128
        Z0 = np.zeros((rp, npad))
        Z0[:rows] = orc.gram_ij(xs, x, theta)
        Z0[R_EQ] = 0.5 * orc.gram_ij(x[:1], x, theta)[0]
        Z0[R_EQ, 0] += 0.5 * VT                                # 0.5 K e_0: the solved row is 0.5 L_00 e_0 up to rounding
        Z0[R_ZERO] = 0.0
        bound = np.zeros(rp)
        bound[:rows] = np.sqrt(V)

        def call(Z, b):
            z, bd = torch.as_tensor(Z).cuda(), torch.as_tensor(b).cuda()
            zs = torch.full_like(z, 7.0)
            st = ctypes.c_int(-1)
            _gpx.check(_gpx.lib.gpx_emu_trsm_left(h, ctypes.c_void_p(z.data_ptr()), npad, rp, ctypes.c_void_p(bd.data_ptr()),
                                                  ctypes.c_void_p(zs.data_ptr()), tile, ctypes.byref(st)), "gpx_emu_trsm_left")
            return zs.cpu().numpy(), z.cpu().numpy(), st.value

        zs1, za1, st1 = call(Z0, bound)
        b2, Z2 = bound.copy(), Z0.copy()
        b2[R_EQ] = np.abs(zs1[R_EQ]).max()
        b2[R_30] = bound[R_30] * 2.0 ** 30
        b2[R_ZERO] = 0.0
        Z2[R_NAN, 5 * 1024 + 17 if npad > 6144 else 4 * 1024 + 17] = np.nan
        zs2, za2, st2 = call(Z2, b2)
        b3 = b2.copy()
        b3[R_BAD] = b2[R_EQ] / 8.0
        _zs3, _za3, st3 = call(Z2, b3)
        b4 = bound.copy()
        b4[20] = -1.0
        st4 = call(Z0, b4)[2]
        _gpx.lib.gpx_free(h)
        k = "%d_%d_%d_" % (npad, rows, tile)
        sel = np.array(sorted({R_EQ, R_30, R_ZERO, 0, rows - 1, rp - 1} | set(np.random.RandomState(npad).randint(0, rows, CHECK_ROWS).tolist()) - {R_NAN}))
        res.update({k + "L": Lf[4096:], k + "sel": sel, k + "Z0": Z2[sel], k + "zs2": zs2[sel], k + "za2": za2[sel], k + "b2": b2[sel],
                    k + "same": np.array([np.array_equal(np.delete(zs1, [R_EQ, R_30, R_ZERO, R_NAN], 0), np.delete(zs2, [R_EQ, R_30, R_ZERO, R_NAN], 0))]),
                    k + "nanrow": zs2[R_NAN], k + "zerorow": zs2[R_ZERO], k + "eqrow": zs1[R_EQ], k + "status": np.array([st1, st2, st3, st4]),
                    k + "z1eq": zs1[R_30], k + "z2eq": zs2[R_30]})
    np.savez(out, **res)


def run_site(out):
    """estimate_many, gpx_predict_kv (also with one kdiag too small by 64), the same query at three places, propagate_GA_many"""
    torch, sk, _gpx, orc = _load()
    res = {}
    for N, M in SITE_CASES:
        x, t, xs = _problem(N, M, seed=1)
        key = "%d_%d" % (N, M)
        gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), THETA.copy())
        res["est" + key] = np.stack(gp.estimate_many(xs))
        if (N, M) == SITE_CASES[0]:
            q = xs[5:6]
            perm = np.concatenate([xs[40:290], q, xs[290:]])                     # the query at position 250 among other neighbours
            few = np.concatenate([q, xs[100:132]])                               # 33 rows: the smallest call on the many-row route
            res["indep"] = np.array([res["est" + key][:, 5], np.stack(gp.estimate_many(perm))[:, 250], np.stack(gp.estimate_many(few))[:, 0]])
        gp._dev().close()
        K, kv = orc.gram(x, THETA), np.ascontiguousarray(orc.gram_ij(xs, x, THETA))
        kd = np.full(M, V + VT)
        tc = np.ascontiguousarray(t - t.mean())
        h = ctypes.c_void_p()
        _gpx.check(_gpx.lib.gpx_fit_matrix(_gpx.ptr(K), _gpx.ptr(tc), N, None, ctypes.byref(h)), "gpx_fit_matrix")
        row7 = kv[7].copy()
        for name, bad in (("kv", False), ("kvbad", True)):
            if bad:                                                              # row 7 = 0.9 K e_0: solved row 0.9 L_00 e_0, its kdiag 64 times too small
                kv[7], kd[7] = 0.9 * K[0], 0.81 * K[0, 0] / 64.0
            mean, var = np.empty(M), np.empty(M)
            _gpx.check(_gpx.lib.gpx_predict_kv(h, _gpx.ptr(kv), M, _gpx.ptr(kd), _gpx.ptr(mean), _gpx.ptr(var)), "gpx_predict_kv")
            res[name + key] = np.stack([mean + t.mean(), var])
        kv[7] = row7
        _gpx.lib.gpx_free(h)
        del K, kv
    N = SITE_N[0]
    x, t, _xs = _problem(N, 1, d=9, seed=2)
    gp = sk.GaussianProcess(x, t, sk.GaussianCovariance(), np.log(np.array([2.0, 0.01] + [0.04] * 9)))
    rng = np.random.RandomState(5)
    U = rng.uniform(0, 10, (10, 9))
    A = rng.uniform(-0.1, 0.1, (10, 9, 9))
    S = np.einsum("bij,bkj->bik", A, A) + 0.005 * np.eye(9)
    res["prop"] = np.stack(sk.UncertaintyPropagationApprox(gp).propagate_GA_many(U, S))
    gp._dev().close()
    np.savez(out, **res)


_RUNS = {}


def _run(tmp_path_factory, name):
    """one child per setting under its own time limit; kept for the tests of this module"""
    mode, env = {"entry": ("entry", {}), "left": ("site", {"GPX_EMU_LEFT": "1", "GPX_DEBUG": "1"}), "binary": ("site", {"GPX_EMU_LEFT": "0"})}[name]
    if name not in _RUNS:
        out = str(tmp_path_factory.mktemp("left") / (name + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, out], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        with np.load(out) as z:
            _RUNS[name] = {k: z[k] for k in z.files}
        _RUNS[name]["stderr"] = r.stderr
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------------------------------
# the entry point
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "npad%d_rows%d_tile%d" % s)
def test_every_emulated_update_within_its_bound(tmp_path_factory, shape):
    r = _run(tmp_path_factory, "entry")
    npad, rows, tile = shape
    k = "%d_%d_%d_" % shape
    slabs = npad // 1024
    abits, bbits = lm.left_bits(slabs)
    Lt, sel, Z0, zs, za, b = (r[k + n] for n in ("L", "sel", "Z0", "zs2", "za2", "b2"))
    assert np.isfinite(zs).all() and np.isfinite(za).all()
    worst = 0.0
    for p in range(4, slabs):
        K = 1024 * p
        A, B, C0 = np.ascontiguousarray(zs[:, :K]), np.ascontiguousarray(Lt[K - 4096:K - 4096 + 1024, :K]), Z0[:, K:K + 1024]
        hi, lo = xp.exact_sub(C0, A, B)
        prod = -xp.exact_sub(np.zeros_like(C0), A, B)[0]
        E = za[:, K:K + 1024]
        bound = lm.left_bound(A, b, B, E, prod, abits, bbits)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where((E - hi) - lo == 0, 0.0, np.abs((E - hi) - lo) / bound)
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        print("EMU-LEFT npad %5d rows %4d tile %3d slab %d (K = %5d): max error/bound %.4f at row %d column %d" % (npad, rows, tile, p, K, ratio[at], sel[at[0]], at[1]), flush=True)
        assert ratio[at] <= 1.0, (p, at, float(E[at]), float(hi[at]), float(bound[at]))
        worst = max(worst, float(ratio[at]))
        zero = list(sel).index(R_ZERO)
        assert not E[zero].any() and not zs[zero].any()
    print("EMU-LEFT npad %5d rows %4d tile %3d: largest share of the bound %.4f" % (npad, rows, tile, worst), flush=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "npad%d_rows%d_tile%d" % s)
def test_bound_edge_rows_and_the_guard(tmp_path_factory, shape):
    r = _run(tmp_path_factory, "entry")
    npad = shape[0]
    k = "%d_%d_%d_" % shape
    st1, st2, st3, st4 = r[k + "status"]
    assert (st1, st2) == (0, 0) and st3 != 0 and st4 != 0      # bounds that hold; one too small by 8; a negative one
    eq = r[k + "eqrow"]
    assert np.abs(eq).argmax() < 4096 and np.abs(eq).max() <= np.sqrt(V)      # its largest entry: in the native slabs, the same in run 2
    assert r[k + "same"][0]                                    # every row without an edge case: the same bits in run 1 and run 2
    nan_col = 5 * 1024 if npad > 6144 else 4 * 1024
    assert np.isfinite(r[k + "nanrow"][:nan_col]).all() and np.isnan(r[k + "nanrow"][nan_col:]).all()
    assert not r[k + "zerorow"].any()
    # 2^-30 below its bound: the native slabs agree bit for bit, the emulated ones not exactly.  Every entry of the image is then held to
    # delta = 2^(31 - abits) (bound sqrt(2) 2^30: scale abits - 2 - 30, half a unit of it): abits - 31 bits for the row's entries of order 1.
    # With e the image's error, |e_j| <= delta, the solve returns z' with z' L^T = k - r exactly, r_j = e[0:K_j) . L[j, 0:K_j) for the
    # columns j of the emulated slabs (K_j = 1024 p: slab p's depth), so |z' - z|_inf <= |r|_2 |L^-1|_2 <= delta |(|L[j, 0:K_j)|_1)_j|_2 /
    # sqrt(vt)  (K = L L^T >= vt I).  Run 1 has the same with delta 2^(1 - abits).  (The sharp statement for this row is the entry-wise
    # bound of test_every_emulated_update_within_its_bound: R_30 is among its rows, with this bound.  On an MI355X: max|z1 - z2| 5.3e-7 ... 6.2e-7
    # against limits of 2.2e-4 (npad = 5120) ... 5.2e-4 (9216): the limit is a worst case over the signs of e.)
    z1, z2 = r[k + "z1eq"], r[k + "z2eq"]
    assert np.array_equal(z1[:4096], z2[:4096]) and not np.array_equal(z1[4096:], z2[4096:])
    abits = lm.left_bits(npad // 1024)[0]
    Lt = np.abs(r[k + "L"])
    l1 = np.concatenate([Lt[1024 * (p - 4):1024 * (p - 3), :1024 * p].sum(1) for p in range(4, npad // 1024)])
    limit = (2.0 ** (31 - abits) + 2.0 ** (1 - abits)) * np.sqrt((l1 ** 2).sum()) / np.sqrt(VT)
    print("EMU-LEFT npad %5d 2^-30 row: max|z1 - z2| %.3e, limit %.3e (delta 2^%d)" % (npad, np.abs(z1 - z2).max(), 1.01 * limit, 31 - abits), flush=True)
    assert np.abs(z1 - z2).max() <= 1.01 * limit                # (1 %: the fp64 roundings of both runs, of order 2^-52 against 2^-24)


# ------------------------------------------------------------------------------------------------------------------------
# the call site
# ------------------------------------------------------------------------------------------------------------------------
def _oracle(N, M):
    """the oracle's estimate_many; the fitted oracle is kept per N (_problem draws x and t before the queries: the same for every M), and
    the queries go through it 1200 at a time (it forms the products between all queries of a call; a query's result does not depend on them)"""
    if ("oracle", N, M) not in _RUNS:
        from oracle import oracle as orc
        x, t, xs = _problem(N, M, seed=1)
        if ("oracle", N) not in _RUNS:
            _RUNS[("oracle", N)] = orc.OracleGP(x, t, THETA)
        parts = [_RUNS[("oracle", N)].estimate_many(xs[i:i + 1200]) for i in range(0, M, 1200)]
        _RUNS[("oracle", N, M)] = np.stack([np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])])
    return _RUNS[("oracle", N, M)]


_case_id = lambda c: "%d" % c[0] if c[1] == SITE_M else "%d-M%d" % c


@pytest.mark.gpu
@pytest.mark.parametrize("case", SITE_CASES, ids=_case_id)
def test_call_site_against_oracle(tmp_path_factory, case):
    """300 queries: the row sums in a pass of their own; 3100 and 14400: in each slab's leaf (launch_slab_reduce / the leaf's epilogue)"""
    left, binary, ref = _run(tmp_path_factory, "left"), _run(tmp_path_factory, "binary"), _oracle(*case)
    for name in ("est%d_%d" % case, "kv%d_%d" % case):
        for got in (left[name], binary[name]):
            assert np.allclose(got[0], ref[0], rtol=1e-6, atol=1e-9) and np.allclose(got[1], ref[1], rtol=1e-6, atol=1e-9 * V), name
        assert not np.array_equal(left[name], binary[name]), name             # the left-looking route was taken
        print("EMU-LEFT %-8s |dmean| %.3e |dvar| %.3e (binary recursion %.3e %.3e)" % (name, np.abs(left[name][0] - ref[0]).max(), np.abs(left[name][1] - ref[1]).max(),
              np.abs(binary[name][0] - ref[0]).max(), np.abs(binary[name][1] - ref[1]).max()), flush=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SITE_CASES, ids=_case_id)
def test_call_site_guard_reruns_the_chunk(tmp_path_factory, case):
    """a kdiag 64 times too small (its root: 8) on a row that reaches its true bound: the status word sends the chunk through the binary
    recursion, whose bits the caller gets (with the fused row sums the second pass writes every partial slot the first one filled); with
    good bounds nothing is rerun"""
    left, binary = _run(tmp_path_factory, "left"), _run(tmp_path_factory, "binary")
    assert np.array_equal(left["kvbad%d_%d" % case], binary["kvbad%d_%d" % case])
    other = [r for r in range(case[1]) if r != 7]
    assert np.array_equal(left["kvbad%d_%d" % case][:, other], binary["kv%d_%d" % case][:, other])      # the other rows: untouched by row 7
    assert left["stderr"].count("a row bound did not hold") == len(SITE_CASES)


@pytest.mark.gpu
def test_a_query_does_not_depend_on_its_neighbours(tmp_path_factory):
    """alone (33 rows: 32 and fewer take the few-vector solver, another algorithm), at position 5 of 300 and at position 250"""
    a = _run(tmp_path_factory, "left")["indep"]
    assert np.array_equal(a[0], a[1]) and np.array_equal(a[0], a[2])


@pytest.mark.gpu
def test_callers_without_bounds_are_untouched(tmp_path_factory):
    assert np.array_equal(_run(tmp_path_factory, "left")["prop"], _run(tmp_path_factory, "binary")["prop"])


def main(argv):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "scikit-gpuppy_amd"), os.path.join(ROOT, "tests")]
    {"entry": run_entry, "site": run_site}[argv[0]](argv[1])


if __name__ == "__main__":
    main(sys.argv[1:])
