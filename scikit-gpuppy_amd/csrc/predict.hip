// predict.hip -- the C-ABI of libgpx (include/gpx.h), part 2: everything that solves against the factor after a fit -- the
// many-row solve behind estimate_many, the few-vector solves, K^-1 and its row panels.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <initializer_list>

#include "common.h"
#include "gram_tile.h"

int ensure_Z(gpx_handle *h, int64_t rows)
{
    if (h->zrows >= rows && h->Z) return 0;
    if (h->Z) { dfree(h->Z); h->Z = nullptr; h->zrows = 0; }
    GPX_TRY(dalloc(&h->Z, rows * h->npad));
    h->zrows = rows;
    return 0;
}

// ---- predict (RowSolve: common.h) ----------------------------------------------------------------
int64_t row_solve_chunk_cap(const gpx_handle *h, int64_t chunk_cap)
{
    int64_t cap = ((int64_t)8 << 30) / (h->npad * (int64_t)sizeof(double));   // rows per 8 GB buffer (two of them: Z and Zs)
    cap = std::max<int64_t>(TILE, cap / TILE * TILE);
    cap = std::min<int64_t>(cap, 32768);   // (tests/test_spgp_pseudo.py, CHUNK_ROWS: its chunk-seam test is cut for this figure)
    if (chunk_cap > 0) cap = std::min<int64_t>(cap, std::max<int64_t>(TILE, chunk_cap / TILE * TILE));
    return cap;
}

int row_solve_begin(gpx_handle *h, int64_t m, RowSolve &rs, bool bounded, bool allow_few, int64_t chunk_cap)
{
    rs.chunk = std::min<int64_t>(round_up(m, TILE), row_solve_chunk_cap(h, chunk_cap));
    GPX_TRY(ensure_Z(h, rs.chunk));
    // the triangular solve runs out of place against the inverted diagonal squares (tsolve.hip): second slab-major buffer
    GPX_TRY(rs.sc.take(&rs.Zs, rs.chunk * h->npad));
    rs.few = allow_few && m <= 32 && h->tri.ready() && h->tri.P >= 2;
    // the emulated updates' workspace (emu.hip), once per call: sized for the chunk, it serves every shorter one
    if (!rs.few) trsm_emu_need(rs.ew, rs.chunk, &h->tri, 0, h->tri.P);
    if (rs.ew.held.img) GPX_TRY(emu_alloc(rs.ew, &rs.sc));
    rs.emu = rs.ew.a.base ? &rs.ew : nullptr;
    // a caller that bounds every solved row (estimate_many) takes the left-looking order over five slabs or more; as above the choice
    // depends on the factor's shape alone.  An image that does not fit leaves the recursion in charge.
    if (emu_left_route(bounded, rs.few, h->tri.ready(), h->tri.P)) {
        rs.left.use(emu_left_plan(rs.chunk, h->tri.P));
        rs.left.reserve(rs.left);
        if (emu_alloc(rs.left, &rs.sc) == 0) rs.use_left = true;
        else {   // (the image, its tiles and arrays went back whole; the refusal is no error of this call)
            if (getenv("GPX_DEBUG")) fprintf(stderr, "[gpx] left-looking solve: no room for the residue image (%s): binary recursion\n", gpx_last_error());
            gpx_set_error("%s", "");
        }
    }
    return 0;
}

int row_solve_run(gpx_handle *h, const RowSolve &rs, int64_t mc, int64_t mp, const GemmReduce *red, bool left)
{
    // a handful of queries (estimate(x_star), plots): the solver for a few right-hand sides -- one forward sweep over the factor's
    // triangle (HBM-bound, ~0.5 ms at N = 16384) instead of the many-right-hand-side recursion on one 128-row tile (its products
    // would be 128 x K strips with K up to N/2: 2.5-3 ms)
    if (!red && rs.few) return h->tri.solve(h->Z, h->npad, (int)mc, rs.Zs, nullptr, h->stream, &h->prof);
    if (left) return trsm_right_lt_slabs(h->Z, rs.Zs, h->npad, mp, &h->tri, h->stream, &h->prof, red, rs.left, rs.emu);
    return trsm_right_lt_squares(h->Z, rs.Zs, h->npad, mp, &h->tri, 0, h->tri.P, h->stream, &h->prof, red, rs.emu);
}

// The chunk loop behind gpx_predict / gpx_predict_kv / gpx_periodic_predict / gpx_matern_predict and gpx_propagate_quadrature_many
// (PredictRun: common.h).
// from_x: the cross-covariance rows come from the Gram kernel on queries that the caller's load leaves on the device in pr.xq; otherwise
// load fills h->Z with the caller's rows kv [m, n] and pr.kd with the prior variance of each query (the diagonal of cov_matrix(x_star),
// GaussianProcess.py:75).
// A periodic handle (pr.periodic): the rows come from periodic_gram_kernel, +vt on equality included, and the prior variance is
// v + vt.  That call promises a result that does not depend on the query's place in the batch or on the chunking: always the many-row
// solver and the stand-alone row reduction (the few-vector solver and the reduction fused into a slab's last product sum in other
// orders), chunks of at most GPX_PERIODIC_CHUNK rows (read at every call; default: the solver's own cap).
// A Matern handle: the rows come from matern_gram_kernel, +vt on equality included, through the routes of a Gaussian handle; the
// row bound of the left-looking solve is sqrt(v + vt) for both kinds whose Gram adds vt itself (handle_gram_has_vt).
int predict_run_begin(gpx_handle *h, bool from_x, int64_t m, PredictRun &pr)
{
    pr.from_x = from_x;
    pr.periodic = from_x && h->kind == KernelKind::Periodic;
    const int d = handle_dim(h);
    RowSolve &rs = pr.rs;
    // |row of Zs|^2 = k*^T K^-1 k* <= k(x*, x*): sqrt(v) for the built-in kernel, sqrt(kdiag) for the caller's (tsolve.hip, launch_row_bounds)
    int64_t chunk_cap = 0;
    if (pr.periodic)
        if (const char *e = getenv("GPX_PERIODIC_CHUNK")) chunk_cap = atoll(e);
    GPX_TRY(row_solve_begin(h, m, rs, true, !pr.periodic, chunk_cap));
    const int64_t chunk = rs.chunk;
    // the row sums |z|^2 and z.y ride in the epilogue of each slab's last product (tsolve.hip): per row one partial pair per 64 columns
    pr.nslots = h->npad / 64;
    pr.fused = chunk >= 3072 && !pr.periodic;
    GPX_TRY(rs.sc.take(&pr.xq, chunk * std::max(d, 1)));
    GPX_TRY(rs.sc.take(&pr.xqw, chunk * std::max(d, 1)));
    GPX_TRY(rs.sc.take(&pr.kd, chunk));
    if (pr.fused) GPX_TRY(rs.sc.take(&pr.part, 2 * chunk * pr.nslots));
    return 0;
}

// One chunk of mc <= pr.rs.chunk rows (m0: the chunk's first row, for the diagnostic alone): load, Gram, solve, row reduction into
// mean_dev / var_dev [mc] (device), then done() -- whatever the caller queues behind the reduction -- the status word and the chunk's one
// synchronisation.
int predict_run_chunk(gpx_handle *h, PredictRun &pr, int64_t m0, int64_t mc, const std::function<int(int64_t, int64_t)> &load, double *mean_dev,
                      double *var_dev, const std::function<hipError_t()> &done)
{
    hipStream_t s = h->stream;
    RowSolve &rs = pr.rs;
    const bool from_x = pr.from_x;
    const int64_t chunk = rs.chunk, nslots = pr.nslots, mp = round_up(mc, TILE);
    double *xq = pr.xq, *xqw = pr.xqw, *kd = pr.kd, *part = pr.part, *Zs = rs.Zs;
    // Z <- the chunk's cross-covariance rows, zero padded
    auto fill = [&]() -> int {
        GPX_TRY(load(mc, mp));
        if (!from_x) return 0;   // the operator's own cross-covariance rows, zero padded to the tile grid by load
        const bool scale = h->kind == KernelKind::Gaussian;   // its Gram kernel reads inputs scaled by sqrt(w)
        if (scale) GPX_TRY(launch_scale_rows(xq, mc, mp, h->d, h->sw, xqw, s));
        // kv = cross-covariance (no add_diag), zero padded: rows >= mc and columns >= n are 0
        return handle_gram(h, scale ? xqw : xq, mc, handle_train_inputs(h), h->n, 0.0, 0, PAD_ZERO, h->Z, h->npad, mp, h->npad, s, &h->prof);
    };
    // Z <- kv L^-T  : row m of Z is (L^-1 kv_m)^T
    // var = k_mm - |z|^2 (k_mm = v + vt for the built-in kernel: k includes vt, GaussianProcess.py:75,78) ; mean = z . y
    auto solve = [&](bool left) -> int {
        if (pr.fused && mp >= 3072) {
            GemmReduce red;
            red.y = h->y; red.p2 = part; red.py = part + chunk * nslots; red.nslots = nslots;
            GPX_TRY(row_solve_run(h, rs, mc, mp, &red, left));
            ProfScope ps(&h->prof, s, GPX_K_REDUCE, 16.0 * (double)mc * (double)nslots);
            return launch_predict_finish(red.p2, red.py, nslots, mc, h->v + h->vt, mean_dev, var_dev, s, from_x ? nullptr : kd);
        }
        GPX_TRY(row_solve_run(h, rs, mc, mp, nullptr, left));
        return launch_predict_reduce(Zs, h->npad, mc, h->npad, h->y, h->v + h->vt, mean_dev, var_dev, s, &h->prof, from_x ? nullptr : kd);
    };
    // a bound that did not hold (the status word of emu.hip, read at the chunk's synchronisation) sends the chunk through the binary
    // recursion once more: Z is consumed by the solve, so it is filled again first
    return emu_left_guarded(rs.use_left, [&](bool left, int *status) -> int {
        GPX_TRY(fill());
        if (left) {
            GPX_TRY(launch_row_bounds(from_x ? nullptr : kd, handle_gram_has_vt(h) ? h->v + h->vt : h->v, mc, rs.left.bound, s));
            GPX_TRY(emu_left_begin(rs.left, rs.left.bound, mc, s));
        }
        GPX_TRY(solve(left));
        // (the status word last: the host-side set-up of the caller's result copies then runs underneath the solve, as before)
        hipError_t e = done();
        if (e == hipSuccess && left) e = hipMemcpyAsync(status, rs.left.status(), sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { gpx_set_error("predict copy-out failed: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
        if (*status && getenv("GPX_DEBUG")) fprintf(stderr, "[gpx] left-looking solve: a row bound did not hold in rows %ld..%ld: binary recursion\n", (long)m0, (long)(m0 + mc));
        return 0;
    });
}

// xs != nullptr: gpx_predict / gpx_periodic_predict; otherwise kv [m, n] and kdiag [m] are the caller's (gpx_predict_kv)
static int predict_common(gpx_handle *h, const double *xs, const double *kv, const double *kdiag, int64_t m, double *mean_out, double *var_out)
{
    hipStream_t s = h->stream;
    PredictRun pr(s);
    GPX_TRY(predict_run_begin(h, xs != nullptr, m, pr));
    const int64_t chunk = pr.rs.chunk;
    const int d = handle_dim(h);
    double *mv = nullptr;
    GPX_TRY(pr.rs.sc.take(&mv, 2 * chunk));
    int rc = 0;
    for (int64_t m0 = 0; m0 < m && rc == 0; m0 += chunk) {
        const int64_t mc = std::min<int64_t>(chunk, m - m0);
        rc = predict_run_chunk(h, pr, m0, mc, [&](int64_t, int64_t mp) -> int {
            hipError_t e = hipSuccess;
            if (xs) {
                e = hipMemcpyAsync(pr.xq, xs + m0 * d, sizeof(double) * mc * d, hipMemcpyDefault, s);
                if (e != hipSuccess) { gpx_set_error("copy xs failed: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
                return 0;
            }
            e = hipMemsetAsync(h->Z, 0, sizeof(double) * mp * h->npad, s);
            if (e == hipSuccess) e = hipMemcpy2DAsync(h->Z, sizeof(double) * h->npad, kv + m0 * h->n, sizeof(double) * h->n, sizeof(double) * h->n, mc, hipMemcpyDefault, s);
            if (e == hipSuccess) e = hipMemcpyAsync(pr.kd, kdiag + m0, sizeof(double) * mc, hipMemcpyDefault, s);
            if (e != hipSuccess) { gpx_set_error("copy kv / kdiag failed: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
            return 0;
        }, mv, mv + chunk, [&]() -> hipError_t {
            hipError_t e = hipMemcpyAsync(mean_out + m0, mv, sizeof(double) * mc, hipMemcpyDefault, s);
            if (e == hipSuccess) e = hipMemcpyAsync(var_out + m0, mv + chunk, sizeof(double) * mc, hipMemcpyDefault, s);
            return e;
        });
    }
    return rc;
}

// gpx_predict / gpx_periodic_predict / gpx_matern_predict after their CHECK_H (which names the entry point): each takes the handles of
// its own kind alone
static int predict_entry(gpx_handle *h, KernelKind kind, const char *what, const double *xs, int64_t m, double *mean_out, double *var_out)
{
    GPX_TRY(kind == KernelKind::Gaussian ? need_kernel(h, what) : need_kind(h, kind, what));
    if (m < 0 || (m > 0 && (!xs || !mean_out || !var_out))) { gpx_set_error("%s: bad arguments", what); return GPX_ERR_BAD_ARG; }
    if (m == 0) return 0;
    return predict_common(h, xs, nullptr, nullptr, m, mean_out, var_out);
}

extern "C" int gpx_predict(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *var_out)
{
    CHECK_H(h);
    return predict_entry(h, KernelKind::Gaussian, "gpx_predict", xs, m, mean_out, var_out);
}

// estimate_many / estimate with cov = PeriodicCovariance (skgpuppy/GaussianProcess.py:68-80, :94-111): kv = cov_matrix_ij(x_star, x) with the
// base class's +vt on equality, k = v + vt for every query; mean WITHOUT meant
extern "C" int gpx_periodic_predict(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *var_out)
{
    CHECK_H(h);
    return predict_entry(h, KernelKind::Periodic, "gpx_periodic_predict", xs, m, mean_out, var_out);
}

// estimate_many / estimate with cov = MaternCovariance: the rows come from matern_gram_kernel with the +vt on equality, k = v + vt for
// every query (also as the row bound of the left-looking solve); the routes are gpx_predict's; mean WITHOUT meant
extern "C" int gpx_matern_predict(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *var_out)
{
    CHECK_H(h);
    return predict_entry(h, KernelKind::Matern, "gpx_matern_predict", xs, m, mean_out, var_out);
}

// estimate_many for ANY operator (skgpuppy/GaussianProcess.py:68-80): kv = cov.cov_matrix_ij(x_star, x) [m, n] and
// kdiag = diag(cov.cov_matrix(x_star)) [m] come from the caller; mean_out = kv alpha (WITHOUT meant), var_out = kdiag - |L^-1 kv^T|^2.
// Works on every handle (gpx_fit and gpx_fit_matrix).
extern "C" int gpx_predict_kv(gpx_handle *h, const double *kv, int64_t m, const double *kdiag, double *mean_out, double *var_out)
{
    CHECK_H(h);
    if (m < 0 || (m > 0 && (!kv || !kdiag || !mean_out || !var_out))) { gpx_set_error("gpx_predict_kv: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (m == 0) return 0;
    return predict_common(h, nullptr, kv, kdiag, m, mean_out, var_out);
}

// The left-looking solve alone on caller device buffers against a fitted handle's factor (tests): Zs [rows, ldz] <- Z L^-T with Z
// [rows, ldz] consumed (afterwards slab p of Z holds Z_p minus its updates: what the leaf products read), bound [rows] the caller's bound
// on every solved row, tile_rows > 0 a smaller row tile of the residue image.  *status_out: the status word (non-zero: a bound did not
// hold and Zs is not to be used).  Synchronous.
extern "C" int gpx_emu_trsm_left(gpx_handle *h, double *Z, int64_t ldz, int64_t rows, const double *bound, double *Zs, int64_t tile_rows,
                                 int *status_out)
{
    CHECK_H(h);
    if (!Z || !Zs || !bound || !status_out || rows <= 0 || rows % TILE || ldz < h->npad || ldz & 1 || tile_rows < 0) {
        gpx_set_error("gpx_emu_trsm_left: bad arguments (rows %ld a multiple of 128, ldz %ld >= %ld and even)", (long)rows, (long)ldz, (long)h->npad);
        return GPX_ERR_BAD_ARG;
    }
    if (!h->tri.ready() || h->tri.P < 5 || !emu_enabled(4096)) { gpx_set_error("gpx_emu_trsm_left: needs a prepared solver over 5 slabs or more and the emulated update"); return GPX_ERR_STATE; }
    hipStream_t s = h->stream;
    Scratch sc(s);
    EmuFrame w;
    w.use(emu_left_plan(rows, h->tri.P, tile_rows));
    w.reserve(w);
    GPX_TRY(emu_alloc(w, &sc));
    GPX_TRY(emu_left_begin(w, bound, rows, s));
    GPX_TRY(trsm_right_lt_slabs(Z, Zs, ldz, rows, &h->tri, s, &h->prof, nullptr, w));
    GPX_HIP(hipMemcpyAsync(status_out, w.status(), sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- a few vectors against the factor ----------------------------------------------------------------
// The block loop of gpx_solve / gpx_chol_mul: the rows of in [nrhs, n], 32 at a time and zero padded to npad, into b; run(nc) queues
// the solver call on that block; every (device block [32, npad], caller's [nrhs, n] or null) pair of outs is then copied out.
template <class Run>
static int row_blocks(gpx_handle *h, const double *in, int nrhs, double *b, Run run, std::initializer_list<std::pair<const double *, double *>> outs)
{
    hipStream_t s = h->stream;
    const size_t rn = sizeof(double) * h->n, rp = sizeof(double) * h->npad;
    for (int c0 = 0; c0 < nrhs; c0 += 32) {
        const int nc = std::min(32, nrhs - c0);
        GPX_HIP(hipMemsetAsync(b, 0, 32 * rp, s));
        GPX_HIP(hipMemcpy2DAsync(b, rp, in + (int64_t)c0 * h->n, rn, rn, nc, hipMemcpyDefault, s));
        GPX_TRY(run(nc));
        for (const auto &o : outs)
            if (o.second) GPX_HIP(hipMemcpy2DAsync(o.second + (int64_t)c0 * h->n, rn, o.first, rp, rn, nc, hipMemcpyDefault, s));
    }
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

// K^-1 B (and L^-1 B) for a few right-hand sides without K^-1: two sweeps over the triangle of L per 32 right-hand sides
extern "C" int gpx_solve(gpx_handle *h, const double *B, int nrhs, double *Linv_B_out, double *Kinv_B_out)
{
    CHECK_H(h);
    if (!B || nrhs < 1 || (!Linv_B_out && !Kinv_B_out)) { gpx_set_error("gpx_solve: bad arguments (nrhs=%d)", nrhs); return GPX_ERR_BAD_ARG; }
    Scratch sc(h->stream);
    double *b = nullptr;   // [3][32][npad]: zero-padded right-hand sides, L^-1 B, K^-1 B
    GPX_TRY(sc.take(&b, 3 * 32 * h->npad));
    double *y = b + 32 * h->npad, *a = y + 32 * h->npad;
    return row_blocks(h, B, nrhs, b, [&](int nc) { return h->tri.solve(b, h->npad, nc, Linv_B_out ? y : nullptr, Kinv_B_out ? a : nullptr, h->stream, &h->prof); },
                      {{y, Linv_B_out}, {a, Kinv_B_out}});
}

// L Z for a few vectors (rows of Z): a draw t = L z ~ N(0, K) for every standard-normal row z
extern "C" int gpx_chol_mul(gpx_handle *h, const double *Z, int nrhs, double *out)
{
    CHECK_H(h);
    if (!Z || !out || nrhs < 1) { gpx_set_error("gpx_chol_mul: bad arguments (nrhs=%d)", nrhs); return GPX_ERR_BAD_ARG; }
    Scratch sc(h->stream);
    double *b = nullptr;   // [2][32][npad]
    GPX_TRY(sc.take(&b, 2 * 32 * h->npad));
    double *o = b + 32 * h->npad;
    return row_blocks(h, Z, nrhs, b, [&](int nc) { return h->tri.mul_lower(b, h->npad, nc, o, h->stream); }, {{o, out}});
}

// ---- K^-1 and its row panels ---------------------------------------------------------------------------
int ensure_kinv(gpx_handle *h)
{
    if (h->Kinv) return 0;
    hipStream_t s = h->stream;
    GPX_TRY(ensure_Z(h, h->npad));
    Scratch sc(s);
    double *K = nullptr;
    GPX_TRY(sc.take(&K, h->npad * h->npad));
    // Z = L^-T (upper triangular, structured recursion) ; Kinv = Z Z^T = L^-T L^-1 (lower strips, then mirrored)
    // (handles without a prepared solver: the 128-column leaves of chol.hip)
    GPX_TRY(h->tri.ready() ? build_kinv_from_solver(&h->tri, h->Z, K, s, &h->prof)
                           : build_kinv_from_factor(h->L, h->npad, h->nblk, h->Dinv, h->Z, K, s, &h->prof));
    const hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) { gpx_set_error("Kinv build failed: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    h->Kinv = sc.release(K);
    return 0;
}

// Rows [row0, row1) (multiples of 128, row1 <= npad) of K^-1 for the row-sharded propagation: the whole matrix if it exists or if the
// range is all of it, otherwise a row PANEL built alone (TriSolver::kinv_rows: 2 m N^2 flop, three m x N buffers) and kept until another
// range is asked for.  Returns in *base a pointer that is indexed with ABSOLUTE row numbers (base + i * npad is row i).
int ensure_kinv_rows(gpx_handle *h, int64_t row0, int64_t row1, const double **base)
{
    const int64_t np = h->npad;
    // a panel that does not contain the range is replaced by one over the hull of both (a rank's Approx and Exact shards differ: equal
    // rows against equal area of the triangle); a hull of three quarters of the rows or more is not worth a panel
    if (h->KinvRows && !(h->kr0 <= row0 && row1 <= h->kr1)) { row0 = std::min(row0, h->kr0); row1 = std::max(row1, h->kr1); }
    if (!h->Kinv && 4 * (row1 - row0) < 3 * np && h->tri.ready() && row1 > row0) {
        if (!(h->KinvRows && h->kr0 <= row0 && row1 <= h->kr1)) {
            hipStream_t s = h->stream;
            if (h->KinvRows) { GPX_HIP(hipStreamSynchronize(s)); dfree(h->KinvRows); h->KinvRows = nullptr; }
            const int64_t m = row1 - row0;
            Scratch sc(s);
            double *X = nullptr, *Zb = nullptr, *Yb = nullptr, *Tb = nullptr;
            GPX_TRY(sc.take(&X, m * np));
            GPX_TRY(sc.take(&Zb, m * np));
            GPX_TRY(sc.take(&Yb, m * np));
            GPX_TRY(sc.take(&Tb, (int64_t)CHOL_PANEL_COLS * np));
            GPX_TRY(h->tri.kinv_rows(row0, row1, X, Zb, Yb, Tb, s, &h->prof));
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) { gpx_set_error("K^-1 row panel failed: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
            h->KinvRows = sc.release(X); h->kr0 = row0; h->kr1 = row1;
        }
        *base = reinterpret_cast<const double *>(reinterpret_cast<uintptr_t>(h->KinvRows) - (uintptr_t)(sizeof(double) * (size_t)(h->kr0 * np)));
        return 0;
    }
    if (h->KinvRows && !h->Kinv) { GPX_HIP(hipStreamSynchronize(h->stream)); dfree(h->KinvRows); h->KinvRows = nullptr; h->kr0 = h->kr1 = 0; }
    GPX_TRY(ensure_kinv(h));
    *base = h->Kinv;
    return 0;
}

// a row range of the sharded entry points: 0 <= row0 <= row1 <= n, each end a multiple of 128 or n
int check_row_range(const gpx_handle *h, int64_t row0, int64_t row1, const char *what)
{
    if (row0 < 0 || row1 < row0 || row1 > h->n || (row0 % TILE && row0 != h->n) || (row1 % TILE && row1 != h->n)) {
        gpx_set_error("%s: bad arguments (rows [%ld, %ld) of %ld)", what, (long)row0, (long)row1, (long)h->n);
        return GPX_ERR_BAD_ARG;
    }
    return 0;
}

// test / tool access: rows [row0, row1) of K^-1 (multiples of 128 or n) -> out [row1 - row0, n] (host or device), built as the
// row-sharded propagation builds them
extern "C" int gpx_kinv_rows(gpx_handle *h, int64_t row0, int64_t row1, double *out)
{
    CHECK_H_PSEUDO_OK(h);
    // (an empty range is an error here alone; with it excluded, row0 == n cannot pass and the shared test is the test of old)
    if (!out || row1 <= row0) { gpx_set_error("gpx_kinv_rows: bad arguments (rows [%ld, %ld) of %ld)", (long)row0, (long)row1, (long)h->n); return GPX_ERR_BAD_ARG; }
    GPX_TRY(check_row_range(h, row0, row1, "gpx_kinv_rows"));
    const double *base = nullptr;
    GPX_TRY(ensure_kinv_rows(h, row0, round_up(row1, TILE), &base));
    GPX_HIP(hipMemcpy2DAsync(out, sizeof(double) * h->n, base + row0 * h->npad, sizeof(double) * h->npad, sizeof(double) * h->n, (size_t)(row1 - row0),
                             hipMemcpyDefault, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int gpx_kinv(gpx_handle *h, double *Kinv_out)
{
    CHECK_H_PSEUDO_OK(h);
    if (!Kinv_out) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(ensure_kinv(h));
    GPX_HIP(hipMemcpy2DAsync(Kinv_out, sizeof(double) * h->n, h->Kinv, sizeof(double) * h->npad, sizeof(double) * h->n, h->n,
                             hipMemcpyDefault, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}
