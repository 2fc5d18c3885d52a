// propagate_api.hip -- the C-ABI of libgpx (include/gpx.h), part 3: the uncertainty-propagation entry points (Approx, Exact, their
// sharded and supplied-matrix forms); the kernels they launch live in propagate.hip.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "common.h"
#include "sym_eig.h"

// ---- propagation -----------------------------------------------------------------------------------
// layout of h->V: [128][npad] rows 0 = C, 1..d = J_k (rest zero, so the block is one GEMM row tile)
// layout of h->KV: [128][npad] = V Kinv ; followed by AUX [(d+1)][npad] (row 0 tr, rows 1..d H_kk),
//                  cplain[npad], udev[GPX_MAX_D], Sigma[GPX_MAX_D^2], out[256]
static inline double *aux_ptr(gpx_handle *h) { return h->KV + (int64_t)TILE * h->npad; }
static inline double *cplain_ptr(gpx_handle *h) { return aux_ptr(h) + (int64_t)(h->d + 1) * h->npad; }
static inline double *udev_ptr(gpx_handle *h) { return cplain_ptr(h) + h->npad; }
static inline double *sigma_ptr(gpx_handle *h) { return udev_ptr(h) + GPX_MAX_D; }
static inline double *out_ptr(gpx_handle *h) { return sigma_ptr(h) + GPX_MAX_D * GPX_MAX_D; }

static int ensure_prop_buffers(gpx_handle *h)
{
    if (h->V) return 0;
    // both buffers are committed to the handle only when both allocations and the clear have been issued
    Scratch sc(h->stream);
    double *V = nullptr, *KV = nullptr;
    GPX_TRY(sc.take(&V, (int64_t)TILE * h->npad));
    GPX_TRY(sc.take(&KV, (int64_t)TILE * h->npad + (int64_t)(h->d + 2) * h->npad + GPX_MAX_D + GPX_MAX_D * GPX_MAX_D + 256));
    if (hipMemsetAsync(V, 0, sizeof(double) * TILE * h->npad, h->stream) != hipSuccess) { gpx_set_error("hipMemsetAsync(V) failed"); return GPX_ERR_HIP; }
    h->V = sc.release(V);
    h->KV = sc.release(KV);
    return 0;
}

// how many new-u propagations are answered by the two streaming triangular solves before K^-1 is materialised
// (49 ms once at N = 16384, then one pass over it per new u): a single propagate_GA after a fit never pays for
// K^-1, an inverse-propagation loop switches over after a while
static int approx_solve_limit()
{
    static const int v = getenv("GPX_APPROX_SOLVE_CALLS") ? atoi(getenv("GPX_APPROX_SOLVE_CALLS")) : 24;
    return v;
}

// u and Sigma (the caller's pointers, host or device; Sigma may be null) into the handle's pinned block and on to udev_ptr / sigma_ptr:
// hstage [0, 64) u | [64, 64 + 4096) Sigma | [4160, ..) results.  The block is pinned, so the uploads are asynchronous: no entry
// point synchronises for its arguments.
static inline double *staged_sigma(gpx_handle *h) { return h->hstage + 64; }
static inline double *staged_out(gpx_handle *h) { return h->hstage + 64 + GPX_MAX_D * GPX_MAX_D; }
static int stage_u_sigma(gpx_handle *h, const double *u, const double *Sigma)
{
    const int d = h->d;
    GPX_TRY(ensure_prop_buffers(h));
    if (!h->hstage && !(h->hstage = pinned_acquire())) { gpx_set_error("hipHostMalloc (staging block) failed"); return GPX_ERR_HIP; }
    double *uh = h->hstage, *Sh = staged_sigma(h);
    GPX_TRY(fetch_small(uh, u, d));
    GPX_HIP(hipMemcpyAsync(udev_ptr(h), uh, sizeof(double) * d, hipMemcpyHostToDevice, h->stream));
    if (!Sigma) return 0;
    GPX_TRY(fetch_small(Sh, Sigma, (size_t)d * d));
    GPX_HIP(hipMemcpyAsync(sigma_ptr(h), Sh, sizeof(double) * d * d, hipMemcpyHostToDevice, h->stream));
    return 0;
}

// V, AUX and KV for the staged u (stage_u_sigma), unless they already belong to it
static int prepare_u(gpx_handle *h)
{
    const bool by_solves = !h->Kinv && h->approx_solves < approx_solve_limit();
    if (!by_solves) GPX_TRY(ensure_kinv(h));
    const double *uh = h->hstage;
    if (h->have_u && memcmp(uh, h->u, sizeof(double) * h->d) == 0) return 0;
    hipStream_t s = h->stream;
    h->have_u = false;
    GPX_TRY(launch_approx_build(h->x, h->n, h->npad, h->d, udev_ptr(h), h->wdev, h->v, handle_vt_on_equal(h), h->V, aux_ptr(h), cplain_ptr(h), s));
    if (by_solves) {
        // KV = V K^-1 row by row: K^-1 v = L^-T (L^-1 v) as two sweeps of the few-right-hand-side triangular solver
        // (tsolve.hip) that read the triangle of L once each -- no K^-1, no transposed copy of the factor
        const int nrhs = h->d + 1;
        for (int c0 = 0; c0 < nrhs; c0 += 32)
            GPX_TRY(h->tri.solve(h->V + (int64_t)c0 * h->npad, h->npad, std::min(32, nrhs - c0), nullptr, h->KV + (int64_t)c0 * h->npad, s, &h->prof));
        ++h->approx_solves;
    } else {
        // KV = V Kinv^T (= V Kinv): rows 0..d are Kinv C, Kinv J_k -- the ONE pass over Kinv shared by K2..K6
        GPX_TRY(launch_kinv_pass(h->Kinv, h->npad, h->npad, h->d + 1, h->V, h->KV, s, &h->prof));
    }
    memcpy(h->u, uh, sizeof(double) * h->d);
    h->have_u = true;
    return 0;
}

extern "C" int gpx_cjh(gpx_handle *h, const double *u, double *C, double *J, double *H)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_cjh");
    if (!u) { gpx_set_error("null u"); return GPX_ERR_BAD_ARG; }
    const int64_t n = h->n;
    const int d = h->d;
    hipStream_t s = h->stream;
    Scratch sc(s);
    double *ud = nullptr, *buf = nullptr;
    GPX_TRY(sc.take(&ud, d));
    GPX_TRY(sc.take(&buf, n * (1 + d + (int64_t)d * d)));
    GPX_HIP(hipMemcpy(ud, u, sizeof(double) * d, hipMemcpyDefault));
    double *Cd = buf, *Jd = buf + n, *Hd = Jd + n * d;
    GPX_TRY(launch_cjh(h->x, n, d, ud, h->wdev, h->v, handle_vt_on_equal(h), C ? Cd : nullptr, J ? Jd : nullptr, H ? Hd : nullptr, s));
    if (C) GPX_HIP(hipMemcpyAsync(C, Cd, sizeof(double) * n, hipMemcpyDefault, s));
    if (J) GPX_HIP(hipMemcpyAsync(J, Jd, sizeof(double) * n * d, hipMemcpyDefault, s));
    if (H) GPX_HIP(hipMemcpyAsync(H, Hd, sizeof(double) * n * d * d, hipMemcpyDefault, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

// The dot pairs of the Approx sums that the vectors k0 <= k < k1 of [C, J_1 .. J_d] carry, over the rows from row0 on.  In the order of
// the whole list -- 0 beta.C  1 beta.tr  2 C.KinvC  3 KinvC.tr (vector 0), then per k >= 1: J_k.KinvJ_k , beta.J_k -- a range of vectors
// is a run of consecutive slots: *slot0 (optional) is the slot of the first pair returned.
typedef std::vector<std::pair<const double *, const double *>> DotPairs;
static DotPairs approx_pairs(gpx_handle *h, int64_t row0, int k0, int k1, int *slot0 = nullptr)
{
    DotPairs pr;
    const double *al = h->alpha + row0, *tr = aux_ptr(h) + row0;
    if (slot0) *slot0 = k0 == 0 ? 0 : 2 + 2 * k0;
    for (int k = k0; k < k1; ++k) {
        const double *v = h->V + (int64_t)k * h->npad + row0, *kv = h->KV + (int64_t)k * h->npad + row0;
        if (k == 0) {
            pr.push_back({al, v});
            pr.push_back({al, tr});
            pr.push_back({v, kv});
            pr.push_back({kv, tr});
        } else {
            pr.push_back({v, kv});
            pr.push_back({al, v});
        }
    }
    return pr;
}

extern "C" int gpx_propagate_approx(gpx_handle *h, const double *u, const double *Sigma, double *mean, double *var,
                                    double *sigma2, double *rest)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_propagate_approx");
    if (!u || !Sigma) { gpx_set_error("null u / Sigma"); return GPX_ERR_BAD_ARG; }
    const int d = h->d;
    const int64_t np = h->npad;
    hipStream_t s = h->stream;
    GPX_TRY(stage_u_sigma(h, u, Sigma));
    GPX_TRY(prepare_u(h));
    const double *Sh = staged_sigma(h);
    double *o = staged_out(h);
    GPX_TRY(launch_trace(h->x, h->n, np, d, udev_ptr(h), h->wdev, sigma_ptr(h), cplain_ptr(h), aux_ptr(h), s));
    const DotPairs pr = approx_pairs(h, 0, 0, d + 1);
    GPX_TRY(launch_dot_pairs(pr, np, out_ptr(h), s));
    GPX_HIP(hipMemcpyAsync(o, out_ptr(h), sizeof(double) * pr.size(), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));                         // the call's one synchronisation
    const double mu = o[0] + 0.5 * o[1];                      // UncertaintyPropagation.py:397-408
    const double s2 = (h->v + h->vt) - o[2];                  // :412-433  (C(u,u) = v + vt)
    double var2 = 0.0;                                        // :435-460
    for (int k = 0; k < d; ++k) var2 += Sh[k * d + k] * (o[4 + 2 * k] - o[5 + 2 * k] * o[5 + 2 * k]);
    var2 = -var2;
    const double var3 = -o[3];                                // :464-479 with Kinv symmetric
    if (mean) *mean = mu;
    if (sigma2) *sigma2 = s2;
    if (rest) *rest = var2 + var3;
    if (var) *var = s2 + var2 + var3;
    return 0;
}

// The batched row calls on a model held as K^-1 (a pseudo-input model: no factor to solve against): the chunk's rows R are built into h->Z as
// for the solve, then Y = R K^-1 is ONE fp64 product per chunk (K^-1 symmetric, so R Kinv^T of launch_gemm_nt is it) and the row reductions
// run in their pair form on (R, Y, alpha).  Chunks are cut as row_solve_begin cuts them; an element of Y is one contraction over npad in the
// order of the k-tiles whatever tile shape the launch takes, so a row's sums do not depend on the batch.
struct PairRows {
    Scratch sc;
    int64_t chunk = 0;
    double *Y = nullptr;   // [chunk, npad]
    explicit PairRows(hipStream_t s) : sc(s) {}
};
static int pair_rows_begin(gpx_handle *h, int64_t m, PairRows &pr)
{
    if (!h->Kinv || !h->alpha) { gpx_set_error("pair rows: the handle holds no K^-1"); return GPX_ERR_STATE; }
    pr.chunk = std::min<int64_t>(round_up(m, TILE), row_solve_chunk_cap(h));
    GPX_TRY(ensure_Z(h, pr.chunk));
    return pr.sc.take(&pr.Y, pr.chunk * h->npad);
}
static int pair_rows_product(gpx_handle *h, const PairRows &pr, int64_t mp)
{
    return launch_gemm_nt(h->Z, h->npad, h->Kinv, h->npad, pr.Y, h->npad, mp, h->npad, h->npad, 1.0, 0.0, 0, h->stream, &h->prof);
}

// ---- the ONE chunk loop of the five batched row calls ------------------------------------------------------------------------------------
// What a layout's reduction leaves in the chunk's device block od and where it goes: part i is `per` doubles an input from od + off bchunk,
// copied to host + b0 per (host null: not wanted; required: the call refuses a null one).
constexpr int ROWS_OUTS = 4;
struct RowsOut { double *host; int64_t off, per; bool required; };

constexpr int GRAD_OUT_DMEAN = 2;   // the part of the GRAD outputs that may be left out

// the row reduction of a chunk's bc inputs into od: on the solved block Zs with y = L^-1 t (a factor handle), or in the pair form on
// (R = h->Z, Y, alpha) (a K^-1 handle)
static int rows_reduce(gpx_handle *h, int layout, int d, const double *Zs, const double *Y, const double *sd, int64_t sstride, int64_t bc, double *od,
                       int64_t bchunk, const RowsOut (&outs)[ROWS_OUTS])
{
    hipStream_t s = h->stream;
    const double kuu = h->v + h->vt;
    if (layout == GPX_ROWS_DVH)   // dvh [bchunk, d] | sigma2 [bchunk]
        return launch_dvh_reduce_many(Zs, h->npad, d, h->y, bc, kuu, od, od + bchunk * d, s, &h->prof);
    if (layout == GPX_ROWS_APPROX) {   // mean | var | sigma2 | rest, [bchunk] each
        if (Y) return launch_approx_reduce_many_pair(h->Z, Y, h->npad, d, h->alpha, sd, sstride, bc, kuu, od, bchunk, s, &h->prof);
        return launch_approx_reduce_many(Zs, h->npad, d, h->y, sd, sstride, bc, kuu, od, bchunk, s, &h->prof);
    }
    double *vd = od + bchunk, *dmd = outs[GRAD_OUT_DMEAN].host ? vd + bchunk : nullptr, *dvd = vd + bchunk + bchunk * d;   // mean | var | dmean [, d] | dvar [, d]
    if (Y) return launch_grad_reduce_many_pair(h->Z, Y, h->npad, d, h->alpha, bc, kuu, od, vd, dmd, dvd, s, &h->prof);
    return launch_grad_reduce_many(Zs, h->npad, d, h->y, bc, kuu, od, vd, dmd, dvd, s, &h->prof);
}

// b inputs as b rows_per_input(layout, d) right-hand sides: per chunk stage U (and Sigma: APPROX alone), build, solve (a factor handle) or
// multiply by K^-1 (h->no_factor), reduce, copy out; one synchronisation per chunk, an input never straddles two chunks.  Scratch goes back
// with the RowSolve / PairRows on every path.
static int rows_many_run(gpx_handle *h, int layout, int d, const double *U, const double *Sigma, int sigma_shared, int64_t b,
                         const RowsOut (&outs)[ROWS_OUTS], const char *what, const RowsBuild &build)
{
    const bool approx = layout == GPX_ROWS_APPROX, pair = h->no_factor;
    bool missing = !U || (approx && !Sigma);
    int64_t nout = 0;
    for (const RowsOut &o : outs) {
        missing = missing || (o.required && !o.host);
        nout = std::max(nout, o.off + o.per);
    }
    if (b < 0 || (b > 0 && missing)) { gpx_set_error("%s: bad arguments", what); return GPX_ERR_BAD_ARG; }
    if (b == 0) return 0;
    assert(!(pair && layout == GPX_ROWS_DVH));   // no pair form of the DVH reduction: its entry points refuse such a handle (CHECK_H)
    hipStream_t s = h->stream;
    const int nrow = rows_per_input(layout, d);
    RowSolve rs(s);
    PairRows pr(s);
    if (pair) GPX_TRY(pair_rows_begin(h, b * nrow, pr));
    else GPX_TRY(row_solve_begin(h, b * nrow, rs));
    Scratch &sc = pair ? pr.sc : rs.sc;
    const int64_t chunk = pair ? pr.chunk : rs.chunk, bchunk = chunk / nrow;   // inputs per chunk
    if (bchunk < 1) { gpx_set_error("%s: a chunk of %ld rows holds no input of %d rows", what, (long)chunk, nrow); return GPX_ERR_STATE; }
    const int64_t d2 = (int64_t)d * d, sstride = sigma_shared ? 0 : d2;
    double *ud = nullptr, *sd = nullptr, *od = nullptr;
    GPX_TRY(sc.take(&ud, bchunk * d));
    if (approx) GPX_TRY(sc.take(&sd, (sigma_shared ? 1 : bchunk) * d2));
    GPX_TRY(sc.take(&od, nout * bchunk));
    if (approx && sigma_shared) GPX_HIP(hipMemcpyAsync(sd, Sigma, sizeof(double) * d2, hipMemcpyDefault, s));
    for (int64_t b0 = 0; b0 < b; b0 += bchunk) {
        const int64_t bc = std::min<int64_t>(bchunk, b - b0), mc = bc * nrow, mp = round_up(mc, TILE);
        GPX_HIP(hipMemcpyAsync(ud, U + b0 * d, sizeof(double) * bc * d, hipMemcpyDefault, s));
        if (approx && !sigma_shared) GPX_HIP(hipMemcpyAsync(sd, Sigma + b0 * d2, sizeof(double) * bc * d2, hipMemcpyDefault, s));
        GPX_TRY(build(ud, sd, sstride, bc, mp));
        if (pair) GPX_TRY(pair_rows_product(h, pr, mp));
        else GPX_TRY(row_solve_run(h, rs, mc, mp, nullptr));
        GPX_TRY(rows_reduce(h, layout, d, rs.Zs, pair ? pr.Y : nullptr, sd, sstride, bc, od, bchunk, outs));
        for (const RowsOut &o : outs)
            if (o.host) GPX_HIP(hipMemcpyAsync(o.host + b0 * o.per, od + o.off * bchunk, sizeof(double) * bc * o.per, hipMemcpyDefault, s));
        GPX_HIP(hipStreamSynchronize(s));             // the chunk's one synchronisation
    }
    return 0;
}

// Batched Approx: b inputs as b (d + 2) right-hand sides [C, tr, J_1..J_d] of the many-right-hand-side solver that serves gpx_predict.  With
// K = L L^T, y = L^-1 t and z_v = L^-1 v every sum of gpx_propagate_approx is a row product of the solved block: beta.v = z_v.y,
// v.Kinv v = |z_v|^2, tr.Kinv C = z_tr.z_C.  No K^-1, no use of the handle's single-u cache.
int approx_many_run(gpx_handle *h, int d, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *mean, double *var, double *sigma2,
                    double *rest, const char *what, const RowsBuild &build)
{
    const RowsOut outs[ROWS_OUTS] = {{mean, 0, 1, true}, {var, 1, 1, true}, {sigma2, 2, 1, false}, {rest, 3, 1, false}};
    return rows_many_run(h, GPX_ROWS_APPROX, d, U, Sigma, sigma_shared, b, outs, what, build);
}

extern "C" int gpx_propagate_approx_many(gpx_handle *h, const double *U, const double *Sigma, int sigma_shared, int64_t b,
                                         double *mean, double *var, double *sigma2, double *rest)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_propagate_approx_many");
    return approx_many_run(h, h->d, U, Sigma, sigma_shared, b, mean, var, sigma2, rest, "gpx_propagate_approx_many", rows_build_of(h, GPX_ROWS_APPROX));
}

// Row-sharded form of the Approx propagation (last row): the 4 + 2 d sums of gpx_propagate_approx restricted to
// the rows [row0, row1) of K^-1 -- (K^-1 v)_i needs row i of K^-1 only, and every quadratic form is a sum over i.  The
// caller adds the partials of all row panels (one all-reduce of 4 + 2 d doubles across the ranks) and finishes with
// skgpuppy_amd.distributed.combine_approx_partials.  partial_out: 0 beta.C  1 beta.tr  2 C.KinvC  3 KinvC.tr, then per k:
// J_k.KinvJ_k, beta.J_k.  row0 must be a multiple of 128; row1 a multiple of 128 or n.
extern "C" int gpx_propagate_approx_rows(gpx_handle *h, const double *u, const double *Sigma, int64_t row0, int64_t row1,
                                         double *partial_out)
{
    CHECK_H(h);
    NEED_KERNEL(h, "gpx_propagate_approx_rows");
    if (!u || !Sigma || !partial_out) { gpx_set_error("gpx_propagate_approx_rows: null argument"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(check_row_range(h, row0, row1, "gpx_propagate_approx_rows"));
    const int d = h->d;
    const int64_t np = h->npad;
    hipStream_t s = h->stream;
    const double *kbase = nullptr;
    if (row1 > row0) GPX_TRY(ensure_kinv_rows(h, row0, round_up(row1, TILE), &kbase));
    h->have_u = false;   // KV is about to hold a row panel only
    GPX_TRY(stage_u_sigma(h, u, Sigma));
    GPX_TRY(launch_approx_build(h->x, h->n, np, d, udev_ptr(h), h->wdev, h->v, handle_vt_on_equal(h), h->V, aux_ptr(h), cplain_ptr(h), s));
    double *tr = aux_ptr(h);
    GPX_TRY(launch_trace(h->x, h->n, np, d, udev_ptr(h), h->wdev, sigma_ptr(h), cplain_ptr(h), tr, s));
    const int64_t r1p = round_up(row1, TILE), len = row1 > row0 ? r1p - row0 : 0;   // rows past n are padding: V and tr are zero there
    const int npair = 4 + 2 * d;
    if (len > 0) {
        GPX_TRY(launch_kinv_pass(kbase + row0 * np, np, np, d + 1, h->V, h->KV + row0, s, &h->prof, len));
        GPX_TRY(launch_dot_pairs(approx_pairs(h, row0, 0, d + 1), len, out_ptr(h), s));
    } else GPX_HIP(hipMemsetAsync(out_ptr(h), 0, sizeof(double) * npair, s));
    double o[4 + 2 * GPX_MAX_D];
    GPX_HIP(hipMemcpyAsync(o, out_ptr(h), sizeof(double) * npair, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    GPX_HIP(hipMemcpy(partial_out, o, sizeof(double) * npair, hipMemcpyDefault));
    return 0;
}

// Right-hand-side-sharded form of the Approx propagation for the multi-GPU host: the share of the 4 + 2 d sums (same order as
// gpx_propagate_approx_rows) that the vectors k0 <= k < k1 of [C, J_1 .. J_d] contribute -- vector 0 carries beta.C, beta.tr,
// C.KinvC, KinvC.tr; vector k >= 1 carries J_k.KinvJ_k and beta.J_k -- with K^-1 v through the two-sweep triangular solver on the
// rank's copy of the factor.  No K^-1 is ever materialised (34 GB per rank at N = 65536); the other entries come back zero, the
// ranks add their vectors in one all-reduce.  (The sweeps are bound by the bytes of the factor, not by the number of vectors:
// the split saves memory, not time.)
extern "C" int gpx_propagate_approx_rhs(gpx_handle *h, const double *u, const double *Sigma, int k0, int k1, double *partial_out)
{
    CHECK_H(h);
    NEED_KERNEL(h, "gpx_propagate_approx_rhs");
    if (!u || !Sigma || !partial_out || k0 < 0 || k1 < k0 || k1 > h->d + 1) {
        gpx_set_error("gpx_propagate_approx_rhs: bad arguments (vectors [%d, %d) of %d)", k0, k1, h->d + 1);
        return GPX_ERR_BAD_ARG;
    }
    const int d = h->d;
    const int64_t np = h->npad;
    hipStream_t s = h->stream;
    h->have_u = false;   // KV is about to hold some rows only
    GPX_TRY(stage_u_sigma(h, u, Sigma));
    const int npair = 4 + 2 * d;
    double o[4 + 2 * GPX_MAX_D];
    for (int i = 0; i < npair; ++i) o[i] = 0.0;
    if (k1 > k0) {
        GPX_TRY(launch_approx_build(h->x, h->n, np, d, udev_ptr(h), h->wdev, h->v, handle_vt_on_equal(h), h->V, aux_ptr(h), cplain_ptr(h), s));
        double *tr = aux_ptr(h);
        GPX_TRY(launch_trace(h->x, h->n, np, d, udev_ptr(h), h->wdev, sigma_ptr(h), cplain_ptr(h), tr, s));
        for (int c0 = k0; c0 < k1; c0 += 32)
            GPX_TRY(h->tri.solve(h->V + (int64_t)c0 * np, np, std::min(32, k1 - c0), nullptr, h->KV + (int64_t)c0 * np, s, &h->prof));
        int slot0 = 0;
        const DotPairs pr = approx_pairs(h, 0, k0, k1, &slot0);
        GPX_TRY(launch_dot_pairs(pr, np, out_ptr(h), s));
        double tmp[4 + 2 * GPX_MAX_D];
        GPX_HIP(hipMemcpyAsync(tmp, out_ptr(h), sizeof(double) * pr.size(), hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i < pr.size(); ++i) o[slot0 + i] = tmp[i];
    }
    GPX_HIP(hipMemcpy(partial_out, o, sizeof(double) * npair, hipMemcpyDefault));
    return 0;
}

extern "C" int gpx_propagate_dvh(gpx_handle *h, const double *u, double *dvh_out)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_propagate_dvh");
    if (!u || !dvh_out) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    const int d = h->d;
    const int64_t np = h->npad;
    hipStream_t s = h->stream;
    GPX_TRY(stage_u_sigma(h, u, nullptr));
    GPX_TRY(prepare_u(h));
    DotPairs pr;
    for (int k = 0; k < d; ++k) {
        pr.push_back({h->V + (int64_t)(k + 1) * np, h->KV + (int64_t)(k + 1) * np});   // J_k Kinv J_k
        pr.push_back({h->alpha, h->V + (int64_t)(k + 1) * np});                        // beta . J_k
        pr.push_back({h->KV, aux_ptr(h) + (int64_t)(k + 1) * np});                     // (Kinv C) . H_kk
    }
    GPX_TRY(launch_dot_pairs(pr, np, out_ptr(h), s));
    double o[3 * GPX_MAX_D];
    GPX_HIP(hipMemcpyAsync(o, out_ptr(h), sizeof(double) * pr.size(), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    double res[GPX_MAX_D];
    for (int k = 0; k < d; ++k) {
        const double v2 = -(o[3 * k] - o[3 * k + 1] * o[3 * k + 1]);   // UncertaintyPropagation.py:593-607
        const double v3 = -o[3 * k + 2];                               // :614-627
        res[k] = v2 + v3;
    }
    GPX_HIP(hipMemcpy(dvh_out, res, sizeof(double) * d, hipMemcpyDefault));
    return 0;
}

// Batched inverse propagation: b inputs as b (2 d + 1) right-hand sides [C, J_1..J_d, H_11..H_dd] of the many-right-hand-side solver, the
// loop of gpx_propagate_approx_many.  With y = L^-1 t and z_v = L^-1 v the three sums of gpx_propagate_dvh are row products of the solved
// block: J_k.Kinv J_k = |z_Jk|^2, beta.J_k = z_Jk.y, (Kinv C).H_kk = z_C.z_Hkk; sigma2 = (v + vt) - |z_C|^2.  No K^-1, no use of the handle's
// single-u cache (have_u, V, KV).
int dvh_many_run(gpx_handle *h, int d, const double *U, int64_t b, double *dvh_out, double *sigma2_out, const char *what, const RowsBuild &build)
{
    const RowsOut outs[ROWS_OUTS] = {{dvh_out, 0, d, true}, {sigma2_out, d, 1, false}, {nullptr, 0, 0, false}, {nullptr, 0, 0, false}};
    return rows_many_run(h, GPX_ROWS_DVH, d, U, nullptr, 0, b, outs, what, build);
}

extern "C" int gpx_propagate_dvh_many(gpx_handle *h, const double *U, int64_t b, double *dvh_out, double *sigma2_out)
{
    CHECK_H(h);
    NEED_KERNEL(h, "gpx_propagate_dvh_many");
    return dvh_many_run(h, h->d, U, b, dvh_out, sigma2_out, "gpx_propagate_dvh_many", rows_build_of(h, GPX_ROWS_DVH));
}

// ---- the predictor's input gradients (kernels: predict_grad.hip) -----------------------------------------------------------------------
// b queries as b (d + 1) right-hand sides [C, J_1..J_d] of the many-right-hand-side solver, the loop of gpx_propagate_approx_many with one row
// fewer: mean = z_C.y, var = (v + vt) - |z_C|^2, dmean_k = -z_Jk.y, dvar_k = 2 z_C.z_Jk.
int grad_many_run(gpx_handle *h, int d, const double *U, int64_t b, double *mean, double *var, double *dmean, double *dvar, const char *what,
                  const RowsBuild &build)
{
    const RowsOut outs[ROWS_OUTS] = {{mean, 0, 1, true}, {var, 1, 1, true}, {dmean, 2, d, false}, {dvar, 2 + d, d, true}};
    return rows_many_run(h, GPX_ROWS_GRAD, d, U, nullptr, 0, b, outs, what, build);
}

// The value differentiated is the handle's own predictor.  gpx_matern_predict's cross-covariance rows carry +vt where a query equals a training
// row elementwise (handle_gram_has_vt), gpx_predict's on a Gaussian handle do not (GaussianCovariance.cov_matrix_ij is the vectorised Gram
// without it, Covariance.py:466-483): the C row of a Gaussian handle is therefore built with vt = 0 here, so that mean and variance are
// gpx_predict's at every query.  No derivative carries the term on either kind.
static inline double grad_row_vt(const gpx_handle *h) { return handle_gram_has_vt(h) ? h->raw->vt : 0.0; }

// the kinds that have a closed-form input gradient: gpx_fit (Gaussian) and gpx_matern_fit (either nu) handles
static int need_grad_kernel(const gpx_handle *h, const char *what)
{
    if (h->kind == KernelKind::Gaussian || h->kind == KernelKind::Matern) return 0;
    if (h->kind == KernelKind::Periodic)
        gpx_set_error("%s: the handle holds a PeriodicCovariance model (gpx_periodic_fit): no closed-form input gradient of that kernel is built", what);
    else
        gpx_set_error("%s: the handle was built from a supplied matrix (gpx_fit_matrix): no inputs / theta to differentiate the kernel on", what);
    return GPX_ERR_STATE;
}

extern "C" int gpx_predict_mean_grad(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *dmean_out)
{
    CHECK_H_PSEUDO_OK(h);
    if (m < 0 || (m > 0 && (!xs || (!mean_out && !dmean_out)))) { gpx_set_error("gpx_predict_mean_grad: bad arguments"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(need_grad_kernel(h, "gpx_predict_mean_grad"));
    if (m == 0) return 0;
    const bool matern = h->kind == KernelKind::Matern;
    const MaternData *md = matern ? handle_matern(h) : nullptr;
    const int d = handle_dim(h);
    const int S = predict_mean_grad_splits(m, h->npad);
    hipStream_t s = h->stream;
    Scratch sc(s);
    double *ud = nullptr, *part = nullptr, *od = nullptr;
    GPX_TRY(sc.take(&ud, m * d));
    GPX_TRY(sc.take(&part, (int64_t)S * m * (1 + d)));
    GPX_TRY(sc.take(&od, m * (1 + d)));
    double *dmd = od + m;
    GPX_HIP(hipMemcpyAsync(ud, xs, sizeof(double) * m * d, hipMemcpyDefault, s));
    GPX_TRY(launch_predict_mean_grad(matern ? md->x : h->x, h->n, h->npad, d, matern ? md->nu2 : 0, ud, m, matern ? md->par : h->wdev, h->alpha,
                                     matern ? md->v : h->v, grad_row_vt(h), S, part, mean_out ? od : nullptr, dmean_out ? dmd : nullptr, s,
                                     &h->prof));
    if (mean_out) GPX_HIP(hipMemcpyAsync(mean_out, od, sizeof(double) * m, hipMemcpyDefault, s));
    if (dmean_out) GPX_HIP(hipMemcpyAsync(dmean_out, dmd, sizeof(double) * m * d, hipMemcpyDefault, s));
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_predict_mean_grad: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    return 0;
}

extern "C" int gpx_predict_grad(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *var_out, double *dmean_out, double *dvar_out)
{
    CHECK_H_PSEUDO_OK(h);
    if (m < 0 || (m > 0 && (!xs || !mean_out || !var_out || !dvar_out))) { gpx_set_error("gpx_predict_grad: bad arguments"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(need_grad_kernel(h, "gpx_predict_grad"));
    return grad_many_run(h, handle_dim(h), xs, m, mean_out, var_out, dmean_out, dvar_out, "gpx_predict_grad", rows_build_of(h, GPX_ROWS_GRAD));
}

// ---- the build of every batched call, and the two stages alone (test / tool access) ----------------------------------------------------
// The lambda writes the rows of bc inputs into h->Z [mp, npad] on the handle's stream; h->Z is read when the build runs (the chunk loop
// has sized it by then).  Sigma reaches the APPROX layout alone.  A Gaussian handle builds its GRAD C row with grad_row_vt.
RowsBuild rows_build_of(gpx_handle *h, int layout)
{
    return [h, layout](const double *ud, const double *sd, int64_t sstride, int64_t bc, int64_t mp) -> int {
        const bool tr = layout == GPX_ROWS_APPROX, matern = h->kind == KernelKind::Matern;
        const MaternData *md = matern ? handle_matern(h) : nullptr;
        const double vt = matern ? md->vt : layout == GPX_ROWS_GRAD ? grad_row_vt(h) : handle_vt_on_equal(h);
        return launch_rows_build(matern ? md->nu2 : 0, layout, matern ? md->x : h->x, h->n, h->npad, matern ? md->d : h->d, ud, tr ? sd : nullptr,
                                 tr ? sstride : 0, bc, mp, matern ? md->par : h->wdev, matern ? md->v : h->v, vt, h->Z, h->stream, &h->prof);
    };
}

extern "C" int gpx_rows_build(gpx_handle *h, int layout, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *rows_out)
{
    CHECK_H(h);
    const bool approx = layout == GPX_ROWS_APPROX;
    if ((layout != GPX_ROWS_APPROX && layout != GPX_ROWS_DVH && layout != GPX_ROWS_GRAD) || b < 0 || !U || !rows_out || (approx && !Sigma)) {
        gpx_set_error("gpx_rows_build: bad arguments (layout %d, b = %ld, or a null pointer)", layout, (long)b);
        return GPX_ERR_BAD_ARG;
    }
    if (h->kind == KernelKind::Periodic || h->kind == KernelKind::Matrix) {
        gpx_set_error("gpx_rows_build: %s", h->kind == KernelKind::Periodic
                                                ? "the handle holds a PeriodicCovariance model (gpx_periodic_fit): no batched call builds rows of that kernel"
                                                : "the handle was built from a supplied matrix (gpx_fit_matrix): no inputs / theta to evaluate the kernel on");
        return GPX_ERR_STATE;
    }
    if (h->kind == KernelKind::Matern && handle_matern(h)->nu2 != 5 && layout != GPX_ROWS_GRAD) {
        gpx_set_error("gpx_rows_build: the handle holds a MaternCovariance model with nu = 3/2 (gpx_matern_fit), which has no Hessian at the origin: "
                      "GPX_ROWS_GRAD is its only layout");
        return GPX_ERR_STATE;
    }
    if (b == 0) return 0;
    const int d = handle_dim(h), nrow = rows_per_input(layout, d);
    const int64_t cap = row_solve_chunk_cap(h);
    if (b > cap / nrow) {
        gpx_set_error("gpx_rows_build: %ld inputs of %d rows are more than one chunk of %ld rows", (long)b, nrow, (long)cap);
        return GPX_ERR_BAD_ARG;
    }
    const int64_t mp = round_up(b * nrow, TILE), nsig = sigma_shared ? 1 : b, d2 = (int64_t)d * d;
    hipStream_t s = h->stream;
    GPX_TRY(ensure_Z(h, mp));
    Scratch sc(s);
    double *ud = nullptr, *sd = nullptr;
    GPX_TRY(sc.take(&ud, b * d));
    GPX_HIP(hipMemcpyAsync(ud, U, sizeof(double) * b * d, hipMemcpyDefault, s));
    if (approx) {
        GPX_TRY(sc.take(&sd, nsig * d2));
        GPX_HIP(hipMemcpyAsync(sd, Sigma, sizeof(double) * nsig * d2, hipMemcpyDefault, s));
    }
    GPX_TRY(rows_build_of(h, layout)(ud, sd, sigma_shared ? 0 : d2, b, mp));
    GPX_HIP(hipMemcpyAsync(rows_out, h->Z, sizeof(double) * mp * h->npad, hipMemcpyDefault, s));
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_rows_build: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    return 0;
}

extern "C" int gpx_rows_reduce(int layout_flags, int d, int64_t npad, const double *Zs, const double *y, const double *Sigma, int sigma_shared,
                               int64_t b, double vplusvt, double *out)
{
    const int layout = layout_flags & ~GPX_ROWS_SKIP_NULLABLE;
    const bool skip = (layout_flags & GPX_ROWS_SKIP_NULLABLE) != 0, approx = layout == GPX_ROWS_APPROX;
    if ((layout != GPX_ROWS_APPROX && layout != GPX_ROWS_DVH && layout != GPX_ROWS_GRAD) || d < 1 || d > GPX_MAX_D || npad < TILE || npad % TILE ||
        b < 0 || !Zs || !y || !out || (approx && !Sigma) || (b > 0 && npad > ((int64_t)1 << 31) / (b * rows_per_input(layout, d)))) {
        gpx_set_error("gpx_rows_reduce: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    GPX_TRY(gpx_require_device());
    if (b == 0) return 0;
    const int64_t rows = b * rows_per_input(layout, d), nsig = sigma_shared ? 1 : b, d2 = (int64_t)d * d;
    Scratch sc(nullptr);
    double *zd = nullptr, *yd = nullptr, *sd = nullptr, *od = nullptr;
    GPX_TRY(sc.take(&zd, rows * npad));
    GPX_TRY(sc.take(&yd, npad));
    GPX_HIP(hipMemcpyAsync(zd, Zs, sizeof(double) * rows * npad, hipMemcpyDefault, sc.s));
    GPX_HIP(hipMemcpyAsync(yd, y, sizeof(double) * npad, hipMemcpyDefault, sc.s));
    if (approx) {
        GPX_TRY(sc.take(&sd, nsig * d2));
        GPX_HIP(hipMemcpyAsync(sd, Sigma, sizeof(double) * nsig * d2, hipMemcpyDefault, sc.s));
        GPX_TRY(sc.take(&od, 4 * b));
        GPX_TRY(launch_approx_reduce_many(zd, npad, d, yd, sd, sigma_shared ? 0 : d2, b, vplusvt, od, b, sc.s, nullptr));
        GPX_HIP(hipMemcpyAsync(out, od, sizeof(double) * 4 * b, hipMemcpyDefault, sc.s));
    } else if (layout == GPX_ROWS_DVH) {
        GPX_TRY(sc.take(&od, b * (d + 1)));            // dvh [b, d] | sigma2 [b]
        GPX_TRY(launch_dvh_reduce_many(zd, npad, d, yd, b, vplusvt, od, skip ? nullptr : od + b * d, sc.s, nullptr));
        GPX_HIP(hipMemcpyAsync(out, od, sizeof(double) * b * (skip ? d : d + 1), hipMemcpyDefault, sc.s));
    } else {
        GPX_TRY(sc.take(&od, b * (2 + 2 * d)));        // mean [b] | var [b] | dmean [b, d] | dvar [b, d]
        double *vd = od + b, *dmd = vd + b, *dvd = dmd + b * d;
        GPX_TRY(launch_grad_reduce_many(zd, npad, d, yd, b, vplusvt, od, vd, skip ? nullptr : dmd, dvd, sc.s, nullptr));
        GPX_HIP(hipMemcpyAsync(out, od, sizeof(double) * 2 * b, hipMemcpyDefault, sc.s));
        if (!skip) GPX_HIP(hipMemcpyAsync(out + 2 * b, dmd, sizeof(double) * b * d, hipMemcpyDefault, sc.s));
        GPX_HIP(hipMemcpyAsync(out + 2 * b + b * d, dvd, sizeof(double) * b * d, hipMemcpyDefault, sc.s));
    }
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_rows_reduce: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    return 0;
}

// ---- numerical propagation (UncertaintyPropagation.py:90-162; kernels: quadrature.hip) -----------------------------------------------
// a caller's array (host or device pointer) into a block of the call's scratch, queued on its stream
static int stage_in(Scratch &sc, const double *src, int64_t count, double **dst)
{
    GPX_TRY(sc.take(dst, std::max<int64_t>(count, 1)));
    if (count > 0) GPX_HIP(hipMemcpyAsync(*dst, src, sizeof(double) * count, hipMemcpyDefault, sc.s));
    return 0;
}

static bool mixture_args_bad(const double *wq, int64_t S, int64_t b, const double *y, int64_t ny, const double *mom, const double *dens)
{
    return b < 0 || S < 1 || ny < 0 || (b > 0 && (!wq || !mom || (ny > 0 && (!y || !dens)))) || (b > 0 && S > ((int64_t)1 << 40) / b);
}

// The b S query rows U_i + A_i z_s go through the predictor's chunk loop (predict.hip, PredictRun: the chunks are cut over the ROWS, so an
// input may straddle a seam and S is not bounded by the chunk): per chunk the node kernel writes the rows straight into the query buffer,
// mu and sigma^2 land in a [2, b S] device block of the call's scratch, and the only device-to-host traffic per chunk is the status word of
// the left-looking solve.  One reduction after the last chunk; its five moment rows and the densities are the call's only results.
extern "C" int gpx_propagate_quadrature_many(gpx_handle *h, const double *U, const double *A, int a_shared, int64_t b, const double *z,
                                             const double *wq, int64_t S, const double *y, int64_t ny, int y_shared, double shift, double *mom,
                                             double *dens)
{
    CHECK_H(h);
    if (mixture_args_bad(wq, S, b, y, ny, mom, dens) || (b > 0 && (!U || !A || !z))) { gpx_set_error("gpx_propagate_quadrature_many: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (!handle_has_kernel(h)) {
        gpx_set_error("gpx_propagate_quadrature_many: the handle was built from a supplied matrix (gpx_fit_matrix): no inputs / theta to evaluate the kernel on");
        return GPX_ERR_STATE;
    }
    if (b == 0) return 0;
    hipStream_t s = h->stream;
    const int64_t rows = b * S;
    PredictRun pr(s);
    GPX_TRY(predict_run_begin(h, true, rows, pr));
    Scratch &sc = pr.rs.sc;
    const int d = handle_dim(h);
    const int64_t d2 = (int64_t)d * d;
    double *Ud = nullptr, *Ad = nullptr, *zd = nullptr, *wqd = nullptr, *yd = nullptr, *mv = nullptr, *momd = nullptr, *densd = nullptr;
    GPX_TRY(stage_in(sc, U, b * d, &Ud));
    GPX_TRY(stage_in(sc, A, (a_shared ? 1 : b) * d2, &Ad));
    GPX_TRY(stage_in(sc, z, S * d, &zd));
    GPX_TRY(stage_in(sc, wq, S, &wqd));
    GPX_TRY(stage_in(sc, y, ny > 0 ? (y_shared ? 1 : b) * ny : 0, &yd));
    GPX_TRY(sc.take(&mv, 2 * rows));
    GPX_TRY(sc.take(&momd, 5 * b));
    if (ny > 0) GPX_TRY(sc.take(&densd, b * ny));
    const int64_t chunk = pr.rs.chunk;
    for (int64_t m0 = 0; m0 < rows; m0 += chunk) {
        const int64_t mc = std::min<int64_t>(chunk, rows - m0);
        GPX_TRY(predict_run_chunk(h, pr, m0, mc,
                                  [&](int64_t, int64_t) -> int { return launch_quad_nodes(Ud, Ad, a_shared ? 0 : d2, zd, S, d, m0, mc, pr.xq, s, &h->prof); },
                                  mv + m0, mv + rows + m0, []() -> hipError_t { return hipSuccess; }));
    }
    GPX_TRY(launch_mixture_reduce(mv, mv + rows, wqd, S, b, yd, ny, y_shared ? 0 : ny, shift, momd, densd, sc, &h->prof));
    GPX_HIP(hipMemcpyAsync(mom, momd, sizeof(double) * 5 * b, hipMemcpyDefault, s));
    if (ny > 0) GPX_HIP(hipMemcpyAsync(dens, densd, sizeof(double) * b * ny, hipMemcpyDefault, s));
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_propagate_quadrature_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    return 0;
}

// the reduction alone, on any model's estimate_many output (mean WITHOUT meant, or pass shift = 0 and keep it in)
extern "C" int gpx_mixture_reduce(const double *mu, const double *var, const double *wq, int64_t S, int64_t b, const double *y, int64_t ny, int y_shared,
                                  double shift, double *mom, double *dens)
{
    if (mixture_args_bad(wq, S, b, y, ny, mom, dens) || (b > 0 && (!mu || !var))) { gpx_set_error("gpx_mixture_reduce: bad arguments"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(gpx_require_device());
    if (b == 0) return 0;
    Scratch sc(nullptr);
    double *mv = nullptr, *wqd = nullptr, *yd = nullptr, *momd = nullptr, *densd = nullptr;
    const int64_t rows = b * S;
    GPX_TRY(sc.take(&mv, 2 * rows));
    GPX_HIP(hipMemcpyAsync(mv, mu, sizeof(double) * rows, hipMemcpyDefault, sc.s));
    GPX_HIP(hipMemcpyAsync(mv + rows, var, sizeof(double) * rows, hipMemcpyDefault, sc.s));
    GPX_TRY(stage_in(sc, wq, S, &wqd));
    GPX_TRY(stage_in(sc, y, ny > 0 ? (y_shared ? 1 : b) * ny : 0, &yd));
    GPX_TRY(sc.take(&momd, 5 * b));
    if (ny > 0) GPX_TRY(sc.take(&densd, b * ny));
    GPX_TRY(launch_mixture_reduce(mv, mv + rows, wqd, S, b, yd, ny, y_shared ? 0 : ny, shift, momd, densd, sc, nullptr));
    GPX_HIP(hipMemcpyAsync(mom, momd, sizeof(double) * 5 * b, hipMemcpyDefault, sc.s));
    if (ny > 0) GPX_HIP(hipMemcpyAsync(dens, densd, sizeof(double) * b * ny, hipMemcpyDefault, sc.s));
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_mixture_reduce: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    return 0;
}

// test / tool access: the node rows alone, out [b S, d] (host or device)
extern "C" int gpx_quadrature_nodes(const double *U, const double *A, int a_shared, int64_t b, const double *z, int64_t S, int d, double *out)
{
    if (b < 0 || S < 1 || d < 1 || d > GPX_MAX_D || (b > 0 && (!U || !A || !z || !out)) || (b > 0 && S > ((int64_t)1 << 31) / ((int64_t)b * d))) {
        gpx_set_error("gpx_quadrature_nodes: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    GPX_TRY(gpx_require_device());
    if (b == 0) return 0;
    Scratch sc(nullptr);
    const int64_t rows = b * S, d2 = (int64_t)d * d;
    double *Ud = nullptr, *Ad = nullptr, *zd = nullptr, *X = nullptr;
    GPX_TRY(stage_in(sc, U, b * d, &Ud));
    GPX_TRY(stage_in(sc, A, (a_shared ? 1 : b) * d2, &Ad));
    GPX_TRY(stage_in(sc, z, S * d, &zd));
    GPX_TRY(sc.take(&X, rows * d));
    GPX_TRY(launch_quad_nodes(Ud, Ad, a_shared ? 0 : d2, zd, S, d, 0, rows, X, sc.s, nullptr));
    GPX_HIP(hipMemcpyAsync(out, X, sizeof(double) * rows * d, hipMemcpyDefault, sc.s));
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_quadrature_nodes: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    return 0;
}

// small dense inverse (Gauss-Jordan, partial pivoting) for (W/2 + Sigma), d <= 64
static int small_inverse(const double *A, int d, double *inv)
{
    std::vector<double> M((size_t)d * 2 * d);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) { M[(size_t)i * 2 * d + j] = A[i * d + j]; M[(size_t)i * 2 * d + d + j] = (i == j); }
    for (int c = 0; c < d; ++c) {
        int p = c;
        for (int r = c + 1; r < d; ++r)
            if (fabs(M[(size_t)r * 2 * d + c]) > fabs(M[(size_t)p * 2 * d + c])) p = r;
        if (M[(size_t)p * 2 * d + c] == 0.0) return -1;
        if (p != c)
            for (int j = 0; j < 2 * d; ++j) std::swap(M[(size_t)p * 2 * d + j], M[(size_t)c * 2 * d + j]);
        const double piv = M[(size_t)c * 2 * d + c];
        for (int j = 0; j < 2 * d; ++j) M[(size_t)c * 2 * d + j] /= piv;
        for (int r = 0; r < d; ++r)
            if (r != c) {
                const double f = M[(size_t)r * 2 * d + c];
                if (f != 0.0)
                    for (int j = 0; j < 2 * d; ++j) M[(size_t)r * 2 * d + j] -= f * M[(size_t)c * 2 * d + j];
            }
    }
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) inv[i * d + j] = M[(size_t)i * 2 * d + d + j];
    return 0;
}

// Girard's constants of the Exact moments (UncertaintyPropagation.py:247-257, :292-303; Winv of the reference holds w): the diagonal dd,
// the normalisers nc1 / nc2 and Ls = the symmetric part of Lambda = 2 W - (Sigma + W^-1 / 2)^-1
struct ExactConstants { std::vector<double> Ls, dd, Ai; double nc1 = 1.0, nc2 = 1.0; };   // Ai = (Sigma + W^-1 / 2)^-1, kept for the batched form
static int exact_constants(const double *w, const double *Sigma, int d, ExactConstants &c)
{
    std::vector<double> A((size_t)d * d), Ai((size_t)d * d);
    c.Ls.resize((size_t)d * d);
    c.dd.resize(d);
    double nc1 = 1.0, nc2 = 1.0;
    for (int k = 0; k < d; ++k) {
        const double wk = w[k], sk = Sigma[k * d + k];
        c.dd[k] = wk - wk / (1.0 + wk * sk);
        nc1 *= (1.0 + wk * sk);
        nc2 *= (2.0 * wk * sk + 1.0);
    }
    c.nc1 = 1.0 / sqrt(nc1);
    c.nc2 = 1.0 / sqrt(nc2);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) A[(size_t)i * d + j] = Sigma[i * d + j] + (i == j ? 0.5 / w[i] : 0.0);
    if (small_inverse(A.data(), d, Ai.data())) { gpx_set_error("W/2 + Sigma is singular"); return GPX_ERR_BAD_ARG; }
    c.Ai = Ai;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            const double lij = (i == j ? 2.0 * w[i] : 0.0) - Ai[(size_t)i * d + j];
            const double lji = (i == j ? 2.0 * w[i] : 0.0) - Ai[(size_t)j * d + i];
            c.Ls[(size_t)i * d + j] = 0.5 * (lij + lji);     // only the symmetric part enters z^T Lambda^-1 z
        }
    return 0;
}

// row0 / row1 (row1 > 0): only the rows [row0, row1) of the sums; then *mean / *var receive the PARTIAL sums  sum_i beta_i l_i
// and  sum_{i in rows, j <= i} w_ij (Kinv_ij - beta_i beta_j) L_ij / nc2,  and *nc2_out the normaliser
static int exact_common(gpx_handle *h, const double *u, const double *Sigma, bool want_var, double *mean, double *var,
                        int64_t row0 = 0, int64_t row1 = 0, double *nc2_out = nullptr)
{
    const int d = h->d;
    const int64_t np = h->npad;
    hipStream_t s = h->stream;
    const double *kbase = nullptr;
    if (want_var) {
        if (row1 > 0) GPX_TRY(ensure_kinv_rows(h, row0, round_up(row1, TILE), &kbase));   // a rank's row panel (gpx_propagate_exact_rows)
        else { GPX_TRY(ensure_kinv(h)); kbase = h->Kinv; }
    }
    GPX_TRY(stage_u_sigma(h, u, Sigma));
    ExactConstants c;
    GPX_TRY(exact_constants(h->w, staged_sigma(h), d, c));
    const double nc2 = c.nc2;
    // device scratch: aT[d][np], bT[d][np], e, F, lm, partial[np/16], consts
    Scratch sc(s);
    double *buf = nullptr;
    GPX_TRY(sc.take(&buf, (2 * (int64_t)d + 4) * np + (int64_t)d * d + d + 8));
    double *aT = buf, *bT = aT + (int64_t)d * np, *e = bT + (int64_t)d * np, *F = e + np, *lm = F + np, *partial = lm + np;
    double *Lsd = partial + np, *ddd = Lsd + (int64_t)d * d, *outd = ddd + d;
    GPX_HIP(hipMemcpyAsync(Lsd, c.Ls.data(), sizeof(double) * d * d, hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(ddd, c.dd.data(), sizeof(double) * d, hipMemcpyHostToDevice, s));
    GPX_TRY(launch_exact_build(h->x, h->n, np, d, udev_ptr(h), h->wdev, Lsd, ddd, h->v, handle_vt_on_equal(h), c.nc1, aT, bT, e, F, lm, s));
    const bool ranged = row1 > 0;
    const int64_t r0 = ranged ? row0 : 0, r1 = ranged ? round_up(row1, TILE) : np;   // rows past n are padding (l, F are zero there)
    if (r1 > r0) GPX_TRY(launch_dot_pairs({{h->alpha + r0, lm + r0}}, r1 - r0, outd, s));
    else GPX_HIP(hipMemsetAsync(outd, 0, sizeof(double) * 2, s));
    if (want_var) GPX_TRY(launch_exact_sum(kbase, np, np, d, h->alpha, aT, bT, e, F, partial, outd + 1, s, &h->prof, r0, ranged ? r1 : 0));
    double o[2] = {0, 0};
    GPX_HIP(hipMemcpyAsync(o, outd, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    const double mu = o[0];
    if (nc2_out) *nc2_out = nc2;
    if (ranged) {   // partial sums: the caller adds them over the row panels and finishes
        if (mean) *mean = o[0];
        if (var) *var = o[1];
        return 0;
    }
    if (mean) *mean = mu;
    if (want_var && var) *var = (h->v + h->vt) - nc2 * o[1] - mu * mu;   // UncertaintyPropagation.py:377
    return 0;
}

// Row-sharded Exact propagation for the multi-GPU host: partial_out = [ sum_{i in rows} beta_i l_i ,
// sum_{i in rows, j <= i} w_ij (Kinv_ij - beta_i beta_j) L_ij / nc2 , nc2 ].  After adding the first two over the row panels:
// mean = p0 (+ meant), var = v + vt - nc2 p1 - p0^2  (UncertaintyPropagation.py:377).  The j <= i triangle makes row i cost
// i + 1 pairs: shard by equal AREA (skgpuppy_amd.distributed.row_shards(..., triangular=True)).
extern "C" int gpx_propagate_exact_rows(gpx_handle *h, const double *u, const double *Sigma, int64_t row0, int64_t row1,
                                        double *partial_out)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_propagate_exact_rows");
    if (!u || !Sigma || !partial_out) { gpx_set_error("gpx_propagate_exact_rows: null argument"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(check_row_range(h, row0, row1, "gpx_propagate_exact_rows"));
    double p[3] = {0.0, 0.0, 0.0};
    if (row1 > row0) GPX_TRY(exact_common(h, u, Sigma, true, &p[0], &p[1], row0, row1, &p[2]));
    else GPX_TRY(exact_common(h, u, Sigma, false, nullptr, nullptr, 0, 0, &p[2]));   // empty panel: the normaliser only
    if (row1 <= row0) { p[0] = 0.0; p[1] = 0.0; }
    GPX_HIP(hipMemcpy(partial_out, p, sizeof(double) * 3, hipMemcpyDefault));
    return 0;
}

extern "C" int gpx_propagate_exact(gpx_handle *h, const double *u, const double *Sigma, double *mean, double *var)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_propagate_exact");
    if (!u || !Sigma) { gpx_set_error("null u / Sigma"); return GPX_ERR_BAD_ARG; }
    return exact_common(h, u, Sigma, true, mean, var);
}

extern "C" int gpx_exact_mean(gpx_handle *h, const double *u, const double *Sigma, double *mean)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_exact_mean");
    if (!u || !Sigma || !mean) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    return exact_common(h, u, Sigma, false, mean, nullptr);
}

// Batched Exact: with per-input Sigma the batch is cut into runs of consecutive inputs whose Sigma are bit-equal (one shared Sigma: one
// run, always on the matrix path).  A run of at least MIN_RUN inputs takes
// the matrix path -- Lo = the weighted lower half of K^-1 built once (exact_weight_kernel), then per slab of inputs H, Y = H Lo^T on the
// fp64 GEMM with a triangular B, and the row products (propagate.hip) --, a shorter one the arithmetic of gpx_propagate_exact, input
// by input, queued without a host synchronisation into device result slots.  Every Sigma's constants are formed, and a singular
// W/2 + Sigma refused, before the first launch; they travel to the device in ONE block that the host keeps until the call's one
// synchronisation.  The staged u / Sigma and the cached u of the single-input calls are not touched.
// MIN_RUN = 5: the smallest run from which the matrix path (one weight pass + one 128-row product, 1.31-1.37 ms at N = 16384, d = 8 whatever
// the run) stays faster than the pair path (0.31 ms per input), measured at N = 2048 and N = 16384 (profiles/r14_exact_many.txt).
static int64_t env_count(const char *name, int64_t dflt)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    return end == e ? dflt : (int64_t)v;
}

extern "C" int gpx_propagate_exact_many(gpx_handle *h, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *mean,
                                        double *var)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_propagate_exact_many");
    if (b < 0 || (b > 0 && (!U || !Sigma || !mean))) { gpx_set_error("gpx_propagate_exact_many: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (b == 0) return 0;
    const int d = h->d;
    const int64_t n = h->n, np = h->npad, d2 = (int64_t)d * d;
    const bool want_var = var != nullptr;
    hipStream_t s = h->stream;
    const int64_t min_run = std::max<int64_t>(1, env_count("GPX_EXACT_MANY_MIN_RUN", 5));
    int64_t slab = env_count("GPX_EXACT_MANY_SLAB", 4096);
    if (slab < TILE || slab % TILE || slab > (1 << 19)) slab = 4096;

    // runs of bit-equal Sigma and their constants, on the host: [Ls d^2 | dd d] and, for a matrix run with variances,
    // [T of Ls / 8 d^2 | its signs d | T of A^-1 / 4 d^2 | its signs d]
    struct Run { int64_t i0, cnt; int64_t off; bool matrix; double nc1, nc2; };
    std::vector<Run> runs;
    std::vector<double> Sh, arena, res;
    int64_t max_matrix = 0;
    bool any_pair = false;
    try {
        Sh.resize((size_t)((sigma_shared ? 1 : b) * d2));
        res.resize((size_t)(2 * b));
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_propagate_exact_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_TRY(fetch_small(Sh.data(), Sigma, Sh.size()));
    for (int64_t i = 0; i < b;) {
        int64_t j = sigma_shared ? b : i + 1;
        while (j < b && memcmp(&Sh[(size_t)(i * d2)], &Sh[(size_t)(j * d2)], sizeof(double) * d2) == 0) ++j;
        runs.push_back({i, j - i, 0, sigma_shared != 0 || j - i >= min_run, 1.0, 1.0});   // one shared Sigma: the matrix path whatever b
        i = j;
    }
    try {
        for (Run &r : runs) {
            const double *Sg = &Sh[(size_t)(sigma_shared ? 0 : r.i0 * d2)];
            ExactConstants c;
            GPX_TRY(exact_constants(h->w, Sg, d, c));
            r.nc1 = c.nc1;
            r.nc2 = c.nc2;
            r.off = (int64_t)arena.size();
            arena.insert(arena.end(), c.Ls.begin(), c.Ls.end());
            arena.insert(arena.end(), c.dd.begin(), c.dd.end());
            if (r.matrix) max_matrix = std::max(max_matrix, r.cnt);
            else any_pair = true;
            if (r.matrix && want_var) {
                const size_t at = arena.size();
                arena.resize(at + 2 * (size_t)(d2 + d));
                sym_square_transform(c.Ls.data(), d, 0.125, &arena[at], &arena[at + d2]);
                sym_square_transform(c.Ai.data(), d, 0.25, &arena[at + d2 + d], &arena[at + 2 * d2 + d]);
            }
        }
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_propagate_exact_many: out of host memory"); return GPX_ERR_HIP; }

    if (want_var) GPX_TRY(ensure_kinv(h));
    Scratch sc(s);
    double *cd = nullptr, *Ud = nullptr, *od = nullptr;
    GPX_TRY(sc.take(&cd, (int64_t)arena.size()));
    GPX_TRY(sc.take(&Ud, b * d));
    GPX_TRY(sc.take(&od, 2 * b));
    // matrix path: slab rows of H and Y, the transformed inputs, Lo; pair path: ONE block of exact_common's per-input scratch, used by
    // the inputs of every short run in stream order
    const int64_t rows = std::min(slab, round_up(std::max<int64_t>(max_matrix, 1), TILE)), npart = np / 64;
    double *mpart = nullptr, *Hd = nullptr, *Yd = nullptr, *Lo = nullptr, *xt = nullptr, *xh = nullptr, *Uh = nullptr, *pb = nullptr;
    if (max_matrix > 0) {
        GPX_TRY(sc.take(&mpart, rows * npart));
        if (want_var) {
            GPX_TRY(sc.take(&xt, np * d));
            GPX_TRY(sc.take(&xh, np * d));
            GPX_TRY(sc.take(&Uh, rows * d));
            GPX_TRY(sc.take(&Hd, rows * np));
            GPX_TRY(sc.take(&Yd, rows * np));
            GPX_TRY(sc.take(&Lo, np * np));
        }
    }
    if (any_pair) GPX_TRY(sc.take(&pb, (2 * (int64_t)d + 4) * np));
    GPX_HIP(hipMemcpyAsync(cd, arena.data(), sizeof(double) * arena.size(), hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(Ud, U, sizeof(double) * b * d, hipMemcpyDefault, s));
    const double vpv = h->v + h->vt;
    // the means alone are N-fold work, like gpx_exact_mean's launches: outside the Exact class, which counts the N^2 passes
    Profiler *prof = want_var ? &h->prof : nullptr;
    for (const Run &r : runs) {
        const double *Lsd = cd + r.off, *ddd = Lsd + d2;
        if (!r.matrix) {
            double *aT = pb, *bT = aT + (int64_t)d * np, *e = bT + (int64_t)d * np, *F = e + np, *lm = F + np, *partial = lm + np;
            for (int64_t i = r.i0; i < r.i0 + r.cnt; ++i) {   // exact_common's launches; od[i] = beta . l, od[b + i] = the double sum / nc2
                GPX_TRY(launch_exact_build(h->x, n, np, d, Ud + i * d, h->wdev, Lsd, ddd, h->v, handle_vt_on_equal(h), r.nc1, aT, bT, e, F, lm, s));
                GPX_TRY(launch_dot_pairs({{h->alpha, lm}}, np, od + i, s));
                if (want_var) GPX_TRY(launch_exact_sum(h->Kinv, np, np, d, h->alpha, aT, bT, e, F, partial, od + b + i, s, &h->prof));
            }
            continue;
        }
        const double *T1 = ddd + d, *s1 = T1 + d2, *T2 = s1 + d, *s2 = T2 + d2;
        if (want_var) {
            GPX_TRY(launch_exact_many_transform(h->x, n, np, d, h->x, T1, xt, s));
            GPX_TRY(launch_exact_weight(h->Kinv, np, n, np, d, h->alpha, xt, s1, Lo, s, &h->prof));
            GPX_TRY(launch_exact_many_transform(h->x, n, np, d, h->x, T2, xh, s));
        }
        for (int64_t b0 = 0; b0 < r.cnt; b0 += rows) {
            const int64_t bc = std::min(rows, r.cnt - b0), bp = round_up(bc, TILE), i0 = r.i0 + b0;
            if (want_var) GPX_TRY(launch_exact_many_transform(Ud + i0 * d, bc, bc, d, h->x, T2, Uh, s));
            GPX_TRY(launch_exact_many_build(h->x, xh, n, np, d, Ud + i0 * d, Uh, bc, bp, h->wdev, ddd, s2, h->alpha, h->v, handle_vt_on_equal(h), r.nc1,
                                            want_var ? Hd : nullptr, mpart, s, prof));
            if (want_var) GPX_TRY(launch_gemm_nt(Hd, np, Lo, np, Yd, np, bp, np, np, 1.0, 0.0, 0, s, &h->prof, 0, GEMM_TRI_B_LOWER));
            GPX_TRY(launch_exact_many_finish(want_var ? Yd : nullptr, Hd, np, mpart, bc, vpv, r.nc2, od + i0, b, s, prof));
        }
    }
    GPX_HIP(hipMemcpyAsync(res.data(), od, sizeof(double) * (want_var ? 2 : 1) * b, hipMemcpyDeviceToHost, s));
    const hipError_t e = sc.wait_and_free();                  // the call's one synchronisation
    if (e != hipSuccess) { gpx_set_error("gpx_propagate_exact_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    if (want_var)
        for (const Run &r : runs)
            if (!r.matrix)
                for (int64_t i = r.i0; i < r.i0 + r.cnt; ++i) {
                    const double mu = res[(size_t)i], nc2 = r.nc2;
                    res[(size_t)(b + i)] = (h->v + h->vt) - nc2 * res[(size_t)(b + i)] - mu * mu;   // as exact_common finishes
                }
    GPX_HIP(hipMemcpy(mean, res.data(), sizeof(double) * b, hipMemcpyDefault));
    if (want_var) GPX_HIP(hipMemcpy(var, res.data() + b, sizeof(double) * b, hipMemcpyDefault));
    return 0;
}

// Batched Exact with its closed-form gradients in u and in the diagonal of Sigma (kernels and arithmetic: exact_grad.hip).  The frame of
// gpx_propagate_exact_many with three differences: every run of bit-equal Sigma takes the matrix path, a run of one included (there is no
// pair-path form of the gradient); an input is 2 d + 1 consecutive rows [h, p_1..p_d, c_1..c_d] of the product, so the slab is counted in
// product ROWS, whole inputs go into each slab and a slab setting below 2 d + 1 rows is raised to hold one input; and the finish kernel
// writes all six outputs.  Without var, dvar_du and dvar_ds the call is N-fold work per input: K^-1 is neither built nor read.
extern "C" int gpx_propagate_exact_grad_many(gpx_handle *h, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *mean,
                                             double *var, double *dmean_du, double *dvar_du, double *dmean_ds, double *dvar_ds)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_propagate_exact_grad_many");
    if (b < 0 || (b > 0 && (!U || !Sigma || (!dmean_du && !dvar_du && !dmean_ds && !dvar_ds)))) {
        gpx_set_error("gpx_propagate_exact_grad_many: bad arguments (b = %ld, a null U / Sigma, or no gradient asked for)", (long)b);
        return GPX_ERR_BAD_ARG;
    }
    if (b == 0) return 0;
    const int d = h->d, nrow = 2 * d + 1;
    const int64_t n = h->n, np = h->npad, d2 = (int64_t)d * d;
    const bool want_var = var || dvar_du || dvar_ds;
    hipStream_t s = h->stream;
    int64_t slab = env_count("GPX_EXACT_MANY_SLAB", 4096);
    if (slab < TILE || slab % TILE || slab > (1 << 19)) slab = 4096;
    slab = std::max<int64_t>(slab, round_up(nrow, TILE));
    const int64_t bslab = slab / nrow;   // whole inputs per slab

    // runs of bit-equal Sigma and their constants, on the host: [dd d | D d | w / (2 w s + 1) d] and, with variances,
    // [T of Ls / 8 d^2 | its signs d | T of A^-1 / 4 d^2 | its signs d | Bm = 4 T^T diag(signs) d^2]
    struct Run { int64_t i0, cnt, off; double nc1, nc2; };
    std::vector<Run> runs;
    std::vector<double> Sh, arena, res;
    const int64_t per = 2 + 4 * (int64_t)d;   // mean | var | four [d] blocks, per input
    int64_t max_cnt = 0;
    try {
        Sh.resize((size_t)((sigma_shared ? 1 : b) * d2));
        res.resize((size_t)(per * b));
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_propagate_exact_grad_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_TRY(fetch_small(Sh.data(), Sigma, Sh.size()));
    for (int64_t i = 0; i < b;) {
        int64_t j = sigma_shared ? b : i + 1;
        while (j < b && memcmp(&Sh[(size_t)(i * d2)], &Sh[(size_t)(j * d2)], sizeof(double) * d2) == 0) ++j;
        runs.push_back({i, j - i, 0, 1.0, 1.0});
        max_cnt = std::max(max_cnt, j - i);
        i = j;
    }
    try {
        for (Run &r : runs) {
            const double *Sg = &Sh[(size_t)(sigma_shared ? 0 : r.i0 * d2)];
            ExactConstants c;
            GPX_TRY(exact_constants(h->w, Sg, d, c));
            r.nc1 = c.nc1;
            r.nc2 = c.nc2;
            r.off = (int64_t)arena.size();
            arena.insert(arena.end(), c.dd.begin(), c.dd.end());
            for (int k = 0; k < d; ++k) arena.push_back(h->w[k] / (1.0 + h->w[k] * Sg[k * d + k]));
            for (int k = 0; k < d; ++k) arena.push_back(h->w[k] / (2.0 * h->w[k] * Sg[k * d + k] + 1.0));
            if (want_var) {
                const size_t at = arena.size();
                arena.resize(at + 3 * (size_t)d2 + 2 * (size_t)d);
                double *T2 = &arena[at + d2 + d], *s2 = T2 + d2, *Bm = s2 + d;
                sym_square_transform(c.Ls.data(), d, 0.125, &arena[at], &arena[at + d2]);
                sym_square_transform(c.Ai.data(), d, 0.25, T2, s2);
                for (int k = 0; k < d; ++k)
                    for (int m = 0; m < d; ++m) Bm[(size_t)k * d + m] = 4.0 * T2[(size_t)m * d + k] * s2[m];
            }
        }
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_propagate_exact_grad_many: out of host memory"); return GPX_ERR_HIP; }

    if (want_var) GPX_TRY(ensure_kinv(h));
    Scratch sc(s);
    double *cd = nullptr, *Ud = nullptr, *od = nullptr;
    GPX_TRY(sc.take(&cd, (int64_t)arena.size()));
    GPX_TRY(sc.take(&Ud, b * d));
    GPX_TRY(sc.take(&od, per * b));
    const int64_t bmax = std::min(bslab, max_cnt), rows = round_up(bmax * nrow, TILE), npart = np / 64;
    double *mpart = nullptr, *Hd = nullptr, *Yd = nullptr, *Lo = nullptr, *xt = nullptr, *xh = nullptr, *Uh = nullptr;
    GPX_TRY(sc.take(&mpart, bmax * nrow * npart));
    if (want_var) {
        GPX_TRY(sc.take(&xt, np * d));
        GPX_TRY(sc.take(&xh, np * d));
        GPX_TRY(sc.take(&Uh, bmax * d));
        GPX_TRY(sc.take(&Hd, rows * np));
        GPX_TRY(sc.take(&Yd, rows * np));
        GPX_TRY(sc.take(&Lo, np * np));
    }
    GPX_HIP(hipMemcpyAsync(cd, arena.data(), sizeof(double) * arena.size(), hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(Ud, U, sizeof(double) * b * d, hipMemcpyDefault, s));
    const double vpv = h->v + h->vt;
    Profiler *prof = want_var ? &h->prof : nullptr;   // the mean sums alone are N-fold work: outside the Exact class, as in gpx_propagate_exact_many
    for (const Run &r : runs) {
        const double *ddd = cd + r.off, *Dkd = ddd + d, *nqd = Dkd + d, *T1 = nqd + d, *s1 = T1 + d2, *T2 = s1 + d, *s2 = T2 + d2, *Bmd = s2 + d;
        if (want_var) {
            GPX_TRY(launch_exact_many_transform(h->x, n, np, d, h->x, T1, xt, s));
            GPX_TRY(launch_exact_weight(h->Kinv, np, n, np, d, h->alpha, xt, s1, Lo, s, &h->prof));
            GPX_TRY(launch_exact_many_transform(h->x, n, np, d, h->x, T2, xh, s));
        }
        for (int64_t b0 = 0; b0 < r.cnt; b0 += bmax) {
            const int64_t bc = std::min(bmax, r.cnt - b0), rp = round_up(bc * nrow, TILE), i0 = r.i0 + b0;
            if (want_var) GPX_TRY(launch_exact_many_transform(Ud + i0 * d, bc, bc, d, h->x, T2, Uh, s));
            GPX_TRY(launch_exact_grad_build(h->x, xh, n, np, d, Ud + i0 * d, Uh, bc, rp, h->wdev, ddd, Dkd, s2, Bmd, h->alpha, h->v, handle_vt_on_equal(h),
                                            r.nc1, want_var ? Hd : nullptr, mpart, s, prof));
            if (want_var) GPX_TRY(launch_gemm_nt(Hd, np, Lo, np, Yd, np, rp, np, np, 1.0, 0.0, 0, s, &h->prof, 0, GEMM_TRI_B_LOWER));
            // the finish kernel indexes its output blocks by the input's place in the whole batch: od + i0 with blocks b inputs long
            GPX_TRY(launch_exact_grad_finish(want_var ? Yd : nullptr, Hd, np, d, mpart, bc, vpv, r.nc2, nqd, od, b, i0, s, prof));
        }
    }
    GPX_HIP(hipMemcpyAsync(res.data(), od, sizeof(double) * per * b, hipMemcpyDeviceToHost, s));
    const hipError_t e = sc.wait_and_free();                  // the call's one synchronisation
    if (e != hipSuccess) { gpx_set_error("gpx_propagate_exact_grad_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    const double *rm = res.data(), *rv = rm + b, *rmu = rv + b, *rvu = rmu + b * d, *rms = rvu + b * d, *rvs = rms + b * d;
    if (mean) GPX_HIP(hipMemcpy(mean, rm, sizeof(double) * b, hipMemcpyDefault));
    if (var) GPX_HIP(hipMemcpy(var, rv, sizeof(double) * b, hipMemcpyDefault));
    if (dmean_du) GPX_HIP(hipMemcpy(dmean_du, rmu, sizeof(double) * b * d, hipMemcpyDefault));
    if (dvar_du) GPX_HIP(hipMemcpy(dvar_du, rvu, sizeof(double) * b * d, hipMemcpyDefault));
    if (dmean_ds) GPX_HIP(hipMemcpy(dmean_ds, rms, sizeof(double) * b * d, hipMemcpyDefault));
    if (dvar_ds) GPX_HIP(hipMemcpy(dvar_ds, rvs, sizeof(double) * b * d, hipMemcpyDefault));
    return 0;
}

// ---- a14 for ANY operator.  The reference's UncertaintyPropagationExact talks to the GP only through _get_beta, _get_W_inv,
// _inv_cov_matrix, _covariance and x (skgpuppy/UncertaintyPropagation.py:269-290, :323-379): with a Covariance subclass of its own
// cov_matrix_ij / __call__ it runs and returns numbers -- Girard's correction factors built from theta[2:2+d], applied to the
// operator's own C(u, x_i).  Here: C_ux [n] and cuu = cov(u, u) from the caller (the operator's scalar kernel on the host, N calls as in
// the reference), x [n, d] and w [d] (the diagonal of _get_W_inv) handle-free, K^-1 and beta from the handle (gpx_fit_matrix or
// gpx_fit) -- or, with h == NULL, explicit Kinv [n, n] and beta [n] (the reference's Kinv attribute, e.g. of an SPGP model); the
// N and N^2 sums run in the kernels of the built-in path.  mean WITHOUT meant.
// lower triangle <- mean of both triangles, padding (rows / columns >= n of the [np, ld] buffer) <- 0, in place: row i's workgroup
// reads A[j][i], j < i, which no other workgroup writes (those write columns below THEIR row index only)
__global__ __launch_bounds__(256) void mean_lower_pad_kernel(double *A, long ld, long n, long np)
{
    const long i = blockIdx.x;
    if (i >= n) {
        for (long j = threadIdx.x; j < np; j += 256) A[i * ld + j] = 0.0;
        return;
    }
    for (long j = threadIdx.x; j < i; j += 256) A[i * ld + j] = 0.5 * (A[i * ld + j] + A[j * ld + i]);
    for (long j = n + threadIdx.x; j < np; j += 256) A[i * ld + j] = 0.0;
}

// An explicit K^-1 / beta kept on the device across calls (gpx_kinv_model_*): uploaded, padded to the tile grid and symmetrised ONCE.
// Uncertainty propagation is typically called many times on one model; without this every call of the h == NULL form moved N^2 doubles
// over PCIe again.
struct gpx_kinv_model {
    int device = 0;
    int64_t n = 0, np = 0;
    double *Kp = nullptr;     // [np, np]: lower triangle = mean of both triangles of the supplied matrix, zero padding
    double *bpad = nullptr;   // [np]: beta, zero padded
};

// device copies of an explicit K^-1 (optional) and beta, queued on the stream of the caller's scratch
static int upload_explicit(const double *Kinv, const double *beta, int64_t n, int64_t np, bool want_kinv, Scratch &sc, double **Kp, double **bpad)
{
    hipStream_t s = sc.s;
    *Kp = nullptr;
    GPX_TRY(sc.take(bpad, np));
    GPX_HIP(hipMemsetAsync(*bpad, 0, sizeof(double) * np, s));
    GPX_HIP(hipMemcpyAsync(*bpad, beta, sizeof(double) * n, hipMemcpyDefault, s));
    if (want_kinv) {
        // K^-1 goes row by row straight into ONE buffer padded to the tile grid (the padding never enters: F = 0 there).  The pair kernel
        // visits j <= i only (weight 2) where the reference sums both triangles: the lower triangle of a supplied K^-1 becomes the mean of
        // both (a Woodbury-built inverse is symmetric to rounding only).
        GPX_TRY(sc.take(Kp, np * np));
        GPX_HIP(hipMemcpy2DAsync(*Kp, sizeof(double) * np, Kinv, sizeof(double) * n, sizeof(double) * n, n, hipMemcpyDefault, s));
        hipLaunchKernelGGL(mean_lower_pad_kernel, dim3((unsigned)np), dim3(256), 0, s, *Kp, (long)np, (long)n, (long)np);
        GPX_HIP(hipGetLastError());
    }
    return 0;
}

// Girard's exact moments from device-resident K^-1 (kbase [np, np], null: mean only) and beta (bdev [np]); everything else from the caller
static int exact_matrix_core(hipStream_t s, Profiler *prof, const double *kbase, const double *bdev, const double *x, int64_t n, int d, const double *w,
                             const double *C_ux, const double *u, const double *Sigma, double cuu, double *mean, double *var)
{
    for (int k = 0; k < d; ++k)
        if (!(w[k] > 0.0) || !isfinite(w[k])) { gpx_set_error("gpx_propagate_exact_matrix: w[%d]=%g", k, w[k]); return GPX_ERR_BAD_ARG; }
    const int64_t np = round_up(n, TILE);
    const bool want_var = var != nullptr && kbase != nullptr;
    ExactConstants c;
    GPX_TRY(exact_constants(w, Sigma, d, c));
    Scratch sc(s);
    double *buf = nullptr;
    GPX_TRY(sc.take(&buf, (2 * (int64_t)d + 6) * np + n * (int64_t)d + (int64_t)d * d + 2 * d + 8));
    double *aT = buf, *bT = aT + (int64_t)d * np, *e = bT + (int64_t)d * np, *F = e + np, *lm = F + np, *partial = lm + np;
    double *Cd = partial + np, *xd = Cd + np, *Lsd = xd + n * (int64_t)d, *ddd = Lsd + (int64_t)d * d, *ud = ddd + d, *outd = ud + d;
    double o[2] = {0, 0};
    GPX_HIP(hipMemcpyAsync(Lsd, c.Ls.data(), sizeof(double) * d * d, hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(ddd, c.dd.data(), sizeof(double) * d, hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(ud, u, sizeof(double) * d, hipMemcpyDefault, s));
    GPX_HIP(hipMemcpyAsync(xd, x, sizeof(double) * n * d, hipMemcpyDefault, s));
    GPX_HIP(hipMemcpyAsync(Cd, C_ux, sizeof(double) * n, hipMemcpyDefault, s));
    GPX_TRY(launch_exact_build_generic(xd, n, np, d, ud, Lsd, ddd, Cd, c.nc1, aT, bT, e, F, lm, s));
    GPX_TRY(launch_dot_pairs({{bdev, lm}}, np, outd, s));
    if (want_var) GPX_TRY(launch_exact_sum(kbase, np, np, d, bdev, aT, bT, e, F, partial, outd + 1, s, prof));
    GPX_HIP(hipMemcpyAsync(o, outd, sizeof(double) * (want_var ? 2 : 1), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (mean) *mean = o[0];
    if (var) *var = cuu - c.nc2 * o[1] - o[0] * o[0];   // UncertaintyPropagation.py:377
    return 0;
}

extern "C" int gpx_propagate_exact_matrix(gpx_handle *h, const double *Kinv, const double *beta, const double *x, int64_t n, int d,
                                          const double *w, const double *C_ux, const double *u, const double *Sigma, double cuu,
                                          double *mean, double *var)
{
    GPX_TRY(gpx_require_device());
    if (h) CHECK_H(h);   // (a pseudo-input model is served by the fused entry points, not by this one: refused like everywhere else)
    if (!x || !w || !C_ux || !u || !Sigma || n < 1 || d < 1 || d > GPX_MAX_D || (!h && (!beta || (var && !Kinv))) || (h && h->n != n)) {
        gpx_set_error("gpx_propagate_exact_matrix: bad arguments (n=%ld d=%d%s)", (long)n, d, (h && h->n != n) ? ": the handle holds another n" : "");
        return GPX_ERR_BAD_ARG;
    }
    const bool want_var = var != nullptr;   // the mean is beta . l alone: no K^-1 (46 ms to build at C3), no N^2 pass
    if (h) {
        if (want_var) GPX_TRY(ensure_kinv(h));
        return exact_matrix_core(h->stream, &h->prof, want_var ? h->Kinv : nullptr, h->alpha, x, n, d, w, C_ux, u, Sigma, cuu, mean, var);
    }
    // explicit K^-1 / beta, one call: upload, use, free (many calls on one model: gpx_kinv_model_create + gpx_propagate_exact_model)
    const int64_t np = round_up(n, TILE);
    Scratch sc(nullptr);
    double *Kp = nullptr, *bpad = nullptr;
    GPX_TRY(upload_explicit(Kinv, beta, n, np, want_var, sc, &Kp, &bpad));
    return exact_matrix_core(nullptr, nullptr, Kp, bpad, x, n, d, w, C_ux, u, Sigma, cuu, mean, var);
}

extern "C" int gpx_kinv_model_create(const double *Kinv, const double *beta, int64_t n, gpx_kinv_model **out)
{
    if (out) *out = nullptr;
    GPX_TRY(gpx_require_device());
    if (!Kinv || !beta || !out || n < 1) { gpx_set_error("gpx_kinv_model_create: bad arguments"); return GPX_ERR_BAD_ARG; }
    int dev = 0;
    GPX_HIP(hipGetDevice(&dev));
    const int64_t np = round_up(n, TILE);
    Scratch sc(nullptr);
    double *Kp = nullptr, *bpad = nullptr;
    GPX_TRY(upload_explicit(Kinv, beta, n, np, true, sc, &Kp, &bpad));
    const hipError_t e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { gpx_set_error("gpx_kinv_model_create: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    gpx_kinv_model *m = new (std::nothrow) gpx_kinv_model();
    if (!m) { gpx_set_error("out of host memory"); return GPX_ERR_HIP; }
    m->device = dev;
    m->n = n;
    m->np = np;
    m->Kp = sc.release(Kp);
    m->bpad = sc.release(bpad);
    *out = m;
    return 0;
}

extern "C" void gpx_kinv_model_free(gpx_kinv_model *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    dfree(m->Kp);
    dfree(m->bpad);
    delete m;
}

extern "C" int gpx_propagate_exact_model(gpx_kinv_model *m, const double *x, int d, const double *w, const double *C_ux, const double *u,
                                         const double *Sigma, double cuu, double *mean, double *var)
{
    if (!m || !x || !w || !C_ux || !u || !Sigma || d < 1 || d > GPX_MAX_D) { gpx_set_error("gpx_propagate_exact_model: bad arguments"); return GPX_ERR_BAD_ARG; }
    GPX_HIP(hipSetDevice(m->device));
    return exact_matrix_core(nullptr, nullptr, m->Kp, m->bpad, x, m->n, d, w, C_ux, u, Sigma, cuu, mean, var);
}
