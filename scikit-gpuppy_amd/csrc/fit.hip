// fit.hip -- the C-ABI of libgpx (include/gpx.h), part 1: the stand-alone Gram and panel entry points, the fit (handle
// construction, factorisation, alpha), the accessors of the factor and the likelihood with its gradients.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <new>

#include "common.h"
#include "gram_tile.h"

static int parse_theta(const double *theta, int d, double *v, double *vt, double *w)
{
    if (!theta || d < 1 || d > GPX_MAX_D) {
        gpx_set_error("bad theta / d=%d (1..%d supported)", d, GPX_MAX_D);
        return GPX_ERR_BAD_ARG;
    }
    *v = exp(theta[0]);
    *vt = exp(theta[1]);   // theta[1] = -inf gives vt = 0 (appears in the reference's tests)
    for (int k = 0; k < d; ++k) w[k] = exp(theta[2 + k]);
    if (!(*v > 0.0) || !isfinite(*v) || !isfinite(*vt)) {
        gpx_set_error("theta gives v=%g vt=%g", *v, *vt);
        return GPX_ERR_BAD_ARG;
    }
    for (int k = 0; k < d; ++k)
        if (!(w[k] >= 0.0) || !isfinite(w[k])) {
            gpx_set_error("theta gives w[%d]=%g", k, w[k]);
            return GPX_ERR_BAD_ARG;
        }
    return 0;
}

__global__ __launch_bounds__(256) void extract_lower_kernel(const double *L, long ld, long n, long r0, double *out, long ldo)
{
    const long i = r0 + blockIdx.x;
    for (long j = threadIdx.x; j < n; j += 256) out[(i - r0) * ldo + j] = (j <= i) ? L[i * ld + j] : 0.0;
}

// K [n, n] (+ add_diag on the diagonal) into the padded [npad, npad] buffer, identity in the padding
__global__ __launch_bounds__(256) void pad_copy_kernel(const double *K, long n, double *L, long npad, double add_diag)
{
    const long i = blockIdx.x;
    for (long j = threadIdx.x; j < npad; j += 256)
        L[i * npad + j] = (i < n && j < n) ? K[i * n + j] + ((i == j) ? add_diag : 0.0) : ((i == j) ? 1.0 : 0.0);
}

// ---- Gram (stand-alone) --------------------------------------------------------------------------
// What the device entry points refuse before anything is queued.  gram_kernel reads row min(r, n1 - 1) of xi for EVERY row of the
// padded grid (the padding rows' results are overwritten): with n1 == 0 that is row -1.  A grid smaller than the data would leave
// entries unwritten without a word.
static int check_gram_args(const char *who, const double *xi, int64_t n1, const double *xj, int64_t n2, const double *out, int64_t rows_pad,
                           int64_t cols_pad)
{
    if (n1 < 0 || n2 < 0 || !out || (n1 > 0 && !xi) || (n2 > 0 && !xj) || (n1 == 0 && rows_pad > 0) || rows_pad < n1 || cols_pad < n2) {
        gpx_set_error("%s: bad arguments (n1=%ld n2=%ld rows_pad=%ld cols_pad=%ld: no null input or output, no padded rows without a row, "
                      "rows_pad >= n1, cols_pad >= n2)", who, (long)n1, (long)n2, (long)rows_pad, (long)cols_pad);
        return GPX_ERR_BAD_ARG;
    }
    return 0;
}

extern "C" int gpx_dev_gram(const double *xi_dev, int64_t n1, const double *xj_dev, int64_t n2, int d, const double *theta,
                            double add_diag, int lower_only, int pad_identity, double *out_dev, int64_t ld,
                            int64_t rows_pad, int64_t cols_pad, void *stream)
{
    GPX_TRY(gpx_require_device());
    double v, vt, w[GPX_MAX_D], sw[GPX_MAX_D];
    GPX_TRY(parse_theta(theta, d, &v, &vt, w));
    GPX_TRY(check_gram_args("gpx_dev_gram", xi_dev, n1, xj_dev, n2, out_dev, rows_pad, cols_pad));
    for (int k = 0; k < d; ++k) sw[k] = sqrt(w[k]);
    hipStream_t s = (hipStream_t)stream;
    Scratch sc(s);   // its synchronisation also covers the copy out of the stack array `sw`
    double *swd = nullptr, *a = nullptr, *b = nullptr;
    GPX_TRY(sc.take(&swd, d));
    GPX_HIP(hipMemcpyAsync(swd, sw, sizeof(double) * d, hipMemcpyHostToDevice, s));
    GPX_TRY(sc.take(&a, std::max<int64_t>(n1, 1) * d));
    GPX_TRY(launch_scale_rows(xi_dev, n1, n1, d, swd, a, s));
    if (xj_dev == xi_dev && n1 == n2) b = a;
    else {
        GPX_TRY(sc.take(&b, std::max<int64_t>(n2, 1) * d));
        GPX_TRY(launch_scale_rows(xj_dev, n2, n2, d, swd, b, s));
    }
    GPX_TRY(launch_gram(a, n1, b, n2, d, v, add_diag, lower_only, pad_identity ? 2 : 1, out_dev, ld, rows_pad, cols_pad, s, nullptr));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

// the same on inputs the caller has already scaled by sqrt(w) (and keeps resident): one asynchronous launch, no allocation,
// no synchronisation -- what the multi-GPU host calls once per owned panel
extern "C" int gpx_dev_gram_scaled(const double *xiw_dev, int64_t n1, const double *xjw_dev, int64_t n2, int d, double v, double add_diag,
                                   int lower_only, int pad_identity, double *out_dev, int64_t ld, int64_t rows_pad, int64_t cols_pad,
                                   void *stream)
{
    GPX_TRY(gpx_require_device());
    if (!xiw_dev || !xjw_dev || !(v > 0.0)) { gpx_set_error("gpx_dev_gram_scaled: bad arguments"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(check_gram_args("gpx_dev_gram_scaled", xiw_dev, n1, xjw_dev, n2, out_dev, rows_pad, cols_pad));
    return launch_gram(xiw_dev, n1, xjw_dev, n2, d, v, add_diag, lower_only, pad_identity ? 2 : 1, out_dev, ld, rows_pad, cols_pad,
                       (hipStream_t)stream, nullptr);
}

extern "C" int gpx_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, int d, const double *theta,
                        double add_diag, double *K_out)
{
    GPX_TRY(gpx_require_device());
    if (!xi || !xj || !K_out || n1 < 0 || n2 < 0) { gpx_set_error("gpx_gram: null pointer / negative size"); return GPX_ERR_BAD_ARG; }
    if (n1 == 0 || n2 == 0) return 0;
    double v, vt, w[GPX_MAX_D];
    GPX_TRY(parse_theta(theta, d, &v, &vt, w));
    const int64_t rp = round_up(n1, TILE), cp = round_up(n2, TILE);
    Scratch sc(nullptr);
    double *a = nullptr, *b = nullptr, *out = nullptr;
    GPX_TRY(sc.take(&a, n1 * d));
    if (hipMemcpy(a, xi, sizeof(double) * n1 * d, hipMemcpyDefault) != hipSuccess) { gpx_set_error("copy xi failed"); return GPX_ERR_HIP; }
    if (xj == xi && n1 == n2) b = a;
    else {
        GPX_TRY(sc.take(&b, n2 * d));
        if (hipMemcpy(b, xj, sizeof(double) * n2 * d, hipMemcpyDefault) != hipSuccess) { gpx_set_error("copy xj failed"); return GPX_ERR_HIP; }
    }
    GPX_TRY(sc.take(&out, rp * cp));
    GPX_TRY(gpx_dev_gram(a, n1, b, n2, d, theta, add_diag, 0, 0, out, cp, rp, cp, nullptr));
    if (hipMemcpy2D(K_out, sizeof(double) * n2, out, sizeof(double) * cp, sizeof(double) * n2, n1, hipMemcpyDefault) != hipSuccess) {
        gpx_set_error("copy K_out failed");
        return GPX_ERR_HIP;
    }
    return 0;
}

extern "C" int gpx_dev_chol_panel(double *L, int64_t ld, int64_t nblk, int64_t B0, int64_t B1, double *dinv, double *diag,
                                  int *info_dev, void *stream)
{
    GPX_TRY(gpx_require_device());
    if (!L || !dinv || !diag || !info_dev || B0 < 0 || B1 <= B0 || B1 > nblk || ld < nblk * TILE) {
        gpx_set_error("gpx_dev_chol_panel: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    return chol_panel_factor_piped(L, ld, nblk, B0, B1, dinv, diag, info_dev, (hipStream_t)stream, nullptr);
}

extern "C" int gpx_dev_chol_panel_next(double *L, int64_t ld, int64_t nblk, int64_t B0, int64_t B1, const double *prev, int64_t ldp,
                                       int64_t kp, double *dinv, double *diag, int *info_dev, void *stream)
{
    GPX_TRY(gpx_require_device());
    if (!L || !prev || !dinv || !diag || !info_dev || B0 < 0 || B1 <= B0 || B1 > nblk || ld < nblk * TILE || ldp < kp || kp <= 0 || kp % 16 ||
        (ldp & 1) || ((uintptr_t)prev & 15)) {
        gpx_set_error("gpx_dev_chol_panel_next: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    return chol_panel_factor_piped(L, ld, nblk, B0, B1, dinv, diag, info_dev, (hipStream_t)stream, nullptr, prev, ldp, kp);
}

extern "C" int gpx_dev_chol_panel_split(double *L, int64_t ld, int64_t nblk, int64_t B0, int64_t B1, int64_t head_blocks, const double *prev,
                                        int64_t ldp, int64_t kp, double *dinv, double *diag, int *info_dev, void *stream, void *stream_head,
                                        void *stream_far)
{
    GPX_TRY(gpx_require_device());
    const bool bad_prev = prev && (ldp < kp || kp <= 0 || kp % 16 || (ldp & 1) || ((uintptr_t)prev & 15));
    if (!L || !dinv || !diag || !info_dev || B0 < 0 || B1 <= B0 || B1 > nblk || ld < nblk * TILE || head_blocks < 0 || bad_prev ||
        !stream_head || !stream_far || stream_head == stream_far || stream_head == stream || stream_far == stream) {
        gpx_set_error("gpx_dev_chol_panel_split: bad arguments (three distinct streams, head and far not the null stream)");
        return GPX_ERR_BAD_ARG;
    }
    return chol_panel_factor_piped(L, ld, nblk, B0, B1, dinv, diag, info_dev, (hipStream_t)stream, nullptr, prev, prev ? ldp : 0, prev ? kp : 0,
                                   head_blocks, (hipStream_t)stream_head, (hipStream_t)stream_far);
}

// ---- fit ---------------------------------------------------------------------------------------
// priority class of the fit's streams: main stream normal, chain and column-solve streams high (GPX_SIDE_PRIO=0: test hook that puts
// all of them into one class, so that they share hardware queues -- tests/test_gpu_parity.py, fall-back schedules)
static int side_stream_prio() { static const int v = [] { const char *e = getenv("GPX_SIDE_PRIO"); return e ? atoi(e) : 1; }(); return v; }
extern "C" void gpx_free(gpx_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->prof.destroy();
    h->tri.release();
    raw_release(h->raw);
    h->raw = nullptr;
    if (h->external_factor) { h->L = nullptr; h->Dinv = nullptr; h->diagL = nullptr; }
    double *bufs[] = {h->Ksrc, h->x, h->xs_w, h->sw, h->wdev, h->L, h->Dinv, h->diagL, h->t, h->y, h->alpha, h->Kinv, h->KinvRows, h->Z, h->small, h->V, h->KV};
    for (double *p : bufs)
        if (p) dfree(p);
    if (h->info_dev) dfree(h->info_dev);
    if (h->hstage) { pinned_release(h->hstage); h->hstage = nullptr; }
    if (h->s_pan) { (void)hipStreamSynchronize(h->s_pan); stream_release(h->s_pan, side_stream_prio()); }
    if (h->s_top) { (void)hipStreamSynchronize(h->s_top); stream_release(h->s_top, side_stream_prio()); }
    if (h->own_stream && h->stream) { (void)hipStreamSynchronize(h->stream); stream_release(h->stream, 0); }
    delete h;
}

// policy of the work that rides along with the factorisation (env GPX_FIT_RIDE=0: everything after it, as before round 3)
static int fit_ride_enabled()
{
    static const int v = [] { const char *e = getenv("GPX_FIT_RIDE"); return e ? atoi(e) : 1; }();
    return v;
}

// info_host[0] = potrf status, info_host[1] = stall word (common.h, chol_factor)
static int factor_once(gpx_handle *h, double add_diag, int *info_host)
{
    hipStream_t s = h->stream;
    GPX_HIP(hipMemsetAsync(h->info_dev, 0, 2 * sizeof(int), s));
    const int64_t c1 = CHOL_PANEL_COLS;
    // y = L^-1 t rides along: the solver's diagonal squares are inverted and the forward substitution advances panel by panel on
    // the main stream while that stream would otherwise idle underneath the tail's diagonal chains (chol.hip: panel_final); only
    // the last panel's share and the backward sweep remain after the factorisation.  In the bulk-bound early panels nothing is
    // queued (the main stream is the critical path there): the last calls catch up.
    GPX_TRY(h->tri.attach(h->L, h->npad, h->nblk, h->Dinv));
    GPX_TRY(h->tri.forward_begin(h->t, h->npad, 1, s));
    int64_t pending = 0;                                       // first outer panel the substitution has not passed yet
    bool finished = false;
    const std::function<int(int64_t, int64_t, bool)> ride = [&](int64_t p_final, int64_t slack, bool last) -> int {
        // slack = outer panels still to be updated.  The main stream idles underneath the chains of the last panels, but what it runs
        // there shares the chip with those chains (the forward updates stream the factor at HBM rate, the chain's small GEMMs slow
        // down: chains of 0.7-0.8 ms grew to 0.9-1.1 ms when the catching-up started with four panels left, and the fit gained
        // nothing).  So: up to eight panels per call once a single panel is left, the rest with the last calls.
        static const std::array<int, 5> budget = {1 << 20, 8, 0, 0, 0};   // panels per call with 1..4 panels left
        if (!last && (!fit_ride_enabled() || slack > 4)) return 0;
        const int64_t upto = last ? p_final + 1 : std::min<int64_t>(p_final + 1, pending + budget[slack]);
        if (upto > pending) {
            const int cls = last ? GPX_K_TRSV : GPX_K_TRSV_RIDE;   // what remains after the factorisation / what hides underneath it
            GPX_TRY(h->tri.invert_squares(pending, upto, s, &h->prof, cls));
            ProfScope ps(&h->prof, s, cls, 0.0);
            for (int64_t p = pending; p < upto; ++p) GPX_TRY(h->tri.forward_step(p, s));
            pending = upto;
        }
        // the last call also queues the backward sweep: the factorisation's own stream synchronisation and clean-up on the host
        // (200 us) then run underneath it instead of in front of it.  Should the factorisation have failed, alpha is rubbish that
        // the retry (or the error return) discards.
        if (last && pending == h->tri.P && !finished) {
            GPX_TRY(h->tri.finish(h->npad, 1, h->y, h->alpha, s, &h->prof));
            finished = true;
        }
        return 0;
    };
    // K into the padded factor buffer (lower half, identity in the padding).  A supplied matrix (gpx_fit_matrix) is copied, + jitter on
    // a retry.  A kernel assembles it there: add_diag = vt + jitter (Gaussian) or the jitter alone (the periodic and Matern kernels add vt themselves,
    // wherever two rows are equal).  Beyond one outer panel, and with a chain stream: the first panel's columns now, the rest of the
    // lower half underneath the first panel's diagonal chain.
    const double *x = handle_has_kernel(h) ? handle_train_inputs(h) : nullptr;
    const bool split = x && h->npad > c1 && h->s_pan;
    const std::function<int()> rest = [&]() -> int {
        const double *xr = x + c1 * handle_dim(h);
        return handle_gram(h, xr, h->n - c1, xr, h->n - c1, add_diag, 1, PAD_IDENT, h->L + c1 * h->npad + c1, h->npad, h->npad - c1, h->npad - c1, s,
                           &h->prof);
    };
    if (!x) {
        hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)h->npad), dim3(256), 0, s, (const double *)h->Ksrc, (long)h->n, h->L, (long)h->npad, add_diag);
        GPX_HIP(hipGetLastError());
    } else {
        const int64_t cols = split ? c1 : h->npad;
        GPX_TRY(handle_gram(h, x, h->n, x, std::min<int64_t>(h->n, cols), add_diag, 1, PAD_IDENT, h->L, h->npad, h->npad, cols, s, &h->prof));
    }
    GPX_TRY(chol_factor(h->L, h->npad, h->nblk, h->Dinv, h->diagL, h->info_dev, s, h->s_pan, &h->prof, h->s_top, split ? &rest : nullptr, &ride));
    GPX_TRY(ride(h->tri.P - 1, 0, true));                      // whatever the factorisation's schedule left over
    GPX_HIP(hipMemcpyAsync(info_host, h->info_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}

// One constructor for both kinds of handle: ext == nullptr factors K here (gpx_fit), otherwise the handle wraps a factor
// that already sits in HBM (gpx_adopt_factor) and only alpha is solved for.
struct ExternalFactor { double *L, *Dinv, *diag; double jitter; };

static void setup_lookahead_streams(gpx_handle *h)
{
    // The diagonal chain of the next panel runs on a second, high-priority stream underneath the main stream's work;
    // a third one carries the pipelined panel solves (chol.hip, TopPipe).
    h->s_pan = stream_acquire(side_stream_prio());
    h->s_top = stream_acquire(side_stream_prio());
}

// Kmat != nullptr: the handle of a SUPPLIED covariance matrix (gpx_fit_matrix; n x n, host or device): no inputs, no kernel
// parameters (d = 0) -- the factor, alpha, K^-1 and the solves work as for any handle, everything that evaluates the kernel does not.
// spec != nullptr: a PeriodicCovariance or MaternCovariance model (gpx_periodic_fit, gpx_matern_fit): as a matrix handle (d = 0), but K is
// assembled on the device from x and the parsed parameters, which the handle keeps (h->raw)
static int make_handle(const double *x, const double *t_centered, int64_t n, int d, const double *theta, void *stream,
                       const ExternalFactor *ext, gpx_handle **out, const double *Kmat = nullptr, const RawModel *spec = nullptr)
{
    gpx_handle *h = new (std::nothrow) gpx_handle();
    if (!h) { gpx_set_error("out of host memory"); return GPX_ERR_HIP; }
    h->device = gpx_thread_device();
    int rc = 0;
    if (spec) {
        h->v = spec->v;
        h->vt = spec->vt;
        d = 0;
    } else if (!Kmat) {
        rc = parse_theta(theta, d, &h->v, &h->vt, h->w);
        if (rc) { delete h; return rc; }
        memcpy(h->theta, theta, sizeof(double) * (d + 2));
    } else d = 0;
    h->kind = spec ? spec->kind : Kmat ? KernelKind::Matrix : KernelKind::Gaussian;
    h->n = n;
    h->d = d;
    h->npad = round_up(n, TILE);
    h->nblk = h->npad / TILE;
    if (stream) h->stream = (hipStream_t)stream;
    else {
        if (!(h->stream = stream_acquire(0))) { gpx_set_error("hipStreamCreate failed"); delete h; return GPX_ERR_HIP; }
        h->own_stream = true;
    }
    hipStream_t s = h->stream;
    if (!ext) setup_lookahead_streams(h);
    auto fail = [&](int code) { gpx_free(h); return code; };
    if (const char *pe = getenv("GPX_PROFILE")) h->prof.level = atoi(pe);   // covers the kernels of the constructor itself

    double sw[GPX_MAX_D];
    for (int k = 0; k < d; ++k) sw[k] = sqrt(h->w[k]);
    if ((rc = dalloc(&h->x, n * d)) || (rc = dalloc(&h->xs_w, h->npad * d)) || (rc = dalloc(&h->sw, std::max(d, 1))) ||
        (rc = dalloc(&h->wdev, std::max(d, 1))) || (rc = dalloc(&h->t, h->npad)) || (rc = dalloc(&h->y, h->npad)) ||
        (rc = dalloc(&h->alpha, h->npad)) || (rc = dalloc(&h->small, 4096 + h->npad)))
        return fail(rc);
    if (ext) {
        h->external_factor = true;
        h->L = ext->L;
        h->Dinv = ext->Dinv;
        h->diagL = ext->diag;
        h->jitter = ext->jitter;
    } else if ((rc = dalloc(&h->L, h->npad * h->npad)) || (rc = dalloc(&h->Dinv, h->nblk * (int64_t)TILE * TILE)) ||
               (rc = dalloc(&h->diagL, h->npad)))
        return fail(rc);
    {
        double *ib = nullptr;
        if ((rc = dalloc(&ib, h->nblk + 8))) return fail(rc);   // (16 + 2 nblk) ints: status, stall, blocker words, per-panel counters
        h->info_dev = reinterpret_cast<int *>(ib);
    }
#define FIT_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { gpx_set_error("%s failed: %s", #call, hipGetErrorString(e_)); return fail(GPX_ERR_HIP); } } while (0)
    FIT_HIP(hipMemsetAsync(h->info_dev, 0, sizeof(int) * (16 + 2 * h->nblk), s));
    if (spec) {
        if (!(h->raw = raw_clone(spec))) { gpx_set_error("out of host memory"); return fail(GPX_ERR_HIP); }
        if ((rc = raw_upload(h->raw, x, n, h->npad, s))) return fail(rc);
    } else if (Kmat) {
        if ((rc = dalloc(&h->Ksrc, n * n))) return fail(rc);
        FIT_HIP(hipMemcpyAsync(h->Ksrc, Kmat, sizeof(double) * n * n, hipMemcpyDefault, s));
    } else {
        FIT_HIP(hipMemcpyAsync(h->x, x, sizeof(double) * n * d, hipMemcpyDefault, s));
        FIT_HIP(hipMemcpyAsync(h->sw, sw, sizeof(double) * d, hipMemcpyHostToDevice, s));
        FIT_HIP(hipMemcpyAsync(h->wdev, h->w, sizeof(double) * d, hipMemcpyHostToDevice, s));
    }
    FIT_HIP(hipMemsetAsync(h->t, 0, sizeof(double) * h->npad, s));
    FIT_HIP(hipMemcpyAsync(h->t, t_centered, sizeof(double) * n, hipMemcpyDefault, s));
    FIT_HIP(hipStreamSynchronize(s));   // sw is a stack buffer: its copy must be complete before any return path
    if (!ext) chol_probe_streams(s, h->s_pan, h->s_top);   // while every stream of the fit is idle (cached per pair of streams)
    if (h->kind == KernelKind::Gaussian && (rc = launch_scale_rows(h->x, n, h->npad, d, h->sw, h->xs_w, s))) return fail(rc);

    if (!ext) {
        // A stalled hand-off (an in-kernel wait of the look-ahead schedule expired: streams that were probed as concurrent no longer
        // are) is not a property of K: that factor is discarded and the fit repeated ONCE on the plain schedule -- no kernel waits
        // for a kernel of another stream there --, never with jitter.
        auto factor = [&](double add_diag, int *info) -> int {
            int st[2] = {0, 0};
            GPX_TRY(factor_once(h, add_diag, st));
            if (st[1]) {
                if (getenv("GPX_DEBUG")) fprintf(stderr, "[gpx] factorisation hand-off stalled: refit on the plain schedule\n");
                chol_concurrency_forget();
                chol_force_plain_schedule(true);
                const int rc2 = factor_once(h, add_diag, st);
                chol_force_plain_schedule(false);
                GPX_TRY(rc2);
                if (st[1]) { gpx_set_error("factorisation stalled on the plain schedule as well"); return GPX_ERR_STATE; }
            }
            *info = st[0];
            return 0;
        };
        int info = 0;
        const double diag0 = h->kind == KernelKind::Gaussian ? h->vt : 0.0;   // (a supplied K carries its own diagonal; the periodic and Matern Grams add vt themselves)
        if ((rc = factor(diag0, &info))) return fail(rc);
        if (info > 0) {
            // reference fallback: cholesky(K + 1e-5 I)   (skgpuppy/Covariance.py:180-185)
            h->jitter = 1e-5;
            if ((rc = factor(diag0 + h->jitter, &info))) return fail(rc);
            if (info > 0) {
                gpx_set_error("covariance matrix not positive definite (leading minor %d), also with +1e-5 jitter", info);
                return fail(info);
            }
        }
    }
    // y = L^-1 t, alpha = L^-T y: the solver's diagonal-square inverses are kept for the propagation right after a fit
    if (ext) {   // (gpx_fit: both sweeps were queued by factor_once)
        if ((rc = h->tri.prepare(h->L, h->npad, h->nblk, h->Dinv, s, &h->prof))) return fail(rc);
        if ((rc = h->tri.solve(h->t, h->npad, 1, h->y, h->alpha, s, &h->prof))) return fail(rc);
    }
    FIT_HIP(hipStreamSynchronize(s));
#undef FIT_HIP
    if (h->Ksrc) { dfree(h->Ksrc); h->Ksrc = nullptr; }   // the factor replaces it
    *out = h;
    return 0;
}

extern "C" int gpx_fit(const double *x, const double *t_centered, int64_t n, int d, const double *theta, void *stream,
                       gpx_handle **out)
{
    if (out) *out = nullptr;
    GPX_TRY(gpx_require_device());
    if (!x || !t_centered || !out || n < 1) { gpx_set_error("gpx_fit: null pointer or n < 1"); return GPX_ERR_BAD_ARG; }
    return make_handle(x, t_centered, n, d, theta, stream, nullptr, out);
}

extern "C" int gpx_adopt_factor(const double *x, const double *t_centered, int64_t n, int d, const double *theta,
                                double *L_dev, double *dinv_dev, double *diag_dev, double jitter, void *stream,
                                gpx_handle **out)
{
    if (out) *out = nullptr;
    GPX_TRY(gpx_require_device());
    if (!x || !t_centered || !out || n < 1 || !L_dev || !dinv_dev || !diag_dev) { gpx_set_error("gpx_adopt_factor: null pointer or n < 1"); return GPX_ERR_BAD_ARG; }
    const ExternalFactor ext{L_dev, dinv_dev, diag_dev, jitter};
    return make_handle(x, t_centered, n, d, theta, stream, &ext, out);
}

// ---- operator interface with a SUPPLIED matrix: what GaussianProcess.__init__ / estimate_many do for ANY Covariance subclass
// (skgpuppy/GaussianProcess.py:39-41, :68-80 talk to cov.cov_matrix / cov.cov_matrix_ij / cov.inv_cov_matrix only; the base-class
// inv_cov_matrix skgpuppy/Covariance.py:167-187 inverts whatever cov_matrix returns, with the +1e-5 I retry) -------------------------
extern "C" int gpx_fit_matrix(const double *K, const double *t_centered, int64_t n, void *stream, gpx_handle **out)
{
    if (out) *out = nullptr;
    GPX_TRY(gpx_require_device());
    if (!K || !t_centered || !out || n < 1) { gpx_set_error("gpx_fit_matrix: null pointer or n < 1"); return GPX_ERR_BAD_ARG; }
    return make_handle(nullptr, t_centered, n, 0, nullptr, stream, nullptr, out, K);
}

// ---- PeriodicCovariance: K = cov_matrix(x, theta) of skgpuppy/Covariance.py:361-386 (through the base class's :137-164) assembled on
// the device, then GaussianProcess.__init__'s inverse (skgpuppy/GaussianProcess.py:39-41, Covariance.py:167-187) as for every handle ----
extern "C" int gpx_periodic_fit(const double *x, const double *t_centered, int64_t n, int d, const double *theta, void *stream,
                                gpx_handle **out)
{
    if (out) *out = nullptr;
    GPX_TRY(gpx_require_device());
    if (!x || !t_centered || !out || n < 1) { gpx_set_error("gpx_periodic_fit: null pointer or n < 1"); return GPX_ERR_BAD_ARG; }
    PeriodicData pd;
    GPX_TRY(periodic_parse(theta, d, &pd));
    return make_handle(x, t_centered, n, 0, nullptr, stream, nullptr, out, nullptr, &pd);
}

// ---- MaternCovariance (nu2 = 2 nu: 3 or 5): K assembled on the device by matern_gram_kernel, everything after it as for every handle ----
extern "C" int gpx_matern_fit(const double *x, const double *t_centered, int64_t n, int d, const double *theta, int nu2, void *stream,
                              gpx_handle **out)
{
    if (out) *out = nullptr;
    GPX_TRY(gpx_require_device());
    if (!x || !t_centered || !out || n < 1) { gpx_set_error("gpx_matern_fit: null pointer or n < 1"); return GPX_ERR_BAD_ARG; }
    MaternData md;
    GPX_TRY(matern_parse(theta, d, nu2, &md));
    return make_handle(x, t_centered, n, 0, nullptr, stream, nullptr, out, nullptr, &md);
}

extern "C" int gpx_n(const gpx_handle *h, int64_t *n, int *d)
{
    if (!h) { gpx_set_error("null handle"); return GPX_ERR_BAD_ARG; }
    if (n) *n = h->n;
    if (d) *d = handle_dim(h);
    return 0;
}

extern "C" int gpx_jitter_used(const gpx_handle *h, double *jitter)
{
    if (!h || !jitter) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    *jitter = h->jitter;
    return 0;
}

extern "C" int gpx_logdet(gpx_handle *h, double *logdet)
{
    CHECK_H(h);
    if (!logdet) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    if (!h->have_logdet) {
        GPX_TRY(launch_logdet(h->diagL, h->n, h->small, h->stream));
        GPX_HIP(hipMemcpyAsync(&h->logdet, h->small, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        GPX_HIP(hipStreamSynchronize(h->stream));
        h->have_logdet = true;
    }
    *logdet = h->logdet;
    return 0;
}

// ---- accessors -----------------------------------------------------------------------------------
extern "C" int gpx_alpha(gpx_handle *h, double *beta_out)
{
    CHECK_H_PSEUDO_OK(h);
    if (!beta_out) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    GPX_HIP(hipMemcpyAsync(beta_out, h->alpha, sizeof(double) * h->n, hipMemcpyDefault, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int gpx_chol_rows(gpx_handle *h, int64_t r0, int64_t r1, double *L_out)
{
    CHECK_H(h);
    if (!L_out || r0 < 0 || r1 < r0 || r1 > h->n) { gpx_set_error("gpx_chol_rows: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (r1 == r0) return 0;
    Scratch sc(h->stream);
    double *tmp = nullptr;
    GPX_TRY(sc.take(&tmp, (r1 - r0) * h->n));
    hipLaunchKernelGGL(extract_lower_kernel, dim3((unsigned)(r1 - r0)), dim3(256), 0, h->stream, (const double *)h->L,
                       (long)h->npad, (long)h->n, (long)r0, tmp, (long)h->n);
    GPX_HIP(hipMemcpyAsync(L_out, tmp, sizeof(double) * (r1 - r0) * h->n, hipMemcpyDefault, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int gpx_chol(gpx_handle *h, double *L_out)
{
    if (!h) { gpx_set_error("null handle"); return GPX_ERR_BAD_ARG; }
    return gpx_chol_rows(h, 0, h->n, L_out);
}

// ---- a4 with a caller-supplied matrix: Covariance.inv_cov_matrix(x, theta, cov_matrix=K) = inv(K)
// (skgpuppy/Covariance.py:186-187).  K must be symmetric positive definite (it is a covariance matrix); it is
// Cholesky-factored on the GPU, status > 0 when it is not.
extern "C" int gpx_spd_inverse(const double *K, int64_t n, double *Kinv_out, double *logdet_out)
{
    GPX_TRY(gpx_require_device());
    if (!K || !Kinv_out || n < 1) { gpx_set_error("gpx_spd_inverse: bad arguments"); return GPX_ERR_BAD_ARG; }
    const int64_t npad = round_up(n, TILE), nblk = npad / TILE;
    hipStream_t s = nullptr;
    Scratch sc(s);
    double *Kd = nullptr, *L = nullptr, *Dinv = nullptr, *diag = nullptr, *Z = nullptr, *Ki = nullptr;
    int *info = nullptr;   // [0] potrf status, [1] stall word (chol_factor)
    int info_h = 0;
    double ld_h = 0.0;
    GPX_TRY(sc.take(&Kd, n * n));
    GPX_TRY(sc.take(&L, npad * npad));
    GPX_TRY(sc.take(&Dinv, nblk * (int64_t)TILE * TILE));
    GPX_TRY(sc.take(&diag, npad + 8));
    GPX_TRY(sc.take(&Z, npad * npad));
    GPX_TRY(sc.take(&Ki, npad * npad));
    GPX_TRY(sc.take(&info, 2));
    GPX_HIP(hipMemsetAsync(info, 0, 2 * sizeof(int), s));
    GPX_HIP(hipMemcpyAsync(Kd, K, sizeof(double) * n * n, hipMemcpyDefault, s));
    hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)npad), dim3(256), 0, s, (const double *)Kd, (long)n, L, (long)npad, 0.0);
    GPX_TRY(chol_factor(L, npad, nblk, Dinv, diag, info, s, nullptr, nullptr, nullptr));
    GPX_HIP(hipMemcpyAsync(&info_h, info, sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (info_h > 0) { gpx_set_error("matrix not positive definite (leading minor %d)", info_h); return info_h; }
    GPX_TRY(build_kinv_from_factor(L, npad, nblk, Dinv, Z, Ki, s, nullptr));
    if (logdet_out) {
        GPX_TRY(launch_logdet(diag, n, diag + npad, s));
        GPX_HIP(hipMemcpyAsync(&ld_h, diag + npad, sizeof(double), hipMemcpyDeviceToHost, s));
    }
    GPX_HIP(hipMemcpy2DAsync(Kinv_out, sizeof(double) * n, Ki, sizeof(double) * npad, sizeof(double) * n, n, hipMemcpyDefault, s));
    GPX_HIP(hipStreamSynchronize(s));
    if (logdet_out) *logdet_out = ld_h;
    return 0;
}

// ---- "next" row f1: negative log likelihood and its gradient at the handle's theta ----------------------------------
extern "C" int gpx_nll(gpx_handle *h, double *nll)
{
    CHECK_H(h);
    if (!nll) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    double logdet = 0.0;
    GPX_TRY(gpx_logdet(h, &logdet));
    std::vector<std::pair<const double *, const double *>> pr;
    pr.push_back({h->t, h->alpha});
    GPX_TRY(launch_dot_pairs(pr, h->npad, h->small, h->stream));
    double ta = 0.0;
    GPX_HIP(hipMemcpyAsync(&ta, h->small, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    // N/2 log(2 pi) + 1/2 log det K + 1/2 t^T K^-1 t     (skgpuppy/Covariance.py:197-216)
    *nll = 0.5 * (double)h->n * log(2.0 * M_PI) + 0.5 * logdet + 0.5 * ta;
    return 0;
}

extern "C" int gpx_nll_grad(gpx_handle *h, double *grad_out)
{
    CHECK_H(h);
    NEED_KERNEL(h, "gpx_nll_grad");
    if (!grad_out) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(ensure_kinv(h));
    const int d = h->d;
    Scratch sc(h->stream);
    double *buf = nullptr;
    const int64_t nb = h->npad / 8;
    GPX_TRY(sc.take(&buf, nb * (GPX_MAX_D + 2) + GPX_MAX_D + 2));
    double *outd = buf + nb * (GPX_MAX_D + 2);
    int dm = 0;
    GPX_TRY(launch_nll_grad(h->Kinv, h->npad, h->n, h->npad, d, h->alpha, h->xs_w, h->v, buf, outd, &dm, h->stream, &h->prof));
    double o[GPX_MAX_D + 2];
    GPX_HIP(hipMemcpyAsync(o, outd, sizeof(double) * (dm + 2), hipMemcpyDeviceToHost, h->stream));
    GPX_HIP(hipStreamSynchronize(h->stream));
    std::vector<double> g(d + 2);
    g[0] = 0.5 * o[0];                                   // dK/dtheta_0 = Kf            (Covariance.py:633-639)
    g[1] = 0.5 * h->vt * o[dm + 1];                      // dK/dtheta_1 = vt I          (Covariance.py:505-510)
    for (int k = 0; k < d; ++k) g[2 + k] = -0.25 * o[1 + k];   // dK/dtheta_{2+k} = -1/2 Kf w_k dx_k^2 (:643-657); w_k is in the scaled inputs
    GPX_HIP(hipMemcpy(grad_out, g.data(), sizeof(double) * (d + 2), hipMemcpyDefault));
    return 0;
}

// d nll / d theta_j for ANY operator from its derivative matrix dK = d cov_matrix / d theta_j [n, n] (Covariance._d_nll_d_theta,
// skgpuppy/Covariance.py:266-282): 1/2 tr(K^-1 dK) - 1/2 alpha^T dK alpha as ONE pass over K^-1 and dK (K^-1 from the factor is
// exactly symmetric, so tr(K^-1 dK) = sum_ij Kinv_ij dK_ij); one wave per row, per-row partials, fixed-order final sum.
__global__ __launch_bounds__(256) void trace_quad_rows_kernel(const double *__restrict__ Kinv, long ldk, const double *__restrict__ dK, long n,
                                                             const double *__restrict__ alpha, double *__restrict__ part)
{
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    double s1 = 0.0, s2 = 0.0;
    for (long j = lane; j < n; j += 64) {
        const double dk = dK[i * n + j];
        s1 = fma(Kinv[i * ldk + j], dk, s1);
        s2 = fma(dk, alpha[j], s2);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) { part[2 * i] = s1; part[2 * i + 1] = alpha[i] * s2; }
}
__global__ __launch_bounds__(256) void sum_pairs_kernel(const double *__restrict__ part, long n, double *__restrict__ out)
{
    __shared__ double r1[256], r2[256];
    double a = 0.0, b = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) { a += part[2 * i]; b += part[2 * i + 1]; }
    r1[threadIdx.x] = a; r2[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = r1[0]; out[1] = r2[0]; }
}

extern "C" int gpx_nll_grad_matrix(gpx_handle *h, const double *dK, double *grad_out)
{
    CHECK_H(h);
    if (!dK || !grad_out) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(ensure_kinv(h));
    hipStream_t s = h->stream;
    const int64_t n = h->n;
    Scratch sc(s);
    double *dKd = nullptr, *part = nullptr;
    GPX_TRY(sc.take(&dKd, n * n));
    GPX_TRY(sc.take(&part, 2 * n + 2));
    double o[2] = {0.0, 0.0};
    GPX_HIP(hipMemcpyAsync(dKd, dK, sizeof(double) * n * n, hipMemcpyDefault, s));
    hipLaunchKernelGGL(trace_quad_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, (const double *)h->Kinv, (long)h->npad,
                       (const double *)dKd, (long)n, (const double *)h->alpha, part);
    hipLaunchKernelGGL(sum_pairs_kernel, dim3(1), dim3(256), 0, s, (const double *)part, (long)n, part + 2 * n);
    GPX_HIP(hipGetLastError());
    GPX_HIP(hipMemcpyAsync(o, part + 2 * n, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    const double g = 0.5 * o[0] - 0.5 * o[1];
    GPX_HIP(hipMemcpy(grad_out, &g, sizeof(double), hipMemcpyDefault));
    return 0;
}

// out[r] = M V[r] for a SUPPLIED symmetric matrix M [n, n] and a few vectors V [nrhs, n] (rows): the reference's quadratic-form
// helpers take an explicit Kinv argument (UncertaintyPropagationApprox._get_sigma2 / _get_variance_rest,
// skgpuppy/UncertaintyPropagation.py:412-481); when it is not the fitted model's own this is the device route for it.
extern "C" int gpx_symv(const double *M, int64_t n, const double *V, int nrhs, double *out)
{
    GPX_TRY(gpx_require_device());
    if (!M || !V || !out || n < 1 || nrhs < 1 || nrhs > 64) { gpx_set_error("gpx_symv: bad arguments (n=%ld, nrhs=%d; at most 64 vectors)", (long)n, nrhs); return GPX_ERR_BAD_ARG; }
    const int64_t npad = round_up(n, TILE);
    hipStream_t s = nullptr;
    Scratch sc(s);
    double *Md = nullptr, *Mp = nullptr, *Vd = nullptr, *KVd = nullptr;
    GPX_TRY(sc.take(&Md, n * n));
    GPX_TRY(sc.take(&Mp, npad * npad));
    GPX_TRY(sc.take(&Vd, (int64_t)nrhs * npad));
    GPX_TRY(sc.take(&KVd, (int64_t)nrhs * npad));
    GPX_HIP(hipMemcpyAsync(Md, M, sizeof(double) * n * n, hipMemcpyDefault, s));
    hipLaunchKernelGGL(pad_copy_kernel, dim3((unsigned)npad), dim3(256), 0, s, (const double *)Md, (long)n, Mp, (long)npad, 0.0);   // (identity padding meets zero-padded vectors)
    GPX_HIP(hipMemsetAsync(Vd, 0, sizeof(double) * nrhs * npad, s));
    GPX_HIP(hipMemcpy2DAsync(Vd, sizeof(double) * npad, V, sizeof(double) * n, sizeof(double) * n, nrhs, hipMemcpyDefault, s));
    GPX_TRY(launch_kinv_pass(Mp, npad, npad, nrhs, Vd, KVd, s, nullptr));
    GPX_HIP(hipMemcpy2DAsync(out, sizeof(double) * n, KVd, sizeof(double) * npad, sizeof(double) * n, nrhs, hipMemcpyDefault, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}
