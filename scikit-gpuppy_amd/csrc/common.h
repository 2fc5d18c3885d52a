// common.h -- shared declarations of libgpx (gfx950 only; no other target is supported)
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stdint.h>
#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "../../include/gpx.h"

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

constexpr int TILE = GPX_TILE;       // 128: diagonal-block size, GEMM block tile
constexpr int GEMM_BK = 16;          // k-depth of one LDS stage

// ---- error plumbing ---------------------------------------------------------------------
void gpx_set_error(const char *fmt, ...);
#define GPX_HIP(call)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            gpx_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return GPX_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)
#define GPX_TRY(call)            \
    do {                         \
        int r_ = (call);         \
        if (r_ != 0) return r_;  \
    } while (0)

static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
// rows an input owns in a right-hand-side block of the batched row calls (GPX_ROWS_*, include/gpx.h): the ONE definition, for the build
// frame (rows_tile.h), its launcher, gpx_rows_build / gpx_rows_reduce and the chunk loop
__host__ __device__ constexpr int rows_per_input(int layout, int d) { return layout == GPX_ROWS_DVH ? 2 * d + 1 : layout == GPX_ROWS_APPROX ? d + 2 : d + 1; }

// ---- exp for non-positive arguments (every exponent on the path is -1/2 of a squared distance, or a sum of such) ----
// Plain Cody-Waite: n = rint(x log2 e), r = x - n ln2 (two-term), degree-12 Taylor polynomial on |r| <= ln2/2
// (truncation 1.7e-16), scaled by v_ldexp_f64 (which also produces the denormal / zero results for very negative x).
// ~18 fp64 ops instead of the ~45 of the generic exp; within 2 ulp of it.
// Nothing in it needs x <= 0: the reduction is exact for |n| < 2^20 (ln2's high part ends in 21 zero bits) and ldexp scales
// either way, so a positive x below 709 is as accurate -- the explicit Exact path (exact_build_generic_kernel) sends exponents of
// +200 through it (tests/test_dense_bounds.py, test_exact_explicit_positive_exponents).  Only the clamp is one-sided: from 709.8
// on the result is +inf, as exp's.
static __device__ __forceinline__ double exp_nonpos(double x)
{
    x = fmax(x, -750.0);
    const double n = rint(x * 1.4426950408889634);
    double r = fma(-n, 6.93147180369123816490e-01, x);
    r = fma(-n, 1.90821492927058770002e-10, r);
    double p = 2.08767569878680989792e-09;          // 1/12!
    p = fma(p, r, 2.50521083854417187751e-08);      // 1/11!
    p = fma(p, r, 2.75573192239858906526e-07);      // 1/10!
    p = fma(p, r, 2.75573192239858906526e-06);      // 1/9!
    p = fma(p, r, 2.48015873015873015873e-05);      // 1/8!
    p = fma(p, r, 1.98412698412698412698e-04);      // 1/7!
    p = fma(p, r, 1.38888888888888888889e-03);      // 1/6!
    p = fma(p, r, 8.33333333333333333333e-03);      // 1/5!
    p = fma(p, r, 4.16666666666666666667e-02);      // 1/4!
    p = fma(p, r, 1.66666666666666666667e-01);      // 1/3!
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}
// ---- the sum over a wave's 64 lanes, in every lane: butterfly, the partner 32 lanes away first ----
static __device__ __forceinline__ double wave_sum(double s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}
// ---- per-kernel-class event profiler ---------------------------------------------------------
struct Profiler {
    int level = 0;   // 0 off; 1 = only the dominant kernel (128x128-tile GEMM launches); 2 = every kernel class
    struct Rec { int cls; double work; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    int64_t launches[GPX_K_COUNT] = {0};
    double ms[GPX_K_COUNT] = {0};
    double work[GPX_K_COUNT] = {0};
    int begin(hipStream_t s, int cls, double w);   // returns record index or -1
    void end(hipStream_t s, int idx);
    int collect(hipStream_t s);                    // synchronises, folds recs into the sums
    void reset();
    void destroy();
};

struct ProfScope {
    Profiler *p; hipStream_t s; int idx;
    ProfScope(Profiler *p_, hipStream_t s_, int cls, double w, int min_level = 2) : p(p_), s(s_), idx(-1) {
        if (p && p->level >= min_level) idx = p->begin(s, cls, w);
    }
    ~ProfScope() { if (idx >= 0) p->end(s, idx); }
};

// ---- triangular solves with a few right-hand sides against a factor (tsolve.hip) -----------------
// prepare() inverts the 1024 x 1024 diagonal squares of the factor once (from the 128-block inverses Dinv); solve() then
// runs N / 1024 fat steps per sweep.  The solver borrows L and Dinv: they must outlive it.
struct TriSolver {
    const double *L = nullptr, *Dinv = nullptr;
    int64_t ld = 0, nblk = 0, npad = 0, P = 0;
    double *Pl = nullptr, *Pz = nullptr;   // [P][1024][1024] inverses of the diagonal squares and their transposes
    double *T = nullptr;                   // [P][512][512] scratch of the doubling levels
    double *W = nullptr, *Y = nullptr;     // [32 npad] right-hand sides / solutions in the pair-major layout
    int cur_ng = 0;                        // stepwise forward substitution in flight: right-hand sides / 16 (0 = none)
    int prepare(const double *L, int64_t ld, int64_t nblk, const double *Dinv, hipStream_t s, Profiler *prof);
    // prepare in pieces (the fit runs them underneath the factorisation's tail): buffers only / squares [p0, p1) of a factor whose
    // outer panels p0..p1-1 are final on stream s
    int attach(const double *L, int64_t ld, int64_t nblk, const double *Dinv);
    int invert_squares(int64_t p0, int64_t p1, hipStream_t s, Profiler *prof, int prof_class = GPX_K_TRSV);
    // forward substitution in steps of one outer panel: begin (pack), step p (needs square p and the factor's columns of panel p),
    // finish = the rest of solve() (Yout / backward sweep / Aout)
    int forward_begin(const double *B, int64_t ldb, int nrhs, hipStream_t s);
    int forward_step(int64_t p, hipStream_t s);
    int finish(int64_t ldb, int nrhs, double *Yout, double *Aout, hipStream_t s, Profiler *prof);
    // B [nrhs][ldb] (right-hand sides as rows, nrhs <= 32) -> Yout = L^-1 B and / or Aout = L^-T L^-1 B (null = skip)
    int solve(const double *B, int64_t ldb, int nrhs, double *Yout, double *Aout, hipStream_t s, Profiler *prof);
    int mul_lower(const double *B, int64_t ldb, int nrhs, double *OUT, hipStream_t s);   // OUT = L B (rows, nrhs <= 32)
    // X [r1 - r0, npad] <- rows [r0, r1) of K^-1 without the rest of it (multiples of 128); Zb, Yb: scratch of X's shape, Tb: [1024, npad]
    int kinv_rows(int64_t r0, int64_t r1, double *X, double *Zb, double *Yb, double *Tb, hipStream_t s, Profiler *prof) const;
    void release();
    bool ready() const { return Pl != nullptr; }
};

// ---- the fitted model held in HBM ------------------------------------------------------------
// What evaluates a handle's kernel: nothing (the matrix was supplied: gpx_fit_matrix), gram_kernel on xs_w (gpx_fit, gpx_adopt_factor)
// periodic_gram_kernel (gpx_periodic_fit) or matern_gram_kernel (gpx_matern_fit) on raw->x.  Callers ask the handle_* helpers below, not
// the fields.
enum class KernelKind { Matrix, Gaussian, Periodic, Matern };
struct gpx_handle {
    int device = 0;
    int64_t n = 0, npad = 0, nblk = 0;
    KernelKind kind = KernelKind::Matrix;
    int d = 0;                  // Gaussian: the input dimension (0 otherwise: handle_dim)
    double v = 0, vt = 0, jitter = 0;
    double theta[GPX_MAX_D + 2];
    double w[GPX_MAX_D];
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool external_factor = false;   // L / Dinv / diagL belong to the caller (gpx_adopt_factor)
    // A pseudo-input model (gpx_spgp_pseudo_handle, spgp.hip): x = the m pseudo-inputs, alpha = beta, Kinv = P resident from the start, and
    // NO factor -- L, Dinv, diagL, tri, t and y stay null.  CHECK_H refuses such a handle; the entry points that read nothing but
    // (x, alpha, Kinv, v, vt, w) take it through CHECK_H_PSEUDO_OK.
    bool no_factor = false;
    hipStream_t s_pan = nullptr;   // side stream (high priority) for the latency-bound diagonal chain
    hipStream_t s_top = nullptr;   // pipelined panel solves of the factorisation (chol.hip, TopPipe)

    double *Ksrc = nullptr;     // gpx_fit_matrix only, during the fit: the supplied matrix [n, n] (kept for the jitter retry)
    double *x = nullptr;        // [n, d] raw inputs (d == 0: a handle built from a supplied matrix)
    double *xs_w = nullptr;     // [npad, d] inputs scaled by sqrt(w) (rows >= n are zero)
    double *sw = nullptr;       // [d] sqrt(w) on device
    double *wdev = nullptr;     // [d] w on device
    double *L = nullptr;        // [npad, npad] lower Cholesky factor (blocks above the diagonal unused)
    double *Dinv = nullptr;     // [nblk, 128, 128] inverses of the diagonal blocks of L
    double *diagL = nullptr;    // [npad]
    double *t = nullptr;        // [npad] centred targets (zero padded)
    double *y = nullptr;        // [npad] L^-1 t
    double *alpha = nullptr;    // [npad] K^-1 t
    TriSolver tri;              // few-right-hand-side solves against L (alpha, the propagation right after a fit)
    double *Kinv = nullptr;     // [npad, npad] lazily materialised
    double *KinvRows = nullptr; // [kr1 - kr0, npad]: a row panel of K^-1 alone (the row-sharded propagation; predict.hip, ensure_kinv_rows)
    int64_t kr0 = 0, kr1 = 0;
    int *info_dev = nullptr;    // [0] potrf info (1-based failing column, 0 = ok)
    double logdet = 0;
    bool have_logdet = false;

    // scratch
    double *Z = nullptr;        // predict / inverse workspace [zrows, npad]
    int64_t zrows = 0;
    double *small = nullptr;    // small device scratch (reductions, propagate vectors)
    double *hstage = nullptr;   // pinned host staging block of the propagation calls (runtime.hip, pinned_acquire)

    // propagate cache (keyed on u)
    int approx_solves = 0;      // new-u propagations served by triangular solves so far (K^-1 is built after a few)
    bool have_u = false;
    double u[GPX_MAX_D];
    double *V = nullptr;        // [ncolV, npad] column-major block of C, J_k, hh_k, tr
    double *KV = nullptr;       // [ncolV, npad] Kinv * V
    struct RawModel *raw = nullptr;   // gpx_periodic_fit / gpx_matern_fit only (rawmodel.hip): inputs and parameters of a raw-input kernel; d stays 0
    Profiler prof;
};

// ---- the raw-input kernels (rawmodel.hip): what PeriodicCovariance and MaternCovariance share ----------------------------------
// Their Gram kernels read the inputs RAW (the periodic factor needs delta itself; equality is decided on max |delta|).  A handle of such
// a kind is a matrix handle (d == 0: K was assembled on the device instead of supplied) that owns ONE RawModel -- a PeriodicData or a
// MaternData, as `kind` says -- with what its predict / nll_grad / propagation entry points evaluate the kernel on.
struct RawModel {
    KernelKind kind;
    int d = 0;
    double v = 0, vt = 0;
    double *x = nullptr;      // [n, d] raw inputs
    double *xT = nullptr;     // [d, npad] the same k-major (the gradient pass reads a column of K^-1 per lane)
    double *par = nullptr;    // the kernels' wave-uniform constants: [4, d] periodic, [d] Matern (raw_pack)
    explicit RawModel(KernelKind k) : kind(k) {}
};
int raw_pack(const RawModel *m, double *host);    // host [<= 4 GPX_MAX_D] <- the content of par; returns its length
// the preamble of both parsers: d in range, v, vt (checked) and w_k = exp(theta[2 + k]) (the kind checks them); `name` opens the texts
int raw_parse_head(const char *name, const double *theta, int d, RawModel *out, double *w);
RawModel *raw_clone(const RawModel *spec);        // a parsed spec's host part on the heap (null: out of host memory)
int raw_upload(RawModel *m, const double *x, int64_t n, int64_t npad, hipStream_t s);   // x (host or device) -> m->x, xT, par; synchronises
void raw_release(RawModel *m);
// out[i][j] of the model's kernel from the raw inputs (launch_periodic_gram / launch_matern_gram by kind)
int launch_raw_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, const RawModel *m, double add_diag, int lower_only,
                    int pad_mode, double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad, hipStream_t s, Profiler *prof, int deriv = -1);
// the stand-alone Gram of a parsed model (gpx_periodic_gram / gpx_matern_gram): raw_gram_args before the parse, raw_gram after it
int raw_gram_args(const char *what, const double *xi, int64_t n1, const double *xj, int64_t n2, const double *out);
int raw_gram(RawModel *m, const double *xi, int64_t n1, const double *xj, int64_t n2, int deriv, double *out);
// the gradient pass of a handle's model and its column sums: o [sweeps * nc] on the host, sweeps = ceil(d / kc)
int raw_nll_grad_sums(gpx_handle *h, int kc, int nc, double *o);

// ---- PeriodicCovariance (periodic.hip; skgpuppy/Covariance.py:361-433) -------------------------------------------------
// theta = (log v, log vt, log w_1..d, log p_1..d, log w2_1..d).  par [4, d]: w / 2, fl(1 / p), its correction (periodic_math.h), w2 / 2.
struct PeriodicData : RawModel {
    double w[GPX_MAX_D], p[GPX_MAX_D], w2[GPX_MAX_D];   // exp(theta)
    PeriodicData() : RawModel(KernelKind::Periodic) {}
};
int periodic_parse(const double *theta, int d, PeriodicData *out);          // host; GPX_ERR_BAD_ARG with text
// out[i][j] = v exp(-q_ij) (+ vt where x_i == x_j in every component) (+ add_diag where row == col), q = 1/2 sum_k w_k delta_k^2 +
// w2_k sin^2(pi delta_k / p_k), from the raw inputs; lower_only / pad_mode / padding contract as launch_gram.
// deriv >= 0: d K / d theta_deriv instead (no add_diag; pd carries the parameters the factor is made of)
int launch_periodic_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, const PeriodicData *pd, double add_diag,
                         int lower_only, int pad_mode, double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad, hipStream_t s,
                         Profiler *prof, int deriv = -1);
constexpr int PER_KC = 8;                        // parameters per sweep of the gradient pass
constexpr int PER_NC = 3 * PER_KC + 2;           // sums per sweep: S_0, (A_k, B_k, C_k) of the sweep's k, T
// the gradient pass alone (raw_nll_grad_sums): partial [sweeps, npad / 8, PER_NC]; sweeps = ceil(d / PER_KC)
int launch_periodic_nll_grad(const double *Kinv, int64_t ld, int64_t n, int64_t npad, const PeriodicData *pd, const double *alpha,
                             double *partial, hipStream_t s);

// ---- MaternCovariance (matern.hip): ARD Matern with nu = 3/2 or 5/2 -------------------------------------------------------
// theta = (log v, log vt, log w_1..d).  par [d]: w.
struct MaternData : RawModel {
    int nu2 = 5;              // 2 nu: 3 or 5
    double w[GPX_MAX_D];      // exp(theta)
    MaternData() : RawModel(KernelKind::Matern) {}
};
int matern_parse(const double *theta, int d, int nu2, MaternData *out);    // host; GPX_ERR_BAD_ARG with text
// out[i][j] = Kf(q_ij) (+ vt where x_i == x_j in every component) (+ add_diag where row == col), q = sum_k w_k delta_k^2, from the raw
// inputs; lower_only / pad_mode / padding contract as launch_gram.  deriv >= 0: d K / d theta_deriv instead (no add_diag)
int launch_matern_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, const MaternData *md, double add_diag, int lower_only,
                       int pad_mode, double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad, hipStream_t s, Profiler *prof, int deriv = -1);
constexpr int MAT_KC = 8;                        // coordinates per sweep of the gradient pass
constexpr int MAT_NC = MAT_KC + 2;               // sums per sweep: S_0, A_k of the sweep's k, T
// the gradient pass alone (raw_nll_grad_sums): partial [sweeps, npad / 8, MAT_NC]; sweeps = ceil(d / MAT_KC)
int launch_matern_nll_grad(const double *Kinv, int64_t ld, int64_t n, int64_t npad, const MaternData *md, const double *alpha, double *partial,
                           hipStream_t s);

// ---- kernels / host launchers implemented across the .hip files -------------------------------
int launch_gram(const double *xi_w, int64_t n1, const double *xj_w, int64_t n2, int d, double v, double add_diag,
                int lower_only, int pad_mode, double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad,
                hipStream_t s, Profiler *prof, const double *colscale = nullptr);   // colscale [n2] (optional): out[i][j] *= colscale[j]
// out[i][k] = (x[i][k] - origin[k]) * sw[k], zero rows in the padding (origin_dev == nullptr: no origin)
int launch_scale_rows(const double *x, int64_t n, int64_t npad, int d, const double *sw_dev, double *out, hipStream_t s,
                      const double *origin_dev = nullptr);
int launch_gemm_nt(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc,
                   int64_t M, int64_t N, int64_t K, double alpha, double beta, int lower_only,
                   hipStream_t s, Profiler *prof, int ktrim = 0, int tri = 0, int small_tiles = 0, int *variant = nullptr);
// narrow update + bulk SYRK of a panel as ONE trapezoid launch that counts its finished narrow tiles in *sig_dev (gemm.hip)
int launch_syrk_trap_signal(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M, int64_t off_cols, int64_t K,
                            double alpha, double beta, int *sig_dev, hipStream_t s, Profiler *prof, int64_t tri_cols = 0);
// batched form: problem z = (p, q), q < nq, has its operand at base + p * sp + q * sq (elements)
// tri (read from the A descriptor; square problems only): the contraction skips the zero part of one triangular operand
enum { GEMM_TRI_NONE = 0, GEMM_TRI_A_UPPER = 1, GEMM_TRI_A_LOWER = 2, GEMM_TRI_B_LOWER = 3, GEMM_TRI_B_LOWER_PAIRED = 4 /* internal */,
       GEMM_TRI_B_UPPER = 5, GEMM_TRI_B_UPPER_PAIRED = 6 /* internal */ };
struct GemmBatch { int nq; long sp, sq; int tri; };
// row reduction in a product's epilogue (gemm.hip, tile_row_reduce): y at C's first column, partial sums [row][nslots]
struct GemmReduce { const double *y = nullptr; double *p2 = nullptr, *py = nullptr; long slot0 = 0, nslots = 0; };
int launch_gemm_nt_tri_reduce(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M, int64_t N,
                              double alpha, const GemmReduce &red, hipStream_t s, Profiler *prof);
int launch_gemm_nt_batched(const double *A, int64_t lda, GemmBatch ba, const double *B, int64_t ldb, GemmBatch bb, double *C, int64_t ldc,
                           GemmBatch bc, int64_t M, int64_t N, int64_t K, double alpha, double beta, int64_t batch, hipStream_t s);
int launch_syrk_lower_splitk(const double *W, int64_t ldw, double *parts, int64_t m, int64_t kchunk, int nchunks, double alpha, hipStream_t s,
                             const double *W2 = nullptr);
int launch_potrf_leaf(double *A, int64_t ld, double *dinv, double *diag_out, int *info_dev, int col_offset,
                      hipStream_t s, Profiler *prof, int exclusive = 0);

// recursive blocked algorithms (chol.hip)
// after_fork: main-stream work that only the panels after the first depend on (called once, right after the first panel's
// chain has been forked off; with the single-stream schedules: before anything else)
constexpr int64_t CHOL_PANEL_COLS = 8 * 128;   // outer panel width (CHOL_NBP tiles)
int chol_factor(double *L, int64_t ld, int64_t nblk, double *Dinv, double *diagL, int *info_dev,
                hipStream_t s, hipStream_t s_pan, Profiler *prof, hipStream_t s_top = nullptr,
                const std::function<int()> *after_fork = nullptr,
                const std::function<int(int64_t, int64_t, bool)> *panel_final = nullptr);
// info_dev (device ints, zero before the call): [0] potrf status (1-based failing column), [1] STALL (an in-kernel wait of the
// look-ahead schedule expired: the factor is invalid, refit with chol_force_plain_schedule(true)); with s_pan != nullptr the schedule
// uses 4 + nblk + 8 ints of it.
void chol_probe_streams(hipStream_t s, hipStream_t s_pan, hipStream_t s_top);
void chol_concurrency_forget();
void chol_force_plain_schedule(bool on);
// panel_final(p, slack, last): queued on the main stream s at a point where the columns of the outer panels 0..p are final for work
// on s; slack = outer panels whose trailing update is still to come (small = the main stream is about to idle underneath the chain:
// the place for work that rides along), last = the factorisation has nothing more to queue
int chol_panel_factor(double *L, int64_t ld, int64_t nblk, int64_t B0, int64_t B1, double *Dinv, double *diagL,
                      int *info_dev, hipStream_t s, Profiler *prof);
int chol_panel_factor_piped(double *L, int64_t ld, int64_t nblk, int64_t B0, int64_t B1, double *Dinv, double *diagL,
                            int *info_dev, hipStream_t s, Profiler *prof, const double *P = nullptr, int64_t ldp = 0, int64_t kp = 0,
                            int64_t head_blocks = 0, hipStream_t s_head = nullptr, hipStream_t s_far = nullptr);
// Z[rows, c0*128 : c1*128) <- Z * L[c0:c1, c0:c1]^-T   (Z row-major, ldz)
int trsm_right_lt(double *Z, int64_t ldz, int64_t rows, const double *L, int64_t ldl, const double *Dinv,
                  int64_t c0, int64_t c1, hipStream_t s, Profiler *prof);
// out of place, in steps of whole diagonal squares (1024 columns) against their inverses: Zs[:, p0..p1) <- Z[:, p0..p1) L^-T
// (Z is consumed; p0, p1 in units of squares).  The solver must be prepared for the same factor.
struct TriSolver;
// red (optional; p2 / py zeroed by the caller, y = the vector at column 0, nslots = ldz / 64): every slab's leaf product also leaves the
// row sums  sum_c Zs_rc^2, sum_c Zs_rc y_c  of its columns in the slots of those columns
// emu (estimate_many only; a workspace grown by trsm_emu_need for at least these rows): the deep updates go through emu_gemm_nt_sub
// where emu_enabled(K) holds
struct EmuFrame;
int trsm_right_lt_squares(double *Z, double *Zs, int64_t ldz, int64_t rows, const TriSolver *ts, int64_t p0, int64_t p1,
                          hipStream_t s, Profiler *prof, const GemmReduce *red = nullptr, const EmuFrame *emu = nullptr);
void trsm_emu_need(EmuFrame &w, int64_t rows, const TriSolver *ts, int64_t p0, int64_t p1);
int launch_slab_reduce(const double *Zs, int64_t ldz, int64_t rows, int64_t width, const double *y, double *p2, double *py, int64_t nslots, int64_t slot,
                       hipStream_t s);
int launch_predict_finish(const double *p2, const double *py, int64_t nslots, int64_t m, double vplusvt, double *mean, double *var, hipStream_t s,
                          const double *kdiag = nullptr);
// squares [p0, p0 + np) of a factor inverted into caller buffers (tsolve.hip): pl / pz [np][1024][1024], scratch tt [np][512][512]
int invert_squares_into(const double *L, int64_t ld, int64_t nblk, const double *Dinv, int64_t p0, int64_t np, double *pl, double *pz, double *tt,
                        hipStream_t s);
int build_kinv_from_factor(const double *L, int64_t ld, int64_t nblk, const double *Dinv, double *Z, double *Kinv,
                           hipStream_t s, Profiler *prof);
// the same from a prepared few-vector solver: its inverted 1024 x 1024 diagonal squares are the leaves (tsolve.hip); Kinv doubles as scratch
int build_kinv_from_solver(const TriSolver *ts, double *Z, double *Kinv, hipStream_t s, Profiler *prof);
int build_linv_t_squares(const TriSolver *ts, double *A, double *Z, hipStream_t s, Profiler *prof);
// Z [npad, npad] <- L^-T (upper triangular, row-major) from the factor and its inverted diagonal blocks
int build_linv_t(const double *L, int64_t ld, int64_t nblk, const double *Dinv, double *Z, hipStream_t s, Profiler *prof);
int launch_logdet(const double *diagL, int64_t n, double *out_dev, hipStream_t s);
int launch_predict_reduce(const double *Z, int64_t ldz, int64_t m, int64_t npad, const double *y, double vplusvt,
                          double *mean, double *var, hipStream_t s, Profiler *prof, const double *kdiag = nullptr);
int launch_set_identity(double *Z, int64_t ld, int64_t n, hipStream_t s);
int launch_symmetrize_lower(double *A, int64_t ld, int64_t n, hipStream_t s);

// device selection (runtime.hip): hipSetDevice to the calling thread's gpx_set_device choice, gfx950 only
int gpx_require_device();
int gpx_thread_device();   // the calling host thread's gpx_set_device choice

// caching device allocator, stream cache and pinned staging blocks (runtime.hip)
int dalloc(double **p, int64_t elems);
void dfree(void *p);   // the caller guarantees that no kernel still uses p
hipStream_t stream_acquire(int high_priority);
void stream_release(hipStream_t s, int high_priority);
double *pinned_acquire();
void pinned_release(double *p);

// The pool blocks a call takes for its own duration.  They go back to the pool in the destructor, after ONE synchronisation of
// the stream the call queues on: no kernel still uses a block when it returns to the pool, on whichever path the call ends.
// (An owner that holds nothing has nothing to wait for.)
struct Scratch {
    hipStream_t s;
    std::vector<void *> blocks;
    explicit Scratch(hipStream_t s_) : s(s_) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch()
    {
        if (!blocks.empty()) (void)wait_and_free();
    }
    // the same before the scope ends, for a call that needs the wait's status (or reads what the stream copied to the host)
    hipError_t wait_and_free()
    {
        const hipError_t e = hipStreamSynchronize(s);
        for (void *p : blocks) dfree(p);
        blocks.clear();
        return e;
    }
    // *p <- count elements of T (double, or the int status words and int8_t residues that share the pool of doubles)
    template <class T> int take(T **p, int64_t count)
    {
        double *q = nullptr;
        *p = nullptr;
        GPX_TRY(dalloc(&q, (count * (int64_t)sizeof(T) + 7) / 8));
        blocks.push_back(q);
        *p = reinterpret_cast<T *>(q);
        return 0;
    }
    // a block that outlives the call (committed to a handle on success) leaves the scope
    double *release(double *p) { blocks.erase(std::find(blocks.begin(), blocks.end(), (void *)p)); return p; }
};

// fp64 product emulated on int8 matrix cores (emu.hip, Ozaki scheme II): C[rows, cols] -= A[rows, K] B[cols, K]^T, row-major;
// K a multiple of 128 below 2^17.  emu_enabled(K): GPX_EMU_F64 (default 1) and K >= GPX_EMU_MIN_K (default 4096); the path depends on K only.
bool emu_enabled(int64_t K);
int emu_moduli();                        // GPX_EMU_MODULI (default 16, 2 .. 16)
constexpr int EMU_SLAB = 1024;           // columns of a slab of the left-looking solve (tsolve.hip: PB) and of a column panel of the symmetric update
// One operand as emu_i8_gemm_kernel reads it: plane l at res + l plane, rows ld bytes apart; the rows' scale exponents (for the rebuild).
struct EmuOperand { const int8_t *res; int64_t ld, plane; const int *scale; };
// A tiled residue image [row tile][l][rt][ld] of rows_pad rows, a row tile's planes at most 2 GiB; from_row: rows `row` .. the end of their tile
struct EmuImage {
    int8_t *base = nullptr;
    int64_t ld = 0, rt = 0, tiles = 0, rows_pad = 0, L = 0;   // row stride (bytes), rows per tile, tiles, padded rows, moduli
    int64_t plane() const { return rt * ld; }
    int8_t *tile(int64_t t) const { return base + t * plane() * L; }
    EmuOperand from_row(int64_t row, const int *sig) const { return {tile(row / rt) + row % rt * ld, ld, plane(), sig + row}; }
};
// A plan is a pure function of a shape: the geometry of A's image, the rows ct of B's column tile, the bits of either role, and what the
// shape needs: bytes of the image, of B's tile and of a tile pair's product residues, the number of scales (ints) and of row bounds (doubles).
struct EmuNeed { int64_t img = 0, b = 0, r = 0, sig = 0, bound = 0; };
struct EmuPlan { EmuImage a; int64_t ct = 0; int abits = 0, bbits = 0; EmuNeed need; };
// The workspace of all three drivers: the plan in use and the blocks held.  reserve() grows what emu_alloc will take so that it covers a
// plan; use() sets the geometry of the next update on the blocks held (every driver checks that they cover it).  emu_alloc takes every
// block of `held` from the pool or none: sc owns them from there on and gives them back, without one the caller does (emu_free).
struct EmuFrame : EmuPlan {
    EmuNeed held;                          // what reserve() has grown and emu_alloc took
    int8_t *rb = nullptr, *rr = nullptr;   // B's tile, the product residues (the image is a.base)
    int *sig = nullptr;                    // the scales of A's rows_pad rows, then of B's tile, then the left-looking solve's status word
    double *bound = nullptr;               // the left-looking solve's row bounds (callers that derive them on the device)
    void reserve(const EmuPlan &p);
    void use(const EmuPlan &p) { int8_t *img = a.base; static_cast<EmuPlan &>(*this) = p; a.base = img; }
    int *status() const { return sig + a.rows_pad + EMU_SLAB; }
};
int emu_alloc(EmuFrame &w, Scratch *sc);
void emu_free(EmuFrame &w);
EmuPlan emu_work_plan(int64_t rows, int64_t cols, int64_t K);   // the recursion's update: reserve the plan of every shape to come
int emu_gemm_nt_sub(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t rows, int64_t cols, int64_t K,
                    const EmuFrame &w, hipStream_t s, Profiler *prof);
// The symmetric update of the factorisation's far columns: C[i, j] -= sum_k A[i, k] A[j, k], j <= i < rows, by column panels of 1024 from ONE
// image of A (ld = K).  Reserve the largest update's plan, emu_alloc, use each update's plan before its split; then the column panels in
// ascending order, each on the stream the caller picks (a panel reads the image and the scales, and writes its own columns of C only).
EmuPlan emu_syrk_plan(int64_t rows, int64_t K, int64_t tile_rows = 0);
int emu_syrk_split(const EmuFrame &w, const double *A, int64_t lda, int64_t rows, hipStream_t s);
int emu_syrk_panel(const EmuFrame &w, int64_t q, double *C, int64_t ldc, int64_t rows, hipStream_t s, Profiler *prof, int diag_tile = 1);
// The left-looking many-row solve (tsolve.hip, trsm_right_lt_slabs): every solved slab is split ONCE into a persistent image (ld = 1024
// (slabs - 1)) with a row scale derived from a bound on the whole solved row; slab p then takes one update of depth 1024 p.  tile_rows > 0:
// a smaller row tile, for tests; begin: a chunk's scales from its bounds, the status word cleared (non-zero afterwards: discard the chunk).
EmuPlan emu_left_plan(int64_t rows, int64_t slabs, int64_t tile_rows = 0);
int emu_left_begin(const EmuFrame &w, const double *bound, int64_t rows, hipStream_t s);
int emu_left_split(const EmuFrame &w, const double *X, int64_t ldx, int64_t rows, int64_t q, hipStream_t s);
int emu_left_update(const EmuFrame &w, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t rows, int64_t cols, int64_t K, hipStream_t s,
                    Profiler *prof);
// Zs <- Z L^-T over all slabs of the solver's factor, left-looking from slab 4 on (slabs 0 .. 3 as trsm_right_lt_squares, their updates
// emulated through emu where emu_enabled(K) holds: with the default GPX_EMU_MIN_K none of them); w: planned and allocated for at least
// these rows, begun with their bounds
int trsm_right_lt_slabs(double *Z, double *Zs, int64_t ldz, int64_t rows, const TriSolver *ts, hipStream_t s, Profiler *prof, const GemmReduce *red,
                        const EmuFrame &w, const EmuFrame *emu = nullptr);
int launch_row_bounds(const double *kdiag, double v, int64_t m, double *bound, hipStream_t s);   // bound_i = sqrt(kdiag_i), or sqrt(v) without kdiag
// The two fall-back decisions of the route, apart from the image that does not fit (emu_alloc).  Which solves take it: the caller bounds
// every solved row, the many-row solver runs (not the few-vector one) against prepared squares over five slabs or more, and the switches
// allow it -- the factor's shape and the kind of call alone, never the number of rows beyond `few`.
bool emu_left_route(bool bounded, bool few, bool ready, int64_t slabs);
// One chunk under the guard: pass(left, &status) fills, solves and synchronises the chunk, left-looking first where use_left holds, and
// leaves the status word it read in status; a word that is raised (a bound did not hold) sends the chunk through pass(false) once more.
template <class Pass> int emu_left_guarded(bool use_left, Pass pass)
{
    for (int p = 0; p < 2; ++p) {
        const bool left = use_left && p == 0;
        int status = 0;
        GPX_TRY(pass(left, &status));
        if (!left || !status) break;
    }
    return 0;
}

// ---- launchers of propagate.hip ----------------------------------------------------------------
int launch_nll_grad(const double *Kinv, int64_t ld, int64_t n, int64_t npad, int d, const double *alpha, const double *xw,
                    double v, double *partial, double *out_dev, int *dmax_used, hipStream_t s, Profiler *prof);
int launch_sum_columns(const double *partial, int64_t nb, int nc, double *out_dev, hipStream_t s);   // out[c] = sum_b partial[b][c], fixed order
int launch_kinv_pass(const double *Kinv, int64_t ld, int64_t npad, int nc, const double *V, double *KV, hipStream_t s,
                     Profiler *prof, int64_t nrows = 0);
int launch_dot_pairs(const std::vector<std::pair<const double *, const double *>> &pr, long n, double *out_dev, hipStream_t s);
int launch_exact_sum(const double *Kinv, int64_t ld, int64_t npad, int d, const double *beta, const double *aT,
                     const double *bT, const double *e, const double *F, double *partial, double *out_dev, hipStream_t s,
                     Profiler *prof, int64_t row0 = 0, int64_t row1 = 0);
int launch_approx_build(const double *x, int64_t n, int64_t npad, int d, const double *u_dev, const double *w_dev, double v,
                        double vt, double *VM, double *AUX, double *cplain, hipStream_t s);
int launch_trace(const double *x, int64_t n, int64_t npad, int d, const double *u_dev, const double *w_dev,
                 const double *Sigma_dev, const double *cplain, double *tr, hipStream_t s);
int launch_cjh(const double *x, int64_t n, int d, const double *u_dev, const double *w_dev, double v, double vt, double *C,
               double *J, double *H, hipStream_t s);
// The right-hand-side rows of nb inputs in the row layout `layout` (GPX_ROWS_*) into Z [rows_pad, npad], the rest of the last 128-row tile
// cleared: the one launcher of every build kernel (frame: rows_tile.h).  nu2 = 0: the Gaussian kernel (propagate.hip), 3 / 5: Matern
// (matern.hip; nu2 = 3: GPX_ROWS_GRAD alone).  Sigma is read for GPX_ROWS_APPROX alone.
int launch_rows_build(int nu2, int layout, const double *x, int64_t n, int64_t npad, int d, const double *U_dev, const double *Sigma_dev,
                      int64_t sigma_stride, int64_t nb, int64_t rows_pad, const double *w_dev, double v, double vt, double *Z, hipStream_t s,
                      Profiler *prof);
// a build kernel by its parameter list (the kernels keep the lists they had): exactly one is set, neither where there is no such kernel
struct RowsKernel {
    void (*with_sigma)(const double *, long, long, int, const double *, const double *, long, long, const double *, double, double, double *);
    void (*plain)(const double *, long, long, int, const double *, long, const double *, double, double, double *);
};
RowsKernel matern_rows_kernel(int nu2, int layout, bool regs);   // matern.hip's kernels of the launcher's table; regs: d <= 8
int launch_approx_reduce_many(const double *Zs, int64_t npad, int d, const double *y, const double *Sigma_dev, int64_t sigma_stride,
                              int64_t nb, double vplusvt, double *out, int64_t ldo, hipStream_t s, Profiler *prof);
// the pair form (a model held as K^-1, not as a factor): R = the built rows, Y = R K^-1, alpha = K^-1 t; v.Kinv v = r_v.y_v, beta.v = r_v.alpha,
// tr.Kinv C = y_C.r_tr
int launch_approx_reduce_many_pair(const double *R, const double *Y, int64_t npad, int d, const double *alpha, const double *Sigma_dev,
                                   int64_t sigma_stride, int64_t nb, double vplusvt, double *out, int64_t ldo, hipStream_t s, Profiler *prof);
// ---- launchers of predict_grad.hip: the predictor's input gradients ----
// mean [nb] and dmean [nb, d] from alpha alone (nu2 = 0: the Gaussian kernel, 3 / 5: Matern; x raw); partial [S, nb, 1 + d] scratch with
// S = predict_mean_grad_splits(nb, npad); either output may be null
int predict_mean_grad_splits(int64_t nb, int64_t npad);
int launch_predict_mean_grad(const double *x, int64_t n, int64_t npad, int d, int nu2, const double *U_dev, int64_t nb, const double *w_dev,
                             const double *alpha, double v, double vt, int S, double *partial, double *mean_dev, double *dmean_dev, hipStream_t s,
                             Profiler *prof);
// the row products of the solved block [C, J_1..J_d] per query: mean, var [nb], dmean (or null), dvar [nb, d]
int launch_grad_reduce_many(const double *Zs, int64_t npad, int d, const double *y, int64_t nb, double vplusvt, double *mean, double *var,
                            double *dmean, double *dvar, hipStream_t s, Profiler *prof);
// the pair form: R = the built rows [C, J_1..J_d], Y = R K^-1, alpha = K^-1 t
int launch_grad_reduce_many_pair(const double *R, const double *Y, int64_t npad, int d, const double *alpha, int64_t nb, double vplusvt, double *mean,
                                 double *var, double *dmean, double *dvar, hipStream_t s, Profiler *prof);
// batched inverse propagation (gpx_propagate_dvh_many): rows [C, J_1..J_d, H_11..H_dd] per input; dvh [nb, d], sigma2 [nb] or null
int launch_dvh_reduce_many(const double *Zs, int64_t npad, int d, const double *y, int64_t nb, double vplusvt, double *dvh, double *sigma2,
                           hipStream_t s, Profiler *prof);
int launch_exact_build(const double *x, int64_t n, int64_t npad, int d, const double *u_dev, const double *w_dev,
                       const double *Ls_dev, const double *dinv_diag_dev, double v, double vt, double nc1, double *aT,
                       double *bT, double *e, double *F, double *lm, hipStream_t s);
int launch_exact_build_generic(const double *x, int64_t n, int64_t npad, int d, const double *u_dev, const double *Ls_dev,
                               const double *dinv_diag_dev, const double *C_dev, double nc1, double *aT, double *bT, double *e, double *F,
                               double *lm, hipStream_t s);

// batched Exact (gpx_propagate_exact_many): coordinates transformed for a signed sum of squares, the weighted lower half of K^-1,
// a slab's H and mean partials (H == nullptr: the means alone), the row products with Y = H Lo^T
int launch_exact_many_transform(const double *x, int64_t n, int64_t npad, int d, const double *x0_dev, const double *T_dev, double *out,
                                hipStream_t s);
int launch_exact_weight(const double *Kinv, int64_t ld, int64_t n, int64_t npad, int d, const double *beta, const double *xt,
                        const double *sgn_dev, double *Lo, hipStream_t s, Profiler *prof);
int launch_exact_many_build(const double *x, const double *xh, int64_t n, int64_t npad, int d, const double *U_dev, const double *Uh_dev,
                            int64_t nb, int64_t rows_pad, const double *w_dev, const double *dinv_diag_dev, const double *sgn_dev,
                            const double *beta, double v, double vt, double nc1, double *H, double *mpart, hipStream_t s, Profiler *prof);
int launch_exact_many_finish(const double *Y, const double *H, int64_t npad, const double *mpart, int64_t nb, double vplusvt, double nc2,
                             double *out, int64_t ldo, hipStream_t s, Profiler *prof);
// the gradients of the batched Exact moments (gpx_propagate_exact_grad_many; exact_grad.hip): a slab's 2 d + 1 rows [h, p_1..p_d, c_1..c_d]
// per input and the partials of the 2 d + 1 mean sums (H == nullptr: those alone), and the six outputs from the rows and Y = H Lo^T;
// out = [mean | var | dmean_du | dvar_du | dmean_ds | dvar_ds], blocks of ldo inputs, the slab's first input at o0
int launch_exact_grad_build(const double *x, const double *xh, int64_t n, int64_t npad, int d, const double *U_dev, const double *Uh_dev,
                            int64_t nb, int64_t rows_pad, const double *w_dev, const double *dinv_diag_dev, const double *Dk_dev,
                            const double *sgn_dev, const double *Bm_dev, const double *beta, double v, double vt, double nc1, double *H,
                            double *mpart, hipStream_t s, Profiler *prof);
int launch_exact_grad_finish(const double *Y, const double *H, int64_t npad, int d, const double *mpart, int64_t nb, double vplusvt, double nc2,
                             const double *nq_dev, double *out, int64_t ldo, int64_t o0, hipStream_t s, Profiler *prof);

// ---- host orchestration shared by fit.hip, predict.hip and propagate_api.hip ---------------------
// (helpers, not interface: they stay out of the library's dynamic symbol table)
#pragma GCC visibility push(hidden)
// Every entry point that takes a gpx_handle begins with one of the two.  CHECK_H refuses a pseudo-input model (no_factor): whatever the
// entry point goes on to read -- L, Dinv, tri, y, t -- is null there, so refusal is the default and serving it is the exception that an
// entry point states by name (CHECK_H_PSEUDO_OK), after its body has been read for uses of the factor.
#define CHECK_H_PSEUDO_OK(h)                                        \
    do {                                                            \
        if (!(h)) { gpx_set_error("null handle"); return GPX_ERR_BAD_ARG; } \
        GPX_HIP(hipSetDevice((h)->device));                         \
    } while (0)
#define CHECK_H(h)                                                  \
    do {                                                            \
        CHECK_H_PSEUDO_OK(h);                                       \
        if ((h)->no_factor) {                                       \
            gpx_set_error("%s: the handle is a pseudo-input model (gpx_spgp_pseudo_handle): it holds beta and P, no factor, no targets", __func__); \
            return GPX_ERR_STATE;                                   \
        }                                                           \
    } while (0)
// ---- the one description of a handle's kernel (KernelKind) ----
static inline bool handle_has_kernel(const gpx_handle *h) { return h->kind != KernelKind::Matrix; }
static inline int handle_dim(const gpx_handle *h) { return h->raw ? h->raw->d : h->d; }   // 0: a supplied matrix
// the training inputs [n, handle_dim] in the form the handle's Gram kernel reads: scaled by sqrt(w) (Gaussian), raw (periodic, Matern)
static inline const double *handle_train_inputs(const gpx_handle *h) { return h->raw ? h->raw->x : h->xs_w; }
// does the handle's Gram kernel add vt wherever two rows are equal (the prior variance of a query is then v + vt also for its bound)
static inline bool handle_gram_has_vt(const gpx_handle *h) { return h->raw != nullptr; }
// the kind's own host fields (w / p / w2; nu2) of a handle of that kind
static inline const PeriodicData *handle_periodic(const gpx_handle *h)
{
    assert(h->kind == KernelKind::Periodic && h->raw && h->raw->kind == h->kind);
    return static_cast<const PeriodicData *>(h->raw);
}
static inline const MaternData *handle_matern(const gpx_handle *h)
{
    assert(h->kind == KernelKind::Matern && h->raw && h->raw->kind == h->kind);
    return static_cast<const MaternData *>(h->raw);
}
// what the builders of C(u, x_i) add where u equals row i elementwise (the reference's scalar kernel, Covariance.py:440-451): vt on a fitted
// model, whose rows are observations; 0 on a pseudo-input model -- a pseudo-input is no observation and SPGP's k(x*) = K(x*, xbar) never
// carries vt.  The prior variance v + vt is not affected.
static inline double handle_vt_on_equal(const gpx_handle *h) { return h->no_factor ? 0.0 : h->vt; }
// launch_gram / launch_raw_gram with the handle's parameters; xi, xj in the form of handle_train_inputs
static inline int handle_gram(const gpx_handle *h, const double *xi, int64_t n1, const double *xj, int64_t n2, double add_diag, int lower_only,
                              int pad_mode, double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad, hipStream_t s, Profiler *prof)
{
    if (h->raw) return launch_raw_gram(xi, n1, xj, n2, h->raw, add_diag, lower_only, pad_mode, out, ld, rows_pad, cols_pad, s, prof);
    if (h->kind == KernelKind::Gaussian) return launch_gram(xi, n1, xj, n2, h->d, h->v, add_diag, lower_only, pad_mode, out, ld, rows_pad, cols_pad, s, prof);
    gpx_set_error("handle_gram: the handle was built from a supplied matrix");
    return GPX_ERR_STATE;
}
// The refusals of a handle of the wrong kind, once, from the names of a raw-input kind: its class <cls>Covariance, its entry points gpx_<fn>_*.
struct KindName { const char *cls, *fn; };
static inline KindName kind_name(KernelKind k) { return k == KernelKind::Periodic ? KindName{"Periodic", "periodic"} : KindName{"Matern", "matern"}; }
// an entry point of one raw-input kind (what) on a handle of another
static inline int need_kind(const gpx_handle *h, KernelKind kind, const char *what)
{
    if (h->kind == kind) return 0;
    gpx_set_error("%s: not a gpx_%s_fit handle", what, kind_name(kind).fn);
    return GPX_ERR_STATE;
}
// entry points that evaluate the GaussianCovariance kernel need the handle's inputs and theta: not a raw-input or gpx_fit_matrix handle
static inline int need_kernel(const gpx_handle *h, const char *what)
{
    if (h->kind == KernelKind::Gaussian) return 0;
    const KindName nm = kind_name(h->kind);
    if (h->raw) gpx_set_error("%s: the handle holds a %sCovariance model (gpx_%s_fit): use the gpx_%s_* entry points", what, nm.cls, nm.fn, nm.fn);
    else gpx_set_error("%s: the handle was built from a supplied matrix (gpx_fit_matrix): no inputs / theta to evaluate the kernel on", what);
    return GPX_ERR_STATE;
}
#define NEED_KERNEL(h, what) GPX_TRY(need_kernel(h, what))

int fetch_small(double *dst, const double *src, size_t n);   // a few doubles from a caller's pointer (host or device) into host memory (runtime.hip)
int ensure_Z(gpx_handle *h, int64_t rows);
int ensure_kinv(gpx_handle *h);
int ensure_kinv_rows(gpx_handle *h, int64_t row0, int64_t row1, const double **base);
int check_row_range(const gpx_handle *h, int64_t row0, int64_t row1, const char *what);   // of the row-sharded entry points (predict.hip)

// The many-right-hand-side solve behind gpx_predict / gpx_predict_kv and gpx_propagate_approx_many (predict.hip): rows of h->Z (leading
// dimension npad, zero padded to the 128-row tile) -> Zs = Z L^-T, in chunks of `chunk` rows.  begin sizes the chunk and takes Z, Zs and
// the emulated updates' workspace once per call; run solves one chunk; the buffers (and whatever else the caller takes from sc) go back
// with the RowSolve.
struct RowSolve {
    Scratch sc;
    int64_t chunk = 0;
    bool few = false;       // a handful of rows: the few-right-hand-side solver (one sweep over the factor's triangle)
    double *Zs = nullptr;   // [chunk, npad]
    EmuFrame ew;
    const EmuFrame *emu = nullptr;
    EmuFrame left;           // the left-looking order's residue image and the chunk's row bounds (device), when the caller bounds its rows
    bool use_left = false;
    explicit RowSolve(hipStream_t s) : sc(s) {}
};
// bounded: the caller will give a bound on every solved row (left = true in row_solve_run after emu_left_begin with rs.left.bound filled)
// allow_few = false: the many-row solver whatever m is (a caller that promises results independent of the batch); chunk_cap > 0: at
// most that many rows a chunk (a multiple of 128)
int row_solve_begin(gpx_handle *h, int64_t m, RowSolve &rs, bool bounded = false, bool allow_few = true, int64_t chunk_cap = 0);
int64_t row_solve_chunk_cap(const gpx_handle *h, int64_t chunk_cap = 0);   // the most rows of a chunk (a multiple of 128)
// Zs[0 : mp) <- Z[0 : mp) L^-T (mc real rows, mp = mc rounded up to the tile); red: the fused row sums of tsolve.hip (many rows only)
int row_solve_run(gpx_handle *h, const RowSolve &rs, int64_t mc, int64_t mp, const GemmReduce *red, bool left = false);

// The chunk loop of the five batched row calls (rows_many_run, propagate_api.hip) under its three names, one per row layout, for any kernel
// that has the right-hand sides: build(U_dev, Sigma_dev, sigma_stride, bc, mp) writes the rows of bc inputs into h->Z [mp, npad] (Sigma for
// GPX_ROWS_APPROX alone); the solve or the product with K^-1, the row reductions and the copies are the loop's own.
using RowsBuild = std::function<int(const double *, const double *, int64_t, int64_t, int64_t)>;
// The build of the handle's kind for a row layout (GPX_ROWS_*): the ONE caller of launch_rows_build, for the five batched entry points and
// for gpx_rows_build alike.  The caller has checked that the kind has the layout (Gaussian: all; Matern 5/2: all; 3/2: GRAD).
RowsBuild rows_build_of(gpx_handle *h, int layout);
int approx_many_run(gpx_handle *h, int d, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *mean, double *var, double *sigma2,
                    double *rest, const char *what, const RowsBuild &build);
int dvh_many_run(gpx_handle *h, int d, const double *U, int64_t b, double *dvh_out, double *sigma2_out, const char *what, const RowsBuild &build);
// the same loop on d + 1 rows a query, [C, J_1..J_d] (no Sigma): gpx_predict_grad's mean, var [b], dmean (or null), dvar [b, d]
int grad_many_run(gpx_handle *h, int d, const double *U, int64_t b, double *mean, double *var, double *dmean, double *dvar, const char *what,
                  const RowsBuild &build);

// The predictor's chunk loop on device-resident queries and outputs (predict.hip): begin sizes the chunk as gpx_predict does (bounded rows;
// a periodic handle: the many-row solver always, and its chunk cap) and takes the query, prior-variance and partial-sum buffers; chunk
// runs load -> (scale, Gaussian alone) -> handle_gram -> guarded solve -> row reduction for one chunk.  gpx_predict, gpx_predict_kv,
// gpx_periodic_predict and gpx_propagate_quadrature_many all go through it.
struct PredictRun {
    RowSolve rs;
    bool from_x = false, fused = false;
    bool periodic = false;   // from_x on a periodic handle: the rows carry +vt on equality, results independent of the batch (predict.hip)
    int64_t nslots = 0;
    double *xq = nullptr, *xqw = nullptr, *kd = nullptr, *part = nullptr;   // [chunk, d] queries, the same scaled (Gaussian), [chunk] prior variances, fused row sums
    explicit PredictRun(hipStream_t s) : rs(s) {}
};
int predict_run_begin(gpx_handle *h, bool from_x, int64_t m, PredictRun &pr);
int predict_run_chunk(gpx_handle *h, PredictRun &pr, int64_t m0, int64_t mc, const std::function<int(int64_t, int64_t)> &load, double *mean_dev,
                      double *var_dev, const std::function<hipError_t()> &done);

// ---- numerical propagation (quadrature.hip) ----
// X [rows, d] <- rows row0 .. row0 + rows of the node set: X[i S + s][k] = U[i][k] + sum_e A_i[k][e] z[s][e]; a_stride = 0: one A for all inputs
int launch_quad_nodes(const double *U, const double *A, int64_t a_stride, const double *z, int64_t S, int d, int64_t row0, int64_t rows, double *X,
                      hipStream_t s, Profiler *prof);
// mom [5, b] = m | var | Ev | m3 | m4 and dens [b, ny] (ny > 0) of the b mixtures of S Gaussians (mu, var [b S], weights wq [S]); everything on the
// device; y_stride = 0: one y [ny] for all inputs, ny: one row per input.  Work buffers come from sc.
int launch_mixture_reduce(const double *mu, const double *var, const double *wq, int64_t S, int64_t b, const double *y, int64_t ny, int64_t y_stride,
                          double shift, double *mom, double *dens, Scratch &sc, Profiler *prof);
#pragma GCC visibility pop
