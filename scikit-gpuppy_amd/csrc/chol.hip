// chol.hip -- blocked fp64 Cholesky, triangular solves and their leaf kernels for gfx950.
//
// Replaces the reference's dense-LA call sites on the hot path: scipy.linalg.inv (LU, 2N^3 flop) at
// skgpuppy/Covariance.py:179 (+ the jittered-Cholesky fallback :182-185), np.linalg.slogdet at :195 and
// the Kinv GEMV/GEMMs at skgpuppy/GaussianProcess.py:77-78,114-119.  K = L L^T is factored once
// (N^3/3 flop); everything downstream solves against L.
//
// Structure: two-level right-looking factorisation with look-ahead down to 128x128 diagonal blocks.  All O(N^3)
// work is issued as calls of the one MFMA GEMM (gemm.hip); the leaf (potrf_trtri128_elim_kernel) factors a diagonal
// block AND inverts its factor in one launch, both on MFMA out of LDS, so that every triangular solve against a
// diagonal block becomes a GEMM with its inverse.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <vector>

#include "common.h"

#include "leaf.h"

// (waves_per_eu 2..2: 185 VGPRs and NO accumulator registers -- without it the allocator books a granule of 32 AGPRs nothing uses, 224 in
// all, and the leaf no longer fits into the 216 registers per SIMD that the CU blockers leave: it then waits ~1 ms for a CU without
// any GEMM workgroup in every reserved panel (fit +1.5 ms; tests/test_kernel_resources.py guards the budget))
__attribute__((amdgpu_waves_per_eu(2, 2))) __global__ __launch_bounds__(256) void potrf_trtri128_elim_kernel(double *A, long ld, double *dinv, double *diag_out, int *info,
                                                                 int col_offset, int prio)
{
    __shared__ __attribute__((aligned(16))) double X[36 * XB];
    __shared__ int bad_s;
    if (prio) __builtin_amdgcn_s_setprio(3);
    leaf_elim_body(A, ld, dinv, diag_out, info, col_offset, X, &bad_s);
}

// exclusive: the launch asks for 52 KB of dynamic LDS on top of the kernel's 78 KB, so that no workgroup of any GEMM variant
// (>= 32 KB) can join it on its CU -- next to a bulk wave on every SIMD the leaf runs 3x slower.  Only where an empty CU is at
// hand: the first leaf of a panel (the main stream has just drained) and every leaf while CUs are reserved for the chain.
static void leaf_exclusive_setup()
{
    static const bool done = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(potrf_trtri128_elim_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 52 * 1024);
        return true;
    }();
    (void)done;
}

int launch_potrf_leaf(double *A, int64_t ld, double *dinv, double *diag_out, int *info_dev, int col_offset,
                      hipStream_t s, Profiler *prof, int exclusive)
{
    ProfScope ps(prof, s, GPX_K_POTRF_LEAF, (double)TILE * TILE * TILE);   // n^3/3 (potrf) + 2n^3/3 (inverse)
    if (exclusive) leaf_exclusive_setup();
    hipLaunchKernelGGL(potrf_trtri128_elim_kernel, dim3(1), dim3(256), exclusive ? 52 * 1024 : 0, s, A, (long)ld, dinv, diag_out, info_dev, col_offset, 1);
    GPX_HIP(hipGetLastError());
    return 0;
}

extern "C" int gpx_dev_potrf_leaf(double *A, int64_t ld, double *dinv, double *diag_out, int *info_dev, int col_offset,
                                  void *stream)
{
    return launch_potrf_leaf(A, ld, dinv, diag_out, info_dev, col_offset, (hipStream_t)stream, nullptr, 0);
}

// ------------------------------------------------------------------------------------------------
// recursive blocked Cholesky / TRSM (host side; block indices in units of 128)
// ------------------------------------------------------------------------------------------------
static inline int64_t split_point(int64_t nb)
{
    // largest power of two strictly below nb keeps the big GEMMs square-ish and aligned
    int64_t h = 1;
    while (h * 2 < nb) h *= 2;
    return h;
}

// Z[0:rows, c0:c1) <- Z[0:rows, c0:c1) * L[c0:c1, c0:c1]^-T      (block units for c0,c1; rows multiple of 128)
int trsm_right_lt(double *Z, int64_t ldz, int64_t rows, const double *L, int64_t ldl, const double *Dinv,
                  int64_t c0, int64_t c1, hipStream_t s, Profiler *prof)
{
    const int64_t nb = c1 - c0;
    if (nb <= 0 || rows <= 0) return 0;
    if (nb == 1) {
        double *Zc = Z + c0 * TILE;
        // in place: the single column tile of each block reads all its k before the epilogue writes
        return launch_gemm_nt(Zc, ldz, Dinv + c0 * (int64_t)TILE * TILE, TILE, Zc, ldz, rows, TILE, TILE, 1.0, 0.0, 0, s, prof);
    }
    const int64_t h = split_point(nb), cm = c0 + h;
    GPX_TRY(trsm_right_lt(Z, ldz, rows, L, ldl, Dinv, c0, cm, s, prof));
    // Z[:, cm:c1) -= Z[:, c0:cm) * L[cm:c1, c0:cm)^T
    GPX_TRY(launch_gemm_nt(Z + c0 * TILE, ldz, L + (cm * TILE) * ldl + c0 * TILE, ldl, Z + cm * TILE, ldz, rows,
                           (c1 - cm) * TILE, h * TILE, -1.0, 1.0, 0, s, prof));
    return trsm_right_lt(Z, ldz, rows, L, ldl, Dinv, cm, c1, s, prof);
}

// Z[0:c1*128, c0*128:c1*128) <- columns c0..c1 of L^-T, given that Z started as the identity and the columns left of
// c0 are done.  L^-T is upper triangular, so only the rows above the column range carry data: a third of the flops of
// the general TRSM on an N x N right-hand side.
static int trtri_upper_rec(double *Z, int64_t ldz, const double *L, int64_t ldl, const double *Dinv, int64_t c0, int64_t c1,
                           hipStream_t s, Profiler *prof)
{
    const int64_t nb = c1 - c0;
    if (nb <= 0) return 0;
    if (nb == 1) {
        double *Zc = Z + c0 * TILE;
        return launch_gemm_nt(Zc, ldz, Dinv + c0 * (int64_t)TILE * TILE, TILE, Zc, ldz, c1 * TILE, TILE, TILE, 1.0, 0.0, 0, s, prof);
    }
    const int64_t h = split_point(nb), cm = c0 + h;
    GPX_TRY(trtri_upper_rec(Z, ldz, L, ldl, Dinv, c0, cm, s, prof));
    // Z[0:cm, c0:cm) is upper triangular below row c0 (Z[r][k] = 0 for k < r): row tiles past c0 start their k loop at
    // their own first row (ktrim shift = c0 * 128) -- at the top level that halves the launch
    GPX_TRY(launch_gemm_nt(Z + c0 * TILE, ldz, L + (cm * TILE) * ldl + c0 * TILE, ldl, Z + cm * TILE, ldz, cm * TILE,
                           (c1 - cm) * TILE, h * TILE, -1.0, 1.0, 0, s, prof, (int)(c0 * TILE) + 1));
    return trtri_upper_rec(Z, ldz, L, ldl, Dinv, cm, c1, s, prof);
}

// Z (npad x npad) <- L^-T (upper triangular, row-major): identity, then the structured recursion above
int build_linv_t(const double *L, int64_t ld, int64_t nblk, const double *Dinv, double *Z, hipStream_t s, Profiler *prof)
{
    const int64_t npad = nblk * TILE;
    GPX_TRY(launch_set_identity(Z, npad, npad, s));
    return trtri_upper_rec(Z, npad, L, ld, Dinv, 0, nblk, s, prof);
}

// Kinv = L^-T L^-1 from the factor: Z (scratch, npad x npad) = L^-T, then Kinv[i,j] = sum_{k >= i} Z[i,k] Z[j,k] for the
// lower triangle in row strips of 1024 (the k range of a strip starts at its first row), mirrored to the upper one.
int build_kinv_from_factor(const double *L, int64_t ld, int64_t nblk, const double *Dinv, double *Z, double *Kinv,
                           hipStream_t s, Profiler *prof)
{
    const int64_t npad = nblk * TILE;
    GPX_TRY(build_linv_t(L, ld, nblk, Dinv, Z, s, prof));
    // ONE lower-only launch whose tile (by, bx) contracts over k >= 128 by only (Z is upper triangular): N^3/3 flop with
    // tiles of length 128 .. N dealt longest-first to whichever workgroup slot frees up (row strips of 1024 with a common
    // k range per strip ran at 49 TFLOP/s: the first strips have few tiles, the last ones short k)
    GPX_TRY(launch_gemm_nt(Z, npad, Z, npad, Kinv, npad, npad, npad, npad, 1.0, 0.0, 1, s, prof, 1));
    return launch_symmetrize_lower(Kinv, npad, npad, s);
}

static int chol_rec(double *L, int64_t ld, int64_t b0, int64_t b1, double *Dinv, double *diagL, int *info_dev,
                    hipStream_t s, Profiler *prof)
{
    const int64_t nb = b1 - b0;
    if (nb <= 0) return 0;
    if (nb == 1)
        return launch_potrf_leaf(L + (b0 * TILE) * ld + b0 * TILE, ld, Dinv + b0 * (int64_t)TILE * TILE,
                                 diagL + b0 * TILE, info_dev, (int)(b0 * TILE), s, prof, 0);
    const int64_t h = split_point(nb), bm = b0 + h;
    GPX_TRY(chol_rec(L, ld, b0, bm, Dinv, diagL, info_dev, s, prof));
    // A21 <- A21 L11^-T : rows [bm,b1), triangle [b0,bm)
    GPX_TRY(trsm_right_lt(L + (bm * TILE) * ld, ld, (b1 - bm) * TILE, L, ld, Dinv, b0, bm, s, prof));
    // A22 -= A21 A21^T (lower tiles only)
    const double *A21 = L + (bm * TILE) * ld + b0 * TILE;
    GPX_TRY(launch_gemm_nt(A21, ld, A21, ld, L + (bm * TILE) * ld + bm * TILE, ld, (b1 - bm) * TILE, (b1 - bm) * TILE,
                           h * TILE, -1.0, 1.0, 1, s, prof));
    return chol_rec(L, ld, bm, b1, Dinv, diagL, info_dev, s, prof);
}

// ------------------------------------------------------------------------------------------------
// Two-level right-looking Cholesky with look-ahead.
//   outer panels of CHOL_NBP blocks (1024 columns): the bulk trailing update is one K=1024 SYRK per panel on
//   the main stream; while it runs, the NEXT panel (already updated by a narrow GEMM issued first) is factored
//   on a second, high-priority stream -- the latency-bound chain  leaf -> panel TRSM -> in-panel update  (128
//   columns at a time) overlaps with the MFMA-bound bulk instead of serialising with it.
// The same outer structure is what the multi-GPU host drives (panel owner factors, RCCL broadcast, everybody
// updates): see skgpuppy_amd/distributed.py.
// ------------------------------------------------------------------------------------------------
constexpr int64_t CHOL_NBP = 8;

// dflow.hip: the trailing panels as one persistent dataflow kernel
int64_t chol_dataflow_state_ints(int64_t nbr);
int64_t chol_dataflow_table_ints(int64_t nbr);
bool chol_dataflow_supported(int64_t nbr);
int64_t chol_dataflow_word_steps();
int64_t chol_dataflow_word_colc(int64_t nbr, int64_t k);
int launch_chol_dataflow(double *L, int64_t ld, int64_t nb, int64_t c0, double *Dinv, double *diag, int *info_dev, int *state_dev,
                         std::vector<int> &host_tab, unsigned long long limit_ticks, hipStream_t s, int workers = 0, int exclusive = 0,
                         const int *tab_ready = nullptr, int first_rows = 0, int extra = 0, const int *gate = nullptr);
int chol_dataflow_fill_tables(int nbr, int first_rows, int *dst, int cap);

static_assert(CHOL_NBP * TILE == CHOL_PANEL_COLS, "common.h: CHOL_PANEL_COLS");

// the schedule's switches: integers from the environment, each read once per process by a one-line getter
static long env_long(const char *name, long dflt) { const char *e = getenv(name); return e ? atol(e) : dflt; }
// GPX_DEBUG: the probes' verdicts and the host's enqueue marks (Lookahead::mark) on stderr
static bool debug_enabled() { static const bool v = getenv("GPX_DEBUG") != nullptr; return v; }

// time limit of the in-kernel waits (GPX_WAIT_LIMIT_MS, default 5000): generous -- it only ever expires when streams that were
// probed as concurrent stop being so
static unsigned long long wait_limit_ticks()
{
    static const unsigned long long v = [] { const char *e = getenv("GPX_WAIT_LIMIT_MS"); const double ms = e ? atof(e) : 5000.0; return (unsigned long long)((ms > 0.01 ? ms : 0.01) * 1e5); }();
    return v;   // s_memrealtime ticks at 100 MHz
}

// holds its stream until the producer launch has counted `want` finished tiles in *ctr.  A time limit that expires (it never should:
// the producer does not depend on this stream) is reported through the factorisation's STALL word -- a word of its own, not the
// potrf status: a scheduling stall is not a non-positive pivot, and the caller answers it by refitting on the plain schedule, never
// with jitter (the consumers behind an expired wait read tiles that are not there: that factor is discarded).
__global__ void wait_count_kernel(const int *ctr, int want, unsigned long long limit_ticks, int *stall)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
        if (__builtin_amdgcn_s_memrealtime() - t0 > limit_ticks) {
            __hip_atomic_store(stall, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        __builtin_amdgcn_s_sleep(8);
    }
}

// that one-thread kernel queued on `on`: whatever follows on the stream runs once *counter has reached `want`
static int queue_wait(hipStream_t on, const int *counter, int want, int *stall, unsigned long long limit_ticks = wait_limit_ticks())
{
    hipLaunchKernelGGL(wait_count_kernel, dim3(1), dim3(1), 0, on, counter, want, limit_ticks, stall);
    GPX_HIP(hipGetLastError());
    return 0;
}

// The events of one factorisation: created through make(), destroyed with the owner -- by then the caller has waited for every stream
// that still refers to them, or has handed them on to a list that is swept later (retire_events).
struct Events {
    std::vector<hipEvent_t> all;
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { clear(); }
    void clear()
    {
        for (hipEvent_t e : all) (void)hipEventDestroy(e);
        all.clear();
    }
    int make(hipEvent_t *e)
    {
        GPX_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        all.push_back(*e);
        return 0;
    }
};

// Pipelining of the rows below a diagonal square ("top slice"): the rows [r0, r1) are solved against the square's triangle column by
// column on a second stream, each column as soon as the chain step that produces its diagonal-block inverse has finished -- instead
// of one recursive TRSM after the whole chain.
struct TopPipe {
    hipStream_t stream = nullptr;
    int64_t r0 = 0, r1 = 0;                 // block rows of the slice
    Events *events = nullptr;               // the caller's: they outlive the queued waits that refer to them
    const int *colsig = nullptr;            // column c of the slice may be read once colsig[c] has reached colwant (the trapezoid launch's
    int colwant = 0;                        // per-column counters); null: the stream is ordered behind the update some other way
    int *stall = nullptr;                   // the factorisation's stall word (an expired wait sets it)
    // right-looking mode (the panel's chain is a square launch of the dataflow kernel): column j is solved as soon as step j is counted in
    // sq_state, then applied to the panel's remaining columns (one K = 128 product over all of them) once the in-square solves of column j
    // are counted -- per step two short, wide launches instead of a product whose contraction grows with j
    const int *sq_state = nullptr;
    int64_t sq_rows = 0;                    // block rows of the square
    int64_t sq_nbr = 0;                     // block rows the square launch owns (its state layout: the square's + the rows it solves below)
    const TopPipe *next = nullptr;          // further slices of the same panel (other rows, other streams) that trail the same chain
    // the panel's chain is a square launch with these state words, `rows` block rows of square and `below` more that it solves itself
    void follow_square(const int *state, int64_t rows, int64_t below)
    {
        sq_state = state;
        sq_rows = rows;
        sq_nbr = rows + below;
    }
};

// a one-thread kernel that holds the slice's stream until the trapezoid launch has counted column c's narrow tiles (on the device it runs
// next to that launch)
static int colsig_wait(const TopPipe *top, int64_t c)
{
    static const bool force_stall = getenv("GPX_TEST_FORCE_STALL") != nullptr;   // test hook: the first wait of the process expires at once
    static bool forced = false;
    const bool force = force_stall && !forced;
    forced = forced || force;
    return queue_wait(top->stream, top->colsig + c, force ? 0x7fffffff : top->colwant, top->stall, force ? 1000ull : wait_limit_ticks());
}

// column j of the slice: X_j = (Z_j - X_{B0..j} L[j, B0..j)^T) Dinv_j^T   (left-looking, two small launches on top->stream)
// part: 0 both launches; 1 the update only -- it needs the columns before j and row j of the square's factor (chain step j - 1), NOT
// chain step j: queued in front of the stream's wait for step j it runs underneath that step's leaf, and only the solve (part 2; 13 us)
// follows the step (the last three column solves of a panel used to trail its chain by 290 us: update 50-67 us + solve per column)
static int top_column(double *L, int64_t ld, int64_t B0, int64_t j, const double *Dinv, const TopPipe *top, Profiler *prof, int part = 0)
{
    double *Zt = L + (top->r0 * TILE) * ld;
    const int64_t M = (top->r1 - top->r0) * TILE;
    if (top->sq_state && part == 1) return 0;   // (right-looking mode has no early part)
    if (top->colsig && part != 2) {
        // left-looking, step j touches column j only; right-looking (square launch) it updates every later column of the slice as
        // well: the first step waits for ALL of the trapezoid launch's column counters (waiting for column j alone raced with the narrow
        // tiles of the later columns once the trapezoid launch was queued behind the column solves of the panel before)
        if (!top->sq_state) GPX_TRY(colsig_wait(top, j - B0));
        else if (j == B0)
            for (int64_t c = 0; c < top->sq_rows; ++c) GPX_TRY(colsig_wait(top, c));
    }
    if (top->sq_state) {
        const int64_t B1 = B0 + top->sq_rows;
        GPX_TRY(queue_wait(top->stream, top->sq_state + chol_dataflow_word_steps(), (int)(j - B0 + 1), top->stall));
        GPX_TRY(launch_gemm_nt(Zt + j * TILE, ld, Dinv + j * (int64_t)TILE * TILE, TILE, Zt + j * TILE, ld, M, TILE, TILE, 1.0, 0.0, 0, top->stream, prof));
        if (j + 1 < B1) {
            GPX_TRY(queue_wait(top->stream, top->sq_state + chol_dataflow_word_colc(top->sq_nbr, j - B0), (int)(4 * (B1 - 1 - j)), top->stall));
            // Z[:, j+1 .. B1) -= X_j L[j+1 .. B1, j]^T
            GPX_TRY(launch_gemm_nt(Zt + j * TILE, ld, L + ((j + 1) * TILE) * ld + j * TILE, ld, Zt + (j + 1) * TILE, ld, M, (B1 - 1 - j) * TILE, TILE,
                                   -1.0, 1.0, 0, top->stream, prof, 0, 0, 1));   // (64 x 64 tiles)
        }
        return 0;
    }
    if (j > B0 && part != 2)
        GPX_TRY(launch_gemm_nt(Zt + B0 * TILE, ld, L + (j * TILE) * ld + B0 * TILE, ld, Zt + j * TILE, ld, M, TILE, (j - B0) * TILE,
                               -1.0, 1.0, 0, top->stream, prof));
    if (part == 1) return 0;
    // (Measured and dropped: the last column's update split into an early K = 768 part behind the solve two steps before and a
    // K = 128 part after the last leaf -- one more launch per panel costs what the shorter tail gains.)
    return launch_gemm_nt(Zt + j * TILE, ld, Dinv + j * (int64_t)TILE * TILE, TILE, Zt + j * TILE, ld, M, TILE, TILE, 1.0, 0.0, 0,
                          top->stream, prof);
}

// steps j in [j0,j1) of the diagonal square [B0,B1): leaf (factor + inverse), in-place TRSM leaf of the rows below
// inside the square, rank-128 update of the square's remaining columns -- the latency-bound chain of small kernels.
// top (optional): the slices of the rows below the square that trail the chain column by column (TopPipe).
static int chol_square_steps(double *L, int64_t ld, int64_t B0, int64_t B1, int64_t j0, int64_t j1, double *Dinv,
                             double *diagL, int *info_dev, hipStream_t s, Profiler *prof, const TopPipe *top = nullptr, int excl = 0)
{
    // excl: 1 = the step j == B0 runs its leaf exclusively (launch_potrf_leaf), 2 = every step
    for (int64_t j = j0; j < j1; ++j) {
        // row j of the square's factor is final once step j - 1 is through (the stream already waits for it): column j's update now,
        // underneath this step's leaf
        for (const TopPipe *t = top; t; t = t->next)
            if (t->stream && t->r1 > t->r0) GPX_TRY(top_column(L, ld, B0, j, Dinv, t, prof, 1));
        GPX_TRY(launch_potrf_leaf(L + (j * TILE) * ld + j * TILE, ld, Dinv + j * (int64_t)TILE * TILE, diagL + j * TILE, info_dev,
                                  (int)(j * TILE), s, prof, excl == 2 || (excl == 1 && j == B0)));
        const int64_t rows_below = B1 - (j + 1);
        if (rows_below > 0) {
            double *Z = L + ((j + 1) * TILE) * ld + j * TILE;                 // rows below the diagonal block, column block j
            GPX_TRY(launch_gemm_nt(Z, ld, Dinv + j * (int64_t)TILE * TILE, TILE, Z, ld, rows_below * TILE, TILE, TILE, 1.0, 0.0, 0, s, prof));
            // right-looking inside the square.  (Left-looking -- only the next block column updated per step, <= 28 workgroups
            // with K up to 896 -- was measured: a step then takes one workgroup's 24 us for a 32 x 128 x 896 tile instead of
            // spreading K = 128 tiles over the chip; the chain of an idle chip went from 480 to 577 us per panel.)
            // Also measured: only the next block column updated on the chain's stream and the remaining columns on a second
            // stream underneath the next leaf (joined one step later) -- two more cross-stream event edges per step cost more than
            // the shorter launches gain (fit 29.7 -> 33.2 ms).
            GPX_TRY(launch_gemm_nt(Z, ld, Z, ld, L + ((j + 1) * TILE) * ld + (j + 1) * TILE, ld, rows_below * TILE,
                                   rows_below * TILE, TILE, -1.0, 1.0, 0, s, prof));
        }
        hipEvent_t e = nullptr;
        for (const TopPipe *t = top; t; t = t->next) {
            if (!t->stream || t->r1 <= t->r0) continue;
            if (!e) {
                GPX_TRY(t->events->make(&e));
                GPX_HIP(hipEventRecord(e, s));
            }
            GPX_HIP(hipStreamWaitEvent(t->stream, e, 0));
            GPX_TRY(top_column(L, ld, B0, j, Dinv, t, prof, 2));
        }
    }
    return 0;
}

// factor block columns [B0,B1) of the rows >= B0 (all updates from columns < B0 already applied):
// (a) the diagonal square, 128 columns at a time; (b) everything below it in ONE recursive TRSM made of large GEMMs
int chol_panel_factor(double *L, int64_t ld, int64_t nblk_all, int64_t B0, int64_t B1, double *Dinv, double *diagL,
                      int *info_dev, hipStream_t s, Profiler *prof)
{
    GPX_TRY(chol_square_steps(L, ld, B0, B1, B0, B1, Dinv, diagL, info_dev, s, prof));
    if (nblk_all > B1)
        GPX_TRY(trsm_right_lt(L + (B1 * TILE) * ld, ld, (nblk_all - B1) * TILE, L, ld, Dinv, B0, B1, s, prof));
    return 0;
}

static void retire_events(const std::vector<hipEvent_t> &fresh)
{
    static std::mutex mu;
    static std::vector<hipEvent_t> pending;
    std::lock_guard<std::mutex> lk(mu);
    size_t keep = 0;
    for (size_t i = 0; i < pending.size(); ++i) {
        if (hipEventQuery(pending[i]) == hipSuccess) (void)hipEventDestroy(pending[i]);
        else pending[keep++] = pending[i];
    }
    pending.resize(keep);
    pending.insert(pending.end(), fresh.begin(), fresh.end());
}

// device buffers whose last use is queued on one or several streams but not waited for by the host: freed (returned to the pool) by a
// later call, once events recorded behind those uses have all passed
static void retire_buffers(const std::vector<void *> &bufs, const std::vector<hipStream_t> &behind)
{
    static std::mutex mu;
    struct Pending { std::vector<hipEvent_t> events; std::vector<void *> bufs; };
    static std::vector<Pending> pending;
    std::lock_guard<std::mutex> lk(mu);
    size_t keep = 0;
    for (size_t i = 0; i < pending.size(); ++i) {
        bool done = true;
        for (hipEvent_t e : pending[i].events) done = done && hipEventQuery(e) == hipSuccess;
        if (done) {
            for (hipEvent_t e : pending[i].events) (void)hipEventDestroy(e);
            for (void *q : pending[i].bufs) dfree(q);
        } else {
            if (keep != i) pending[keep] = std::move(pending[i]);
            ++keep;
        }
    }
    pending.resize(keep);
    if (bufs.empty()) return;
    Pending fresh;
    fresh.bufs = bufs;
    for (hipStream_t st : behind) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess || hipEventRecord(e, st) != hipSuccess) {
            (void)hipStreamSynchronize(st);          // (cannot track it: wait for this stream instead)
            if (e) (void)hipEventDestroy(e);
            continue;
        }
        fresh.events.push_back(e);
    }
    pending.push_back(std::move(fresh));
}

// status words of a square launch (dflow.hip: [0] potrf status, [1] stall) folded into the caller's ONE status word: a non-positive
// pivot as it is, an expired in-kernel wait as GPX_INFO_STALLED (the multi-GPU host raises on it: that factor is invalid, and it is not
// a property of K -- never answered with jitter)
// Launched on up to three unjoined streams (s, sh, sf): the merge is monotonic -- STALLED is the largest value, and atomicMax / a
// compare-and-swap from 0 cannot put a pivot index over a STALLED another stream's merge has written in between.
__global__ void merge_info_kernel(const int *two, int *one)
{
    if (two[1]) atomicMax(one, (int)GPX_INFO_STALLED);
    else if (two[0]) atomicCAS(one, 0, two[0]);
}

// How many ranks share the trailing update this thread's owner steps run beside (gpx_dev_set_panel_share; 1 = all of it, the default).
// At R ranks an owner's chain runs next to 1 / R of the update: "short trailing update -> square launch" is decided on the tiles divided
// by R.  Measured where it can be on one GPU (profiles/r06_multi_device_abi_one_gpu.txt): square launches for EVERY panel cost one rank
// nothing (C3 29.2 vs 29.3 ms, C4 1.371 vs 1.366 s) and take 6 % off two ranks that share the chip (39.2 vs 41.6 ms).
static thread_local int g_panel_share = 1;
extern "C" int gpx_dev_set_panel_share(int ranks)
{
    if (ranks < 1) { gpx_set_error("gpx_dev_set_panel_share: ranks must be >= 1"); return GPX_ERR_BAD_ARG; }
    g_panel_share = ranks;
    return 0;
}

// Square-kernel mode: the diagonal chain of a panel -- 8 x (leaf, in-square solve, rank-128 update) = 24 dependent launches -- is ONE
// small launch of the dataflow kernel on the panel's square (leaf + side workers, dflow.hip; ~56 us per 128-column step instead of
// ~100-250 us of dependent launches that wait for places), and the column solves of the rows below wait for its step counter instead
// of for events.  THE rule for where, of the single-GPU schedule (chol_factor) and of the multi-GPU owner's panel step alike: where the
// chain is the critical path and the chip has empty CUs for it -- a square launch needs whole CUs, which a long trailing update beside
// it does not give up.  That is the first panel (nothing but the Gram kernel's remainder runs beside it) and the panels whose trailing
// update has fewer than GPX_SQK_TILES tiles left (default 1000: the last six panels at N = 16384).  GPX_SQK_FROM = p forces it from
// panel p on (0: everywhere; -1: never).
//   b0: the panel's first block column, beside: tiles of the trailing update that runs beside the chain (with nrem block rows below a
//   square of `rows`: nrem (nrem + 1) / 2 tiles of triangle + nrem x rows of the panel's own columns -- fewer where the update stops
//   at a group's last column, Lookahead::beside_tiles), share: ranks that split it
//   from_p: GPX_SQK_FROM = p > 0 counts (the owner's panel step has always read only 0 and -1, and keeps doing so)
static long sqk_from() { static const long v = env_long("GPX_SQK_FROM", -2); return v; }   // -2: the rule decides
static bool square_launch_wanted(int64_t b0, int64_t beside, int share, bool from_p)
{
    static const long tiles = env_long("GPX_SQK_TILES", 1000);
    if (sqk_from() == -1 || !chol_dataflow_supported(CHOL_NBP)) return false;
    if (sqk_from() == 0) return true;
    if (sqk_from() > 0 && from_p) return b0 >= sqk_from() * CHOL_NBP;
    return b0 == 0 || beside / share < tiles;
}

// The panel step of the multi-GPU host's panel owner (skgpuppy_amd/distributed.py -> gpx_dev_chol_panel / gpx_dev_chol_panel_next /
// gpx_dev_chol_panel_split): factor block columns [B0, B1) of the rows >= B0 with the rows below the square solved column by column
// alongside the chain (TopPipe, as in chol_factor).  Nothing is waited for on the host.
//   P (optional): rows >= B0 * 128 of the PREVIOUS panel (kp columns, leading dimension ldp) whose rank-kp update this panel still
//   lacks.  The diagonal square gets it first, on `s`, so that the chain starts at once; the rows below get it on their slice's stream,
//   ahead of the column solves that need them (the single-GPU schedule's order).
//   Slices of the rows below: without caller streams ONE slice on an internal stream, forked from and joined back into `s` (on return
//   everything is ordered behind `s`).  With caller streams (sh, sf; round 5, the split panel message): the first `hb` block rows -- the
//   NEXT panel's square, what its owner needs to start its chain -- on sh, the rest on sf; both are ordered behind `s` as it stood at
//   the call (plus the square's update), are NOT joined back, and the caller orders whatever else their updates need (the arrival of
//   P's far rows) on those streams before the call.  After the call `s` holds the square, Dinv and diag; sh the head rows; sf the rest.
// Where square_launch_wanted says so (full panels only) the chain is ONE square launch of the dataflow kernel and the column solves
// follow the launch's step counter.  (A panel solve by one product with the square's inverse was measured here too: slower in the
// one-rank rehearsal, tools/native/rejected/r05_owner_step_square_launch_product_solve.patch.)
int chol_panel_factor_piped(double *L, int64_t ld, int64_t nblk_all, int64_t B0, int64_t B1, double *Dinv, double *diagL,
                            int *info_dev, hipStream_t s, Profiler *prof, const double *P, int64_t ldp, int64_t kp,
                            int64_t hb, hipStream_t sh, hipStream_t sf)
{
    const int64_t c0 = B0 * TILE, w = (B1 - B0) * TILE;
    const bool own_streams = sh && sf;
    double *Csq = L + c0 * ld + c0;
    if (P) GPX_TRY(launch_gemm_nt(P, ldp, P, ldp, Csq, ld, w, w, kp, -1.0, 1.0, 0, s, prof));
    const int64_t nrem = nblk_all - B1;
    const bool sqk = B1 - B0 == CHOL_NBP && B0 % CHOL_NBP == 0 && square_launch_wanted(B0, nrem * (nrem + 1) / 2 + nrem * (B1 - B0), g_panel_share, false);
    // what the call leaves queued (buffer, events, internal stream): everything queued sits in body(), every way out passes the hand-over below it
    std::vector<void *> scratch;
    Events events;
    hipStream_t st_int = nullptr;
    struct Slice { hipStream_t st; int64_t r0, r1; bool joined; };
    std::vector<Slice> slices;   // of the rows below the square
    int *two = nullptr, *state = nullptr, *tab_dev = nullptr;
    auto chain = [&](const TopPipe *top) -> int {
        if (!sqk) return chol_square_steps(L, ld, B0, B1, B0, B1, Dinv, diagL, info_dev, s, prof, top);
        static thread_local std::vector<int> tab;
        GPX_TRY(launch_chol_dataflow(L, ld, B1, B0, Dinv, diagL, two, state, tab, wait_limit_ticks(), s, 32, 1, tab_dev));
        for (int64_t j = B0; j < B1; ++j)
            for (const TopPipe *t = top; t; t = t->next) GPX_TRY(top_column(L, ld, B0, j, Dinv, t, prof));
        return 0;
    };
    auto merge_info = [&](hipStream_t on) -> int {   // behind the launch (on s) / behind a slice's waits (its stall word)
        if (!sqk) return 0;
        hipLaunchKernelGGL(merge_info_kernel, dim3(1), dim3(1), 0, on, (const int *)two, info_dev);
        GPX_HIP(hipGetLastError());
        return 0;
    };
    auto body = [&]() -> int {
        if (sqk) {
            // status pair, state words and task tables of the launch: zeroed / uploaded on `s` BEFORE the fork, so that the column solves on
            // the slices' streams never poll a recycled buffer's old counters
            static thread_local std::vector<int> tab_host;   // (uploaded asynchronously: must outlive this call)
            const int64_t nstate = chol_dataflow_state_ints(CHOL_NBP), ntab = chol_dataflow_table_ints(CHOL_NBP);
            tab_host.assign((size_t)ntab, 0);
            if (chol_dataflow_fill_tables((int)CHOL_NBP, (int)CHOL_NBP, tab_host.data(), (int)ntab) < 0) { gpx_set_error("chol_panel_factor_piped: task tables"); return GPX_ERR_STATE; }
            double *buf = nullptr;
            GPX_TRY(dalloc(&buf, (4 + nstate + ntab) / 2 + 2));
            scratch.push_back(buf);
            two = reinterpret_cast<int *>(buf); state = two + 4; tab_dev = state + nstate;
            GPX_HIP(hipMemsetAsync(two, 0, sizeof(int) * (size_t)(4 + nstate), s));
            GPX_HIP(hipMemcpyAsync(tab_dev, tab_host.data(), sizeof(int) * (size_t)ntab, hipMemcpyHostToDevice, s));
        }
        if (nrem > 0) {
            if (own_streams) {
                const int64_t h = hb < 0 ? 0 : (hb > nrem ? nrem : hb);
                if (h > 0) slices.push_back({sh, B1, B1 + h, false});
                if (h < nrem) slices.push_back({sf, B1 + h, nblk_all, false});
            } else if ((st_int = stream_acquire(1)) != nullptr) {
                slices.push_back({st_int, B1, nblk_all, true});
            }
        }
        if (slices.empty()) {   // no rows below -- or no second stream to be had: everything on s
            if (nrem > 0 && P) GPX_TRY(launch_gemm_nt(P + w * ldp, ldp, P, ldp, Csq + w * ld, ld, nrem * TILE, w, kp, -1.0, 1.0, 0, s, prof));
            GPX_TRY(chain(nullptr));
            GPX_TRY(merge_info(s));
            return nrem > 0 ? trsm_right_lt(L + (B1 * TILE) * ld, ld, nrem * TILE, L, ld, Dinv, B0, B1, s, prof) : 0;
        }
        std::vector<TopPipe> tops(slices.size());
        hipEvent_t e0 = nullptr;
        GPX_TRY(events.make(&e0));
        GPX_HIP(hipEventRecord(e0, s));
        for (size_t i = 0; i < slices.size(); ++i) {
            const Slice &sl = slices[i];
            GPX_HIP(hipStreamWaitEvent(sl.st, e0, 0));
            if (P) GPX_TRY(launch_gemm_nt(P + (sl.r0 * TILE - c0) * ldp, ldp, P, ldp, L + (sl.r0 * TILE) * ld + c0, ld, (sl.r1 - sl.r0) * TILE, w, kp,
                                          -1.0, 1.0, 0, sl.st, prof));
            TopPipe &top = tops[i];
            top.stream = sl.st; top.r0 = sl.r0; top.r1 = sl.r1; top.events = &events;
            if (sqk) { top.follow_square(state, B1 - B0, 0); top.stall = two + 1; }
            top.next = i + 1 < slices.size() ? &tops[i + 1] : nullptr;
        }
        GPX_TRY(chain(&tops[0]));
        for (const Slice &sl : slices) {
            if (sl.joined) {
                hipEvent_t e1 = nullptr;
                GPX_TRY(events.make(&e1));
                GPX_HIP(hipEventRecord(e1, sl.st));
                GPX_HIP(hipStreamWaitEvent(s, e1, 0));
            } else {
                GPX_TRY(merge_info(sl.st));   // (a wait of this slice that expired: its stream is not joined into s)
            }
        }
        return merge_info(s);
    };
    const int rc = body();
    // No host synchronisation here (unless something failed): the caller goes on queueing its trailing updates while the panel is being
    // factored.  The events are still referenced by queued waits, so they retire through a list that later calls sweep once
    // hipEventQuery says the GPU has passed them (the launch's state buffer likewise, behind every stream that polls it); the internal
    // stream goes back to the cache (whoever takes it next queues behind the work it still holds).
    std::vector<hipStream_t> behind{s};
    for (const Slice &sl : slices) if (!sl.joined) behind.push_back(sl.st);
    if (rc) for (hipStream_t q : behind) (void)hipStreamSynchronize(q);
    if (rc && st_int) (void)hipStreamSynchronize(st_int);
    retire_buffers(scratch, behind);
    retire_events(events.all);
    events.all.clear();
    if (st_int) stream_release(st_int, 1);
    return rc;
}

// ------------------------------------------------------------------------------------------------
// CU reservation for the diagonal chain.  Measured (tools/native/probe_slot.hip, probe_leafk.hip): while a bulk
// launch saturates the chip (two workgroups per CU, 224 VGPRs per wave), a small kernel of the chain waits 40-130 us for a
// retiring bulk workgroup's place -- equal-length tiles retire in bursts -- and then runs 3x (next to one bulk wave per SIMD)
// to 10x (next to two) slower than alone; kernels small enough to be placed at once (<= 64 VGPRs, <= 16 KB of LDS) pay the
// 10x.  Neither stream priorities nor s_setprio change that.  What does: a few CUs that the bulk cannot enter.  A "blocker"
// workgroup of four sleeping waves that each hold 296 VGPRs leaves 216 registers per SIMD: no bulk wave (224) fits there, the
// chain's kernels (leaf 216, 32/64-row GEMM tiles 80-122 VGPRs) do, and the whole LDS stays free.  R blockers launched on an
// idle chip take R distinct CUs (two cannot share one), dealt round-robin over the XCDs; they leave when the flag is set (after
// the last bulk launch of the factorisation) or, whatever happens to the host, when their time limit expires.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cu_blocker_kernel(const int *stop, int *placed, unsigned long long limit_ticks)
{
    asm volatile("v_mov_b32 v255, 0\n\tv_accvgpr_write_b32 a39, 0" ::: "v255", "a39");   // 256 VGPRs + 40 AGPRs: 296 registers per wave
    if (threadIdx.x == 0) __hip_atomic_fetch_add(placed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x < 64) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // 100 MHz
        while (__hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 &&
               __builtin_amdgcn_s_memrealtime() - t0 < limit_ticks)
            __builtin_amdgcn_s_sleep(127);
    }
    __syncthreads();                                     // the other three waves wait here without issuing anything
}

__global__ void set_flag_kernel(int *flag, int value) { __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// holds its stream until `want` blockers have taken their CUs (or the time limit expires: the reservation is an optimisation)
__global__ void wait_placed_kernel(const int *placed, int want, unsigned long long limit_ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(placed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want && __builtin_amdgcn_s_memrealtime() - t0 < limit_ticks)
        __builtin_amdgcn_s_sleep(16);
}

// The trapezoid hand-off and the CU reservation rely on kernels of DIFFERENT streams running at the same time (a one-thread kernel
// waits for a count another launch produces; blockers sleep until a later launch releases them).  Counter-collecting profilers
// (rocprofv3 --pmc) run one kernel at a time: the waits would sit out their time limits.  Checked once per process with a 2 ms probe: a
// waiting kernel on one stream, the kernel that releases it launched afterwards on another.
namespace {
std::mutex g_conc_mu;
std::map<std::pair<hipStream_t, hipStream_t>, bool> g_conc_seen;
thread_local bool g_force_plain = false;   // (per host thread) set while a stalled fit is repeated: no kernel waits for a kernel of another stream
}
// forget every verdict (streams were destroyed, or a wait expired although its pair had been probed as concurrent)
void chol_concurrency_forget()
{
    std::lock_guard<std::mutex> lk(g_conc_mu);
    g_conc_seen.clear();
}
void chol_force_plain_schedule(bool on) { g_force_plain = on; }

static bool streams_run_concurrently(hipStream_t a, hipStream_t b)
{
    // a: the stream whose kernel waits, b: the stream whose later launch releases it.  Probed once per pair of streams (they come from
    // the library's stream cache, so the same pairs recur) on the caller's own streams: extra streams would change
    // which streams share a hardware queue.  Two streams of one priority class may share a hardware queue when the process has
    // more streams than the runtime has queues for that class: the waiting kernel then sits in front of its own release.
    // The fit probes its pairs while its streams are still idle (chol_probe_streams, before the Gram launch): a busy releasing stream
    // would read as "not concurrent" for the rest of the process.
    if (g_force_plain) return false;
    if (const char *e = getenv("GPX_CONCURRENT_STREAMS")) return atoi(e) != 0;
    if (!a || !b) return false;
    std::lock_guard<std::mutex> lk(g_conc_mu);
    auto it = g_conc_seen.find({a, b});
    if (it != g_conc_seen.end()) return it->second;
    double *wd = nullptr;                       // a scratch word from the library's pool (no hipMalloc / hipFree inside a fit)
    bool good = false;
    if (dalloc(&wd, 2) == 0) {
        int *w = reinterpret_cast<int *>(wd);
        if (hipMemsetAsync(w, 0, 2 * sizeof(int), a) == hipSuccess && hipStreamSynchronize(a) == hipSuccess) {
            hipLaunchKernelGGL(wait_count_kernel, dim3(1), dim3(1), 0, a, (const int *)w, 1, 200000ull, w + 1);   // <= 2 ms (its own check: a failed probe sets no error text)
            const bool l1 = hipGetLastError() == hipSuccess;
            hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1), 0, b, w, 1);
            const bool l2 = hipGetLastError() == hipSuccess;
            int h[2] = {0, 1};
            if (hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess && l1 && l2 &&
                hipMemcpy(h, w, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
                good = (h[1] == 0);
        }
        dfree(wd);
    }
    (void)hipGetLastError();
    if (debug_enabled()) fprintf(stderr, "[gpx] concurrent-streams probe (%p waits, %p releases): %d\n", (void *)a, (void *)b, (int)good);
    g_conc_seen[{a, b}] = good;
    return good;
}
// the blockers sleep until a launch of any of the other three streams releases them
static bool blockers_may_wait_on(hipStream_t s_blk, hipStream_t s, hipStream_t s_pan, hipStream_t s_top)
{
    return streams_run_concurrently(s_blk, s) && streams_run_concurrently(s_blk, s_pan) && (!s_top || streams_run_concurrently(s_blk, s_top));
}

static int reserve_cus() { static const int v = (int)std::min(128L, std::max(0L, env_long("GPX_RESERVE_CUS", 32))); return v; }
// the reservation starts with the first panel whose bulk launch has fewer 128 x 128 tiles than this (the tail of the factorisation,
// where the chain, not the bulk, is the critical path)
static long reserve_below_tiles() { static const long v = env_long("GPX_RESERVE_TILES", 3000); return v; }
// (high priority: that class has its own hardware queues, which an application's ordinary streams do not crowd)
static int blocker_stream_prio() { static const int v = (int)env_long("GPX_BLK_PRIO", 1); return v; }
static int sqk_workers() { static const int v = (int)env_long("GPX_SQK_WORKERS", 32); return v; }
static bool trap_enabled() { static const bool v = env_long("GPX_TRAP", 1) != 0; return v; }
// Fits of at most this many block rows (GPX_DFLOW_MAX_BLOCKS, default 0 = none) run as ONE launch of the persistent dataflow kernel
// (dflow.hip) instead of the multi-stream schedule.  Measured at N = 4096 (32 block rows, round 5, profiles/r05_probe_c2_*): 3.0 ms
// against 2.36 ms -- with four square launches the multi-stream schedule already pays one launch per panel, and the whole-matrix
// kernel's workers poll queues in HBM between tasks: not the default at any size; tests/test_dataflow.py runs a fit through it.
static int64_t dflow_max_blocks() { static const int64_t v = env_long("GPX_DFLOW_MAX_BLOCKS", 0); return v; }
// Callers without look-ahead streams (SPGP's M x M blocks, gpx_spd_inverse) use the kernel between 9 and 64 block rows (GPX_DFLOW_SMALL=0:
// never) -- a 2048 x 2048 factorisation is a chain of 16 steps, 1.0 ms there against 2.2 ms of dependent launches.
static bool dflow_small_enabled() { static const bool v = env_long("GPX_DFLOW_SMALL", 1) != 0; return v; }
// The far columns by group on the int8 path (Lookahead::group_boundary).  GPX_FIT_EMU: 0 never (the fp64 schedule, bit for bit), 1
// wherever the rules below allow it, unset: from FIT_EMU_MIN_BLOCKS block rows on; GPX_FIT_EMU_GROUP: outer panels per group.
// Panels per group for a factor of nblk block rows, 0 = the fp64 schedule: the emulated path takes K = 1024 G (emu_enabled: GPX_EMU_F64,
// GPX_EMU_MIN_K) and there are at least two groups.  A function of nblk and the environment alone.
// Measured (profiles/r25_fit_emu.txt; G = 4 and 8 against the fp64 schedule at N = 8192 ... 32768, interleaved on one box): groups of
// four win at every size: by 2 % at N = 8192 (5.94 against 6.07-6.11 ms), by 8 % at 12288 and more above.  On from N = 12288: below it
// the fit keeps the fp64 tile arithmetic, which every other schedule of such a fit reproduces bit for bit -- the whole matrix as one
// dataflow launch among them (GPX_DFLOW_MAX_BLOCKS; tests/test_dataflow.py holds alpha at N = 9000 to the last bit), and that launch
// has no emulated update.  The 0.13 ms at 8192 do not pay for giving that up.
constexpr long FIT_EMU_MIN_BLOCKS = 96, FIT_EMU_GROUP = 4;
static int64_t fit_emu_group(int64_t nblk)
{
    static const long on = env_long("GPX_FIT_EMU", -1), group = std::max(1L, env_long("GPX_FIT_EMU_GROUP", FIT_EMU_GROUP));
    if (on == 0 || (on < 0 && nblk < FIT_EMU_MIN_BLOCKS)) return 0;
    const int64_t panels = (nblk + CHOL_NBP - 1) / CHOL_NBP;
    return emu_enabled(CHOL_PANEL_COLS * group) && panels > group ? group : 0;
}

// Probes every pair of streams the look-ahead schedule lets wait for each other (cached per pair).  Called by the fit while the
// streams are still idle -- before the Gram launch is queued on `s`.
void chol_probe_streams(hipStream_t s, hipStream_t s_pan, hipStream_t s_top)
{
    if (!s_pan) return;
    const bool concurrent = streams_run_concurrently(s_pan, s) && (!s_top || streams_run_concurrently(s_top, s));
    if (!concurrent || reserve_cus() == 0) return;
    hipStream_t s_blk = stream_acquire(blocker_stream_prio());   // the cache hands the same stream to chol_factor's own acquire
    if (!s_blk) return;
    (void)blockers_may_wait_on(s_blk, s, s_pan, s_top);
    stream_release(s_blk, blocker_stream_prio());
}

namespace {
// The whole matrix as ONE launch of the dataflow kernel on `s`: take() the kernel's state words and task tables from the pool, launch().
// The block and the host copy of the tables (uploaded asynchronously) live until the owner has waited for the stream: `tab` is declared
// in front of `sc`, so it is destroyed after Scratch's wait.
struct WholeDataflow {
    std::vector<int> tab;
    Scratch sc;
    double *state = nullptr;
    explicit WholeDataflow(hipStream_t s) : sc(s) {}
    int take(int64_t nblk) { return sc.take(&state, (chol_dataflow_state_ints(nblk) + chol_dataflow_table_ints(nblk)) / 2 + 2); }
    int launch(double *L, int64_t ld, int64_t nblk, double *Dinv, double *diagL, int *info_dev)
    {
        return launch_chol_dataflow(L, ld, nblk, 0, Dinv, diagL, info_dev, reinterpret_cast<int *>(state), tab, wait_limit_ticks(), sc.s, 0, 0);
    }
};

// The small form (dflow_small_enabled).  The kernel's in-kernel waits are bounded; one that expires (it never has) is reported, not
// retried: the matrix is overwritten by then.  The call synchronises the stream (the kernel's state words are freed here).
int small_dataflow_factor(double *L, int64_t ld, int64_t nblk, double *Dinv, double *diagL, int *info_dev, hipStream_t s)
{
    WholeDataflow df(s);
    int st_host[2] = {0, 0};
    GPX_TRY(df.take(nblk));
    GPX_HIP(hipMemsetAsync(info_dev + 1, 0, sizeof(int), s));
    GPX_TRY(df.launch(L, ld, nblk, Dinv, diagL, info_dev));
    GPX_HIP(hipMemcpyAsync(st_host, info_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    GPX_HIP(df.sc.wait_and_free());
    if (!st_host[1]) return 0;
    gpx_set_error("factorisation of a %ld-row block: an in-kernel hand-off timed out (GPX_WAIT_LIMIT_MS); GPX_DFLOW_SMALL=0 selects the launch chain",
                  (long)(nblk * TILE));
    return GPX_ERR_STATE;
}

// ONE look-ahead factorisation per device at a time takes the schedule with CU blockers, exclusive square launches and kernels that
// wait for counters of other streams: two of them side by side (two host threads, each with a handle of its own) hold 64 CUs with
// blockers, compete for whole CUs with their square launches and sit in each other's way for milliseconds (measured: two threads,
// four fits each at N = 12288 / 16384, 3.3x the serial sum; no stall, but nothing bounds the wait either).  A fit that finds another
// one in flight on its device takes the plain schedule instead (events only, no reservation): the same tile arithmetic, the GPU is
// the shared resource either way.
struct SoloToken {
    int dev = 0; bool solo = false;
    static std::atomic<int> &count(int d) { static std::atomic<int> c[64]; return c[d & 63]; }
    SoloToken() { (void)hipGetDevice(&dev); solo = count(dev).fetch_add(1) == 0; }
    ~SoloToken() { count(dev).fetch_sub(1); }
};

// The look-ahead schedule of one factorisation (chol_factor): what its steps share, and the steps themselves in the order the host
// queues them.  That order -- every launch, event record and stream wait -- is part of the schedule: the runtime binds a stream to a
// hardware queue at its first use, and the tail of the factorisation is bound by the host's enqueue rate (about 60 launches per panel).
// The object also owns the way out, however chol_factor returns (the destructor).
struct Lookahead {
    double *L;
    int64_t ld, nblk;
    double *Dinv, *diagL;
    int *info_dev;
    hipStream_t s, s_pan, s_top;   // main (bulk), chain, column solves
    Profiler *prof;
    const std::function<int()> *after_fork;
    const std::function<int(int64_t, int64_t, bool)> *panel_final;
    // outer panel boundaries (block units).  Wider early panels (12..32 blocks) were measured and are slower.
    std::vector<int64_t> Bs{0};
    int64_t P = 0;
    SoloToken token;
    bool concurrent = false;   // the streams run side by side and no other look-ahead factorisation is in flight: kernels may wait for kernels
    bool trap_on = false;      // trapezoid launches with in-kernel hand-off
    // Square launches (square_launch_wanted).  State words: 1024 ints per panel (chol_dataflow_state_ints(8) = 656), zeroed on the MAIN
    // stream in front of the factorisation's first event -- the column solves on s_top poll them, and a recycled buffer holds the previous
    // fit's finished counters; the task tables of a full square and of a shorter last one are uploaded once, behind the states.
    // The square launch also solves the NEXT diagonal square's rows for its columns (COL tasks of SQK_EXTRA more workgroups, in step
    // with the chain), so that the update of the next square -- what the next chain waits for -- follows the launch at once instead of
    // waiting for the column solves of ALL rows below on the third stream; those keep the rows further down, which only the trailing
    // update needs.  The rows reach the launch through another stream's update: gate word per panel, set behind it.
    static constexpr int64_t SQK_STATE = 1024, SQK_TAB = 256, SQK_GATE = 1008;
    static constexpr int SQK_EXTRA = 32;
    std::vector<char> sqk_use;   // per panel: its chain is a square launch
    double *sqk_buf = nullptr;
    std::vector<std::vector<int>> sqk_tabs;
    std::vector<int> sqk_tab_host;
    std::vector<TopPipe> tops;   // per panel: the column solves of the rows below its square
    // info_dev: [0] potrf status, [1] stall, [2] the blockers' stop flag, [3] their placement counter, then CHOL_NBP counters per
    // panel: finished narrow tiles of its trapezoid launch by tile column
    int *stall = nullptr, *stop_flag = nullptr, *placed = nullptr, *sig = nullptr;
    hipStream_t s_blk = nullptr;   // CU reservation: the blockers (nres of them) run on a stream of their own
    int nres = 0;
    bool reserved = false, released = false;
    bool blk_gone = false;         // a reservation was dropped at a group boundary: ev_blk_gone passes once its blockers have left
    // The far columns by group (fit_emu_group): T(p) stops at the first column of the group after p's; behind a group's last panel ONE
    // emulated symmetric update of depth 1024 G brings every column right of the group up to date (group_boundary).
    int64_t G = 0;                 // panels per group; 0: every T(p) runs to the last column (the fp64 schedule)
    EmuFrame esy;
    bool sq_split_prev = false;   // T(p - 1) ran in the split tail form: diagonal square p + 1 has its tiles marked by ev_sqp[p - 1]
    Events events;
    hipEvent_t ev0 = nullptr, ev_blk = nullptr, ev_blk_gone = nullptr;
    std::vector<hipEvent_t> ev_pf, ev_next, ev_top, ev_tu, ev_first, ev_sqp;
    // GPX_DEBUG: host clock (us since the factorisation's first launch) at which each panel's launches had been queued -- in the tail the
    // kernels are so short that the HOST's enqueue rate (60 launches per panel) can become the critical path
    double host_t0 = 0.0;
    std::vector<double> host_marks;
    static double host_now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void mark() { if (debug_enabled()) host_marks.push_back(host_now() - host_t0); }
    // The way out, after a failure as after the last panel: the blockers leave; the host waits for the column solves' stream, the chain's
    // and -- where there are blockers -- the main stream and theirs (events must not be destroyed while still referenced by queued
    // waits, a buffer not go back to the pool while a kernel polls it); then the blocker stream returns to the cache, the main stream is
    // waited for, and the events and the buffer go.
    ~Lookahead()
    {
        if (debug_enabled()) {
            fprintf(stderr, "[gpx] host enqueue marks, panel by panel (us): ");
            for (double m : host_marks) fprintf(stderr, "%.0f ", m);
            fprintf(stderr, "\n");
        }
        release_blockers();
        if (s_top) (void)hipStreamSynchronize(s_top);
        (void)hipStreamSynchronize(s_pan);
        if (s_blk) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamSynchronize(s_blk);
            stream_release(s_blk, blocker_stream_prio());
        }
        (void)hipStreamSynchronize(s);
        events.clear();
        if (sqk_buf) dfree(sqk_buf);
        emu_free(esy);
    }
    int64_t bnd(int64_t p) const { return Bs[std::min<int64_t>(p, P)]; }
    // first block column that T(p) leaves to the next group boundary (nblk: none)
    int64_t far_blk(int64_t p) const { return G ? bnd((p / G + 1) * G) : nblk; }
    // panel p ends a group that another one follows: the boundary's update takes the place of Q(p) and T(p)
    bool boundary(int64_t p) const { return G && (p + 1) % G == 0 && p + 1 < P; }
    // tiles of T(p)'s triangle part: rows [B2, nblk), columns [B2, far) at and below the diagonal
    int64_t bulk_tiles(int64_t p) const
    {
        const int64_t nrem = nblk - bnd(p + 2), wt = std::max<int64_t>(0, std::min(nrem, far_blk(p) - bnd(p + 2)));
        return nrem <= 0 ? 0 : wt * (wt + 1) / 2 + (nrem - wt) * wt;
    }
    // tiles of the fp64 update that runs beside chain(pp): T(pp - 1), its narrow part included; behind a boundary none
    int64_t beside_tiles(int64_t pp) const
    {
        if (pp == 0 || boundary(pp - 1)) return 0;
        return (nblk - bnd(pp + 1)) * (bnd(pp + 1) - bnd(pp)) + bulk_tiles(pp - 1);
    }
    // work of the caller that rides along on the main stream, behind panel p's trailing update (common.h: panel_final)
    int hook(int64_t p, int64_t slack, bool last) const { return panel_final ? (*panel_final)(p, slack, last) : 0; }
    // panel q has rows below its square, and a stream to solve them on column by column alongside its chain
    bool piped(int64_t q) const { return s_top && bnd(q + 1) < nblk; }
    bool use_sqk(int64_t pp) const { return pp >= 0 && pp < P && sqk_use[(size_t)pp]; }
    int *sqk_state(int64_t pp) const { return reinterpret_cast<int *>(sqk_buf) + pp * SQK_STATE; }
    int *sqk_tab(int64_t pp) const { return reinterpret_cast<int *>(sqk_buf) + P * SQK_STATE + pp * SQK_TAB; }
    int *sqk_gate(int64_t pp) const { return sqk_state(pp) + SQK_GATE; }
    // block rows below panel pp's square that its square launch solves as well (the next square's)
    int64_t sqk_below(int64_t pp) const { return s_top ? bnd(pp + 2) - bnd(pp + 1) : 0; }
    // a square launch that solved the rows [B1, B2) itself: the square update needs nothing else -- the column solves of the rows
    // further down are waited for behind it, in front of the updates that read them
    bool top_late(int64_t p) const { return piped(p) && use_sqk(p) && sqk_below(p) == bnd(p + 2) - bnd(p + 1) && bnd(p + 2) > bnd(p + 1); }
    bool q_on_chain(int64_t p) const { return sq_split_prev && piped(p); }   // Q(p) goes on the chain's stream (square_update)
    // Everything the schedule needs before its first launch, none of it queued on a stream of the fit (the stream probes are cached from
    // chol_probe_streams): which kernels may wait for kernels, which panels run as square launches and their buffer, every event of
    // the per-panel hand-offs (created here, not inside the loop: the tail is bound by the host), the blockers' stream.
    int setup()
    {
        while (Bs.back() < nblk) Bs.push_back(std::min<int64_t>(nblk, Bs.back() + CHOL_NBP));
        P = (int64_t)Bs.size() - 1;
        stall = info_dev + 1;
        stop_flag = info_dev + 2;
        placed = info_dev + 3;
        sig = info_dev + 4;
        // (the column solves wait for the kernels' counters from another stream: needs streams that run side by side)
        concurrent = token.solo && streams_run_concurrently(s_pan, s) && (!s_top || streams_run_concurrently(s_top, s));
        trap_on = trap_enabled() && concurrent;
        // the group route: decided by nblk and the environment -- and by the pool: a workspace that does not fit (dalloc trims the pool
        // before it gives up) leaves the fp64 schedule, the one way the route depends on anything but size
        G = fit_emu_group(nblk);
        if (G) {
            esy.reserve(emu_syrk_plan((nblk - bnd(G)) * TILE, (int64_t)CHOL_PANEL_COLS * G));   // the first boundary's update, the largest
            if (emu_alloc(esy, nullptr)) G = 0;
        }
        sqk_use.assign((size_t)P, 0);
        for (int64_t pp = 0; concurrent && pp < P; ++pp)
            sqk_use[(size_t)pp] = square_launch_wanted(bnd(pp), beside_tiles(pp), 1, true);
        sqk_tabs.resize((size_t)P);
        tops.resize((size_t)P + 1);
        if (std::count(sqk_use.begin(), sqk_use.end(), 1)) GPX_TRY(dalloc(&sqk_buf, (P * SQK_STATE + P * SQK_TAB) / 2 + 2));
        for (std::vector<hipEvent_t> *v : {&ev_pf, &ev_next, &ev_top, &ev_tu, &ev_first, &ev_sqp}) v->resize((size_t)P + 1);
        GPX_TRY(events.make(&ev0));
        for (int64_t p = 0; p < P; ++p)
            for (hipEvent_t *e : {&ev_pf[p], &ev_next[p], &ev_top[p], &ev_tu[p], &ev_first[p], &ev_sqp[p]}) GPX_TRY(events.make(e));
        GPX_TRY(events.make(&ev_top[P]));
        // CU reservation (above) for the tail of the factorisation: flag and placement counter live behind the status word
        nres = concurrent ? reserve_cus() : 0;
        s_blk = nres ? stream_acquire(blocker_stream_prio()) : nullptr;
        if (s_blk && !blockers_may_wait_on(s_blk, s, s_pan, s_top)) {   // the blockers would sit in front of launches their release depends on
            stream_release(s_blk, blocker_stream_prio());
            s_blk = nullptr;
        }
        if (s_blk) GPX_TRY(events.make(&ev_blk));
        if (s_blk && G) GPX_TRY(events.make(&ev_blk_gone));
        host_t0 = debug_enabled() ? host_now() : 0.0;
        return 0;
    }
    // the chain of panel pp's square [Ba, Bb) as one launch on s_pan; its column solves (rows below, stream s_top) per finished step
    int sqk_launch(int64_t pp, int64_t Ba, int64_t Bb)
    {
        const int64_t below = sqk_below(pp);
        return launch_chol_dataflow(L, ld, Bb + below, Ba, Dinv, diagL, info_dev, sqk_state(pp), sqk_tabs[(size_t)pp], wait_limit_ticks(), s_pan,
                                    std::min<int>(sqk_workers(), (int)(4 * (Bb - Ba - 1) + 4)), 1, sqk_tab(pp), (int)(Bb - Ba),
                                    below > 0 ? SQK_EXTRA : 0, sqk_gate(pp));
    }
    // the rows below panel pp's square have their update (queued on `on` just now): its square launch may solve them
    void sqk_open_gate(int64_t pp, hipStream_t on)
    {
        if (use_sqk(pp) && sqk_below(pp) > 0) hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1), 0, on, sqk_gate(pp), 1);
    }
    // the column solves of panel q follow its square launch's step counter (top_column waits for the step itself)
    void follow_square(int64_t q) { tops[(size_t)q].follow_square(sqk_state(q), bnd(q + 1) - bnd(q), sqk_below(q)); }
    // The blockers leave (the flag is set behind whatever the main stream holds): from the first tail panel that runs as a square
    // launch, behind the last bulk launch, and on the way out.
    void release_blockers()
    {
        if (!reserved || released) return;
        hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1), 0, s, stop_flag, 1);
        released = true;
    }
    // A group boundary gives the reserved CUs back: the int8 product (128 KiB of LDS, more than 216 registers per SIMD) cannot use them.
    // The next short panel reserves again (reserve_now).
    int drop_reservation()
    {
        if (!reserved) return 0;
        release_blockers();
        GPX_HIP(hipEventRecord(ev_blk_gone, s_blk));
        reserved = released = false;
        blk_gone = true;
        return 0;
    }
    // The reservation starts in front of panel p's square update, with the first panel whose bulk launch is short (reserve_below_tiles).
    // (not where the next chain is a square launch already -- small factors, N <= 5120 at the default thresholds: the blockers
    // would be released again a few lines below, 30 us of memset / placement wait / release on the critical path for nothing)
    // (the column solves keep their small tiles and share the reserved CUs with the chain: measured better than 224-register
    // tiles that stay off them, fit 28.9 -> 28.1 ms)
    // Called where the main stream has just drained (it waits for panel p's chain): the blockers find an empty chip.
    // (the waiting kernel on the chain's stream, its release on the main stream: the order in which the fit first uses its streams --
    // the runtime binds a stream to a hardware queue at its first launch, and another order was measured to cost 5 ms per fit)
    int reserve_now(int64_t p)
    {
        const int64_t nrem = nblk - bnd(p + 2);
        if (!s_blk || reserved || nrem <= 0 || bulk_tiles(p) >= reserve_below_tiles() || (sqk_from() < 0 && use_sqk(p + 1))) return 0;
        if (blk_gone) GPX_HIP(hipStreamWaitEvent(s, ev_blk_gone, 0));   // (the flag is cleared only once the blockers it released have read it)
        blk_gone = false;
        GPX_HIP(hipMemsetAsync(stop_flag, 0, 2 * sizeof(int), s));
        GPX_HIP(hipEventRecord(ev_blk, s));
        GPX_HIP(hipStreamWaitEvent(s_blk, ev_blk, 0));
        // time limit: generous multiple of the factorisation's expected duration (N^3/3 flop at 20 TFLOP/s), at least 50 ms
        const double expect_s = (double)(nblk * TILE) * (double)(nblk * TILE) * (double)(nblk * TILE) / 3.0 / 20e12;
        const unsigned long long limit = (unsigned long long)((0.05 + 4.0 * expect_s) * 1e8);
        hipLaunchKernelGGL(cu_blocker_kernel, dim3((unsigned)nres), dim3(256), 0, s_blk, (const int *)stop_flag, placed, limit);
        hipLaunchKernelGGL(wait_placed_kernel, dim3(1), dim3(1), 0, s, (const int *)placed, nres, 20000ull);   // <= 200 us
        GPX_HIP(hipGetLastError());
        reserved = true;
        return 0;
    }
    // On the main stream, in front of the factorisation's first event: the trapezoid launches' counters and the square launches' state
    // words zeroed, every square launch's tables uploaded (one copy), the first panel's gate opened (its columns are complete when the
    // factorisation is called); then the chain's stream and the column solves' are forked off.
    int prepare()
    {
        if (trap_on) GPX_HIP(hipMemsetAsync(sig, 0, sizeof(int) * (size_t)(P * CHOL_NBP), s));
        if (sqk_buf) {
            sqk_tab_host.assign((size_t)(P * SQK_TAB), 0);
            for (int64_t pp = 0; pp < P; ++pp) {
                const int rows = (int)(bnd(pp + 1) - bnd(pp)), nbr = rows + (int)sqk_below(pp);
                if (use_sqk(pp) && (chol_dataflow_state_ints(nbr) > SQK_GATE || chol_dataflow_fill_tables(nbr, rows, sqk_tab_host.data() + pp * SQK_TAB, (int)SQK_TAB) < 0)) {
                    gpx_set_error("chol_factor: square launch of %d + %d block rows does not fit its state / table slot", rows, nbr - rows);
                    return GPX_ERR_STATE;
                }
            }
            GPX_HIP(hipMemsetAsync(sqk_buf, 0, sizeof(int) * (size_t)(P * SQK_STATE), s));
            GPX_HIP(hipMemcpyAsync(sqk_tab(0), sqk_tab_host.data(), sizeof(int) * sqk_tab_host.size(), hipMemcpyHostToDevice, s));
        }
        sqk_open_gate(0, s);
        GPX_HIP(hipEventRecord(ev0, s));
        GPX_HIP(hipStreamWaitEvent(s_pan, ev0, 0));
        for (int64_t q = 0; q < P; ++q) {
            tops[q].stream = piped(q) ? s_top : nullptr;
            tops[q].r0 = bnd(q + 1) + (use_sqk(q) ? sqk_below(q) : 0);   // (a square launch solves the next square's rows itself)
            tops[q].r1 = nblk;
            tops[q].events = &events;
        }
        if (piped(0)) GPX_HIP(hipStreamWaitEvent(s_top, ev0, 0));
        return 0;
    }
    // chain(0) and S(0).  after_fork -- main-stream work of the caller that only the later panels need (the rest of the Gram matrix) --
    // is queued behind the square launch, or behind the chain's first step, and runs underneath the first panel's chain.
    // (the first step is queued ahead of that launch; its leaf is NOT exclusive: the Gram kernel, released on the main stream at
    // the same moment, usually wins the race for the places, and an exclusive leaf would then wait for the whole launch to drain)
    int first_panel()
    {
        if (use_sqk(0)) {
            GPX_TRY(sqk_launch(0, 0, bnd(1)));
            follow_square(0);
            if (after_fork) GPX_TRY((*after_fork)());
            if (tops[0].stream && tops[0].r1 > tops[0].r0)
                for (int64_t j = 0; j < bnd(1); ++j) GPX_TRY(top_column(L, ld, 0, j, Dinv, &tops[0], prof));
        } else {
            GPX_TRY(chol_square_steps(L, ld, 0, bnd(1), 0, 1, Dinv, diagL, info_dev, s_pan, prof, &tops[0], 0));
            if (after_fork) GPX_TRY((*after_fork)());
            GPX_TRY(chol_square_steps(L, ld, 0, bnd(1), 1, bnd(1), Dinv, diagL, info_dev, s_pan, prof, &tops[0], 2));   // nothing else fills the chip yet: every leaf finds an empty CU
        }
        if (piped(0)) GPX_HIP(hipEventRecord(ev_top[0], s_top));
        GPX_HIP(hipEventRecord(ev_pf[0], s_pan));
        return 0;
    }
    // Q(p): the update of diagonal square p + 1 with panel p's rows [B1, B2).  Only those rows and that square gate the next chain: the
    // square is updated before anything else so that the side stream starts early.  Without a column stream the rows below panel p are
    // solved here first, in one recursive TRSM on the main stream.
    // Which stream: the main one -- except in the tail of the factorisation (short trailing updates, issued as separate launches), where
    // T(p-1) computed the tiles of diagonal square p + 1 FIRST, as a launch of their own, and marked them (ev_sqp): Q(p) -- what
    // chain(p + 1) waits for -- then runs on the CHAIN's stream right behind chain(p) instead of on the main stream behind all of T(p-1),
    // which runs beside chain(p) at a fraction of the chip (65 CUs belong to the square launch) and used to end 60-240 us after it.
    int square_update(int64_t p)
    {
        const int64_t B0 = bnd(p), B1 = bnd(p + 1), B2 = bnd(p + 2);
        const bool late = top_late(p), on_chain = q_on_chain(p);
        if (piped(p) && !late) GPX_HIP(hipStreamWaitEvent(s, ev_top[p], 0));          // solved column by column alongside the chain
        else if (!piped(p)) GPX_TRY(trsm_right_lt(L + (B1 * TILE) * ld, ld, (nblk - B1) * TILE, L, ld, Dinv, B0, B1, s, prof));
        const double *Ptop = L + (B1 * TILE) * ld + B0 * TILE;         // panel p, rows [B1,B2)
        if (on_chain) {
            // (chain(p) precedes on s_pan; the rows [B1, B2) of panel p: a square launch solved them itself, else the column stream)
            GPX_HIP(hipStreamWaitEvent(s_pan, ev_sqp[p - 1], 0));
            if (!late) GPX_HIP(hipStreamWaitEvent(s_pan, ev_top[p], 0));
        }
        // (lower 32 x 32 tiles only: nothing reads the square above its diagonal -- the bulk launches never updated it there)
        GPX_TRY(launch_gemm_nt(Ptop, ld, Ptop, ld, L + (B1 * TILE) * ld + B1 * TILE, ld, (B2 - B1) * TILE, (B2 - B1) * TILE, (B1 - B0) * TILE,
                               -1.0, 1.0, 1, on_chain ? s_pan : s, prof));
        if (!on_chain) GPX_HIP(hipEventRecord(ev_next[p], s));
        // from the first tail panel that runs as a square launch the chain no longer lives on the reserved CUs (a square launch brings
        // its own: one workgroup per CU): the blockers would only keep 32 CUs from the short bulk launches beside it
        if (sqk_from() < 0 && use_sqk(p + 1)) release_blockers();
        return 0;
    }
    // The chain of panel q = p + 1 starts behind Q(p): the whole of it where it is a square launch, else its first step.
    // Host enqueue order: first step of the chain, then the main stream's bulk work (trailing_update), then the rest of the chain
    // (finish_chain), so neither stream starves while the other's launches are being queued.
    // (the first leaf is exclusive only where a free CU is certain -- reserved CUs, or no bulk launch left: next to the main stream's
    // launch, which becomes ready at the same moment, an exclusive leaf that loses the race for a place waits for a whole CU to drain)
    int start_chain(int64_t q)
    {
        const int64_t p = q - 1, B1 = bnd(q), B2 = bnd(q + 1);
        if (!q_on_chain(p)) GPX_HIP(hipStreamWaitEvent(s_pan, ev_next[p], 0));
        if (use_sqk(q)) return sqk_launch(q, B1, B2);
        GPX_TRY(chol_square_steps(L, ld, B1, B2, B1, B1 + 1, Dinv, diagL, info_dev, s_pan, prof, nullptr, (reserved || B2 >= nblk) ? 1 : 0));
        if (piped(q)) GPX_HIP(hipEventRecord(ev_first[p], s_pan));
        return 0;
    }
    // T(p) on the main stream: the rest of panel p + 1's columns (the narrow part), then the bulk SYRK of everything right of them; and
    // S(p + 1)'s first column, which may start as soon as the narrow part is through.  Three forms:
    //  - ONE trapezoid launch for the narrow part AND the bulk (gemm.hip, launch_syrk_trap_signal): its narrow tiles come first and are
    //    counted in sig[p]; every column solve of the next panel waits for its own column's count (top_column), not for a launch boundary.
    //    Handing the count over as an event from a stream of its own was measured too: one more cross-stream edge per panel, fit +1.4 ms.
    //  - small trailing matrices (fewer than trap_min tiles; 100 tiles measured, no difference) keep the two launches, narrow and bulk.
    //    Beside a square launch the next panel's column solves wait for the narrow launch and the chip is nearly empty: it then runs on
    //    64 x 64 tiles, which finish in a third of a 128 x 128 tile's time (the short bulk launch on such tiles: measured, no difference).
    //  - the split tail form of the bulk: the tiles of diagonal square p + 2 first and marked (ev_sqp: see square_update), then the rows
    //    below them (trapezoid: the square's columns in full, then the triangle) -- the same tiles with the same arithmetic as the one launch.
    int trailing_update(int64_t p)
    {
        const int64_t B0 = bnd(p), B1 = bnd(p + 1), B2 = bnd(p + 2), B3 = bnd(p + 3), K = (B1 - B0) * TILE, nrem = nblk - B2;
        if (top_late(p)) GPX_HIP(hipStreamWaitEvent(s, ev_top[p], 0));
        sq_split_prev = false;
        if (nrem <= 0) return 0;
        const double *Ptop = L + (B1 * TILE) * ld + B0 * TILE;     // panel p, rows [B1,B2)
        const double *Pr = L + (B2 * TILE) * ld + B0 * TILE;       // panel p, rows >= B2
        int merged = GPX_ERR_STATE;
        constexpr long trap_min = 1024;
        // the group route: the triangle part ends at column far(p) -- wt of its nrem tile columns (rows still run to nblk)
        const int64_t fc = std::min(nblk, std::max(B2, far_blk(p))), wt = fc - B2;
        if (trap_on && bulk_tiles(p) >= trap_min && B2 - B1 == CHOL_NBP)
            merged = launch_syrk_trap_signal(Pr, ld, Ptop, ld, L + (B2 * TILE) * ld + B1 * TILE, ld, nrem * TILE, (B2 - B1) * TILE, K, -1.0, 1.0,
                                             sig + p * CHOL_NBP, s, prof, wt * TILE);
        if (merged != 0 && merged != GPX_ERR_STATE) return merged;
        if (merged != 0)
            GPX_TRY(launch_gemm_nt(Pr, ld, Ptop, ld, L + (B2 * TILE) * ld + B1 * TILE, ld, nrem * TILE, (B2 - B1) * TILE,
                                   K, -1.0, 1.0, 0, s, prof, 0, 0, (use_sqk(p + 1) && p + 1 > 0) ? 1 : 0));
        sqk_open_gate(p + 1, s);   // panel p+1's columns have their update: its square launch may solve the rows below its square
        if (piped(p + 1)) {   // panel p+1's rows below its square are complete: its column solves may start (first column now)
            TopPipe &top = tops[(size_t)p + 1];
            if (merged == 0) {
                top.colsig = sig + p * CHOL_NBP;
                top.colwant = (int)nrem;
                top.stall = stall;
            } else {
                GPX_HIP(hipEventRecord(ev_tu[p], s));
                GPX_HIP(hipStreamWaitEvent(s_top, ev_tu[p], 0));
            }
            if (use_sqk(p + 1)) follow_square(p + 1);
            else GPX_HIP(hipStreamWaitEvent(s_top, ev_first[p], 0));
            GPX_TRY(top_column(L, ld, B1, B1, Dinv, &top, prof));
        }
        if (merged != 0 && wt < nrem) {
            // the same in the group route (nothing where panel p + 1 ends its group): diagonal square p + 2 first and marked, the rows
            // below it down to row far(p) as a trapezoid, the rows from far(p) on as a rectangle
            if (wt > 0) {
                GPX_TRY(launch_gemm_nt(Pr, ld, Pr, ld, L + (B2 * TILE) * ld + B2 * TILE, ld, (B3 - B2) * TILE, (B3 - B2) * TILE, K, -1.0, 1.0, 1, s, prof));
                GPX_HIP(hipEventRecord(ev_sqp[p], s));
                sq_split_prev = true;
                if (B3 < fc)
                    GPX_TRY(launch_gemm_nt(Pr + ((B3 - B2) * TILE) * ld, ld, Pr, ld, L + (B3 * TILE) * ld + B2 * TILE, ld, (fc - B3) * TILE, wt * TILE, K,
                                           -1.0, 1.0, 1, s, prof));
                GPX_TRY(launch_gemm_nt(Pr + (wt * TILE) * ld, ld, Pr, ld, L + (fc * TILE) * ld + B2 * TILE, ld, (nblk - fc) * TILE, wt * TILE, K, -1.0, 1.0, 0,
                                       s, prof));
            }
        } else if (merged != 0 && p + 2 < P && B3 > B2) {
            GPX_TRY(launch_gemm_nt(Pr, ld, Pr, ld, L + (B2 * TILE) * ld + B2 * TILE, ld, (B3 - B2) * TILE, (B3 - B2) * TILE, K, -1.0, 1.0, 1, s, prof));
            GPX_HIP(hipEventRecord(ev_sqp[p], s));
            sq_split_prev = true;
            if (B3 < nblk)
                GPX_TRY(launch_gemm_nt(Pr + ((B3 - B2) * TILE) * ld, ld, Pr, ld, L + (B3 * TILE) * ld + B2 * TILE, ld, (nblk - B3) * TILE,
                                       nrem * TILE, K, -1.0, 1.0, 1, s, prof));
        } else if (merged != 0)
            GPX_TRY(launch_gemm_nt(Pr, ld, Pr, ld, L + (B2 * TILE) * ld + B2 * TILE, ld, nrem * TILE, nrem * TILE, K, -1.0, 1.0, 1, s, prof));
        // once the remaining bulk launches no longer fill the chip the reservation has nothing left to protect
        if (B3 >= nblk) release_blockers();   // the last bulk launch is queued
        return 0;
    }
    // Group boundary behind panel p, in the place of Q(p) and T(p): every column right of the group takes the group's columns at once,
    // C[i, j] -= sum_k L[i, k] L[j, k] over the group's k for far <= j <= i, on the int8 path (emu.hip: emu_syrk_split, emu_syrk_panel).
    // All of it on the main stream, column panels in ascending order, so that every later T(q) -- which rewrites the same columns -- is
    // ordered behind it; the new cross-stream edges are events: the next chain and the next panel's column solves wait for column
    // panel 0 alone (ev_next, ev_tu) and run underneath the remaining column panels.  The group's rows >= far are complete: the column
    // solves of the earlier panels were waited for by their T(q), panel p's are waited for here (its square launch's share: ev_pf).
    // A failed pivot leaves NaN rows whose residues are zero and whose outputs are NaN: no wait depends on them.
    int group_boundary(int64_t p)
    {
        const int64_t g0 = bnd(p + 1 - G), B1 = bnd(p + 1), rows = (nblk - B1) * TILE, K = (B1 - g0) * TILE;
        if (piped(p)) GPX_HIP(hipStreamWaitEvent(s, ev_top[p], 0));
        else GPX_TRY(trsm_right_lt(L + (B1 * TILE) * ld, ld, (nblk - B1) * TILE, L, ld, Dinv, bnd(p), B1, s, prof));
        GPX_TRY(drop_reservation());
        sq_split_prev = false;
        double *C = L + (B1 * TILE) * ld + B1 * TILE;
        esy.use(emu_syrk_plan(rows, K));
        GPX_TRY(emu_syrk_split(esy, L + (B1 * TILE) * ld + g0 * TILE, ld, rows, s));
        GPX_TRY(emu_syrk_panel(esy, 0, C, ld, rows, s, prof, TILE));
        GPX_HIP(hipEventRecord(ev_next[p], s));
        GPX_TRY(start_chain(p + 1));
        sqk_open_gate(p + 1, s);
        if (piped(p + 1)) {   // as behind a narrow launch (trailing_update): panel p + 1's rows below its square are complete
            GPX_HIP(hipEventRecord(ev_tu[p], s));
            GPX_HIP(hipStreamWaitEvent(s_top, ev_tu[p], 0));
            if (use_sqk(p + 1)) follow_square(p + 1);
            else GPX_HIP(hipStreamWaitEvent(s_top, ev_first[p], 0));
            GPX_TRY(top_column(L, ld, B1, B1, Dinv, &tops[(size_t)p + 1], prof));
        }
        for (int64_t q = 1; q * CHOL_PANEL_COLS < rows; ++q) GPX_TRY(emu_syrk_panel(esy, q, C, ld, rows, s, prof, TILE));
        return 0;
    }
    // The rest of chain(q) and of S(q), q = p + 1, behind the main stream's launches of this panel: a square launch runs already (one
    // launch) and the column solves of the rows below follow its step counter; else the chain's remaining steps, each with its column
    // solve, every leaf exclusive where it finds an empty CU -- reserved CUs, or (last panels) a nearly empty chip.
    int finish_chain(int64_t q)
    {
        const int64_t B1 = bnd(q), B2 = bnd(q + 1);
        const TopPipe &top = tops[(size_t)q];
        if (!use_sqk(q))
            GPX_TRY(chol_square_steps(L, ld, B1, B2, B1 + 1, B2, Dinv, diagL, info_dev, s_pan, prof, &top, (reserved || bnd(q + 2) >= nblk) ? 2 : 0));
        else if (top.stream && top.r1 > top.r0)
            for (int64_t j = B1 + 1; j < B2; ++j) GPX_TRY(top_column(L, ld, B1, j, Dinv, &top, prof));
        if (piped(q)) GPX_HIP(hipEventRecord(ev_top[q], s_top));
        GPX_HIP(hipEventRecord(ev_pf[q], s_pan));
        return 0;
    }
};
}   // namespace

// The factorisation (the picture: DESIGN.md, section 5.1).  Per outer panel p the main stream runs, in order: update of panel p+1's diagonal
// square (panel p's rows of that square are solved by then) -> event: the side stream starts the next chain;  update of the remaining rows
// of panel p+1's columns;  bulk SYRK of everything right of panel p+1.  The side stream runs the diagonal-square chain of panel p+1 (leaf
// kernels and tiny GEMMs, pure latency) underneath all of that, and the third stream solves ALL rows below panel p's square column by
// column alongside panel p's chain (TopPipe), so that neither a top slice nor a panel TRSM remains on the main stream.
int chol_factor(double *L, int64_t ld, int64_t nblk, double *Dinv, double *diagL, int *info_dev, hipStream_t s,
                hipStream_t s_pan, Profiler *prof, hipStream_t s_top, const std::function<int()> *after_fork,
                const std::function<int(int64_t, int64_t, bool)> *panel_final)
{
    const int64_t last = (nblk + CHOL_NBP - 1) / CHOL_NBP - 1;   // the last outer panel
    const bool lookahead = nblk > CHOL_NBP && s_pan != nullptr;
    const bool whole = !g_force_plain && chol_dataflow_supported(nblk);   // the whole factorisation may be the dataflow kernel's
    if (!lookahead) {   // everything on s
        if (after_fork) GPX_TRY((*after_fork)());
        if (whole && nblk > CHOL_NBP && nblk <= 64 && dflow_small_enabled())
            GPX_TRY(small_dataflow_factor(L, ld, nblk, Dinv, diagL, info_dev, s));
        else
            GPX_TRY((nblk <= CHOL_NBP) ? chol_panel_factor(L, ld, nblk, 0, nblk, Dinv, diagL, info_dev, s, prof)
                                       : chol_rec(L, ld, 0, nblk, Dinv, diagL, info_dev, s, prof));
        if (panel_final) GPX_TRY((*panel_final)(last, 0, true));
        return 0;
    }
    if (whole && nblk <= dflow_max_blocks()) {
        SoloToken token;       // (a look-ahead fit on another thread sees this one in flight)
        WholeDataflow df(s);   // (waits for s on the way out, behind whatever the caller's hooks queue)
        GPX_TRY(df.take(nblk));
        if (after_fork) GPX_TRY((*after_fork)());
        GPX_TRY(df.launch(L, ld, nblk, Dinv, diagL, info_dev));
        if (panel_final) GPX_TRY((*panel_final)(last, 0, true));
        return 0;
    }
    Lookahead la{L, ld, nblk, Dinv, diagL, info_dev, s, s_pan, s_top, prof, after_fork, panel_final};
    GPX_TRY(la.setup());
    GPX_TRY(la.prepare());
    GPX_TRY(la.first_panel());
    for (int64_t p = 0; p <= last; ++p) {
        GPX_HIP(hipStreamWaitEvent(s, la.ev_pf[p], 0));   // diagonal square of panel p is factored
        if (p == last) return la.hook(p, 0, true);
        if (la.boundary(p)) GPX_TRY(la.group_boundary(p));
        else {
            GPX_TRY(la.reserve_now(p));
            GPX_TRY(la.square_update(p));
            GPX_TRY(la.start_chain(p + 1));
            GPX_TRY(la.trailing_update(p));
        }
        GPX_TRY(la.hook(p, (nblk - la.bnd(p + 2) + CHOL_NBP - 1) / CHOL_NBP, false));
        GPX_TRY(la.finish_chain(p + 1));
        la.mark();
    }
    return 0;
}
