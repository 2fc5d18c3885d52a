// Host-only replay of the emulated updates' three drivers (emu.hip: the left-looking solve's image with tsolve.hip trsm_right_lt_slabs, the
// recursion's emu_gemm_nt_sub, the factorisation's symmetric update), in the manner of replay_chol.hip: both files are compiled into this
// program, every launch and HIP runtime call is replaced by a function that checks it and prints one line.  The checks: every byte a
// launch reads or writes lies inside a block the driver took (the image, the B tile, the product residues, the scales) or the caller's
// matrices, 16-byte alignment where the kernels store 16 bytes, a row tile's image spans at most 2 GiB, the grids match the tile counts;
// left-looking solve: each solved slab is split exactly once and before its first use, an image that does not fit is given back whole,
// the route is chosen by the kind of call and the factor's shape, and a raised status word reruns the chunk once through the recursion;
// symmetric update: B's window lies inside the image and starts on a 1024-row boundary of a row tile, nothing stays held after a pool that
// is too small.  Needs no GPU; meant to run under the host sanitizers:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I<tree>/scikit-gpuppy_amd/csrc \
//         -DTSOLVE_PATH='"<tree>/scikit-gpuppy_amd/csrc/tsolve.hip"' -DEMU_PATH='"<tree>/scikit-gpuppy_amd/csrc/emu.hip"' replay_left.hip -o replay_left
//   ./replay_left          the left-looking solve (exit status 0: every check held)
//   ./replay_left drives   the recursion's update and the symmetric update
// REPLAY_LOG=1 adds one line per launch (kernel, grid.x, block.x, every scalar argument, every pointer as block-in-order-of-allocation +
// byte offset) and per dalloc / dfree: build the program for two trees and diff (profiles/r27_emu_frame.txt).  A tree from before the one
// workspace frame (EmuWork / EmuLeft / EmuSyrk): add -DREPLAY_THREE_FRAMES.
#include TSOLVE_PATH
#include EMU_PATH
#include <cstdarg>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#ifdef REPLAY_THREE_FRAMES
typedef EmuLeft LeftW;
typedef EmuWork WorkW;
typedef EmuSyrk SyrkW;
struct Geo { int64_t ld, rt, tiles, img_bytes; int L, abits, bbits; };
static Geo left_plan(LeftW &w, int64_t rows, int64_t slabs, int64_t tile_rows) { emu_left_plan(w, rows, slabs, tile_rows); return {w.lda, w.rt, w.tiles, w.img_bytes, w.L, w.abits, w.bbits}; }
static int left_alloc(LeftW &w, Scratch &sc) { return emu_left_alloc(w, sc); }
static int work_alloc(WorkW &w, Scratch &sc, int64_t rows, int64_t cols, int64_t K) { emu_work_need(w, rows, cols, K); return emu_work_alloc(w, sc); }
static int syrk_alloc(SyrkW &w, int64_t rows, int64_t K, int64_t tile_rows) { emu_syrk_plan(w, rows, K, tile_rows); return emu_syrk_alloc(w); }
static Geo syrk_use(SyrkW &w, int64_t rows, int64_t K, int64_t tile_rows) { emu_syrk_plan(w, rows, K, tile_rows); return {w.K, w.rt, w.tiles, w.tiles * w.rt * w.K * w.L, w.L, w.bits, w.bits}; }
static void syrk_free(SyrkW &w) { emu_syrk_free(w); }
static const int8_t *image_of(const SyrkW &w) { return w.img; }
#else
typedef EmuFrame LeftW, WorkW, SyrkW;
struct Geo { int64_t ld, rt, tiles, img_bytes; int L, abits, bbits; };
static Geo geo(const EmuFrame &w) { return {w.a.ld, w.a.rt, w.a.tiles, w.need.img, (int)w.a.L, w.abits, w.bbits}; }
static Geo left_plan(LeftW &w, int64_t rows, int64_t slabs, int64_t tile_rows) { w.use(emu_left_plan(rows, slabs, tile_rows)); w.reserve(w); return geo(w); }
static int left_alloc(LeftW &w, Scratch &sc) { return emu_alloc(w, &sc); }
static int work_alloc(WorkW &w, Scratch &sc, int64_t rows, int64_t cols, int64_t K) { w.reserve(emu_work_plan(rows, cols, K)); return emu_alloc(w, &sc); }
static int syrk_alloc(SyrkW &w, int64_t rows, int64_t K, int64_t tile_rows) { w.reserve(emu_syrk_plan(rows, K, tile_rows)); return emu_alloc(w, nullptr); }
static Geo syrk_use(SyrkW &w, int64_t rows, int64_t K, int64_t tile_rows) { w.use(emu_syrk_plan(rows, K, tile_rows)); return geo(w); }
static void syrk_free(SyrkW &w) { emu_free(w); }
static const int8_t *image_of(const SyrkW &w) { return w.a.base; }
#endif

static char *const BASE = (char *)0x100000000000ull;
struct Block { size_t bytes; int index; };
static std::map<char *, Block> g_blocks;           // live pool blocks, numbered in order of allocation
static char *g_pool = BASE;
static int g_next_index = 0;
static int64_t g_budget = -1;                      // bytes the pool may still hand out (-1: unlimited)
static int g_fail = 0;
static std::set<long> g_split;                     // slabs of the image that have been written
static int64_t g_lda = 0;                          // the row stride every int8 product must read A with
enum { LEFT, GEMM, SYRK };
static int g_drive = LEFT;
static const int8_t *g_image = nullptr;            // GEMM, SYRK: A's residues (a split that writes there is A's)
static Geo g_geo;                                  // SYRK: the image's geometry
static const bool g_log = getenv("REPLAY_LOG") != nullptr;

#define CHECK(c, ...) do { if (!(c)) { printf("CHECK FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); ++g_fail; } } while (0)

static std::map<char *, Block>::iterator block_of(const void *p)
{
    auto it = g_blocks.upper_bound((char *)p);
    if (it == g_blocks.begin()) return g_blocks.end();
    --it;
    return (char *)p < it->first + it->second.bytes ? it : g_blocks.end();
}
static bool inside(const void *p, size_t first, size_t last)   // bytes [first, last] from p inside one live block
{
    auto it = block_of((char *)p + first);
    return it != g_blocks.end() && (char *)p + last < it->first + it->second.bytes;
}

// one log line: the kernel, grid.x, block.x and its arguments by kind -- p: pointer, l: long, i: int, -: not printed (a table by value)
template <class T> static T arg(void **a, int i) { return *(T *)a[i]; }
static void log_launch(const char *name, dim3 g, dim3 b, void **a, const char *kinds)
{
    if (!g_log) return;
    printf("L %s g%u b%u", name, g.x, b.x);
    for (int i = 0; kinds[i]; ++i) {
        if (kinds[i] == 'l') printf(" %ld", arg<long>(a, i));
        else if (kinds[i] == 'i') printf(" %d", arg<int>(a, i));
        else if (kinds[i] == 'p') {
            const char *p = arg<char *>(a, i);
            auto it = block_of(p);
            if (it == g_blocks.end()) printf(" %s", p ? "?" : "null");
            else printf(" #%d+%ld", it->second.index, (long)(p - it->first));
        }
    }
    printf("\n");
}

int Profiler::begin(hipStream_t, int, double) { return -1; }
void Profiler::end(hipStream_t, int) {}
static char g_err[256];
void gpx_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int gpx_require_device() { return 0; }
int dalloc(double **p, int64_t elems)
{
    const size_t bytes = ((size_t)elems * 8 + 255) / 256 * 256;
    if (g_budget >= 0 && (int64_t)bytes > g_budget) { *p = nullptr; gpx_set_error("out of memory"); if (g_log) printf("L dalloc %zu refused\n", bytes); return GPX_ERR_HIP; }
    if (g_budget >= 0) g_budget -= bytes;
    *p = (double *)g_pool;
    g_blocks[g_pool] = {bytes, g_next_index};
    if (g_log) printf("L dalloc #%d %zu\n", g_next_index, bytes);
    ++g_next_index;
    g_pool += bytes + (1 << 20);
    return 0;
}
void dfree(void *p)
{
    if (!p) return;   // (as the pool: nothing to give back)
    auto it = g_blocks.find((char *)p);
    CHECK(it != g_blocks.end(), "free of an unknown block");
    if (it == g_blocks.end()) return;
    if (g_log) printf("L dfree #%d\n", it->second.index);
    g_blocks.erase(it);
}
int launch_gemm_nt(const double *, int64_t, const double *, int64_t, double *, int64_t, int64_t M, int64_t N, int64_t K, double, double, int, hipStream_t,
                   Profiler *, int, int, int, int *)
{
    printf("  gemm %ld x %ld x %ld\n", (long)M, (long)N, (long)K);
    return 0;
}
int launch_gemm_nt_tri_reduce(const double *, int64_t, const double *, int64_t, double *, int64_t, int64_t M, int64_t N, double, const GemmReduce &, hipStream_t,
                              Profiler *)
{
    printf("  leaf+reduce %ld x %ld\n", (long)M, (long)N);
    return 0;
}
int launch_gemm_nt_batched(const double *, int64_t, GemmBatch, const double *, int64_t, GemmBatch, double *, int64_t, GemmBatch, int64_t, int64_t, int64_t, double,
                           double, int64_t, hipStream_t) { return 0; }

int launch_symmetrize_lower(double *, int64_t, int64_t, hipStream_t) { return 0; }

// SYRK: an operand of the int8 product is a window of `rows` rows of the image that starts at p -- inside one row tile's plane 0, on a row
static void check_window(const int8_t *p, long rows, long plane, bool on_slab, const char *what)
{
    const long K = g_geo.ld, tile_bytes = g_geo.rt * K * g_geo.L, off = (long)(p - g_image), within = off % tile_bytes, row = within / K;
    CHECK(off >= 0 && off / tile_bytes < g_geo.tiles && plane == g_geo.rt * K, "%s: not a row tile of the image", what);
    CHECK(within % K == 0 && row + rows <= g_geo.rt, "%s: rows %ld .. %ld leave the row tile's plane", what, row, row + rows);
    if (on_slab) CHECK(row % 1024 == 0, "%s starts at row %ld of its tile, not on a 1024-row boundary", what, row);
}

extern "C" {
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipMemsetAsync(void *p, int, size_t n, hipStream_t) { CHECK(inside(p, 0, n - 1), "memset outside a block"); return hipSuccess; }
hipError_t hipMemcpyAsync(void *, const void *, size_t, hipMemcpyKind, hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *, hipEvent_t, hipEvent_t) { return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
static dim3 g_grid, g_block; static size_t g_shm; static hipStream_t g_st;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t shm, hipStream_t s) { g_grid = g; g_block = b; g_shm = shm; g_st = s; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *shm, hipStream_t *s) { *g = g_grid; *b = g_block; *shm = g_shm; *s = g_st; return hipSuccess; }
hipError_t hipLaunchKernel(const void *f, dim3 g, dim3 b, void **a, size_t, hipStream_t)
{
    if (f == (const void *)emu_scale_from_bound_kernel) {
        log_launch("scale_from_bound", g, b, a, "pllipp");
        const long rows = arg<long>(a, 1), rp = arg<long>(a, 2);
        CHECK((long)g.x * 256 >= rp && rows <= rp, "scale grid");
        CHECK(inside(arg<int *>(a, 4), 0, 4 * rp - 1) && inside(arg<int *>(a, 5), 0, 3), "scales / status outside their block");
        printf("  scales %ld rows (%ld padded)\n", rows, rp);
    } else if (f == (const void *)emu_split_fixed_kernel) {      // one wave per row, four rows per workgroup
        log_launch("split_fixed", g, b, a, "pllliiipllpp");
        const long ldx = arg<long>(a, 1), real = arg<long>(a, 2), rp = arg<long>(a, 3), ldr = arg<long>(a, 8), plane = arg<long>(a, 9);
        const int width = arg<int>(a, 4), L = arg<int>(a, 6);
        int8_t *res = arg<int8_t *>(a, 7);
        (void)ldx;
        CHECK(real <= rp && rp % 256 == 0 && (long)g.x * 4 >= rp, "split rows");
        CHECK(width % 16 == 0 && width <= 1024 && ldr % 16 == 0 && plane % 16 == 0 && (uintptr_t)res % 16 == 0, "fixed split: 16-byte stores");
        CHECK(inside(res, 0, (size_t)(L - 1) * plane + (size_t)(rp - 1) * ldr + width - 1), "fixed split writes outside the image");
        CHECK((size_t)L * plane <= ((size_t)1 << 31), "a row tile's image spans more than 2 GiB");
        CHECK(inside(arg<int *>(a, 10), 0, 4 * real - 1) && inside(arg<int *>(a, 11), 0, 3), "fixed split scales / status");
        auto it = g_blocks.upper_bound((char *)res);
        const long off = it == g_blocks.begin() ? 0 : (long)((char *)res - (--it)->first), q = off % ldr / 1024;
        if (off < ldr) CHECK(g_split.insert(q).second, "slab %ld split twice", q);      // (the first row tile's launch)
        else CHECK(g_split.count(q) == 1, "slab %ld: a later row tile first", q);
        printf("  split slab rows %ld\n", rp);
    } else if (f == (const void *)emu_row_scale_kernel) {        // one workgroup per padded row: writes every scale of the tile
        log_launch("row_scale", g, b, a, "plliip");
        const long ldx = arg<long>(a, 1), real = arg<long>(a, 2);
        const int K = arg<int>(a, 3);
        CHECK(real <= (long)g.x && inside(arg<int *>(a, 5), 0, 4 * g.x - 1), "B scales outside their block");
        CHECK(real == 0 || inside(arg<const double *>(a, 0), 0, 8 * ((size_t)(real - 1) * ldx + K) - 1), "the scales' rows outside the matrix");
        printf("  B scales %u x %d\n", g.x, K);
    } else if (f == (const void *)emu_split_kernel) {            // one wave per (row, stretch of 1024 columns)
        log_launch("split", g, b, a, "pllliiplp");
        const long ldx = arg<long>(a, 1), real = arg<long>(a, 2), rp = arg<long>(a, 3), plane = arg<long>(a, 7);
        const int K = arg<int>(a, 4), L = arg<int>(a, 5);
        const int8_t *res = arg<int8_t *>(a, 6);
        const bool is_a = g_drive != LEFT && block_of(res) == block_of(g_image);
        CHECK(real <= rp && (g_drive == SYRK ? plane >= rp * K : plane == rp * K) && (long)g.x * 4 >= rp * ((K + 1023) / 1024), "B split shape");
        CHECK(K % 16 == 0 && plane % 16 == 0 && (uintptr_t)res % 16 == 0, "B split: 16-byte stores");
        CHECK(inside(res, 0, (size_t)(L - 1) * plane + (size_t)rp * K - 1) && inside(arg<const int *>(a, 8), 0, 4 * real - 1), "B split writes outside its tile");
        CHECK((size_t)L * plane <= ((size_t)1 << 31), "a tile's planes span more than 2 GiB");
        CHECK(real == 0 || inside(arg<const double *>(a, 0), 0, 8 * ((size_t)(real - 1) * ldx + K) - 1), "the split's rows outside the matrix");
        if (g_drive == LEFT)
            for (long q = 0; q < K / 1024; ++q) CHECK(g_split.count(q) == 1, "slab %ld read before it was split", q);
        if (g_drive == SYRK) check_window(res, rp, plane, true, "the split");
        printf("  split %s %ld x %d\n", is_a ? "A" : "B", rp, K);
    } else if (f == (const void *)emu_i8_gemm_kernel) {
        log_launch("i8_gemm", g, b, a, "ppllipllii" "i");
        const long sa = arg<long>(a, 2), sb = arg<long>(a, 3), ldr = arg<long>(a, 6), sr = arg<long>(a, 7);
        const int K = arg<int>(a, 4), tm = arg<int>(a, 8), tn = arg<int>(a, 9), lda = arg<int>(a, 10);
        const int L = (int)(g.x / (tm * tn));
        CHECK((int)g.x == tm * tn * L && L == emu_moduli() && b.x == 512 && lda >= K && lda == g_lda, "int8 grid / stride");
        CHECK(inside(arg<const int8_t *>(a, 0), 0, (size_t)(L - 1) * sa + (size_t)(256 * tm - 1) * lda + K - 1), "int8 product reads outside the image");
        CHECK(inside(arg<const int8_t *>(a, 1), 0, (size_t)(L - 1) * sb + (size_t)(256 * tn) * K - 1), "int8 product reads outside the B tile");
        CHECK(inside(arg<int8_t *>(a, 5), 0, (size_t)(L - 1) * sr + (size_t)(256 * tm - 1) * ldr + 256 * tn - 1), "int8 product writes outside the residues");
        CHECK((size_t)255 * lda + K < ((size_t)1 << 31), "a panel's 32-bit byte offset");
        CHECK((size_t)L * sa <= ((size_t)1 << 31) && (size_t)L * sb <= ((size_t)1 << 31) && ldr == 256 * tn && sr == 256l * tm * ldr, "int8 planes");
        if (g_drive == SYRK) {
            check_window(arg<const int8_t *>(a, 0), 256l * tm, sa, false, "A's window");
            check_window(arg<const int8_t *>(a, 1), 256l * tn, sb, true, "B's window");
        }
        printf("  int8 %d x %d tiles, K %d, lda %d\n", tm, tn, K, lda);
    } else if (f == (const void *)emu_rebuild_kernel) {
        log_launch("rebuild", g, b, a, "plli-ppplllll");
        const long ldr = arg<long>(a, 1), sr = arg<long>(a, 2), ldc = arg<long>(a, 8), rows = arg<long>(a, 9), cols = arg<long>(a, 10);
        const int L = arg<int>(a, 3);
        CHECK((long)g.x * 256 >= rows * ((cols + 3) / 4) && ((long)g.x - 1) * 256 < rows * ((cols + 3) / 4) && ldr >= (cols + 3) / 4 * 4 && sr >= rows * ldr, "rebuild grid / planes");
        CHECK(inside(arg<const int8_t *>(a, 0), 0, (size_t)(L - 1) * sr + (size_t)(rows - 1) * ldr + ((cols + 3) / 4 * 4) - 1), "rebuild reads outside the residues");
        CHECK(inside(arg<const int *>(a, 5), 0, 4 * rows - 1) && inside(arg<const int *>(a, 6), 0, 4 * cols - 1), "rebuild scales");
        CHECK(inside(arg<double *>(a, 7), 0, 8 * ((size_t)(rows - 1) * ldc + cols) - 1), "rebuild writes outside C");
        printf("  rebuild %ld x %ld\n", rows, cols);
    } else {
        log_launch("other", g, b, a, "");
        printf("  kernel (other) grid %u\n", g.x);
    }
    return hipSuccess;
}
}

static void begin_drive(int drive)
{
    g_blocks.clear();
    g_split.clear();
    g_budget = -1;
    g_next_index = 0;
    g_drive = drive;
    g_image = nullptr;
}

static int run(int64_t rows, int64_t npad, int64_t tile_rows, int64_t budget)
{
    printf("== rows %ld npad %ld tile_rows %ld budget %ld\n", (long)rows, (long)npad, (long)tile_rows, (long)budget);
    begin_drive(LEFT);
    TriSolver ts;
    double *Lf = nullptr, *Z = nullptr, *Zs = nullptr, *bound = nullptr, *pl = nullptr;
    dalloc(&Lf, npad * npad); dalloc(&Z, rows * npad); dalloc(&Zs, rows * npad); dalloc(&bound, rows); dalloc(&pl, 8);
    ts.L = Lf; ts.ld = npad; ts.npad = npad; ts.nblk = npad / TILE; ts.P = (npad + PB - 1) / PB; ts.Pl = pl;
    const size_t before = g_blocks.size();
    int rc = 0;
    {
        Scratch sc(nullptr);
        LeftW w;
        const Geo p = left_plan(w, rows, ts.P, tile_rows);
        g_lda = p.ld;
        printf("  plan: lda %ld, %ld tile(s) of %ld rows, image %ld bytes, abits %d bbits %d\n", (long)p.ld, (long)p.tiles, (long)p.rt, (long)p.img_bytes, p.abits, p.bbits);
        CHECK(p.rt * p.ld * p.L <= ((int64_t)1 << 31) && p.tiles * p.rt >= round_up(rows, 256), "plan");
        g_budget = budget;
        rc = left_alloc(w, sc);
        g_budget = -1;
        if (rc) {
            CHECK(sc.blocks.empty() && g_blocks.size() == before, "an image that did not fit was not given back whole");
            printf("  no room: rc %d, %zu blocks held\n", rc, sc.blocks.size());
        } else {
            rc = emu_left_begin(w, bound, rows, nullptr);
            if (!rc) rc = trsm_right_lt_slabs(Z, Zs, npad, rows, &ts, nullptr, nullptr, nullptr, w);
            for (long q = 0; q + 1 < ts.P; ++q) CHECK(g_split.count(q) == 1, "slab %ld never split", q);
            CHECK(g_split.count(ts.P - 1) == 0, "the last slab needs no residues");
        }
    }
    CHECK(g_blocks.size() == before, "blocks left behind");
    ts.Pl = nullptr;   // (borrowed above: nothing for release() to free)
    printf("rc %d\n", rc);
    return rc;
}

// the recursion's update C[rows, cols] -= A B^T of depth K in a workspace made for it (A, B with a padded row stride)
static int run_gemm(int64_t rows, int64_t cols, int64_t K)
{
    printf("== gemm %ld x %ld x %ld\n", (long)rows, (long)cols, (long)K);
    begin_drive(GEMM);
    const int64_t lda = K + 128, ldc = cols + 2;
    double *A = nullptr, *B = nullptr, *C = nullptr;
    dalloc(&A, rows * lda); dalloc(&B, cols * lda); dalloc(&C, rows * ldc);
    g_lda = K;
    int rc = 0;
    {
        Scratch sc(nullptr);
        WorkW w;
        rc = work_alloc(w, sc, rows, cols, K);
        if (!rc) {
            g_image = (const int8_t *)sc.blocks.front();   // (the first block taken: A's row tile)
            rc = emu_gemm_nt_sub(A, lda, B, lda, C, ldc, rows, cols, K, w, nullptr, nullptr);
        }
    }
    CHECK(g_blocks.size() == 3, "blocks left behind");
    if (rc) printf("  error: %s\n", g_err);
    printf("rc %d\n", rc);
    return rc;
}

// the symmetric update of `rows` rows at depth K as gpx_emu_syrk_lower_sub_ex drives it: the workspace made for plan_rows rows (0: for
// `rows`) out of a pool of `budget` bytes, the geometry of `rows` rows set before the split, the column panels in ascending order
static int run_syrk(int64_t rows, int64_t K, int64_t tile_rows, int diag_tile, int64_t plan_rows, int64_t budget)
{
    printf("== syrk rows %ld K %ld tile_rows %ld diag_tile %d plan_rows %ld budget %ld\n", (long)rows, (long)K, (long)tile_rows, diag_tile, (long)plan_rows, (long)budget);
    begin_drive(SYRK);
    const int64_t lda = K + 128, ldc = rows + 2;
    double *A = nullptr, *C = nullptr;
    dalloc(&A, rows * lda); dalloc(&C, rows * ldc);
    g_lda = K;
    SyrkW w;
    g_budget = budget;
    int rc = syrk_alloc(w, std::max(rows, plan_rows), K, tile_rows);
    g_budget = -1;
    if (rc) printf("  no room: rc %d, %zu blocks held\n", rc, g_blocks.size() - 2);
    else {
        g_geo = syrk_use(w, rows, K, tile_rows);
        g_image = image_of(w);
        printf("  plan: %ld tile(s) of %ld rows, image %ld bytes, bits %d\n", (long)g_geo.tiles, (long)g_geo.rt, (long)g_geo.img_bytes, g_geo.abits);
        CHECK(g_geo.rt * K * g_geo.L <= ((int64_t)1 << 31) && g_geo.tiles * g_geo.rt >= round_up(rows, 256) && (g_geo.tiles == 1 || g_geo.rt % 1024 == 0), "plan");
        rc = emu_syrk_split(w, A, lda, rows, nullptr);
        for (int64_t q = 0; !rc && q * 1024 < rows; ++q) rc = emu_syrk_panel(w, q, C, ldc, rows, nullptr, nullptr, diag_tile);
        syrk_free(w);
    }
    CHECK(g_blocks.size() == 2, "blocks left behind");
    if (rc) printf("  error: %s\n", g_err);
    printf("rc %d\n", rc);
    return rc;
}

// the two fall-back decisions next to the image that does not fit: which solves take the route, and the rerun of a chunk whose status
// word came back raised
static void decisions()
{
    printf("== decisions\n");
    CHECK(emu_left_route(true, false, true, 5) && emu_left_route(true, false, true, 16), "a bounded many-row solve over 5 slabs or more takes the route");
    CHECK(!emu_left_route(false, false, true, 16), "no bounds (propagate_GA_many, K^-1): the recursion");
    CHECK(!emu_left_route(true, true, true, 16), "the few-vector solver: not this route");
    CHECK(!emu_left_route(true, false, false, 16), "no prepared squares: the recursion");
    CHECK(!emu_left_route(true, false, true, 4), "4 slabs: nothing deep enough");
    for (int use_left = 0; use_left < 2; ++use_left)
        for (int raise = 0; raise < 2; ++raise)
            for (int fail = 0; fail < 2; ++fail) {
                std::vector<int> seen;
                const int rc = emu_left_guarded(use_left != 0, [&](bool left, int *status) -> int {
                    seen.push_back(left);
                    if (fail) return GPX_ERR_HIP;
                    *status = left ? raise : 7;   // (a pass through the recursion reads no status word: whatever it leaves is not looked at)
                    return 0;
                });
                const std::vector<int> want = !use_left ? std::vector<int>{0} : (raise && !fail) ? std::vector<int>{1, 0} : std::vector<int>{1};
                CHECK(seen == want && rc == (fail ? GPX_ERR_HIP : 0), "guard use_left %d raise %d fail %d: %zu passes, rc %d", use_left, raise, fail, seen.size(), rc);
                printf("  use_left %d status %d error %d: %zu pass(es)\n", use_left, raise, fail, seen.size());
            }
}

int main(int argc, char **argv)
{
    int bad = 0;
    if (argc > 1 && !strcmp(argv[1], "drives")) {
        bad += run_gemm(1100, 1060, 130944) != 0;        // 2 x 2 tiles of 1024 (tests/test_emulated_bound.py)
        bad += run_gemm(46000, 3000, 128) != 0;          // the column tile shrunk under 2 GiB of product residues (the same)
        bad += run_gemm(16384, 8192, 8192) != 0;         // the C3 recursion's deepest update: one tile
        bad += run_gemm(300, 200, 4096) != 0;            // ragged padding on both sides
        for (int dt : {1, 32}) {
            bad += run_syrk(8192, 4096, 0, dt, 0, -1) != 0;        // one row tile, 8 column panels
            bad += run_syrk(2304, 4096, 1024, dt, 0, -1) != 0;     // 3 row tiles: panels 1 and 2 read B from inside tiles 1 and 2
            bad += run_syrk(1100, 512, 0, dt, 0, -1) != 0;         // ragged rows, a ragged last panel
            bad += run_syrk(8192, 4096, 0, dt, 28672, -1) != 0;    // the fit's order: made for the largest update, used for a later one
            bad += run_syrk(8192, 4096, 0, dt, 0, (int64_t)8192 * 4096 * emu_moduli() + 4096) == 0;   // the image fits, the product residues do not
        }
    } else {
        decisions();
        bad += run(384, 5120, 0, -1) != 0;
        bad += run(384, 6144, 0, -1) != 0;
        bad += run(384, 5248, 0, -1) != 0;            // a ragged last slab of 128 columns
        bad += run(640, 5120, 256, -1) != 0;          // three row tiles
        bad += run(16384, 16384, 0, -1) != 0;         // the flagship shape: two row tiles of 8192
        bad += run(32768, 65536, 0, -1) != 0;         // 63 slabs, row tiles of 2048
        bad += run(16384, 16384, 0, (int64_t)4200 << 20) == 0;   // the image fits, the rest does not: everything goes back
        bad += run(16384, 16384, 0, ((int64_t)4208 << 20) + 70000) == 0;   // all but the row bounds (the last block taken) fit: the same
        bad += run(16384, 16384, 0, (int64_t)1 << 30) == 0;   // nothing fits
    }
    printf("%s (%d failed checks, %d wrong results)\n", g_fail || bad ? "FAILED" : "ok", g_fail, bad);
    return g_fail || bad ? 1 : 0;
}
