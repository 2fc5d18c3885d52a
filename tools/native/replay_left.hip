// Host-only replay of the left-looking solve's driver (tsolve.hip trsm_right_lt_slabs, emu.hip EmuLeft), in the manner of replay_chol.hip:
// both files are compiled into this program, every launch and HIP runtime call is replaced by a function that checks it and prints one
// line.  The checks: every byte a launch reads or writes lies inside a block the driver took (the image, the B tile, the product
// residues, the scales), a row tile's image spans at most 2 GiB, each solved slab is split exactly once and before its first use, an
// image that does not fit is given back whole, the route is chosen by the kind of call and the factor's shape, and a raised status word
// reruns the chunk once through the recursion.  Needs no GPU; meant to run under the host sanitizers:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I<tree>/scikit-gpuppy_amd/csrc \
//         -DTSOLVE_PATH='"<tree>/scikit-gpuppy_amd/csrc/tsolve.hip"' -DEMU_PATH='"<tree>/scikit-gpuppy_amd/csrc/emu.hip"' replay_left.hip -o replay_left
//   ./replay_left          (exit status 0: every check held)
#include TSOLVE_PATH
#include EMU_PATH
#include <cstdarg>
#include <map>
#include <set>
#include <vector>

static char *const BASE = (char *)0x100000000000ull;
static std::map<char *, size_t> g_blocks;          // live pool blocks
static char *g_pool = BASE;
static int64_t g_budget = -1;                      // bytes the pool may still hand out (-1: unlimited)
static int g_fail = 0;
static std::set<long> g_split;                     // slabs of the image that have been written
static int64_t g_lda = 0;

#define CHECK(c, ...) do { if (!(c)) { printf("CHECK FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); ++g_fail; } } while (0)

static bool inside(const void *p, size_t first, size_t last)   // bytes [first, last] from p inside one live block
{
    auto it = g_blocks.upper_bound((char *)p + first);
    if (it == g_blocks.begin()) return false;
    --it;
    return (char *)p + first >= it->first && (char *)p + last < it->first + it->second;
}

int Profiler::begin(hipStream_t, int, double) { return -1; }
void Profiler::end(hipStream_t, int) {}
static char g_err[256];
void gpx_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int gpx_require_device() { return 0; }
int dalloc(double **p, int64_t elems)
{
    const size_t bytes = ((size_t)elems * 8 + 255) / 256 * 256;
    if (g_budget >= 0 && (int64_t)bytes > g_budget) { *p = nullptr; gpx_set_error("out of memory"); return GPX_ERR_HIP; }
    if (g_budget >= 0) g_budget -= bytes;
    *p = (double *)g_pool;
    g_blocks[g_pool] = bytes;
    g_pool += bytes + (1 << 20);
    return 0;
}
void dfree(void *p) { CHECK(g_blocks.erase((char *)p) == 1, "free of an unknown block"); }
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

template <class T> static T arg(void **a, int i) { return *(T *)a[i]; }

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
hipError_t hipLaunchKernel(const void *f, dim3 g, dim3, void **a, size_t, hipStream_t)
{
    if (f == (const void *)emu_scale_from_bound_kernel) {
        const long rows = arg<long>(a, 1), rp = arg<long>(a, 2);
        CHECK((long)g.x * 256 >= rp && rows <= rp, "scale grid");
        CHECK(inside(arg<int *>(a, 4), 0, 4 * rp - 1) && inside(arg<int *>(a, 5), 0, 3), "scales / status outside their block");
        printf("  scales %ld rows (%ld padded)\n", rows, rp);
    } else if (f == (const void *)emu_split_fixed_kernel) {      // one wave per row, four rows per workgroup
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
        const long real = arg<long>(a, 2);
        CHECK(real <= (long)g.x && inside(arg<int *>(a, 5), 0, 4 * g.x - 1), "B scales outside their block");
        printf("  B scales %u x %d\n", g.x, arg<int>(a, 3));
    } else if (f == (const void *)emu_split_kernel) {            // one wave per (row, stretch of 1024 columns)
        const long real = arg<long>(a, 2), rp = arg<long>(a, 3), plane = arg<long>(a, 7);
        const int K = arg<int>(a, 4), L = arg<int>(a, 5);
        CHECK(real <= rp && plane == rp * K && (long)g.x * 4 >= rp * ((K + 1023) / 1024), "B split shape");
        CHECK(K % 16 == 0 && plane % 16 == 0 && (uintptr_t)arg<int8_t *>(a, 6) % 16 == 0, "B split: 16-byte stores");
        CHECK(inside(arg<int8_t *>(a, 6), 0, (size_t)L * plane - 1) && inside(arg<const int *>(a, 8), 0, 4 * real - 1), "B split writes outside its tile");
        for (long q = 0; q < K / 1024; ++q) CHECK(g_split.count(q) == 1, "slab %ld read before it was split", q);
        printf("  split B %ld x %d\n", rp, K);
    } else if (f == (const void *)emu_i8_gemm_kernel) {
        const long sa = arg<long>(a, 2), sb = arg<long>(a, 3), ldr = arg<long>(a, 6), sr = arg<long>(a, 7);
        const int K = arg<int>(a, 4), tm = arg<int>(a, 8), tn = arg<int>(a, 9), lda = arg<int>(a, 10);
        const int L = (int)(g.x / (tm * tn));
        CHECK((int)g.x == tm * tn * L && lda >= K && lda == g_lda, "int8 grid / stride");
        CHECK(inside(arg<const int8_t *>(a, 0), 0, (size_t)(L - 1) * sa + (size_t)(256 * tm - 1) * lda + K - 1), "int8 product reads outside the image");
        CHECK(inside(arg<const int8_t *>(a, 1), 0, (size_t)(L - 1) * sb + (size_t)(256 * tn) * K - 1), "int8 product reads outside the B tile");
        CHECK(inside(arg<int8_t *>(a, 5), 0, (size_t)(L - 1) * sr + (size_t)(256 * tm - 1) * ldr + 256 * tn - 1), "int8 product writes outside the residues");
        CHECK((size_t)255 * lda + K < ((size_t)1 << 31), "a panel's 32-bit byte offset");
        printf("  int8 %d x %d tiles, K %d, lda %d\n", tm, tn, K, lda);
    } else if (f == (const void *)emu_rebuild_kernel) {
        const long ldr = arg<long>(a, 1), sr = arg<long>(a, 2), rows = arg<long>(a, 9), cols = arg<long>(a, 10);
        const int L = arg<int>(a, 3);
        CHECK(inside(arg<const int8_t *>(a, 0), 0, (size_t)(L - 1) * sr + (size_t)(rows - 1) * ldr + ((cols + 3) / 4 * 4) - 1), "rebuild reads outside the residues");
        CHECK(inside(arg<const int *>(a, 5), 0, 4 * rows - 1) && inside(arg<const int *>(a, 6), 0, 4 * cols - 1), "rebuild scales");
        printf("  rebuild %ld x %ld\n", rows, cols);
    } else
        printf("  kernel (other) grid %u\n", g.x);
    return hipSuccess;
}
}

static int run(int64_t rows, int64_t npad, int64_t tile_rows, int64_t budget)
{
    printf("== rows %ld npad %ld tile_rows %ld budget %ld\n", (long)rows, (long)npad, (long)tile_rows, (long)budget);
    g_blocks.clear();
    g_split.clear();
    g_budget = -1;
    TriSolver ts;
    double *Lf = nullptr, *Z = nullptr, *Zs = nullptr, *bound = nullptr, *pl = nullptr;
    dalloc(&Lf, npad * npad); dalloc(&Z, rows * npad); dalloc(&Zs, rows * npad); dalloc(&bound, rows); dalloc(&pl, 8);
    ts.L = Lf; ts.ld = npad; ts.npad = npad; ts.nblk = npad / TILE; ts.P = (npad + PB - 1) / PB; ts.Pl = pl;
    const size_t before = g_blocks.size();
    int rc = 0;
    {
        Scratch sc(nullptr);
        EmuLeft w;
        emu_left_plan(w, rows, ts.P, tile_rows);
        g_lda = w.lda;
        printf("  plan: lda %ld, %ld tile(s) of %ld rows, image %ld bytes, abits %d bbits %d\n", (long)w.lda, (long)w.tiles, (long)w.rt, (long)w.img_bytes, w.abits, w.bbits);
        CHECK(w.rt * w.lda * w.L <= ((int64_t)1 << 31) && w.tiles * w.rt >= round_up(rows, 256), "plan");
        g_budget = budget;
        rc = emu_left_alloc(w, sc);
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

int main()
{
    int bad = 0;
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
    printf("%s (%d failed checks, %d wrong results)\n", g_fail || bad ? "FAILED" : "ok", g_fail, bad);
    return g_fail || bad ? 1 : 0;
}
