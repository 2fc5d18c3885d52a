// Host-only replay of chol.hip's schedule, for refactors that must not change it: chol.hip is compiled into this program, every HIP
// runtime call it makes (launches, event records, stream waits, memsets, synchronisations) and every external launcher it calls is
// replaced by a function that prints one line -- streams, events (numbered by first use) and pointers (as offsets) by name.  Needs no GPU.
//   hipcc -O1 -std=c++17 --offload-arch=gfx950 -I<tree>/scikit-gpuppy_amd/csrc -DCHOL_PATH='"<tree>/scikit-gpuppy_amd/csrc/chol.hip"' \
//         -x hip replay_chol.hip -o replay          (a tree from before fills.hip / the three-argument panel hook: add -DREPLAY_R10_TREE;
//                                                    from before the far columns by group: -DREPLAY_NO_FIT_EMU; from before the
//                                                    emulated updates' one workspace frame: -DREPLAY_THREE_FRAMES)
//   GPX_CONCURRENT_STREAMS=1 [GPX_SQK_FROM=.. ...] ./replay NBLK MODE > log
//   MODE 0: chol_factor on one stream, 1: with a chain stream, 2: chain + column streams; 3 .. 6: the panel step over all panels
//   (3: internal slice stream, 4: caller streams, no head rows, 5 / 6: caller streams, head rows, two / three ranks share the update).
// Build it for two trees and diff the logs (profiles/r11_chol_refactor.txt).  MOCK_TRAP_FAIL=1: the trapezoid launch declines.
#include CHOL_PATH
#include <cstdarg>
#include <cstring>

static char *const BASE = (char *)0x100000000000ull;
static long off(const void *p) { return p ? (long)((const char *)p - BASE) : -1; }
static int sid(hipStream_t s) { return (int)((uintptr_t)s >> 4); }
static std::map<hipEvent_t, int> g_ev;
static int eid(hipEvent_t e) { if (!g_ev.count(e)) { int n = (int)g_ev.size(); g_ev[e] = n; } return g_ev[e]; }   // numbered by first use
static uintptr_t g_next_ev = 0x1000;

int Profiler::begin(hipStream_t, int, double) { return -1; }
void Profiler::end(hipStream_t, int) {}
void gpx_set_error(const char *fmt, ...) { printf("ERROR %s\n", fmt); }
int launch_gemm_nt(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M, int64_t N, int64_t K, double alpha,
                   double beta, int lower_only, hipStream_t s, Profiler *, int ktrim, int tri, int small_tiles, int *)
{
    printf("gemm s%d A%ld B%ld C%ld %ld %ld %ld a%g b%g lo%d kt%d tri%d sm%d\n", sid(s), off(A), off(B), off(C), (long)M, (long)N, (long)K, alpha, beta, lower_only, ktrim, tri, small_tiles);
    return 0;
}
#ifdef REPLAY_NO_FIT_EMU   // a tree from before the far columns by group (no tri_cols, no emu_syrk_*)
int launch_syrk_trap_signal(const double *A, int64_t, const double *B, int64_t, double *C, int64_t, int64_t M, int64_t oc, int64_t K, double, double, int *sig,
                            hipStream_t s, Profiler *)
{
    const int64_t tc = 0;
#else
int launch_syrk_trap_signal(const double *A, int64_t, const double *B, int64_t, double *C, int64_t, int64_t M, int64_t oc, int64_t K, double, double, int *sig,
                            hipStream_t s, Profiler *, int64_t tc)
{
#endif
    if (getenv("MOCK_TRAP_FAIL")) return GPX_ERR_STATE;
    printf("trap s%d A%ld B%ld C%ld %ld %ld %ld sig%ld", sid(s), off(A), off(B), off(C), (long)M, (long)oc, (long)K, off(sig));
    if (tc > 0 && tc < M) printf(" cols%ld", (long)tc);
    printf("\n");
    return 0;
}
#ifndef REPLAY_NO_FIT_EMU
bool emu_enabled(int64_t K) { const char *e = getenv("GPX_EMU_MIN_K"); return K >= (e ? atol(e) : 4096L) && K % 128 == 0; }
#ifdef REPLAY_THREE_FRAMES   // a tree from before the one workspace frame (EmuSyrk with its own plan / alloc / free)
void emu_syrk_plan(EmuSyrk &w, int64_t rows, int64_t K, int64_t) { w.rows_pad = rows; w.K = K; }
int emu_syrk_alloc(EmuSyrk &) { return getenv("MOCK_EMU_NO_ROOM") ? GPX_ERR_HIP : 0; }
void emu_syrk_free(EmuSyrk &) {}
static long depth(const EmuSyrk &w) { return (long)w.K; }
#else
typedef EmuFrame EmuSyrk;
void EmuFrame::reserve(const EmuPlan &) {}
EmuPlan emu_syrk_plan(int64_t rows, int64_t K, int64_t) { EmuPlan p; p.a.rows_pad = rows; p.a.ld = K; return p; }
int emu_alloc(EmuFrame &, Scratch *) { return getenv("MOCK_EMU_NO_ROOM") ? GPX_ERR_HIP : 0; }
void emu_free(EmuFrame &) {}
static long depth(const EmuFrame &w) { return (long)w.a.ld; }
#endif
int emu_syrk_split(const EmuSyrk &w, const double *A, int64_t, int64_t rows, hipStream_t s) { printf("emu-split s%d A%ld %ld %ld\n", sid(s), off(A), (long)rows, depth(w)); return 0; }
int emu_syrk_panel(const EmuSyrk &w, int64_t q, double *C, int64_t, int64_t rows, hipStream_t s, Profiler *, int dt) { printf("emu-panel s%d q%ld C%ld %ld %ld dt%d\n", sid(s), (long)q, off(C), (long)rows, depth(w), dt); return 0; }
#endif
int64_t chol_dataflow_state_ints(int64_t nbr) { return 41 * nbr; }
int64_t chol_dataflow_table_ints(int64_t nbr) { return 12 * nbr; }
bool chol_dataflow_supported(int64_t nbr) { return nbr <= 128; }
int64_t chol_dataflow_word_steps() { return 3; }
int64_t chol_dataflow_word_colc(int64_t nbr, int64_t k) { return 10 + nbr + k; }
int chol_dataflow_fill_tables(int nbr, int first_rows, int *, int cap) { printf("fill_tables %d %d %d\n", nbr, first_rows, cap); return 0; }
int launch_chol_dataflow(double *L, int64_t ld, int64_t nb, int64_t c0, double *Dinv, double *diag, int *info, int *state, std::vector<int> &, unsigned long long,
                         hipStream_t s, int workers, int exclusive, const int *tab_ready, int first_rows, int extra, const int *gate)
{
    printf("dataflow s%d nb%ld c0 %ld info%ld state%ld w%d x%d tab%ld fr%d ex%d gate%ld\n", sid(s), (long)nb, (long)c0, off(info), off(state), workers, exclusive,
           off(tab_ready), first_rows, extra, off(gate));
    return 0;
}
static char *g_pool = BASE + (1ll << 40);
int dalloc(double **p, int64_t elems) { *p = (double *)g_pool; g_pool += ((elems * 8 + 255) / 256) * 256 + (1 << 20); printf("dalloc %ld\n", (long)(((elems * 8 + 255) / 256) * 256)); return 0; }
void dfree(void *p) { printf("dfree %ld\n", off(p)); }
hipStream_t stream_acquire(int hp) { static int n = 0; ++n; printf("stream_acquire %d\n", hp); return (hipStream_t)(uintptr_t)(0x40 + 0x10 * (n % 4)); }
void stream_release(hipStream_t s, int hp) { printf("stream_release s%d %d\n", sid(s), hp); }
#ifndef REPLAY_R10_TREE
int launch_set_identity(double *, int64_t, int64_t, hipStream_t) { return 0; }
int launch_symmetrize_lower(double *, int64_t, int64_t, hipStream_t) { return 0; }
#endif

extern "C" {
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)(g_next_ev += 16); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { printf("evdestroy\n"); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { printf("record e%d s%d\n", eid(e), sid(s)); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { printf("wait s%d e%d\n", sid(s), eid(e)); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { printf("sync s%d\n", sid(s)); return hipSuccess; }
hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t s) { printf("memset s%d %ld %zu\n", sid(s), off(p), n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *, size_t n, hipMemcpyKind k, hipStream_t s) { printf("memcpy s%d %zu kind%d\n", sid(s), n, (int)k); return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
static dim3 g_grid, g_block; static size_t g_shm; static hipStream_t g_st;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t shm, hipStream_t s) { g_grid = g; g_block = b; g_shm = shm; g_st = s; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *shm, hipStream_t *s) { *g = g_grid; *b = g_block; *shm = g_shm; *s = g_st; return hipSuccess; }
hipError_t hipLaunchKernel(const void *f, dim3 g, dim3 b, void **args, size_t shm, hipStream_t s)
{
    if (f == (const void *)wait_count_kernel) { printf("K wait_count s%d ctr%ld want%d lim%llu stall%ld\n", sid(s), off(*(void **)args[0]), *(int *)args[1], *(unsigned long long *)args[2], off(*(void **)args[3])); return hipSuccess; }
    if (f == (const void *)set_flag_kernel) { printf("K set_flag s%d %ld %d\n", sid(s), off(*(void **)args[0]), *(int *)args[1]); return hipSuccess; }
    if (f == (const void *)cu_blocker_kernel) { printf("K cu_blocker s%d g%u stop%ld placed%ld lim%llu\n", sid(s), g.x, off(*(void **)args[0]), off(*(void **)args[1]), *(unsigned long long *)args[2]); return hipSuccess; }
    if (f == (const void *)wait_placed_kernel) { printf("K wait_placed s%d %ld want%d\n", sid(s), off(*(void **)args[0]), *(int *)args[1]); return hipSuccess; }
    if (f == (const void *)merge_info_kernel) { printf("K merge_info s%d %ld %ld\n", sid(s), off(*(void **)args[0]), off(*(void **)args[1])); return hipSuccess; }
    if (f == (const void *)potrf_trtri128_elim_kernel) { printf("K leaf s%d A%ld shm%zu col%d\n", sid(s), off(*(void **)args[0]), shm, *(int *)args[5]); return hipSuccess; }
    printf("K ? s%d g%u\n", sid(s), g.x);
    return hipSuccess;
}
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s NBLK MODE\n", argv[0]); return 2; }
    const int64_t nblk = atol(argv[1]);
    const int mode = atoi(argv[2]);   // 0: s only, 1: s + s_pan, 2: s + s_pan + s_top, 3..: panel step forms
    const int64_t ld = nblk * TILE;
    double *L = (double *)BASE, *Dinv = L + ld * ld, *diag = Dinv + nblk * TILE * TILE;
    int *info = (int *)(diag + ld);
    hipStream_t s = (hipStream_t)0x10, sp = (hipStream_t)0x20, st = (hipStream_t)0x30;
    const std::function<int()> fork = [] { printf("CB after_fork\n"); return 0; };
#ifndef REPLAY_R10_TREE
    const std::function<int(int64_t, int64_t, bool)> fin = [](int64_t p, int64_t sl, bool last) { printf("CB panel_final %ld %ld %d\n", (long)p, (long)sl, (int)last); return 0; };
#else
    const std::function<int(int64_t, int64_t, bool, hipStream_t)> fin = [](int64_t p, int64_t sl, bool last, hipStream_t on) { printf("CB panel_final %ld %ld %d\n", (long)p, (long)sl, (int)last); return 0; };
#endif
    int rc = 0;
    for (int rep = 0; rep < 2; ++rep) {   // twice: the second call meets recycled state
        printf("== call %d\n", rep);
        if (mode <= 2) rc = chol_factor(L, ld, nblk, Dinv, diag, info, s, mode >= 1 ? sp : nullptr, nullptr, mode >= 2 ? st : nullptr, &fork, &fin);
        else {
            if (mode >= 5) gpx_dev_set_panel_share(mode - 3);
            const double *P = (mode & 1) ? L + 5 : nullptr;
            for (int64_t B0 = 0; B0 < nblk && !rc; B0 += CHOL_NBP) {
                const int64_t B1 = std::min(nblk, B0 + CHOL_NBP);
                printf("-- panel %ld\n", (long)B0);
                rc = chol_panel_factor_piped(L, ld, nblk, B0, B1, Dinv, diag, info, s, nullptr, B0 ? P : nullptr, ld, CHOL_NBP * TILE, mode == 4 ? 0 : 8, mode >= 4 ? sp : nullptr, mode >= 4 ? st : nullptr);
            }
        }
        printf("rc %d\n", rc);
    }
    return 0;
}
