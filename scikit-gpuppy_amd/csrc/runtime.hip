// runtime.hip -- what every entry point of libgpx stands on: the error text, device selection, the event profiler, the caching
// device allocator with the stream cache and the pinned staging blocks, and the HBM micro-benchmark.
// Every entry point returns an int status; no exception crosses the boundary; there is no CPU
// fallback (a missing/unsupported device is an error, never a silent host computation).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <mutex>

#include "common.h"

// ---- error text -----------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static thread_local int g_device = 0;   // per host thread: gpx_set_device selects the device of handles created by THIS thread

void gpx_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *gpx_last_error(void) { return g_err; }
extern "C" int gpx_abi_version(void) { return GPX_ABI_VERSION; }

extern "C" int gpx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int gpx_set_device(int device)
{
    int n = gpx_device_count();
    if (device < 0 || device >= n) {
        gpx_set_error("gpx_set_device: device %d not available (%d visible)", device, n);
        return n == 0 ? GPX_ERR_NO_DEVICE : GPX_ERR_BAD_ARG;
    }
    g_device = device;
    return 0;
}

int gpx_thread_device() { return g_device; }   // (multi.hip saves / restores the calling thread's choice around its per-device work)

int gpx_require_device()
{
    int n = gpx_device_count();
    if (n == 0) {
        gpx_set_error("no HIP device visible: libgpx has no CPU fallback");
        return GPX_ERR_NO_DEVICE;
    }
    if (g_device >= n) g_device = 0;
    GPX_HIP(hipSetDevice(g_device));
    hipDeviceProp_t prop;
    GPX_HIP(hipGetDeviceProperties(&prop, g_device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        gpx_set_error("device %d is %s; libgpx is built for gfx950 (MI355X) only", g_device, prop.gcnArchName);
        return GPX_ERR_NO_DEVICE;
    }
    return 0;
}

// ---- profiler ----------------------------------------------------------------------------------
int Profiler::begin(hipStream_t s, int cls, double w)
{
    std::pair<hipEvent_t, hipEvent_t> ev;
    if (!pool.empty()) {
        ev = pool.back();
        pool.pop_back();
    } else {
        if (hipEventCreate(&ev.first) != hipSuccess || hipEventCreate(&ev.second) != hipSuccess) return -1;
    }
    if (hipEventRecord(ev.first, s) != hipSuccess) return -1;
    recs.push_back({cls, w, ev.first, ev.second});
    return (int)recs.size() - 1;
}
void Profiler::end(hipStream_t s, int idx) { (void)hipEventRecord(recs[idx].b, s); }
int Profiler::collect(hipStream_t s)
{
    if (hipStreamSynchronize(s) != hipSuccess) return GPX_ERR_HIP;
    for (auto &r : recs) {
        float t = 0;
        if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            launches[r.cls] += 1;
            ms[r.cls] += t;
            work[r.cls] += r.work;
        }
        pool.push_back({r.a, r.b});
    }
    recs.clear();
    return 0;
}
void Profiler::reset()
{
    for (auto &r : recs) pool.push_back({r.a, r.b});
    recs.clear();
    for (int i = 0; i < GPX_K_COUNT; ++i) { launches[i] = 0; ms[i] = 0; work[i] = 0; }
}
void Profiler::destroy()
{
    reset();
    for (auto &p : pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    pool.clear();
}

// ---- helpers -----------------------------------------------------------------------------------
// Caching device allocator: a fit + predict cycle allocates and frees the same multi-GB buffers every time;
// hipMalloc/hipFree of that size cost milliseconds and hipFree synchronises the device.  Freed blocks are
// kept (exact-size buckets, per device) and handed back to the next request; gpx_pool_trim() releases them.
namespace {
struct PoolKey { int dev; size_t bytes; bool operator<(const PoolKey &o) const { return dev != o.dev ? dev < o.dev : bytes < o.bytes; } };
std::mutex g_pool_mu;
std::map<PoolKey, std::vector<void *>> g_pool_free;
std::map<void *, PoolKey> g_pool_live;
}   // namespace

int dalloc(double **p, int64_t elems)
{
    *p = nullptr;
    if (elems <= 0) elems = 1;
    const size_t bytes = ((sizeof(double) * (size_t)elems + 255) / 256) * 256;
    int dev = 0;
    GPX_HIP(hipGetDevice(&dev));
    const PoolKey key{dev, bytes};
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        auto it = g_pool_free.find(key);
        if (it != g_pool_free.end() && !it->second.empty()) {
            void *q = it->second.back();
            it->second.pop_back();
            g_pool_live[q] = key;
            *p = (double *)q;
            return 0;
        }
    }
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {   // out of memory: drop the cache and retry once
        (void)hipGetLastError();
        gpx_pool_trim();
        e = hipMalloc(&q, bytes);
    }
    if (e != hipSuccess) {
        gpx_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return GPX_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_live[q] = key;
    *p = (double *)q;
    return 0;
}

// the caller guarantees that no kernel still uses p (every entry point synchronises its stream before freeing)
void dfree(void *p)
{
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool_live.find(p);
    if (it == g_pool_live.end()) { (void)hipFree(p); return; }
    g_pool_free[it->second].push_back(p);
    g_pool_live.erase(it);
}

// Streams are cached like device buffers: creating and (synchronously) destroying the two or three streams of a handle
// costs more than a small fit (0.8 ms per gpx_free measured with hipStreamDestroy / hipFree in it).
namespace {
std::map<std::pair<int, int>, std::vector<hipStream_t>> g_stream_cache;   // (device, high priority) -> idle streams
}

hipStream_t stream_acquire(int high_priority)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        auto it = g_stream_cache.find({dev, high_priority});
        if (it != g_stream_cache.end() && !it->second.empty()) {
            hipStream_t s = it->second.back();
            it->second.pop_back();
            return s;
        }
    }
    hipStream_t s = nullptr;
    hipError_t e;
    if (high_priority) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest);
    } else
        e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return s;
}

// the stream must be idle (callers synchronise it first)
void stream_release(hipStream_t s, int high_priority)
{
    if (!s) return;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipStreamDestroy(s); return; }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_stream_cache[{dev, high_priority}].push_back(s);
}

// Pinned host staging blocks (64 KB) for the few-byte arguments and results of the propagation calls: copies to / from them are truly
// asynchronous, so a call needs ONE stream synchronisation (for its result) instead of one per stack buffer.  hipHostMalloc costs
// ~100 us: the blocks are pooled like the device buffers.
namespace { std::vector<double *> g_pinned_free; }
constexpr size_t PINNED_DOUBLES = 8192;
double *pinned_acquire()
{
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (!g_pinned_free.empty()) { double *p = g_pinned_free.back(); g_pinned_free.pop_back(); return p; }
    }
    void *q = nullptr;
    if (hipHostMalloc(&q, PINNED_DOUBLES * sizeof(double), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return (double *)q;
}
void pinned_release(double *p)
{
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pinned_free.push_back(p);
}
// a few doubles from a caller's pointer (host or device: include/gpx.h) into host memory
int fetch_small(double *dst, const double *src, size_t n)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, src) != hipSuccess) { (void)hipGetLastError(); memcpy(dst, src, sizeof(double) * n); return 0; }   // ordinary host memory
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) { GPX_HIP(hipMemcpy(dst, src, sizeof(double) * n, hipMemcpyDeviceToHost)); return 0; }
    memcpy(dst, src, sizeof(double) * n);
    return 0;
}

extern "C" int gpx_pool_trim(void)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (double *hp : g_pinned_free) (void)hipHostFree(hp);
    g_pinned_free.clear();
    for (auto &kv : g_pool_free)
        for (void *q : kv.second) (void)hipFree(q);   // cached blocks are no longer in g_pool_live: release them to the driver
    g_pool_free.clear();
    for (auto &kv : g_stream_cache)
        for (hipStream_t st : kv.second) (void)hipStreamDestroy(st);
    g_stream_cache.clear();
    chol_concurrency_forget();   // verdicts are keyed by stream: a new stream at a recycled address may sit on another hardware queue
    return 0;
}

// ---- profiling ---------------------------------------------------------------------------------
extern "C" int gpx_profile_enable(gpx_handle *h, int on)
{
    if (!h) { gpx_set_error("null handle"); return GPX_ERR_BAD_ARG; }
    h->prof.level = on < 0 ? 0 : on;
    return 0;
}
extern "C" int gpx_profile_reset(gpx_handle *h)
{
    if (!h) { gpx_set_error("null handle"); return GPX_ERR_BAD_ARG; }
    h->prof.reset();
    return 0;
}
extern "C" int gpx_profile_read(gpx_handle *h, int cls, int64_t *launches, double *total_ms, double *total_work)
{
    CHECK_H_PSEUDO_OK(h);
    if (cls < 0 || cls >= GPX_K_COUNT) { gpx_set_error("bad kernel class"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(h->prof.collect(h->stream));
    if (launches) *launches = h->prof.launches[cls];
    if (total_ms) *total_ms = h->prof.ms[cls];
    if (total_work) *total_work = h->prof.work[cls];
    return 0;
}

// ---- HBM micro-benchmark -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void hbm_fill_kernel(v2d *p, long n16)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) p[i] = (v2d){1.0, 2.0};
}
__global__ __launch_bounds__(256) void hbm_copy_kernel(const v2d *__restrict__ a, v2d *__restrict__ b, long n16)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) b[i] = a[i];
}

extern "C" int gpx_bench_hbm(int64_t bytes, int iters, double *write_gbs, double *copy_gbs)
{
    GPX_TRY(gpx_require_device());
    if (bytes < (1 << 20) || iters < 1) { gpx_set_error("gpx_bench_hbm: bytes >= 1 MiB, iters >= 1"); return GPX_ERR_BAD_ARG; }
    const long n16 = bytes / 16;
    v2d *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float mw = 0, mc = 0;
    // (hipMalloc, not the pool: the figure is that of fresh memory; everything is released on every path)
    hipError_t e = hipMalloc((void **)&a, n16 * 16);
    if (e == hipSuccess) e = hipMalloc((void **)&b, n16 * 16);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hbm_fill_kernel, dim3(2048), dim3(256), 0, 0, a, n16);
        (void)hipEventRecord(e0, 0);
        for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(hbm_fill_kernel, dim3(2048), dim3(256), 0, 0, a, n16);
        (void)hipEventRecord(e1, 0);
        (void)hipEventSynchronize(e1);
        (void)hipEventElapsedTime(&mw, e0, e1);
        hipLaunchKernelGGL(hbm_copy_kernel, dim3(2048), dim3(256), 0, 0, (const v2d *)a, b, n16);
        (void)hipEventRecord(e0, 0);
        for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(hbm_copy_kernel, dim3(2048), dim3(256), 0, 0, (const v2d *)a, b, n16);
        (void)hipEventRecord(e1, 0);
        (void)hipEventSynchronize(e1);
        (void)hipEventElapsedTime(&mc, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(a);
    (void)hipFree(b);
    if (e != hipSuccess) { (void)hipGetLastError(); gpx_set_error("gpx_bench_hbm: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    if (write_gbs) *write_gbs = (double)n16 * 16 * iters / (mw * 1e-3) / 1e9;
    if (copy_gbs) *copy_gbs = 2.0 * (double)n16 * 16 * iters / (mc * 1e-3) / 1e9;
    return 0;
}
