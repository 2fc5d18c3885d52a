// rawmodel.hip -- what the raw-input kernels (periodic.hip, matern.hip) share on the host: the common part of a parsed model (RawModel,
// common.h), its inputs and constants on the device, the stand-alone Gram and the driver of the one-pass likelihood gradient.  What a
// kind computes stays in its own file; here a kind is a tag that picks its launcher.
#include <math.h>
#include <string.h>

#include "common.h"
#include "gram_tile.h"

// the kernels' constant block: periodic [4][d]: w / 2, ih = fl(1 / p), il = fl((1 - ih p) ih) (periodic_math.h), w2 / 2; Matern [d]: w
int raw_pack(const RawModel *m, double *host)
{
    const int d = m->d;
    if (m->kind == KernelKind::Matern) {
        memcpy(host, static_cast<const MaternData *>(m)->w, sizeof(double) * d);
        return d;
    }
    const PeriodicData &pd = *static_cast<const PeriodicData *>(m);
    for (int k = 0; k < d; ++k) {
        const double ih = 1.0 / pd.p[k];
        host[k] = 0.5 * pd.w[k];
        host[d + k] = ih;
        host[2 * d + k] = isfinite(ih) ? fma(-ih, pd.p[k], 1.0) * ih : 0.0;   // (a subnormal p: ih = inf is refused by nothing, q is then NaN)
        host[3 * d + k] = 0.5 * pd.w2[k];
    }
    return 4 * d;
}

int raw_parse_head(const char *name, const double *theta, int d, RawModel *out, double *w)
{
    if (!theta || d < 1 || d > GPX_MAX_D) {
        gpx_set_error("%s kernel: bad theta / d=%d (1..%d supported)", name, d, GPX_MAX_D);
        return GPX_ERR_BAD_ARG;
    }
    out->d = d;
    out->v = exp(theta[0]);
    out->vt = exp(theta[1]);   // theta[1] = -inf gives vt = 0
    if (!(out->v > 0.0) || !isfinite(out->v) || !isfinite(out->vt)) {
        gpx_set_error("%s kernel: theta gives v=%g vt=%g", name, out->v, out->vt);
        return GPX_ERR_BAD_ARG;
    }
    for (int k = 0; k < d; ++k) w[k] = exp(theta[2 + k]);
    return 0;
}

RawModel *raw_clone(const RawModel *spec)
{
    if (spec->kind == KernelKind::Periodic) return new (std::nothrow) PeriodicData(*static_cast<const PeriodicData *>(spec));
    return new (std::nothrow) MaternData(*static_cast<const MaternData *>(spec));
}

__global__ __launch_bounds__(256) void raw_transpose_kernel(const double *__restrict__ x, long n, long npad, int d, double *__restrict__ xT)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npad * d) return;
    const long k = e / npad, j = e - k * npad;
    xT[e] = j < n ? x[j * d + k] : 0.0;
}

int raw_upload(RawModel *m, const double *x, int64_t n, int64_t npad, hipStream_t s)
{
    const int d = m->d;
    double host[4 * GPX_MAX_D];
    const int npar = raw_pack(m, host);
    GPX_TRY(dalloc(&m->par, npar));
    GPX_TRY(dalloc(&m->x, n * d));
    GPX_TRY(dalloc(&m->xT, npad * d));
    GPX_HIP(hipMemcpyAsync(m->par, host, sizeof(double) * npar, hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(m->x, x, sizeof(double) * n * d, hipMemcpyDefault, s));
    hipLaunchKernelGGL(raw_transpose_kernel, dim3((unsigned)((npad * d + 255) / 256)), dim3(256), 0, s, (const double *)m->x, (long)n, (long)npad, d,
                       m->xT);
    GPX_HIP(hipGetLastError());
    GPX_HIP(hipStreamSynchronize(s));   // host is a stack buffer
    return 0;
}

void raw_release(RawModel *m)
{
    if (!m) return;
    for (double *p : {m->x, m->xT, m->par})
        if (p) dfree(p);
    if (m->kind == KernelKind::Periodic) delete static_cast<PeriodicData *>(m);
    else delete static_cast<MaternData *>(m);
}

int launch_raw_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, const RawModel *m, double add_diag, int lower_only, int pad_mode,
                    double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad, hipStream_t s, Profiler *prof, int deriv)
{
    if (m->kind == KernelKind::Periodic)
        return launch_periodic_gram(xi, n1, xj, n2, static_cast<const PeriodicData *>(m), add_diag, lower_only, pad_mode, out, ld, rows_pad,
                                    cols_pad, s, prof, deriv);
    return launch_matern_gram(xi, n1, xj, n2, static_cast<const MaternData *>(m), add_diag, lower_only, pad_mode, out, ld, rows_pad, cols_pad, s,
                              prof, deriv);
}

int raw_gram_args(const char *what, const double *xi, int64_t n1, const double *xj, int64_t n2, const double *out)
{
    GPX_TRY(gpx_require_device());
    if (!xi || !xj || !out || n1 < 1 || n2 < 1) { gpx_set_error("%s: null pointer or n < 1", what); return GPX_ERR_BAD_ARG; }
    return 0;
}

int raw_gram(RawModel *m, const double *xi, int64_t n1, const double *xj, int64_t n2, int deriv, double *out)
{
    const int d = m->d;
    const int64_t rp = round_up(n1, TILE), cp = round_up(n2, TILE);
    hipStream_t s = nullptr;
    Scratch sc(s);
    double *a = nullptr, *b = nullptr, *o = nullptr;
    // (the parameter block through the call's own scratch: nothing of m outlives the call)
    double host[4 * GPX_MAX_D];
    const int npar = raw_pack(m, host);
    GPX_TRY(sc.take(&m->par, npar));
    GPX_HIP(hipMemcpy(m->par, host, sizeof(double) * npar, hipMemcpyHostToDevice));
    GPX_TRY(sc.take(&a, n1 * d));
    GPX_HIP(hipMemcpy(a, xi, sizeof(double) * n1 * d, hipMemcpyDefault));
    if (xj == xi && n1 == n2) b = a;
    else {
        GPX_TRY(sc.take(&b, n2 * d));
        GPX_HIP(hipMemcpy(b, xj, sizeof(double) * n2 * d, hipMemcpyDefault));
    }
    GPX_TRY(sc.take(&o, rp * cp));
    GPX_TRY(launch_raw_gram(a, n1, b, n2, m, 0.0, 0, PAD_ZERO, o, cp, rp, cp, s, nullptr, deriv));
    GPX_HIP(hipMemcpy2D(out, sizeof(double) * n2, o, sizeof(double) * cp, sizeof(double) * n2, n1, hipMemcpyDefault));
    return 0;
}

int raw_nll_grad_sums(gpx_handle *h, int kc, int nc, double *o)
{
    const RawModel *m = h->raw;
    const int sweeps = (m->d + kc - 1) / kc;
    hipStream_t s = h->stream;
    Scratch sc(s);
    double *partial = nullptr;   // [sweeps, npad / 8, nc], then the column sums [sweeps, nc]
    const int64_t nb = h->npad / 8;
    GPX_TRY(sc.take(&partial, (nb + 1) * sweeps * nc));
    double *sums = partial + nb * sweeps * nc;
    {
        ProfScope ps(&h->prof, s, GPX_K_QUAD, 4.0 * (double)h->npad * (double)h->npad * sweeps);
        if (m->kind == KernelKind::Periodic)
            GPX_TRY(launch_periodic_nll_grad(h->Kinv, h->npad, h->n, h->npad, handle_periodic(h), h->alpha, partial, s));
        else
            GPX_TRY(launch_matern_nll_grad(h->Kinv, h->npad, h->n, h->npad, handle_matern(h), h->alpha, partial, s));
    }
    for (int y = 0; y < sweeps; ++y) GPX_TRY(launch_sum_columns(partial + (int64_t)y * nb * nc, nb, nc, sums + y * nc, s));
    GPX_HIP(hipMemcpyAsync(o, sums, sizeof(double) * sweeps * nc, hipMemcpyDeviceToHost, s));
    GPX_HIP(hipStreamSynchronize(s));
    return 0;
}
