// quadrature.hip -- numerical uncertainty propagation (skgpuppy/UncertaintyPropagation.py:90-162: UncertaintyPropagationMC,
// UncertaintyPropagationNumericalHG), gfx950: the node set of a quadrature or sampling rule built on the device, and the reduction of the
// predictor's mu / sigma^2 at those nodes to the moments and the density of the mixture  p(y) = sum_s wq_s N(y; mu_s, sigma^2_s)
// (Girard 2004, p. 32).  The S reference calls of gp(x) in between are rows of the many-row solver (predict.hip, PredictRun).
#include "common.h"

// ---------------------------------------------------------------------------------------------
// Nodes.  Query row g = i S + s (input i, node s), component k:
//   X[g][k] = fma(A_i[k][d-1], z[s][d-1], ... fma(A_i[k][1], z[s][1], fma(A_i[k][0], z[s][0], U[i][k])) ...)
// ONE fma chain over e in increasing order that starts from U[i][k] (tests/_quadrature_model.py restates it bit for bit).
// One thread per element of the chunk's [rows, d] block; U, A and z are read with plain loads.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quad_nodes_kernel(const double *__restrict__ U, const double *__restrict__ A, long a_stride,
                                                        const double *__restrict__ z, long S, int d, long row0, long rows,
                                                        double *__restrict__ X)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * d) return;
    const long r = idx / d;
    const int k = (int)(idx - r * d);
    const long g = row0 + r, i = g / S, s = g - i * S;
    const double *a = A + i * a_stride + (long)k * d, *zs = z + s * d;
    double acc = U[i * d + k];
    for (int e = 0; e < d; ++e) acc = fma(a[e], zs[e], acc);
    X[idx] = acc;
}

int launch_quad_nodes(const double *U, const double *A, int64_t a_stride, const double *z, int64_t S, int d, int64_t row0, int64_t rows, double *X,
                      hipStream_t s, Profiler *prof)
{
    if (rows <= 0) return 0;
    if (d < 1 || d > GPX_MAX_D || S < 1 || row0 < 0) { gpx_set_error("quad_nodes: bad shape (d=%d S=%ld)", d, (long)S); return GPX_ERR_BAD_ARG; }
    ProfScope ps(prof, s, GPX_K_GRAM, 8.0 * (double)rows * (double)d * (double)(d + 2));
    const int64_t nblk = (rows * d + 255) / 256;
    hipLaunchKernelGGL(quad_nodes_kernel, dim3((unsigned)nblk), dim3(256), 0, s, U, A, (long)a_stride, z, (long)S, d, (long)row0, (long)rows, X);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Mixture moments.  An input's S nodes are cut into segments of MIX_SEG = 1024; workgroup (segment, input), 256 threads:
//   thread t takes the nodes  seg 1024 + t + 256 j, j = 0..3, in that order, each sum one fma chain from 0  (nodes >= S: skipped)
//   -> xor-butterfly over the wave's 64 lanes -> LDS slot of the wave -> thread 0: (p0 + p1) + (p2 + p3) -> part[q][i nseg + seg]
// and one workgroup per input adds the segments: thread t the segments t, t + 256, ... in that order, butterfly, LDS, the same final sum.
// No atomics, and nothing in the map depends on b or on the input's place: the same mu, sigma^2, wq give the same bits.
//   pass 1:  m = sum wq mu,  Ev = sum wq sigma^2
//   pass 2 (about the m of pass 1, dm = mu - m):  c2 = sum wq dm^2,  m3 = sum wq (dm^3 + 3 dm sigma^2),
//            m4 = sum wq (dm^4 + 6 dm^2 sigma^2 + 3 sigma^4);  var = Ev + c2 -- the CENTRAL second moment, not E[mu^2] - m^2 (which cancels)
// ---------------------------------------------------------------------------------------------
constexpr int MIX_SEG = 1024;

template <int NQ> __device__ __forceinline__ void block_sum_store(double (&acc)[NQ], double *__restrict__ out, long stride, long at)
{
    __shared__ double slot[NQ][4];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double w = wave_sum(acc[q]);
        if (lane == 0) slot[q][wave] = w;
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) out[q * stride + at] = (slot[q][0] + slot[q][1]) + (slot[q][2] + slot[q][3]);
    }
}

// part [2][b nseg]
__global__ __launch_bounds__(256) void mixture_mean_kernel(const double *__restrict__ mu, const double *__restrict__ var, const double *__restrict__ wq,
                                                          long S, long nseg, double *__restrict__ part, long pstride)
{
    const long seg = blockIdx.x, i = blockIdx.y;
    const double *m = mu + i * S, *v = var + i * S;
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long s = seg * MIX_SEG + threadIdx.x + 256 * j;
        if (s < S) {
            const double w = wq[s];
            acc[0] = fma(w, m[s], acc[0]);
            acc[1] = fma(w, v[s], acc[1]);
        }
    }
    block_sum_store<2>(acc, part, pstride, i * nseg + seg);
}

// part [3][b nseg]; mom row 0 holds the m of pass 1
__global__ __launch_bounds__(256) void mixture_central_kernel(const double *__restrict__ mu, const double *__restrict__ var, const double *__restrict__ wq,
                                                             long S, long nseg, const double *__restrict__ mom, double *__restrict__ part, long pstride)
{
    const long seg = blockIdx.x, i = blockIdx.y;
    const double *m = mu + i * S, *v = var + i * S;
    const double mean = mom[i];
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long s = seg * MIX_SEG + threadIdx.x + 256 * j;
        if (s < S) {
            const double w = wq[s], dm = m[s] - mean, vv = v[s];
            const double d2 = dm * dm;
            const double t3 = dm * fma(3.0, vv, d2);                          // dm^3 + 3 dm sigma^2
            const double t4 = fma(d2, d2, fma(6.0 * d2, vv, 3.0 * (vv * vv)));   // dm^4 + 6 dm^2 sigma^2 + 3 sigma^4
            acc[0] = fma(w, d2, acc[0]);
            acc[1] = fma(w, t3, acc[1]);
            acc[2] = fma(w, t4, acc[2]);
        }
    }
    block_sum_store<3>(acc, part, pstride, i * nseg + seg);
}

// the segments of input i = blockIdx.x added up; PASS 1: mom[0] = m, mom[2] = Ev; PASS 2: mom[1] = Ev + c2, mom[3] = m3, mom[4] = m4
template <int PASS> __global__ __launch_bounds__(256) void mixture_finish_kernel(const double *__restrict__ part, long pstride, long nseg, long b,
                                                                               double *__restrict__ mom)
{
    constexpr int NQ = PASS == 1 ? 2 : 3;
    __shared__ double slot[NQ][4];
    const long i = blockIdx.x;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        acc[q] = 0.0;
        for (long g = t; g < nseg; g += 256) acc[q] += part[q * pstride + i * nseg + g];
        const double w = wave_sum(acc[q]);
        if (lane == 0) slot[q][wave] = w;
    }
    __syncthreads();
    if (t == 0) {
        double tot[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) tot[q] = (slot[q][0] + slot[q][1]) + (slot[q][2] + slot[q][3]);
        if (PASS == 1) { mom[i] = tot[0]; mom[2 * b + i] = tot[1]; }
        else { mom[b + i] = mom[2 * b + i] + tot[0]; mom[3 * b + i] = tot[1]; mom[4 * b + i] = tot[2]; }
    }
}

// ---------------------------------------------------------------------------------------------
// Mixture density  p[i][j] = sum_s wq_s exp(-(y_j - shift - mu_s)^2 / (2 sigma^2_s)) / sqrt(2 pi sigma^2_s), b S ny exponentials.
// Workgroup (segment of 1024 nodes, tile of 16 y, input).  The segment's nodes are staged ONCE in LDS as (mu_s, h_s = 1 / (2 sigma^2_s),
// c_s = wq_s / sqrt(2 pi sigma^2_s)) -- one division, one square root per node, not per (node, y); nodes >= S get c = h = 0 and add
// an exact +0.  Thread t = 16 q + jy: y_j of the tile's column jy, the nodes q, q + 16, .. of the segment in that order, one fma chain
// p = fma(c_s, exp(-(dy dy) h_s), p); a wave's 64 lanes read 4 distinct LDS addresses (16-lane broadcast: no bank conflict).  The 16
// partial sums of a column go through LDS and are added in the order q = 0..15 by the thread q = 0; the segments by the finish kernel in
// increasing order.  No clamping: sigma^2 = 0 gives c = inf, exp = 0 and a NaN, sigma^2 < 0 a NaN from the square root, as the
// reference's expression; the moments never read these.  exp is exp_nonpos (common.h): the exponent is never positive and a far tail
// (exponent below -745) goes to 0, not NaN.
// ---------------------------------------------------------------------------------------------
constexpr int MIX_YT = 16;

__global__ __launch_bounds__(256) void mixture_density_kernel(const double *__restrict__ mu, const double *__restrict__ var, const double *__restrict__ wq,
                                                             long S, long nseg, const double *__restrict__ y, long ny, long y_stride, double shift,
                                                             double *__restrict__ part)
{
    __shared__ double nm[MIX_SEG], nh[MIX_SEG], nc[MIX_SEG];
    __shared__ double col[16][MIX_YT + 1];
    const long seg = blockIdx.x, i = blockIdx.z;
    const int t = threadIdx.x, jy = t & (MIX_YT - 1), q = t >> 4;
    const long j = (long)blockIdx.y * MIX_YT + jy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = t + 256 * k;
        const long s = seg * MIX_SEG + l;
        double m = 0.0, hh = 0.0, c = 0.0;
        if (s < S) {
            const double vv = var[i * S + s];
            m = mu[i * S + s];
            hh = 0.5 / vv;
            c = wq[s] / sqrt(6.283185307179586477 * vv);
        }
        nm[l] = m; nh[l] = hh; nc[l] = c;
    }
    __syncthreads();
    double p = 0.0;
    if (j < ny) {
        const double ys = y[i * y_stride + j] - shift;
        for (int l = q; l < MIX_SEG; l += 16) {
            const double dy = ys - nm[l];
            p = fma(nc[l], exp_nonpos(-(dy * dy) * nh[l]), p);
        }
    }
    col[q][jy] = p;
    __syncthreads();
    if (q == 0 && j < ny) {
        double tot = col[0][jy];
#pragma unroll
        for (int k = 1; k < 16; ++k) tot += col[k][jy];
        part[(i * nseg + seg) * ny + j] = tot;
    }
}

// dens[i][j] = sum over the segments in increasing order, one thread per (i, j)
__global__ __launch_bounds__(256) void mixture_density_finish_kernel(const double *__restrict__ part, long nseg, long ny, long total, double *__restrict__ dens)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long i = idx / ny, j = idx - i * ny;
    double tot = part[(i * nseg) * ny + j];
    for (long g = 1; g < nseg; ++g) tot += part[(i * nseg + g) * ny + j];
    dens[idx] = tot;
}

int launch_mixture_reduce(const double *mu, const double *var, const double *wq, int64_t S, int64_t b, const double *y, int64_t ny, int64_t y_stride,
                          double shift, double *mom, double *dens, Scratch &sc, Profiler *prof)
{
    if (b <= 0) return 0;
    hipStream_t s = sc.s;
    const int64_t nseg = (S + MIX_SEG - 1) / MIX_SEG, nyt = (ny + MIX_YT - 1) / MIX_YT;
    if (S < 1 || ny < 0 || b > 65535 * (int64_t)65535 || nyt > 65535) { gpx_set_error("mixture_reduce: bad shape (S=%ld b=%ld ny=%ld)", (long)S, (long)b, (long)ny); return GPX_ERR_BAD_ARG; }
    double *part = nullptr, *dpart = nullptr;
    const int64_t pstride = b * nseg;
    GPX_TRY(sc.take(&part, 3 * pstride));
    if (ny > 0) GPX_TRY(sc.take(&dpart, pstride * ny));
    ProfScope ps(prof, s, GPX_K_REDUCE, 8.0 * (double)b * (double)S * (double)(4 + ny));
    // (grid.y / grid.z hold the input: at most 65535 each, so the batch goes in slices of that many inputs; an input's map is the same in every slice)
    for (int64_t i0 = 0; i0 < b; i0 += 65535) {
        const int64_t bc = std::min<int64_t>(65535, b - i0);
        const double *mu_c = mu + i0 * S, *var_c = var + i0 * S;
        double *part_c = part + i0 * nseg;
        hipLaunchKernelGGL(mixture_mean_kernel, dim3((unsigned)nseg, (unsigned)bc), dim3(256), 0, s, mu_c, var_c, wq, (long)S, (long)nseg, part_c, (long)pstride);
        hipLaunchKernelGGL(mixture_finish_kernel<1>, dim3((unsigned)bc), dim3(256), 0, s, part_c, (long)pstride, (long)nseg, (long)b, mom + i0);
        hipLaunchKernelGGL(mixture_central_kernel, dim3((unsigned)nseg, (unsigned)bc), dim3(256), 0, s, mu_c, var_c, wq, (long)S, (long)nseg, mom + i0, part_c, (long)pstride);
        hipLaunchKernelGGL(mixture_finish_kernel<2>, dim3((unsigned)bc), dim3(256), 0, s, part_c, (long)pstride, (long)nseg, (long)b, mom + i0);
        if (ny > 0) {
            hipLaunchKernelGGL(mixture_density_kernel, dim3((unsigned)nseg, (unsigned)nyt, (unsigned)bc), dim3(256), 0, s, mu_c, var_c, wq, (long)S, (long)nseg,
                               y + i0 * y_stride, (long)ny, (long)y_stride, shift, dpart + i0 * nseg * ny);
        }
    }
    if (ny > 0) {
        const int64_t total = b * ny;
        hipLaunchKernelGGL(mixture_density_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dpart, (long)nseg, (long)ny, (long)total, dens);
    }
    GPX_HIP(hipGetLastError());
    return 0;
}
