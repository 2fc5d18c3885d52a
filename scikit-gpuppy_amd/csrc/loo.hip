// loo.hip -- leave-one-out cross-validation on the device: the LOO predictions, the negative log predictive probability and its
// gradient in theta (Rasmussen & Williams 5.4.2; Sundararajan & Keerthi 2001).  gfx950 only.
//
// With P = K^-1 (K the fitted matrix: vt and any jitter included) and alpha = P t, the mean held fixed:
//   mu_-i = t_i - alpha_i / P_ii,   sigma^2_-i = 1 / P_ii,   L = N/2 log 2pi + sum_i (-1/2 log P_ii + 1/2 alpha_i^2 / P_ii).
// From dP = -P dK P and d alpha = -P dK alpha, with c_i = 1/2 (1 / P_ii + alpha_i^2 / P_ii^2), a_i = alpha_i / P_ii and g = P a:
//   dL / d theta_j = sum_kl W_kl (dK / d theta_j)_kl,   W = P diag(c) P - 1/2 (g alpha^T + alpha g^T)
// -- ONE symmetric N^3 product for all 2 + d parameters instead of one per parameter, and W is never stored: loo_grad_kernel
// contracts a 128 x 128 tile of P diag(c) P on the fp64 matrix cores (gemm_tile_x without GT_STORE hands the accumulators back) and
// reduces it against the Gaussian kernel's derivative factors in place:
//   S_0 = sum W Kf,   S_k = sum W Kf (sqrt(w_k) delta_k)^2,   T = tr W;   dL/dtheta_0 = S_0, dL/dtheta_1 = vt T, dL/dtheta_{2+k} = -S_k / 2
// (no 1/2 outside the sums: the likelihood's M = P - alpha alpha^T carries one, W does not).  Only the lower tiles run (W is symmetric:
// weight 2 below the diagonal, 1 on it), in lower_tile's XCD-aware order.  Per-tile partial sums, one fixed-order column sum: no
// atomics, the bits do not depend on what ran before.
//
// The padding: rows and columns >= n of a handle's K^-1 hold the identity (K is padded block-diagonally with an identity block) and
// exact zeros elsewhere.  Nothing of it reaches a sum: c_i = a_i = 0 for i >= n (loo_point_kernel), so column i >= n of
// Pc = P diag(c) is exactly 0 and the contraction over [0, npad) adds exact zeros; rows >= n of Pc are written as zeros; entries
// of a tile at or beyond n are SELECTED to 0 (not multiplied by 0) before any sum.
#include "common.h"

#include "gemm_tile.h"

constexpr int LOO_DC = 16;                     // coordinates staged in LDS at a time (rows and columns of the tile)

// The kernel-specific part of the epilogue: the pair factor Kf(q) and the weight of coordinate k's sum at the scaled difference e.
// (Matern / periodic gradients need another one of these and nothing else.)
struct LooGaussPair {
    double v;
    __device__ __forceinline__ double add_q(double e, double q) const { return fma(e, e, q); }
    __device__ __forceinline__ double scale() const { return v; }
    __device__ __forceinline__ double factor(double q) const { return exp_nonpos(-0.5 * q); }   // Kf / scale of a block of coordinates
    __device__ __forceinline__ double coord(double e) const { return e * e; }
};

// vec [5, npad]: c, a, mu_-i (centred), sigma^2_-i, -1/2 log P_ii + 1/2 alpha_i^2 / P_ii; zeros at i >= n
__global__ __launch_bounds__(256) void loo_point_kernel(const double *__restrict__ P, long ld, long n, long npad, const double *__restrict__ alpha,
                                                       const double *__restrict__ t, double *__restrict__ vec)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    double c = 0.0, a = 0.0, mu = 0.0, s2 = 0.0, term = 0.0;
    if (i < n) {
        const double p = P[i * ld + i], al = alpha[i], ip = 1.0 / p;
        a = al * ip;
        c = 0.5 * (ip + a * a);
        mu = t[i] - a;
        s2 = ip;
        term = 0.5 * (al * a - log(p));
    }
    vec[i] = c;
    vec[npad + i] = a;
    vec[2 * npad + i] = mu;
    vec[3 * npad + i] = s2;
    vec[4 * npad + i] = term;
}

// Pc = P diag(c), rows >= n zero.  One block per row, 16-byte accesses.
__global__ __launch_bounds__(256) void loo_scale_kernel(const double *__restrict__ P, long npad, long n, const double *__restrict__ c,
                                                       double *__restrict__ Pc)
{
    const long i = blockIdx.x;
    for (long j = 2 * threadIdx.x; j < npad; j += 512) {
        const v2d p = *reinterpret_cast<const v2d *>(P + i * npad + j), cj = *reinterpret_cast<const v2d *>(c + j);
        *reinterpret_cast<v2d *>(Pc + i * npad + j) = i < n ? p * cj : (v2d){0.0, 0.0};
    }
}

// One workgroup = one lower 128 x 128 tile (by, bx <= by) of W.  partial [tiles, d + 2]: S_0, S_1..S_d, T of the tile.
// Epilogue (the stage buffers are free after the k loop): alpha and g of the tile's rows and columns, and LOO_DC coordinates of both at
// a time, sit in LDS coordinate-major (lanes that share a row read one address, the 16 columns of a lane group are consecutive).
// Accumulator register r of MFMA tile (i, j) is row wr 64 + 16 i + 4 r + fq, column wc 64 + 16 j + fr of the tile.  A first pass turns
// each of the lane's 64 entries into (acc - 1/2 (g_k alpha_l + alpha_k g_l)) wgt v; pass A multiplies on exp(-q / 2) of the staged
// coordinates (four entries of one row at a time); pass B walks the coordinates ONE at a time, s = sum_entries m delta^2: the live
// state is the 64 entries and a handful of registers at every d, no array indexed by the coordinate.  228 VGPRs, 64 KiB LDS, no scratch.
template <class Pair>
__global__ __launch_bounds__(256, 2) void loo_grad_kernel(const double *__restrict__ P, const double *__restrict__ Pc, long npad, long n, int d,
                                                         int nt, const double *__restrict__ xw, const double *__restrict__ alpha,
                                                         const double *__restrict__ g, Pair pair, double *__restrict__ partial)
{
    __shared__ __attribute__((aligned(1024))) double smem[2 * (128 + 128) * 16];
    int bx, by;
    const int lid = xcd_chunk_start(gridDim.x, blockIdx.x & 7) + (blockIdx.x >> 3);
    lower_tile(lid, 0, nt, by, bx);
    v4d acc[4][4];
    gemm_tile_x<4, 4>(P, npad, Pc, npad, nullptr, 0, bx, by, 0, (int)npad, 1.0, 0.0, smem, false, acc, GT_INIT);

    double *xr = smem, *xc = smem + LOO_DC * 128;          // [LOO_DC][128] each
    double *ar = smem + 2 * LOO_DC * 128, *gr = ar + 128, *ac = gr + 128, *gc = ac + 128;
    double *red = gc + 128;                                // [4][GPX_MAX_D + 2]
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
    const long r0 = (long)by * 128, c0 = (long)bx * 128;
    const int lr0 = wr * 64 + fq, lc0 = wc * 64 + fr;      // the lane's first row / column inside the tile
    __syncthreads();                                       // every wave is past its last fragment read
    if (t < 128) { ar[t] = alpha[r0 + t]; gr[t] = g[r0 + t]; }
    else { ac[t - 128] = alpha[c0 + t - 128]; gc[t - 128] = g[c0 + t - 128]; }
    // coordinates [k0, k0 + dc) of the tile's rows and columns (xw is [npad, d], zero rows in the padding)
    auto stage = [&](int k0, int dc) {
        for (int e = t; e < dc * 128; e += 256) {
            const int kk = e >> 7, p = e & 127;
            xr[e] = xw[(r0 + p) * d + k0 + kk];
            xc[e] = xw[(c0 + p) * d + k0 + kk];
        }
    };
    // the entries without the kernel's factor: m0 = acc - 1/2 (g_k alpha_l + alpha_k g_l), T from the diagonal, the weight, the scale
    __syncthreads();
    double tsum = 0.0, w[4][4][4];                         // the entries of W (then W Kf) as scalars: [i][j][r] as acc
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // one MFMA tile's four registers at a time: its tuple is free afterwards
            const int lc = lc0 + 16 * j;
            const int gl = (int)c0 + lc;
            const double al = ac[lc], gll = gc[lc];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = lr0 + 16 * i + 4 * r;
                const int gk = (int)r0 + lr;
                const bool live = gk < (int)n && gl <= gk;
                const double m = acc[i][j][r] - 0.5 * fma(gr[lr], al, ar[lr] * gll);
                if (live && gl == gk) tsum += m;
                w[i][j][r] = live ? m * ((gl < gk) ? 2.0 : 1.0) * pair.scale() : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    // pass A: every entry times Kf / scale of its pair, LOO_DC coordinates at a time (exp of a sum = product of the blocks' exps)
    for (int k0 = 0; k0 < d; k0 += LOO_DC) {
        const int dc = min(LOO_DC, d - k0);
        if (k0) __syncthreads();
        stage(k0, dc);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = lr0 + 16 * i + 4 * r;
                double q[4] = {0.0, 0.0, 0.0, 0.0};
                for (int kk = 0; kk < dc; ++kk) {
                    const double xa = xr[kk * 128 + lr];
#pragma unroll
                    for (int j = 0; j < 4; ++j) q[j] = pair.add_q(xa - xc[kk * 128 + lc0 + 16 * j], q[j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    w[i][j][r] *= pair.factor(q[j]);
                    // pins the product here: left alone, the compiler sinks all 64 factors below the 16 loops and keeps every q alive
                    asm volatile("" : "+v"(w[i][j][r]));
                }
            }
    }
    double s0 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) s0 += w[i][j][r];
    s0 = wave_sum(s0);
    tsum = wave_sum(tsum);
    if (lane == 0) { red[wave * (GPX_MAX_D + 2)] = s0; red[wave * (GPX_MAX_D + 2) + d + 1] = tsum; }
    for (int k0 = 0; k0 < d; k0 += LOO_DC) {
        const int dc = min(LOO_DC, d - k0);
        if (d > LOO_DC) {          // (a single block of coordinates is still staged)
            __syncthreads();
            stage(k0, dc);
            __syncthreads();
        }
        for (int kk = 0; kk < dc; ++kk) {
            double xb[4], s = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) xb[j] = xc[kk * 128 + lc0 + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double xa = xr[kk * 128 + lr0 + 16 * i + 4 * r];
#pragma unroll
                    for (int j = 0; j < 4; ++j) s = fma(w[i][j][r], pair.coord(xa - xb[j]), s);
                }
            s = wave_sum(s);
            if (lane == 0) red[wave * (GPX_MAX_D + 2) + 1 + k0 + kk] = s;
        }
    }
    __syncthreads();
    if (t < d + 2) {
        const double *q = red + t;
        partial[(long)lid * (d + 2) + t] = (q[0] + q[GPX_MAX_D + 2]) + (q[2 * (GPX_MAX_D + 2)] + q[3 * (GPX_MAX_D + 2)]);
    }
}

int64_t loo_tiles(int64_t npad) { return (npad / TILE) * (npad / TILE + 1) / 2; }

int launch_loo_point(const double *Kinv, int64_t ld, int64_t n, int64_t npad, const double *alpha, const double *t, double *vec, hipStream_t s)
{
    hipLaunchKernelGGL(loo_point_kernel, dim3((unsigned)(npad / 256 + 1)), dim3(256), 0, s, Kinv, (long)ld, (long)n, (long)npad, alpha, t, vec);
    GPX_HIP(hipGetLastError());
    return 0;
}

// out_dev [d + 2] = S_0, S_1..S_d, T.  vec: launch_loo_point's; gv [npad], Pc [npad, npad], partial [loo_tiles(npad), d + 2]: scratch.
int launch_loo_grad(const double *Kinv, int64_t n, int64_t npad, int d, const double *alpha, const double *xw, double v, const double *vec,
                    double *gv, double *Pc, double *partial, double *out_dev, hipStream_t s, Profiler *prof)
{
    const int nt = (int)(npad / TILE);
    const int64_t tiles = loo_tiles(npad);
    GPX_TRY(launch_kinv_pass(Kinv, npad, npad, 1, vec + npad, gv, s, prof));          // g = P a (a is zero in the padding)
    {
        ProfScope ps(prof, s, GPX_K_QUAD, 16.0 * (double)npad * (double)npad);
        hipLaunchKernelGGL(loo_scale_kernel, dim3((unsigned)npad), dim3(256), 0, s, Kinv, (long)npad, (long)n, vec, Pc);
    }
    {
        ProfScope ps(prof, s, GPX_K_GEMM, 2.0 * (double)tiles * TILE * TILE * (double)npad, 1);
        hipLaunchKernelGGL(loo_grad_kernel<LooGaussPair>, dim3((unsigned)tiles), dim3(256), 0, s, Kinv, (const double *)Pc, (long)npad, (long)n, d, nt,
                           xw, alpha, (const double *)gv, LooGaussPair{v}, partial);
    }
    GPX_HIP(hipGetLastError());
    return launch_sum_columns(partial, tiles, d + 2, out_dev, s);
}
