// predict_grad.hip -- the predictor's input gradients on the device: d mu / d x* and d sigma^2 / d x* at many queries, gfx950.
//
// With delta = x_i - u and c_i the noise-free kernel at (x_i, u):  d c_i / d u_k = +w_k delta_k g_i,  g = c for the Gaussian kernel and
// G of radial.h for Matern (nu = 3/2 is once differentiable: enough).  The rows J_k of propagate.hip / matern.hip carry the reference's sign,
// J_ik = -w_k delta_k g_i (Covariance.py:687 admits it), so with y = L^-1 t, z_v = L^-1 v:
//   mu = sum_i C_i alpha_i = z_C.y            grad mu_k      = sum_i alpha_i w_k delta_k g_i = -z_Jk.y
//   sigma^2 = (v + vt) - |z_C|^2              grad sigma^2_k = -2 (L^-1 C).(L^-1 d_k c)      = +2 z_C.z_Jk
// Two routes:
//   predict_mean_grad_kernel (+ predict_mean_grad_sum_kernel)   mu and grad mu from alpha alone: one fused pass over the M x N pairs, no solve,
//                                                               nothing N-wide stored                                (gpx_predict_mean_grad)
//   grad_reduce_many_kernel                                     the row products of the solved block [C, J_1..J_d] of every query
//                                                               (built by the GRAD instantiations of rows_build_tile, rows_tile.h)
//                                                                                                                     (gpx_predict_grad)
#include "common.h"
#include "radial.h"

// ---------------------------------------------------------------------------------------------
// mu and grad mu from alpha.  A workgroup owns PG_QUERIES queries, four per wave (u and w are wave-uniform: scalar loads), and one of the
// S ranges of 128-column tiles; a tile of x sits k-major in LDS (the staging of rows_build_tile, rows_tile.h), alpha comes as 16-byte loads.
// A lane forms q and the radial factors of its two columns and accumulates, per query,
//   sum C_i alpha_i  (C_i = c_i + vt iff x_i == u elementwise: gpx_predict's mean)   and   sum w_k delta_k g_i alpha_i  (no vt)
// for the PG_KC coordinates of its sweep: blockIdx.z sweeps of PG_KC coordinates each (1 + d accumulators for four queries do not fit in
// registers beyond d = 8).  DR > 0: d <= DR = PG_KC, one sweep, the scaled differences stay in registers; DR = 0: any d, every sweep forms q
// over all d coordinates and recomputes its own differences from the LDS tile.
// No atomics: lane -> column, tile order, the wave sum and the order of the S partials are fixed, so a query's result depends neither on its
// place in the batch nor on M beyond the choice of S.  partial: [S][M][1 + d].
// ---------------------------------------------------------------------------------------------
constexpr int PG_COLS = 128;
constexpr int PG_QUERIES = 16;
constexpr int PG_KC = 8;

template <int DR, int NU2>
__global__ __launch_bounds__(256) void predict_mean_grad_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                               const double *__restrict__ U, long nb, const double *__restrict__ w_in,
                                                               const double *__restrict__ alpha, double v, double vt,
                                                               double *__restrict__ partial)
{
    typedef typename RadialOf<NU2>::type Radial;
    const double *w = w_in;
    static_assert(DR == 0 || DR == PG_KC, "one sweep holds PG_KC coordinates");
    extern __shared__ __attribute__((aligned(16))) double pg_smem[];
    double *x_s = pg_smem;   // [d][128] raw inputs of the tile's columns, k-major
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const long ntiles = npad / PG_COLS;
    const long tile0 = ntiles * blockIdx.y / gridDim.y, tile1 = ntiles * (blockIdx.y + 1) / gridDim.y;
    const int k0 = blockIdx.z * PG_KC;
    double acc[PG_QUERIES / 4][PG_KC + 1];
#pragma unroll
    for (int j = 0; j < PG_QUERIES / 4; ++j)
#pragma unroll
        for (int e = 0; e <= PG_KC; ++e) acc[j][e] = 0.0;
    for (long tile = tile0; tile < tile1; ++tile) {
        const long col0 = tile * PG_COLS;
        __syncthreads();   // the previous tile has been read
        for (int e = t; e < PG_COLS * d; e += 256) {
            const int c = e & (PG_COLS - 1), k = e >> 7;
            const long gc = col0 + c;
            x_s[k * PG_COLS + c] = (gc < n) ? x[gc * d + k] : 0.0;
        }
        __syncthreads();
        const long c = col0 + 2 * lane;
        const bool in0 = c < n, in1 = c + 1 < n;
        const v2d al = *reinterpret_cast<const v2d *>(alpha + c);
        const double al0 = in0 ? al.x : 0.0, al1 = in1 ? al.y : 0.0;
#pragma unroll
        for (int j = 0; j < PG_QUERIES / 4; ++j) {
            long nbq = nb, b = (long)blockIdx.x * PG_QUERIES + wave;   // wave-uniform
            asm volatile("" : "+s"(nbq), "+s"(b));                    // (the four slots' numbers and tests: formed here, not held)
            b += 4 * j;
            if (b < nbq) {
                // u, w and the tests k < d are formed again for every (query, tile) -- scalar loads that the scalar cache serves: held across
                // the tile loop, four queries' u, w and the predicates would take over a hundred scalar registers beside the constants of exp
                // and spill.  The empty statement keeps them (and the query's pointer, the sweep's coordinate numbers) from being hoisted out
                // of the loop.
                int ks = k0;
                asm volatile("" : "+s"(w), "+s"(d), "+s"(ks));
                const double *u = U + (long)b * d;
                double wd0[PG_KC], wd1[PG_KC];
                double q0 = 0.0, q1 = 0.0;
                bool same0 = true, same1 = true;
                if constexpr (DR > 0) {
#pragma unroll
                    for (int k = 0; k < DR; ++k) {
                        wd0[k] = 0.0; wd1[k] = 0.0;
                        if (k < d) {
                            const v2d xv = *reinterpret_cast<const v2d *>(&x_s[k * PG_COLS + 2 * lane]);
                            const double uk = u[k], wk = w[k];
                            const double d0 = xv.x - uk, d1 = xv.y - uk;
                            same0 = same0 && (xv.x == uk);
                            same1 = same1 && (xv.y == uk);
                            wd0[k] = wk * d0; wd1[k] = wk * d1;
                            q0 = fma(wd0[k], d0, q0);
                            q1 = fma(wd1[k], d1, q1);
                        }
                    }
                } else {
#pragma unroll 2
                    for (int k = 0; k < d; ++k) {
                        const v2d xv = *reinterpret_cast<const v2d *>(&x_s[k * PG_COLS + 2 * lane]);
                        const double uk = u[k], wk = w[k];
                        const double d0 = xv.x - uk, d1 = xv.y - uk;
                        same0 = same0 && (xv.x == uk);
                        same1 = same1 && (xv.y == uk);
                        q0 = fma(wk * d0, d0, q0);
                        q1 = fma(wk * d1, d1, q1);
                    }
                    asm volatile("" : "+s"(u), "+s"(w), "+s"(d), "+s"(ks));   // the sweep's own operands only after the loop over all d
#pragma unroll
                    for (int kk = 0; kk < PG_KC; ++kk) {
                        // a coordinate past d: the last one with weight zero (a select, no predicate kept in scalar registers)
                        const int k = ks + kk, kc = k < d ? k : d - 1;
                        const v2d xv = *reinterpret_cast<const v2d *>(&x_s[kc * PG_COLS + 2 * lane]);
                        const double uk = u[kc], wk = k < d ? w[kc] : 0.0;
                        wd0[kk] = wk * (xv.x - uk); wd1[kk] = wk * (xv.y - uk);
                    }
                }
                // columns past n: alpha is taken as zero there, so every term is
                const Radial r0(v, q0), r1(v, q1);
                const double c0 = r0.kf(), c1 = r1.kf();
                const double C0 = (in0 && same0) ? c0 + vt : c0, C1 = (in1 && same1) ? c1 + vt : c1;
                acc[j][0] = fma(C1, al1, fma(C0, al0, acc[j][0]));
                const double ga0 = r0.g() * al0, ga1 = r1.g() * al1;
#pragma unroll
                for (int kk = 0; kk < PG_KC; ++kk) acc[j][1 + kk] = fma(wd1[kk], ga1, fma(wd0[kk], ga0, acc[j][1 + kk]));
            }
            __builtin_amdgcn_sched_barrier(0);   // one query's scalar operands at a time
        }
    }
    const int nout = 1 + d;
#pragma unroll
    for (int j = 0; j < PG_QUERIES / 4; ++j) {
        const long b = (long)blockIdx.x * PG_QUERIES + 4 * j + wave;
        if (b < nb) {
            double *p = partial + ((long)blockIdx.y * nb + b) * nout;
            const double s0 = wave_sum(acc[j][0]);
            if (lane == 0 && k0 == 0) p[0] = s0;
#pragma unroll
            for (int kk = 0; kk < PG_KC; ++kk) {
                const double sk = wave_sum(acc[j][1 + kk]);
                if (lane == 0 && k0 + kk < d) p[1 + k0 + kk] = sk;
            }
        }
    }
}

// mean[b] / dmean[b][k] = the S partials of the output added in index order (either output may be null)
__global__ __launch_bounds__(256) void predict_mean_grad_sum_kernel(const double *__restrict__ partial, int S, long nb, int d,
                                                                   double *__restrict__ mean, double *__restrict__ dmean)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x, nout = 1 + d;
    if (e >= nb * nout) return;
    double s = 0.0;
    for (int i = 0; i < S; ++i) s += partial[(long)i * nb * nout + e];
    const long b = e / nout;
    const int r = (int)(e - b * nout);
    if (r == 0) { if (mean) mean[b] = s; }
    else if (dmean) dmean[b * d + (r - 1)] = s;
}

// S: the column ranges a query block is cut into, from M and npad alone -- 768 workgroups where M allows (three per compute unit, which is
// what the kernel's 3 waves per SIMD hold at once: 4096 queries at N = 16384 take 0.323 ms with 768, 0.343 ms with 1024 -- a second, thin
// round -- and 0.372 ms with 512), never more ranges than there are tiles, at most 64
int predict_mean_grad_splits(int64_t nb, int64_t npad)
{
    const int64_t qblocks = (nb + PG_QUERIES - 1) / PG_QUERIES, ntiles = npad / PG_COLS;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ntiles, 64), (768 + qblocks - 1) / qblocks));
}

// nu2 = 0: the Gaussian kernel; 3 / 5: Matern.  x raw [n, d]; U_dev [nb, d]; partial [S, nb, 1 + d] scratch; mean_dev [nb] / dmean_dev [nb, d]
// (either may be null)
int launch_predict_mean_grad(const double *x, int64_t n, int64_t npad, int d, int nu2, const double *U_dev, int64_t nb, const double *w_dev,
                             const double *alpha, double v, double vt, int S, double *partial, double *mean_dev, double *dmean_dev, hipStream_t s,
                             Profiler *prof)
{
    if (nb <= 0) return 0;
    const int64_t qblocks = (nb + PG_QUERIES - 1) / PG_QUERIES;
    if (npad % PG_COLS || d < 1 || d > GPX_MAX_D || S < 1 || S > npad / PG_COLS || S > 65535 || qblocks > 0x7fffffff ||
        (nu2 != 0 && nu2 != 3 && nu2 != 5)) {
        gpx_set_error("predict_mean_grad: bad shape (nb=%ld npad=%ld d=%d S=%d nu2=%d)", (long)nb, (long)npad, d, S, nu2);
        return GPX_ERR_BAD_ARG;
    }
    {
        ProfScope ps(prof, s, GPX_K_GRAM, 8.0 * (double)nb * (double)npad);
        const int sweeps = d <= PG_KC ? 1 : (d + PG_KC - 1) / PG_KC;
        const dim3 grid((unsigned)qblocks, (unsigned)S, (unsigned)sweeps);
        const size_t lds = sizeof(double) * PG_COLS * d;
#define PG_LAUNCH(DR, NU2)                                                                                                                  \
    hipLaunchKernelGGL((predict_mean_grad_kernel<DR, NU2>), grid, dim3(256), lds, s, x, (long)n, (long)npad, d, U_dev, (long)nb, w_dev, alpha, v, vt, \
                       partial)
        if (d <= PG_KC) {
            if (nu2 == 0) PG_LAUNCH(PG_KC, 0);
            else if (nu2 == 3) PG_LAUNCH(PG_KC, 3);
            else PG_LAUNCH(PG_KC, 5);
        } else {
            if (nu2 == 0) PG_LAUNCH(0, 0);
            else if (nu2 == 3) PG_LAUNCH(0, 3);
            else PG_LAUNCH(0, 5);
        }
#undef PG_LAUNCH
        GPX_HIP(hipGetLastError());
    }
    ProfScope ps(prof, s, GPX_K_REDUCE, 8.0 * (double)S * (double)nb * (double)(1 + d));
    const int64_t nout = nb * (1 + d);
    hipLaunchKernelGGL(predict_mean_grad_sum_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, (const double *)partial, S, (long)nb, d,
                       mean_dev, dmean_dev);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// One pass over the solved block Zs (row b (d + 1) + r = L^-1 of [C, J_1..J_d] of query b), one workgroup per query, the layout of
// approx_reduce_many_kernel: z_C.y, |z_C|^2 and per k z_Jk.y, z_C.z_Jk, then
//   mean = z_C.y    var = (v + vt) - |z_C|^2    dmean_k = -z_Jk.y    dvar_k = 2 z_C.z_Jk        (dmean may be null)
// DR > 0 (d <= DR): columns outside, k inside, every solved row read once; DR = 0 (any d): rows outside, the z_C row (it stays in L2) read
// again for every k.  No atomics; thread -> column, wave -> LDS slot and the final sum are fixed.
// ---------------------------------------------------------------------------------------------
// PAIR: the model is held as K^-1 (a pseudo-input model), not as a factor.  Zs = R, the rows as built, Ys = R K^-1 and y = alpha: z_C.y becomes
// r_C.alpha, |z_C|^2 becomes r_C.y_C, z_Jk.y becomes r_Jk.alpha and z_C.z_Jk becomes y_C.r_Jk (the row of R K^-1 that a query needs is y_C
// alone); thread -> column, the order of the terms and the finish are the same.  PAIR = false does not touch Ys.  One body, two kernels:
// grad_reduce_many_kernel<DR> keeps its signature and its code, grad_reduce_pair_kernel<DR> is the K^-1 form.
template <int DR, bool PAIR>
static __device__ __forceinline__ void grad_reduce_body(const double *__restrict__ Zs, const double *__restrict__ Ys, long npad, int d,
                                                        const double *__restrict__ y, double vplusvt, double *__restrict__ mean,
                                                        double *__restrict__ var, double *__restrict__ dmean, double *__restrict__ dvar)
{
    __shared__ double part[2 * GPX_MAX_D + 2][4];   // 2 k: z_Jk.y   2 k + 1: z_C.z_Jk   2 d: z_C.y   2 d + 1: |z_C|^2
    const long b = blockIdx.x;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const double *zc = Zs + b * (d + 1) * npad;
    const double *pc = PAIR ? Ys + b * (d + 1) * npad : zc;   // the C row's second factor: y_C (pair form), z_C itself otherwise
    if constexpr (DR > 0) {
        double yj[DR], cj[DR], yc = 0.0, qc = 0.0;
#pragma unroll
        for (int k = 0; k < DR; ++k) { yj[k] = 0.0; cj[k] = 0.0; }
        for (long c = 2 * t; c < npad; c += 512) {
            const v2d a = *reinterpret_cast<const v2d *>(zc + c);
            const v2d yy = *reinterpret_cast<const v2d *>(y + c);
            v2d p = a;
            if constexpr (PAIR) p = *reinterpret_cast<const v2d *>(pc + c);
            yc = fma(a.x, yy.x, yc); yc = fma(a.y, yy.y, yc);
            qc = fma(a.x, p.x, qc); qc = fma(a.y, p.y, qc);
#pragma unroll
            for (int k = 0; k < DR; ++k) {
                if (k < d) {
                    const v2d zj = *reinterpret_cast<const v2d *>(zc + (long)(1 + k) * npad + c);
                    yj[k] = fma(zj.x, yy.x, yj[k]); yj[k] = fma(zj.y, yy.y, yj[k]);
                    cj[k] = fma(p.x, zj.x, cj[k]); cj[k] = fma(p.y, zj.y, cj[k]);
                }
            }
        }
        yc = wave_sum(yc); qc = wave_sum(qc);
        if (lane == 0) { part[2 * d][wave] = yc; part[2 * d + 1][wave] = qc; }
#pragma unroll
        for (int k = 0; k < DR; ++k) {
            if (k < d) {
                const double sy = wave_sum(yj[k]), sc = wave_sum(cj[k]);
                if (lane == 0) { part[2 * k][wave] = sy; part[2 * k + 1][wave] = sc; }
            }
        }
    } else {
        double yc = 0.0, qc = 0.0;
        for (long c = 2 * t; c < npad; c += 512) {
            const v2d a = *reinterpret_cast<const v2d *>(zc + c);
            const v2d yy = *reinterpret_cast<const v2d *>(y + c);
            v2d p = a;
            if constexpr (PAIR) p = *reinterpret_cast<const v2d *>(pc + c);
            yc = fma(a.x, yy.x, yc); yc = fma(a.y, yy.y, yc);
            qc = fma(a.x, p.x, qc); qc = fma(a.y, p.y, qc);
        }
        yc = wave_sum(yc); qc = wave_sum(qc);
        if (lane == 0) { part[2 * d][wave] = yc; part[2 * d + 1][wave] = qc; }
        for (int k = 0; k < d; ++k) {
            const double *zjr = zc + (long)(1 + k) * npad;
            double sy = 0.0, sc = 0.0;
            for (long c = 2 * t; c < npad; c += 512) {
                const v2d a = *reinterpret_cast<const v2d *>(pc + c);
                const v2d yy = *reinterpret_cast<const v2d *>(y + c);
                const v2d zj = *reinterpret_cast<const v2d *>(zjr + c);
                sy = fma(zj.x, yy.x, sy); sy = fma(zj.y, yy.y, sy);
                sc = fma(a.x, zj.x, sc); sc = fma(a.y, zj.y, sc);
            }
            sy = wave_sum(sy); sc = wave_sum(sc);
            if (lane == 0) { part[2 * k][wave] = sy; part[2 * k + 1][wave] = sc; }
        }
    }
    __syncthreads();
    auto tot = [&](int i) { return (part[i][0] + part[i][1]) + (part[i][2] + part[i][3]); };
    if (t < d) {
        if (dmean) dmean[b * d + t] = -tot(2 * t);
        dvar[b * d + t] = 2.0 * tot(2 * t + 1);
    }
    if (t == 64) { mean[b] = tot(2 * d); var[b] = vplusvt - tot(2 * d + 1); }
}

template <int DR>
__global__ __launch_bounds__(256) void grad_reduce_many_kernel(const double *__restrict__ Zs, long npad, int d, const double *__restrict__ y,
                                                              double vplusvt, double *__restrict__ mean, double *__restrict__ var,
                                                              double *__restrict__ dmean, double *__restrict__ dvar)
{
    grad_reduce_body<DR, false>(Zs, nullptr, npad, d, y, vplusvt, mean, var, dmean, dvar);
}

template <int DR>
__global__ __launch_bounds__(256) void grad_reduce_pair_kernel(const double *__restrict__ R, const double *__restrict__ Y, long npad, int d,
                                                              const double *__restrict__ alpha, double vplusvt, double *__restrict__ mean,
                                                              double *__restrict__ var, double *__restrict__ dmean, double *__restrict__ dvar)
{
    grad_reduce_body<DR, true>(R, Y, npad, d, alpha, vplusvt, mean, var, dmean, dvar);
}

int launch_grad_reduce_many(const double *Zs, int64_t npad, int d, const double *y, int64_t nb, double vplusvt, double *mean, double *var,
                            double *dmean, double *dvar, hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    if (npad % 2 || d < 1 || d > GPX_MAX_D) { gpx_set_error("grad_reduce_many: bad block shape"); return GPX_ERR_BAD_ARG; }
    ProfScope ps(prof, s, GPX_K_REDUCE, 8.0 * (double)nb * (double)(d + 1) * (double)npad);
    if (d <= 8)
        hipLaunchKernelGGL(grad_reduce_many_kernel<8>, dim3((unsigned)nb), dim3(256), 0, s, Zs, (long)npad, d, y, vplusvt, mean, var, dmean, dvar);
    else
        hipLaunchKernelGGL(grad_reduce_many_kernel<0>, dim3((unsigned)nb), dim3(256), 0, s, Zs, (long)npad, d, y, vplusvt, mean, var, dmean, dvar);
    GPX_HIP(hipGetLastError());
    return 0;
}

int launch_grad_reduce_many_pair(const double *R, const double *Y, int64_t npad, int d, const double *alpha, int64_t nb, double vplusvt, double *mean,
                                 double *var, double *dmean, double *dvar, hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    if (!R || !Y || !alpha || npad % 2 || d < 1 || d > GPX_MAX_D) { gpx_set_error("grad_reduce_many_pair: bad block shape"); return GPX_ERR_BAD_ARG; }
    ProfScope ps(prof, s, GPX_K_REDUCE, 8.0 * (double)nb * (double)(d + 2) * (double)npad);
    if (d <= 8)
        hipLaunchKernelGGL(grad_reduce_pair_kernel<8>, dim3((unsigned)nb), dim3(256), 0, s, R, Y, (long)npad, d, alpha, vplusvt, mean, var, dmean, dvar);
    else
        hipLaunchKernelGGL(grad_reduce_pair_kernel<0>, dim3((unsigned)nb), dim3(256), 0, s, R, Y, (long)npad, d, alpha, vplusvt, mean, var, dmean, dvar);
    GPX_HIP(hipGetLastError());
    return 0;
}
