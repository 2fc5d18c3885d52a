// propagate.hip -- Girard uncertainty propagation (Approx and Exact) on the fitted model, gfx950.
//
// Device equivalents of the reference's only native component, skgpuppy/UncertaintyPropagation2.pyx
// (Cython twins of skgpuppy/UncertaintyPropagation.py:246-630), loops K1..K8 of SURVEY.md 2a:
//   K8  C_ux / J_ux / H_ux build (3N Python calls in the reference)      -> approx_build_kernel / cjh_kernel
//   K2..K6  sum_ij Kinv_ij a_i b_j quadratic forms (serial N^2 passes)     -> ONE pass Kinv x [C, J_1..J_d]
//           (the forms against tr / H_hh reuse Kinv C by symmetry)        +  row dot products
//   K7  exact mean  sum_i beta_i l_i                                       -> exact_build_kernel + dot
//   K1  exact variance double sum over L_ij = C_i C_j nc exp(1/2 z^T Lambda^-1 z)
//       -> exact_sum_kernel: each thread owns a column j (coalesced Kinv reads), a workgroup owns 16
//          rows; the d^2 inner loop is factorised as exp(e_i + e_j + b_i . a_j), b_i = Lambda^-1 a_i / 4.
#include "common.h"
#include "rows_tile.h"

// ---------------------------------------------------------------------------------------------
// Approx: per-row quantities for a given u.   VM rows: 0 = C, 1..d = J_k.   AUX rows: 1..d = H_kk
// c_i = v exp(-1/2 sum w_k delta_k^2), delta = x_i - u          (Covariance.py:660-689)
// C_i = c_i + vt iff x_i == u elementwise                        (Covariance.py:440-451)
// J_i[k] = -delta_k w_k c_i ; H_i[k][k] = ((w_k delta_k)^2 - w_k) c_i
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void approx_build_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                          const double *__restrict__ u, const double *__restrict__ w,
                                                          double v, double vt, double *__restrict__ VM,
                                                          double *__restrict__ AUX, double *__restrict__ cplain)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    if (i >= n) {
        for (int k = 0; k <= d; ++k) VM[(long)k * npad + i] = 0.0;
        for (int k = 0; k <= d; ++k) AUX[(long)k * npad + i] = 0.0;
        cplain[i] = 0.0;
        return;
    }
    double q = 0.0;
    bool same = true;
    for (int k = 0; k < d; ++k) {
        const double xv = x[i * d + k], uv = u[k];
        const double dl = xv - uv;
        same = same && (xv == uv);
        q = fma(w[k] * dl, dl, q);
    }
    const double c = v * exp(-0.5 * q);
    cplain[i] = c;
    VM[i] = same ? c + vt : c;
    for (int k = 0; k < d; ++k) {
        const double dl = x[i * d + k] - u[k];
        const double wd = w[k] * dl;
        VM[(long)(k + 1) * npad + i] = -dl * w[k] * c;
        AUX[(long)(k + 1) * npad + i] = (wd * wd - w[k]) * c;
    }
}

// tr_i = tr(H_i Sigma) = c_i ( (w delta)^T Sigma (w delta) - sum_k w_k Sigma_kk )   -> AUX row 0
// (tracedot(H, Sigma), UncertaintyPropagation.py:464 / Covariance.py:101-109; full Sigma allowed)
__global__ __launch_bounds__(256) void trace_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                   const double *__restrict__ u, const double *__restrict__ w,
                                                   const double *__restrict__ Sigma, const double *__restrict__ cplain,
                                                   double *__restrict__ tr)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    if (i >= n) { tr[i] = 0.0; return; }
    double s = 0.0, wdiag = 0.0;
    for (int a = 0; a < d; ++a) {
        const double wa = w[a] * (x[i * d + a] - u[a]);
        double row = 0.0;
        for (int b = 0; b < d; ++b) row = fma(Sigma[a * d + b], w[b] * (x[i * d + b] - u[b]), row);
        s = fma(wa, row, s);
        wdiag = fma(w[a], Sigma[a * d + a], wdiag);
    }
    tr[i] = cplain[i] * (s - wdiag);
}

// out[p] = sum_i P_p[i] Q_p[i], one workgroup per pair, fixed summation order (deterministic)
struct DotPairs { const double *p[80]; const double *q[80]; };
// (1024 threads, 16-byte loads where the operands allow them: a pair of 16384 entries is 8 dependent loads per thread -- the
// 256-thread, 8-byte version was a chain of 64 and took 22 us, a quarter of a propagation call's overhead)
__global__ __launch_bounds__(1024) void dot_pairs_kernel(DotPairs pairs, long n, double *__restrict__ out)
{
    __shared__ double ws[16];
    const double *P = pairs.p[blockIdx.x], *Q = pairs.q[blockIdx.x];
    double s0 = 0.0, s1 = 0.0;
    const bool wide = !(n & 1) && !(((uintptr_t)P | (uintptr_t)Q) & 15);      // uniform per workgroup
    if (wide) {
        const long half = n >> 1;
        for (long i = threadIdx.x; i < half; i += 1024) {
            const v2d a = reinterpret_cast<const v2d *>(P)[i], b = reinterpret_cast<const v2d *>(Q)[i];
            s0 = fma(a.x, b.x, s0);
            s1 = fma(a.y, b.y, s1);
        }
    } else
        for (long i = threadIdx.x; i < n; i += 1024) s0 = fma(P[i], Q[i], s0);
    double s = wave_sum(s0 + s1);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += ws[w];
        out[blockIdx.x] = t;
    }
}

int launch_dot_pairs(const std::vector<std::pair<const double *, const double *>> &pr, long n, double *out_dev,
                     hipStream_t s)
{
    size_t done = 0;
    while (done < pr.size()) {
        DotPairs dp;
        size_t cnt = std::min<size_t>(80, pr.size() - done);
        for (size_t i = 0; i < cnt; ++i) { dp.p[i] = pr[done + i].first; dp.q[i] = pr[done + i].second; }
        hipLaunchKernelGGL(dot_pairs_kernel, dim3((unsigned)cnt), dim3(1024), 0, s, dp, n, out_dev + done);
        done += cnt;
    }
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The build kernels of the batched row calls on the Gaussian kernel: the frame of rows_tile.h with the GaussRows policy.
// approx_build_many_kernel<DR, GRAD>: the APPROX rows [C, tr, J_1..J_d] (GRAD: the rows [C, J_1..J_d] of gpx_predict_grad, Sigma not read);
// dvh_build_many_kernel<DR>: the DVH rows [C, J_1..J_d, H_11..H_dd].  DR = 8: d <= 8; DR = 0: any d.
// ---------------------------------------------------------------------------------------------
template <int DR, bool GRAD = false>
__global__ __launch_bounds__(256) void approx_build_many_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                               const double *__restrict__ U, const double *__restrict__ Sigma,
                                                               long sigma_stride, long nb, const double *__restrict__ w, double v,
                                                               double vt, double *__restrict__ Z)
{
    rows_build_tile<DR, GRAD ? GPX_ROWS_GRAD : GPX_ROWS_APPROX>(GaussRows{v, vt}, x, n, npad, d, U, Sigma, sigma_stride, nb, w, Z);
}

template <int DR>
__global__ __launch_bounds__(256) void dvh_build_many_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                            const double *__restrict__ U, long nb, const double *__restrict__ w, double v,
                                                            double vt, double *__restrict__ Z)
{
    rows_build_tile<DR, GPX_ROWS_DVH>(GaussRows{v, vt}, x, n, npad, d, U, nullptr, 0, nb, w, Z);
}

// this file's part of launch_rows_build's table (matern.hip's: matern_rows_kernel)
static RowsKernel gauss_rows_kernel(int layout, bool regs)
{
    if (layout == GPX_ROWS_APPROX) return {regs ? approx_build_many_kernel<8, false> : approx_build_many_kernel<0, false>, nullptr};
    if (layout == GPX_ROWS_GRAD) return {regs ? approx_build_many_kernel<8, true> : approx_build_many_kernel<0, true>, nullptr};
    if (layout == GPX_ROWS_DVH) return {nullptr, regs ? dvh_build_many_kernel<8> : dvh_build_many_kernel<0>};
    return {nullptr, nullptr};
}

// The ONE launcher of every build kernel.  nu2 = 0: the Gaussian kernel, 3 / 5: Matern (RadialOf's convention, radial.h; nu2 = 3 has the
// GRAD layout alone).  Z [rows_pad, npad]: rows [0, nb rows_per_input(layout, d)) are written by the kernel (every column, zeros from n
// on), the rest of the last 128-row tile is cleared.  Sigma is read for GPX_ROWS_APPROX alone.
int launch_rows_build(int nu2, int layout, const double *x, int64_t n, int64_t npad, int d, const double *U_dev, const double *Sigma_dev,
                      int64_t sigma_stride, int64_t nb, int64_t rows_pad, const double *w_dev, double v, double vt, double *Z, hipStream_t s,
                      Profiler *prof)
{
    if (nb <= 0) return 0;
    const int64_t rows = nb * rows_per_input(layout, d);
    const RowsKernel k = nu2 == 0 ? gauss_rows_kernel(layout, d <= 8) : matern_rows_kernel(nu2, layout, d <= 8);   // (family, layout, d <= 8)
    if (npad % RT_COLS || rows > rows_pad || d < 1 || d > GPX_MAX_D || (!k.with_sigma && !k.plain)) {
        gpx_set_error("rows_build: bad block shape (nu2=%d layout=%d npad=%ld d=%d rows_pad=%ld)", nu2, layout, (long)npad, d, (long)rows_pad);
        return GPX_ERR_BAD_ARG;
    }
    ProfScope ps(prof, s, GPX_K_GRAM, 8.0 * (double)rows_pad * (double)npad);
    if (rows_pad > rows) GPX_HIP(hipMemsetAsync(Z + rows * npad, 0, sizeof(double) * (rows_pad - rows) * npad, s));
    const dim3 grid((unsigned)(npad / RT_COLS), (unsigned)((nb + RT_INPUTS - 1) / RT_INPUTS));
    const size_t lds = sizeof(double) * RT_COLS * d;
    if (k.with_sigma)
        hipLaunchKernelGGL(k.with_sigma, grid, dim3(256), lds, s, x, (long)n, (long)npad, d, U_dev, Sigma_dev, (long)sigma_stride, (long)nb, w_dev, v, vt, Z);
    else
        hipLaunchKernelGGL(k.plain, grid, dim3(256), lds, s, x, (long)n, (long)npad, d, U_dev, (long)nb, w_dev, v, vt, Z);
    GPX_HIP(hipGetLastError());
    return 0;
}

// One pass over the solved block Zs (row b (d + 2) + r = L^-1 of the vector above), one workgroup per input: per row |z_r|^2 and
// z_r . y, for rows 0 and 1 also z_C . z_tr, then the four outputs (UncertaintyPropagation.py:397-481 with K^-1 = L^-T L^-1):
//   mean = z_C.y + 1/2 z_tr.y   sigma2 = (v + vt) - |z_C|^2   rest = -sum_k Sigma_kk (|z_Jk|^2 - (z_Jk.y)^2) - z_C.z_tr
// No atomics; thread -> column, wave -> LDS slot and the final sum are fixed, so an input's result does not depend on its
// place in the batch.  out: [4][ldo] = mean | var | sigma2 | rest.
// PAIR: the model is held as K^-1 (a pseudo-input model), not as a factor.  Zs = R, the rows as built, Ys = R K^-1 and y = alpha = K^-1 t: every
// |z_r|^2 becomes r_r.y_r, every z_r.y becomes r_r.alpha and z_C.z_tr becomes y_C.r_tr; the thread -> column map, the order of the terms
// and everything after the sums are the same.  PAIR = false reads Zs alone (Ys is not touched).  One body, two kernels:
// approx_reduce_many_kernel keeps its signature and its code, approx_reduce_pair_kernel is the K^-1 form.
template <bool PAIR>
static __device__ __forceinline__ void approx_reduce_body(const double *__restrict__ Zs, const double *__restrict__ Ys, long npad, int d,
                                                          const double *__restrict__ y, const double *__restrict__ Sigma, long sigma_stride,
                                                          double vplusvt, double *__restrict__ out, long ldo)
{
    __shared__ double part[(GPX_MAX_D + 2) * 2 + 1][4];
    const long b = blockIdx.x;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const double *z0 = Zs + b * (d + 2) * npad, *z1 = z0 + npad;
    const double *p0 = PAIR ? Ys + b * (d + 2) * npad : z0;   // the second factor of every square
    {
        double q0 = 0.0, y0 = 0.0, q1 = 0.0, y1 = 0.0, x01 = 0.0;
        for (long c = 2 * t; c < npad; c += 512) {
            const v2d a = *reinterpret_cast<const v2d *>(z0 + c), e = *reinterpret_cast<const v2d *>(z1 + c);
            const v2d yy = *reinterpret_cast<const v2d *>(y + c);
            if constexpr (PAIR) {
                const v2d pa = *reinterpret_cast<const v2d *>(p0 + c);
                q0 = fma(a.x, pa.x, q0); q0 = fma(a.y, pa.y, q0);
                y0 = fma(a.x, yy.x, y0); y0 = fma(a.y, yy.y, y0);
                y1 = fma(e.x, yy.x, y1); y1 = fma(e.y, yy.y, y1);
                x01 = fma(pa.x, e.x, x01); x01 = fma(pa.y, e.y, x01);   // (tr.Kinv tr is no output: q1 stays 0)
            } else {
                q0 = fma(a.x, a.x, q0); q0 = fma(a.y, a.y, q0);
                y0 = fma(a.x, yy.x, y0); y0 = fma(a.y, yy.y, y0);
                q1 = fma(e.x, e.x, q1); q1 = fma(e.y, e.y, q1);
                y1 = fma(e.x, yy.x, y1); y1 = fma(e.y, yy.y, y1);
                x01 = fma(a.x, e.x, x01); x01 = fma(a.y, e.y, x01);
            }
        }
        q0 = wave_sum(q0); y0 = wave_sum(y0); q1 = wave_sum(q1); y1 = wave_sum(y1); x01 = wave_sum(x01);
        if (lane == 0) { part[0][wave] = q0; part[1][wave] = y0; part[2][wave] = q1; part[3][wave] = y1; part[2 * (d + 2)][wave] = x01; }
    }
    for (int r = 2; r < d + 2; ++r) {
        const double *zr = z0 + (long)r * npad;
        double q = 0.0, sy = 0.0;
        for (long c = 2 * t; c < npad; c += 512) {
            const v2d a = *reinterpret_cast<const v2d *>(zr + c);
            const v2d yy = *reinterpret_cast<const v2d *>(y + c);
            if constexpr (PAIR) {
                const v2d pa = *reinterpret_cast<const v2d *>(p0 + (long)r * npad + c);
                q = fma(a.x, pa.x, q); q = fma(a.y, pa.y, q);
            } else {
                q = fma(a.x, a.x, q); q = fma(a.y, a.y, q);
            }
            sy = fma(a.x, yy.x, sy); sy = fma(a.y, yy.y, sy);
        }
        q = wave_sum(q); sy = wave_sum(sy);
        if (lane == 0) { part[2 * r][wave] = q; part[2 * r + 1][wave] = sy; }
    }
    __syncthreads();
    if (t == 0) {
        auto tot = [&](int i) { return (part[i][0] + part[i][1]) + (part[i][2] + part[i][3]); };
        const double *S = Sigma + b * sigma_stride;
        const double mean = tot(1) + 0.5 * tot(3);
        const double s2 = vplusvt - tot(0);
        double var2 = 0.0;
        for (int k = 0; k < d; ++k) {
            const double zy = tot(2 * (k + 2) + 1);
            var2 += S[k * d + k] * (tot(2 * (k + 2)) - zy * zy);
        }
        const double rest = -var2 - tot(2 * (d + 2));
        out[b] = mean;
        out[ldo + b] = s2 + rest;
        out[2 * ldo + b] = s2;
        out[3 * ldo + b] = rest;
    }
}

__global__ __launch_bounds__(256) void approx_reduce_many_kernel(const double *__restrict__ Zs, long npad, int d,
                                                                const double *__restrict__ y, const double *__restrict__ Sigma,
                                                                long sigma_stride, double vplusvt, double *__restrict__ out, long ldo)
{
    approx_reduce_body<false>(Zs, nullptr, npad, d, y, Sigma, sigma_stride, vplusvt, out, ldo);
}

__global__ __launch_bounds__(256) void approx_reduce_pair_kernel(const double *__restrict__ R, const double *__restrict__ Y, long npad, int d,
                                                                const double *__restrict__ alpha, const double *__restrict__ Sigma,
                                                                long sigma_stride, double vplusvt, double *__restrict__ out, long ldo)
{
    approx_reduce_body<true>(R, Y, npad, d, alpha, Sigma, sigma_stride, vplusvt, out, ldo);
}

int launch_approx_reduce_many(const double *Zs, int64_t npad, int d, const double *y, const double *Sigma_dev, int64_t sigma_stride,
                              int64_t nb, double vplusvt, double *out, int64_t ldo, hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    ProfScope ps(prof, s, GPX_K_REDUCE, 8.0 * (double)nb * (double)(d + 2) * (double)npad);
    hipLaunchKernelGGL(approx_reduce_many_kernel, dim3((unsigned)nb), dim3(256), 0, s, Zs, (long)npad, d, y, Sigma_dev,
                       (long)sigma_stride, vplusvt, out, (long)ldo);
    GPX_HIP(hipGetLastError());
    return 0;
}

int launch_approx_reduce_many_pair(const double *R, const double *Y, int64_t npad, int d, const double *alpha, const double *Sigma_dev,
                                   int64_t sigma_stride, int64_t nb, double vplusvt, double *out, int64_t ldo, hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    if (!R || !Y || !alpha || npad % 2 || d < 1 || d > GPX_MAX_D) { gpx_set_error("approx_reduce_many_pair: bad block shape"); return GPX_ERR_BAD_ARG; }
    ProfScope ps(prof, s, GPX_K_REDUCE, 16.0 * (double)nb * (double)(d + 2) * (double)npad);
    hipLaunchKernelGGL(approx_reduce_pair_kernel, dim3((unsigned)nb), dim3(256), 0, s, R, Y, (long)npad, d, alpha, Sigma_dev,
                       (long)sigma_stride, vplusvt, out, (long)ldo);
    GPX_HIP(hipGetLastError());
    return 0;
}

// One pass over the solved block Zs (row b (2 d + 1) + r = L^-1 of the vector above), one workgroup per input: |z_C|^2 and per k
// |z_Jk|^2, z_Jk . y and z_C . z_Hkk, then (UncertaintyPropagation.py:564-630 and :412-433 with K^-1 = L^-T L^-1, y = L^-1 t)
//   dvh[b][k] = -(|z_Jk|^2 - (z_Jk.y)^2) - z_C.z_Hkk      sigma2[b] = (v + vt) - |z_C|^2      (sigma2 may be null)
// DR > 0 (d <= DR): columns outside, k inside, the 3 d + 1 sums in registers, every solved row read once.  DR = 0 (any d): rows outside;
// the z_C row (8 npad bytes, it stays in L2) is read again for every k.  No atomics; thread -> column, wave -> LDS slot and the final sum
// are fixed, so an input's result does not depend on its place in the batch.
template <int DR>
__global__ __launch_bounds__(256) void dvh_reduce_many_kernel(const double *__restrict__ Zs, long npad, int d, const double *__restrict__ y,
                                                             double vplusvt, double *__restrict__ dvh, double *__restrict__ sigma2)
{
    __shared__ double part[3 * GPX_MAX_D + 1][4];   // 3 k: |z_Jk|^2   3 k + 1: z_Jk.y   3 k + 2: z_C.z_Hkk   3 d: |z_C|^2
    const long b = blockIdx.x;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const double *zc = Zs + b * (2 * d + 1) * npad;
    if constexpr (DR > 0) {
        double qj[DR], yj[DR], ch[DR], qc = 0.0;
#pragma unroll
        for (int k = 0; k < DR; ++k) { qj[k] = 0.0; yj[k] = 0.0; ch[k] = 0.0; }
        for (long c = 2 * t; c < npad; c += 512) {
            const v2d a = *reinterpret_cast<const v2d *>(zc + c);
            const v2d yy = *reinterpret_cast<const v2d *>(y + c);
            qc = fma(a.x, a.x, qc); qc = fma(a.y, a.y, qc);
#pragma unroll
            for (int k = 0; k < DR; ++k) {
                if (k < d) {
                    const v2d zj = *reinterpret_cast<const v2d *>(zc + (long)(1 + k) * npad + c);
                    const v2d zh = *reinterpret_cast<const v2d *>(zc + (long)(1 + d + k) * npad + c);
                    qj[k] = fma(zj.x, zj.x, qj[k]); qj[k] = fma(zj.y, zj.y, qj[k]);
                    yj[k] = fma(zj.x, yy.x, yj[k]); yj[k] = fma(zj.y, yy.y, yj[k]);
                    ch[k] = fma(a.x, zh.x, ch[k]); ch[k] = fma(a.y, zh.y, ch[k]);
                }
            }
        }
        qc = wave_sum(qc);
        if (lane == 0) part[3 * d][wave] = qc;
#pragma unroll
        for (int k = 0; k < DR; ++k) {
            if (k < d) {
                const double q = wave_sum(qj[k]), sy = wave_sum(yj[k]), sh = wave_sum(ch[k]);
                if (lane == 0) { part[3 * k][wave] = q; part[3 * k + 1][wave] = sy; part[3 * k + 2][wave] = sh; }
            }
        }
    } else {
        double qc = 0.0;
        for (long c = 2 * t; c < npad; c += 512) {
            const v2d a = *reinterpret_cast<const v2d *>(zc + c);
            qc = fma(a.x, a.x, qc); qc = fma(a.y, a.y, qc);
        }
        qc = wave_sum(qc);
        if (lane == 0) part[3 * d][wave] = qc;
        for (int k = 0; k < d; ++k) {
            const double *zjr = zc + (long)(1 + k) * npad, *zhr = zc + (long)(1 + d + k) * npad;
            double q = 0.0, sy = 0.0, sh = 0.0;
            for (long c = 2 * t; c < npad; c += 512) {
                const v2d a = *reinterpret_cast<const v2d *>(zc + c);
                const v2d yy = *reinterpret_cast<const v2d *>(y + c);
                const v2d zj = *reinterpret_cast<const v2d *>(zjr + c), zh = *reinterpret_cast<const v2d *>(zhr + c);
                q = fma(zj.x, zj.x, q); q = fma(zj.y, zj.y, q);
                sy = fma(zj.x, yy.x, sy); sy = fma(zj.y, yy.y, sy);
                sh = fma(a.x, zh.x, sh); sh = fma(a.y, zh.y, sh);
            }
            q = wave_sum(q); sy = wave_sum(sy); sh = wave_sum(sh);
            if (lane == 0) { part[3 * k][wave] = q; part[3 * k + 1][wave] = sy; part[3 * k + 2][wave] = sh; }
        }
    }
    __syncthreads();
    auto tot = [&](int i) { return (part[i][0] + part[i][1]) + (part[i][2] + part[i][3]); };
    if (t < d) {
        const double zy = tot(3 * t + 1);
        const double v2 = -(tot(3 * t) - zy * zy);   // UncertaintyPropagation.py:593-607
        const double v3 = -tot(3 * t + 2);           // :614-627
        dvh[b * d + t] = v2 + v3;
    }
    if (t == 0 && sigma2) sigma2[b] = vplusvt - tot(3 * d);
}

int launch_dvh_reduce_many(const double *Zs, int64_t npad, int d, const double *y, int64_t nb, double vplusvt, double *dvh, double *sigma2,
                           hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    if (npad % 2 || d < 1 || d > GPX_MAX_D) { gpx_set_error("dvh_reduce_many: bad block shape"); return GPX_ERR_BAD_ARG; }
    ProfScope ps(prof, s, GPX_K_REDUCE, 8.0 * (double)nb * (double)(2 * d + 1) * (double)npad);
    if (d <= 8)
        hipLaunchKernelGGL(dvh_reduce_many_kernel<8>, dim3((unsigned)nb), dim3(256), 0, s, Zs, (long)npad, d, y, vplusvt, dvh, sigma2);
    else
        hipLaunchKernelGGL(dvh_reduce_many_kernel<0>, dim3((unsigned)nb), dim3(256), 0, s, Zs, (long)npad, d, y, vplusvt, dvh, sigma2);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// KV[c][i] = sum_j Kinv[i][j] V[c][j] for c < nc: the ONE pass over Kinv that feeds every quadratic form of
// the Approx propagation (loops K2..K6 of the reference, UncertaintyPropagation2.pyx:221-257,340-380, each of
// which re-reads the whole N x N matrix serially).  HBM-bound: 8 N^2 bytes.
// Workgroup = R rows x all columns; thread = column j (512-byte coalesced Kinv reads per wave and row); the thread's
// nc values V[.][j] sit in registers and are reused for the R rows; per-thread partial sums acc[R][NC] are
// reduced across the wave with shuffles and across the 4 waves through LDS (fixed order: deterministic).
// ---------------------------------------------------------------------------------------------
template <int NC, int R>
__global__ __launch_bounds__(256) void kinv_pass_kernel(const double *__restrict__ Kinv, long ld, long npad, int nc,
                                                       const double *__restrict__ V, double *__restrict__ KV)
{
    __shared__ double red[4][R * NC];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long i0 = (long)blockIdx.x * R;
    double acc[R][NC];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[r][c] = 0.0;
    // thread = two adjacent columns: 16-byte loads, 1 KiB per wave-instruction and row (npad is a multiple of 128)
    for (long j = 2 * t; j < npad; j += 512) {
        v2d k[R];
#pragma unroll
        for (int r = 0; r < R; ++r) k[r] = *reinterpret_cast<const v2d *>(Kinv + (i0 + r) * ld + j);
        v2d v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = (c < nc) ? *reinterpret_cast<const v2d *>(V + (long)c * npad + j) : (v2d){0.0, 0.0};
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[r][c] = fma(k[r].y, v[c].y, fma(k[r].x, v[c].x, acc[r][c]));
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const double s = wave_sum(acc[r][c]);
            if (lane == 0) red[wave][r * NC + c] = s;
        }
    __syncthreads();
    for (int e = t; e < R * NC; e += 256) {
        const int r = e / NC, c = e - r * NC;
        if (c < nc) KV[(long)c * npad + i0 + r] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    }
}

// nrows (> 0): only the first nrows rows of the Kinv pointer passed (a row panel; KV offset accordingly by the caller)
int launch_kinv_pass(const double *Kinv, int64_t ld, int64_t npad, int nc, const double *V, double *KV, hipStream_t s,
                     Profiler *prof, int64_t nrows)
{
    const int64_t nr = nrows > 0 ? nrows : npad;   // a multiple of 8
    ProfScope ps(prof, s, GPX_K_QUAD, 8.0 * (double)nr * (double)npad);
    if (nc <= 9)
        hipLaunchKernelGGL((kinv_pass_kernel<9, 8>), dim3((unsigned)(nr / 8)), dim3(256), 0, s, Kinv, (long)ld, (long)npad, nc, V, KV);
    else if (nc <= 17)
        hipLaunchKernelGGL((kinv_pass_kernel<17, 4>), dim3((unsigned)(nr / 4)), dim3(256), 0, s, Kinv, (long)ld, (long)npad, nc, V, KV);
    else if (nc <= 33)
        hipLaunchKernelGGL((kinv_pass_kernel<33, 2>), dim3((unsigned)(nr / 2)), dim3(256), 0, s, Kinv, (long)ld, (long)npad, nc, V, KV);
    else
        hipLaunchKernelGGL((kinv_pass_kernel<65, 1>), dim3((unsigned)nr), dim3(256), 0, s, Kinv, (long)ld, (long)npad, nc, V, KV);
    GPX_HIP(hipGetLastError());
    return 0;
}

// full C / J / H arrays for the host-side attributes C_ux, J_ux, H_ux
__global__ __launch_bounds__(256) void cjh_kernel(const double *__restrict__ x, long n, int d,
                                                 const double *__restrict__ u, const double *__restrict__ w, double v,
                                                 double vt, double *C, double *J, double *H)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double q = 0.0;
    bool same = true;
    for (int k = 0; k < d; ++k) {
        const double xv = x[i * d + k], uv = u[k];
        const double dl = xv - uv;
        same = same && (xv == uv);
        q = fma(w[k] * dl, dl, q);
    }
    const double c = v * exp(-0.5 * q);
    if (C) C[i] = same ? c + vt : c;
    if (J)
        for (int k = 0; k < d; ++k) J[i * d + k] = -(x[i * d + k] - u[k]) * w[k] * c;
    if (H)
        for (int a = 0; a < d; ++a) {
            const double wa = w[a] * (x[i * d + a] - u[a]);
            for (int b = 0; b < d; ++b) {
                const double wb = w[b] * (x[i * d + b] - u[b]);
                H[(i * d + a) * d + b] = (wa * wb - (a == b ? w[a] : 0.0)) * c;
            }
        }
}

// ---------------------------------------------------------------------------------------------
// Exact: per-row quantities.  a_i = u - x_i.
//   aT[k][i] = a_ik                       (k-major so the pair kernel loads it coalesced)
//   bT[k][i] = 1/4 (Ls a_i)_k             Ls = symmetric part of Lambda^-1 (UP.py:292-303)
//   e_i  = -1/2 a_i^T W^-1 a_i + 1/8 a_i^T Ls a_i          (log of C_i exp(1/8 ...), without v and quirk)
//   F_i  = v f_i,  f_i = (v+vt)/v when x_i == u else 1      (the +vt quirk folded into a factor)
//   lm_i = C_i nc1 exp(1/2 a_i^T Delta^-1 a_i), Delta^-1 = diag(w_k - w_k/(1+w_k s_k))   (UP.py:247-290)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void exact_build_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                         const double *__restrict__ u, const double *__restrict__ w,
                                                         const double *__restrict__ Ls, const double *__restrict__ dinv_diag,
                                                         double v, double vt, double nc1, double *__restrict__ aT,
                                                         double *__restrict__ bT, double *__restrict__ e,
                                                         double *__restrict__ F, double *__restrict__ lm)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    if (i >= n) {
        for (int k = 0; k < d; ++k) { aT[(long)k * npad + i] = 0.0; bT[(long)k * npad + i] = 0.0; }
        e[i] = 0.0; F[i] = 0.0; lm[i] = 0.0;     // F = 0 removes padded rows/columns from every sum
        return;
    }
    double qw = 0.0, qd = 0.0, ql = 0.0;
    bool same = true;
    for (int k = 0; k < d; ++k) {
        const double xv = x[i * d + k], uv = u[k];
        same = same && (xv == uv);
        const double ak = uv - xv;
        aT[(long)k * npad + i] = ak;
        qw = fma(w[k] * ak, ak, qw);
        qd = fma(dinv_diag[k] * ak, ak, qd);
    }
    for (int k = 0; k < d; ++k) {
        double row = 0.0;
        for (int b = 0; b < d; ++b) row = fma(Ls[k * d + b], u[b] - x[i * d + b], row);
        bT[(long)k * npad + i] = 0.25 * row;
        ql = fma(u[k] - x[i * d + k], row, ql);
    }
    e[i] = -0.5 * qw + 0.125 * ql;
    const double c = v * exp(-0.5 * qw);
    const double Ci = same ? c + vt : c;
    F[i] = same ? (v + vt) : v;
    lm[i] = Ci * nc1 * exp(0.5 * qd);
}

// exp(x) for the pair kernel: on the built-in path x = e_i + e_j + b_i.a_j is <= ~0 by construction (it is the log of
// L_ij / (F_i F_j nc2), a product of Gaussian factors); on the explicit path (exact_build_generic_kernel) the kernel's own factor
// stays in F and x = z^T Ls z / 2 >= 0.  exp_nonpos (common.h) serves both: it is as accurate for positive arguments.
// S = sum_ij (Kinv_ij - beta_i beta_j) F_i F_j exp(e_i + e_j + b_i . a_j); the caller multiplies by nc2.
// Kinv and L_ij are symmetric: only the pairs j <= i are visited (weight 2 off the diagonal), halving both the
// HBM bytes (4 N^2) and the exp count of the reference's full double loop (UncertaintyPropagation2.pyx:173-179).
// Workgroup = EXR rows; thread = column j (stride 256, coalesced Kinv reads); heavy (bottom) row blocks first.
constexpr int EXR = 8;   // rows per workgroup: 8 keeps the kernel at <=128 VGPRs (2+ waves/SIMD hide the HBM latency)
template <int DMAX>
__global__ __launch_bounds__(256, 2) void exact_sum_kernel(const double *__restrict__ Kinv, long ld, long npad, int d,
                                                       const double *__restrict__ beta, const double *__restrict__ aT,
                                                       const double *__restrict__ bT, const double *__restrict__ e,
                                                       const double *__restrict__ F, double *__restrict__ partial, int rb_base)
{
    __shared__ __attribute__((aligned(16))) double bs[EXR][DMAX];   // b_i for the block's 16 rows (broadcast reads), zero padded
    __shared__ double rs[EXR][3];                                   // e_i, F_i, beta_i
    __shared__ double ws[4];
    const int t = threadIdx.x;
    const int rb = rb_base + gridDim.x - 1 - blockIdx.x;           // the launch covers row blocks [rb_base, rb_base + gridDim.x)
    const long i0 = (long)rb * EXR;
    for (int q = t; q < EXR * DMAX; q += 256) {
        const int r = q / DMAX, k = q - r * DMAX;
        bs[r][k] = (k < d) ? bT[(long)k * npad + i0 + r] : 0.0;
    }
    if (t < EXR) { rs[t][0] = e[i0 + t]; rs[t][1] = F[i0 + t]; rs[t][2] = beta[i0 + t]; }
    __syncthreads();

    double acc[EXR];
#pragma unroll
    for (int r = 0; r < EXR; ++r) acc[r] = 0.0;

    for (long j = t; j < i0 + EXR; j += 256) {
        double aj[DMAX];
#pragma unroll
        for (int k = 0; k < DMAX; ++k) aj[k] = (k < d) ? aT[(long)k * npad + j] : 0.0;
        const double ej = e[j], Fj = F[j], bj = beta[j];
#pragma unroll
        for (int r = 0; r < EXR; ++r) {
            double dot = rs[r][0] + ej;
#pragma unroll
            for (int k = 0; k < DMAX; k += 2) {
                const v2d b2 = *reinterpret_cast<const v2d *>(&bs[r][k]);
                dot = fma(b2.x, aj[k], dot);
                dot = fma(b2.y, aj[k + 1], dot);
            }
            const double kij = Kinv[(i0 + r) * ld + j];
            const long i = i0 + r;
            const double wgt = (j < i) ? 2.0 : ((j == i) ? 1.0 : 0.0);
            acc[r] = fma((kij - rs[r][2] * bj) * (Fj * wgt), exp_nonpos(dot), acc[r]);
        }
    }
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < EXR; ++r) s = fma(acc[r], rs[r][1], s);
    s = wave_sum(s);
    if ((t & 63) == 0) ws[t >> 6] = s;
    __syncthreads();
    if (t == 0) partial[rb - rb_base] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// ---------------------------------------------------------------------------------------------
// Gradient of the negative log likelihood ("next" row f1: Covariance._d_nll_d_theta, skgpuppy/Covariance.py:266-282
// with GaussianCovariance._d_cov_matrix_d_theta_ij, :605-657).  The reference forms 2+d derivative matrices dK/dtheta_j
// (N x N each) and evaluates 1/2 tr(Kinv dK) - 1/2 a^T dK a per parameter; here ONE pass over the j <= i half of Kinv
// recomputes the noise-free Gram entry Kf_ij on the fly and accumulates, with M_ij = Kinv_ij - a_i a_j,
//   S_0 = sum M_ij Kf_ij,   S_{1+k} = sum M_ij Kf_ij (x_ik - x_jk)^2,   T = tr(Kinv) - a^T a
// so that  dNLL/dtheta_0 = S_0/2,  dNLL/dtheta_1 = vt T/2,  dNLL/dtheta_{2+k} = -w_k S_{1+k}/4.
// partial[block][DMAX+2]: [0] = S_0, [1..d] = S_k, [DMAX+1] = T.
// ---------------------------------------------------------------------------------------------
template <int DMAX>
__global__ __launch_bounds__(256, 2) void nll_grad_kernel(const double *__restrict__ Kinv, long ld, long n, long npad, int d,
                                                         const double *__restrict__ alpha, const double *__restrict__ xw,
                                                         double v, double *__restrict__ partial)
{
    constexpr int R = 8;
    __shared__ double xs[R][DMAX];     // sqrt(w)-scaled rows of the block (broadcast reads)
    __shared__ double as[R];
    __shared__ double red[4][DMAX + 2];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int rb = gridDim.x - 1 - blockIdx.x;
    const long i0 = (long)rb * R;
    for (int q = t; q < R * DMAX; q += 256) {
        const int r = q / DMAX, k = q - r * DMAX;
        xs[r][k] = (k < d && i0 + r < n) ? xw[(i0 + r) * d + k] : 0.0;
    }
    if (t < R) as[t] = alpha[i0 + t];
    __syncthreads();
    double acc[DMAX + 2];
#pragma unroll
    for (int c = 0; c < DMAX + 2; ++c) acc[c] = 0.0;
    for (long j = t; j < i0 + R && j < n; j += 256) {
        double xj[DMAX];
#pragma unroll
        for (int k = 0; k < DMAX; ++k) xj[k] = (k < d) ? xw[j * d + k] : 0.0;
        const double aj = alpha[j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long i = i0 + r;
            if (i >= n || j > i) continue;
            double q = 0.0, dk[DMAX];
#pragma unroll
            for (int k = 0; k < DMAX; ++k) {
                const double df = xs[r][k] - xj[k];
                dk[k] = df * df;               // = w_k (x_ik - x_jk)^2  (inputs are sqrt(w)-scaled)
                q += dk[k];
            }
            const double kij = Kinv[i * ld + j];
            const double wgt = (j < i) ? 2.0 : 1.0;
            const double m = (kij - as[r] * aj) * wgt * v * exp_nonpos(-0.5 * q);
            acc[0] += m;
#pragma unroll
            for (int k = 0; k < DMAX; ++k) acc[1 + k] = fma(m, dk[k], acc[1 + k]);
            if (j == i) acc[DMAX + 1] += kij - as[r] * aj;
        }
    }
#pragma unroll
    for (int c = 0; c < DMAX + 2; ++c) {
        const double s = wave_sum(acc[c]);
        if (lane == 0) red[wave][c] = s;
    }
    __syncthreads();
    if (t < DMAX + 2) partial[(long)rb * (DMAX + 2) + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// out[c] = sum_b partial[b][c]   (fixed order)
__global__ __launch_bounds__(256) void sum_columns_kernel(const double *__restrict__ partial, long nb, int nc, double *out)
{
    __shared__ double ws[4];
    const int c = blockIdx.x;
    double s = 0.0;
    for (long b = threadIdx.x; b < nb; b += 256) s += partial[b * nc + c];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[c] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

int launch_sum_columns(const double *partial, int64_t nb, int nc, double *out_dev, hipStream_t s)
{
    hipLaunchKernelGGL(sum_columns_kernel, dim3((unsigned)nc), dim3(256), 0, s, partial, (long)nb, nc, out_dev);
    GPX_HIP(hipGetLastError());
    return 0;
}

// out_dev[0..dmax+1] (layout above); returns the DMAX used so the caller can index T
int launch_nll_grad(const double *Kinv, int64_t ld, int64_t n, int64_t npad, int d, const double *alpha, const double *xw,
                    double v, double *partial, double *out_dev, int *dmax_used, hipStream_t s, Profiler *prof)
{
    const unsigned nblk = (unsigned)(npad / 8);
    int dm;
    {
        ProfScope ps(prof, s, GPX_K_QUAD, 4.0 * (double)npad * (double)npad);
#define GPX_NG(DM)                                                                                                     \
    dm = DM;                                                                                                           \
    hipLaunchKernelGGL(nll_grad_kernel<DM>, dim3(nblk), dim3(256), 0, s, Kinv, (long)ld, (long)n, (long)npad, d, alpha, xw, v, partial)
        if (d <= 2) { GPX_NG(2); }
        else if (d <= 4) { GPX_NG(4); }
        else if (d <= 8) { GPX_NG(8); }
        else if (d <= 16) { GPX_NG(16); }
        else if (d <= 32) { GPX_NG(32); }
        else { GPX_NG(64); }
#undef GPX_NG
    }
    hipLaunchKernelGGL(sum_columns_kernel, dim3((unsigned)(dm + 2)), dim3(256), 0, s, (const double *)partial, (long)nblk, dm + 2, out_dev);
    GPX_HIP(hipGetLastError());
    *dmax_used = dm;
    return 0;
}

__global__ __launch_bounds__(256) void sum_vector_kernel(const double *__restrict__ p, long n, double *out)
{
    __shared__ double ws[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) s += p[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// rows [row0, row1) of the j <= i half (multiples of EXR; row1 <= 0: all rows)
int launch_exact_sum(const double *Kinv, int64_t ld, int64_t npad, int d, const double *beta, const double *aT,
                     const double *bT, const double *e, const double *F, double *partial, double *out_dev,
                     hipStream_t s, Profiler *prof, int64_t row0, int64_t row1)
{
    if (row1 <= 0) { row0 = 0; row1 = npad; }
    const int rb0 = (int)(row0 / EXR);
    const unsigned nblk = (unsigned)((row1 - row0) / EXR);
    if (nblk == 0) {
        GPX_HIP(hipMemsetAsync(out_dev, 0, sizeof(double), s));
        return 0;
    }
    {
        // algorithmic flops: N^2 (2d + ~25) + N^2 exp, j <= i pairs only
        ProfScope ps(prof, s, GPX_K_EXACT, 0.5 * ((double)row1 * (double)row1 - (double)row0 * (double)row0) * (2.0 * d + 25.0));
#define GPX_EXACT(DM) hipLaunchKernelGGL(exact_sum_kernel<DM>, dim3(nblk), dim3(256), 0, s, Kinv, (long)ld, (long)npad, d, beta, aT, bT, e, F, partial, rb0)
        if (d <= 2) GPX_EXACT(2);
        else if (d <= 4) GPX_EXACT(4);
        else if (d <= 8) GPX_EXACT(8);
        else if (d <= 16) GPX_EXACT(16);
        else if (d <= 32) GPX_EXACT(32);
        else GPX_EXACT(64);
#undef GPX_EXACT
    }
    hipLaunchKernelGGL(sum_vector_kernel, dim3(1), dim3(256), 0, s, (const double *)partial, (long)nblk, out_dev);
    GPX_HIP(hipGetLastError());
    return 0;
}

int launch_approx_build(const double *x, int64_t n, int64_t npad, int d, const double *u_dev, const double *w_dev,
                        double v, double vt, double *VM, double *AUX, double *cplain, hipStream_t s)
{
    hipLaunchKernelGGL(approx_build_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, x, (long)n, (long)npad,
                       d, u_dev, w_dev, v, vt, VM, AUX, cplain);
    GPX_HIP(hipGetLastError());
    return 0;
}

int launch_trace(const double *x, int64_t n, int64_t npad, int d, const double *u_dev, const double *w_dev,
                 const double *Sigma_dev, const double *cplain, double *tr, hipStream_t s)
{
    hipLaunchKernelGGL(trace_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, x, (long)n, (long)npad, d,
                       u_dev, w_dev, Sigma_dev, cplain, tr);
    GPX_HIP(hipGetLastError());
    return 0;
}

int launch_cjh(const double *x, int64_t n, int d, const double *u_dev, const double *w_dev, double v, double vt,
               double *C, double *J, double *H, hipStream_t s)
{
    hipLaunchKernelGGL(cjh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, (long)n, d, u_dev, w_dev, v, vt,
                       C, J, H);
    GPX_HIP(hipGetLastError());
    return 0;
}

// The same per-row quantities for ANY operator (gpx_propagate_exact_matrix): C_i = cov(u, x_i) comes from the caller -- the operator's own
// scalar kernel, as in the reference (UncertaintyPropagation.py:269-276, :339-343) --, so nothing of the built-in kernel is folded
// into the exponent: F_i = C_i, e_i = a_i^T Lambda^-1 a_i / 8, l_i = C_i nc1 exp(a_i^T Delta^-1 a_i / 2)   (:257-266, :292-321)
__global__ __launch_bounds__(256) void exact_build_generic_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                                 const double *__restrict__ u, const double *__restrict__ Ls,
                                                                 const double *__restrict__ dinv_diag, const double *__restrict__ C, double nc1,
                                                                 double *__restrict__ aT, double *__restrict__ bT, double *__restrict__ e,
                                                                 double *__restrict__ F, double *__restrict__ lm)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    if (i >= n) {
        for (int k = 0; k < d; ++k) { aT[(long)k * npad + i] = 0.0; bT[(long)k * npad + i] = 0.0; }
        e[i] = 0.0; F[i] = 0.0; lm[i] = 0.0;
        return;
    }
    double qd = 0.0, ql = 0.0;
    for (int k = 0; k < d; ++k) {
        const double ak = u[k] - x[i * d + k];
        aT[(long)k * npad + i] = ak;
        qd = fma(dinv_diag[k] * ak, ak, qd);
    }
    for (int k = 0; k < d; ++k) {
        double row = 0.0;
        for (int b = 0; b < d; ++b) row = fma(Ls[k * d + b], u[b] - x[i * d + b], row);
        bT[(long)k * npad + i] = 0.25 * row;
        ql = fma(u[k] - x[i * d + k], row, ql);
    }
    e[i] = 0.125 * ql;
    F[i] = C[i];
    lm[i] = C[i] * nc1 * exp(0.5 * qd);
}

int launch_exact_build_generic(const double *x, int64_t n, int64_t npad, int d, const double *u_dev, const double *Ls_dev,
                               const double *dinv_diag_dev, const double *C_dev, double nc1, double *aT, double *bT, double *e, double *F,
                               double *lm, hipStream_t s)
{
    hipLaunchKernelGGL(exact_build_generic_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, x, (long)n, (long)npad, d, u_dev,
                       Ls_dev, dinv_diag_dev, C_dev, nc1, aT, bT, e, F, lm);
    GPX_HIP(hipGetLastError());
    return 0;
}

int launch_exact_build(const double *x, int64_t n, int64_t npad, int d, const double *u_dev, const double *w_dev,
                       const double *Ls_dev, const double *dinv_diag_dev, double v, double vt, double nc1, double *aT,
                       double *bT, double *e, double *F, double *lm, hipStream_t s)
{
    hipLaunchKernelGGL(exact_build_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s, x, (long)n, (long)npad,
                       d, u_dev, w_dev, Ls_dev, dinv_diag_dev, v, vt, nc1, aT, bT, e, F, lm);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Batched Exact (gpx_propagate_exact_many): for every input u that shares one Sigma the pair weight factorises,
//   L_ij / nc2 = h_i(u) h_j(u) E_ij,   h_i(u) = F_i exp(-1/4 a_i^T A^-1 a_i),   E_ij = exp(-1/8 (x_i - x_j)^T Ls (x_i - x_j)),
// (a_i = u - x_i, A = Sigma + W^-1 / 2; a_i - a_j does not hold u and -W / 2 + Ls / 4 = -A^-1 / 4), so the double sum of
// exact_sum_kernel is the quadratic form h^T M h with M = (Kinv - beta beta^T) o E built ONCE per Sigma.  Both quadratic forms run on
// coordinates transformed by the eigenvectors of their matrix (sym_eig.h): a signed sum of d squared DIFFERENCES per pair.
// ---------------------------------------------------------------------------------------------
// out[i][k] = sum_m T[k][m] (x[i][m] - x0[m]) for i < n, zero rows from n to npad
__global__ __launch_bounds__(256) void exact_many_transform_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                                  const double *__restrict__ x0, const double *__restrict__ T,
                                                                  double *__restrict__ out)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npad * d) return;
    const long i = e / d;
    const int k = (int)(e - i * d);
    double s = 0.0;
    if (i < n)
        for (int m = 0; m < d; ++m) s = fma(T[k * d + m], x[i * d + m] - x0[m], s);
    out[e] = s;
}

int launch_exact_many_transform(const double *x, int64_t n, int64_t npad, int d, const double *x0_dev, const double *T_dev, double *out,
                                hipStream_t s)
{
    if (npad <= 0) return 0;
    hipLaunchKernelGGL(exact_many_transform_kernel, dim3((unsigned)((npad * d + 255) / 256)), dim3(256), 0, s, x, (long)n, (long)npad, d,
                       x0_dev, T_dev, out);
    GPX_HIP(hipGetLastError());
    return 0;
}

// Lo (ld = npad) from the j <= i half of Kinv, one 64 x 64 tile per workgroup:
//   Lo_ij = (Kinv_ij - beta_i beta_j) exp(-sum_k s_k (xt_ik - xt_jk)^2) for j < i, half of it for j == i, 0 for j > i and for i, j >= n.
// The workgroups past the triangle clear the one 64 x 64 tile above the diagonal inside every 128 x 128 tile that the diagonal crosses
// (the read contract of a triangular GEMM operand, gpx.h); tiles wholly above the diagonal are neither written nor read.
// LDS: the tile's rows [64][d] (broadcast reads) and columns [d][64] (k-major, lane = column): 64 KB at d = 64, two workgroups per CU.
// Thread = column j (512-byte loads and stores per wave and row), wave w = rows w, w + 4, ..
constexpr int EW_T = 64;
__global__ __launch_bounds__(256, 2) void exact_weight_kernel(const double *__restrict__ Kinv, long ld, long n, long npad, int d,
                                                             const double *__restrict__ beta, const double *__restrict__ xt,
                                                             const double *__restrict__ sgn, double *__restrict__ Lo)
{
    extern __shared__ __attribute__((aligned(16))) double ew_smem[];
    double *xi_s = ew_smem;                // [64][d]
    double *xj_s = ew_smem + EW_T * d;     // [d][64]
    const int t = threadIdx.x, c = t & 63, w = t >> 6;
    const long nt = npad / EW_T, ntri = nt * (nt + 1) / 2;
    const long idx = blockIdx.x;
    if (idx >= ntri) {
        const long ti = 2 * (idx - ntri);          // even tile row: the tile to its right lies in the same 128 x 128 diagonal tile
        if (ti + 1 >= nt) return;
        const long i0 = ti * EW_T, j0 = (ti + 1) * EW_T;
        for (int r = w; r < EW_T; r += 4) Lo[(i0 + r) * ld + j0 + c] = 0.0;
        return;
    }
    long ti = (long)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > idx) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= idx) ++ti;
    const long tj = idx - ti * (ti + 1) / 2;
    const long i0 = ti * EW_T, j0 = tj * EW_T;
    for (int e = t; e < EW_T * d; e += 256) {
        xi_s[e] = xt[i0 * d + e];
        const int cc = e / d, k = e - cc * d;
        xj_s[k * EW_T + cc] = xt[j0 * d + e];
    }
    __syncthreads();
    double acc[EW_T / 4];
#pragma unroll
    for (int r = 0; r < EW_T / 4; ++r) acc[r] = 0.0;
    for (int k = 0; k < d; ++k) {
        const double xj = xj_s[k * EW_T + c], sk = sgn[k];
#pragma unroll
        for (int r = 0; r < EW_T / 4; ++r) {
            const double df = xi_s[(w + 4 * r) * d + k] - xj;
            acc[r] = fma(sk * df, df, acc[r]);
        }
    }
    const long j = j0 + c;
    const double bj = beta[j];
#pragma unroll
    for (int r = 0; r < EW_T / 4; ++r) {
        const long i = i0 + w + 4 * r;
        const double val = (Kinv[i * ld + j] - beta[i] * bj) * exp_nonpos(-acc[r]);
        Lo[i * ld + j] = (i >= n || j > i) ? 0.0 : (j == i ? 0.5 * val : val);
    }
}

int launch_exact_weight(const double *Kinv, int64_t ld, int64_t n, int64_t npad, int d, const double *beta, const double *xt,
                        const double *sgn_dev, double *Lo, hipStream_t s, Profiler *prof)
{
    if (npad % TILE || ld < npad) { gpx_set_error("exact_weight: bad shape"); return GPX_ERR_BAD_ARG; }
    const int64_t nt = npad / EW_T;
    ProfScope ps(prof, s, GPX_K_EXACT, 0.5 * (double)npad * (double)npad * (2.0 * d + 25.0));
    hipLaunchKernelGGL(exact_weight_kernel, dim3((unsigned)(nt * (nt + 1) / 2 + nt / 2)), dim3(256), sizeof(double) * 2 * EW_T * d, s, Kinv,
                       (long)ld, (long)n, (long)npad, d, beta, xt, sgn_dev, Lo);
    GPX_HIP(hipGetLastError());
    return 0;
}

// A slab of inputs: H [rows, npad] with H_ij = F_ij exp(-sum_k s_k (uh_ik - xh_jk)^2) (= F exp(-1/4 a^T A^-1 a), a = u_i - x_j, ONE signed
// sum of squares; F = v + vt iff x_j == u_i elementwise, else v; zero for j >= n), and in the same pass the mean's terms
// beta_j lm_ij, lm as exact_build_kernel defines it, summed over the workgroup's 64 columns into mpart[i][column tile] (wave shuffle,
// fixed order; exact_many_finish_kernel adds the tiles).  A workgroup owns 64 columns and EM_INPUTS inputs, four per wave; the raw
// and the transformed inputs of its columns sit in LDS k-major (64 KB at d = 64); u, uh, w, dd, sgn are wave-uniform loads.
// WANT_H = false: the means alone, nothing of xh / Uh / sgn / H is touched.
constexpr int EM_COLS = 64;
constexpr int EM_INPUTS = 16;
template <bool WANT_H>
__global__ __launch_bounds__(256) void exact_many_build_kernel(const double *__restrict__ x, const double *__restrict__ xh, long n, long npad,
                                                              int d, const double *__restrict__ U, const double *__restrict__ Uh, long nb,
                                                              const double *__restrict__ w, const double *__restrict__ dinv_diag,
                                                              const double *__restrict__ sgn, const double *__restrict__ beta, double v,
                                                              double vt, double nc1, double *__restrict__ H, double *__restrict__ mpart,
                                                              long npart)
{
    extern __shared__ __attribute__((aligned(16))) double em_smem[];
    double *x_s = em_smem;                  // [d][64] raw inputs of the tile's columns
    double *xh_s = em_smem + EM_COLS * d;   // [d][64] transformed ones (WANT_H)
    const int t = threadIdx.x;
    const long col0 = (long)blockIdx.x * EM_COLS;
    for (int e = t; e < EM_COLS * d; e += 256) {
        const int cc = e / d, k = e - cc * d;
        const long gc = col0 + cc;
        x_s[k * EM_COLS + cc] = (gc < n) ? x[gc * d + k] : 0.0;
        if constexpr (WANT_H) xh_s[k * EM_COLS + cc] = xh[gc * d + k];
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const long j = col0 + lane;
    const bool inb = j < n;
    const double bj = beta[j];
    for (int q = 0; q < EM_INPUTS / 4; ++q) {
        const long i = (long)blockIdx.y * EM_INPUTS + 4 * q + wave;   // wave-uniform
        if (i >= nb) break;
        const double *u = U + i * d;
        double qw = 0.0, qd = 0.0, qa = 0.0;
        bool same = true;
        for (int k = 0; k < d; ++k) {
            const double xv = x_s[k * EM_COLS + lane], uk = u[k];
            same = same && (xv == uk);
            const double ak = uk - xv;
            qw = fma(w[k] * ak, ak, qw);
            qd = fma(dinv_diag[k] * ak, ak, qd);
            if constexpr (WANT_H) {
                const double df = Uh[i * d + k] - xh_s[k * EM_COLS + lane];
                qa = fma(sgn[k] * df, df, qa);
            }
        }
        const double c = v * exp(-0.5 * qw);
        const double Ci = same ? c + vt : c;
        const double lm = inb ? Ci * nc1 * exp(0.5 * qd) : 0.0;
        if constexpr (WANT_H) H[i * npad + j] = inb ? (same ? (v + vt) : v) * exp_nonpos(-qa) : 0.0;
        const double m = wave_sum(bj * lm);
        if (lane == 0) mpart[i * npart + blockIdx.x] = m;
    }
}

// H [rows_pad, npad]: rows [0, nb) written by the kernel (every column), the rest of the last 128-row tile cleared; mpart [nb, npad / 64]
int launch_exact_many_build(const double *x, const double *xh, int64_t n, int64_t npad, int d, const double *U_dev, const double *Uh_dev,
                            int64_t nb, int64_t rows_pad, const double *w_dev, const double *dinv_diag_dev, const double *sgn_dev,
                            const double *beta, double v, double vt, double nc1, double *H, double *mpart, hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    const bool want_h = H != nullptr;
    const int64_t ygrid = (nb + EM_INPUTS - 1) / EM_INPUTS;
    if (npad % EM_COLS || (want_h && nb > rows_pad) || ygrid > 65535) { gpx_set_error("exact_many_build: bad block shape"); return GPX_ERR_BAD_ARG; }
    // algorithmic flops per (input, column): 7 d for the three sums (4 d without H) and three exponentials at ~20
    ProfScope ps(prof, s, GPX_K_EXACT, (double)nb * (double)npad * ((want_h ? 7.0 : 4.0) * d + (want_h ? 65.0 : 45.0)));
    if (want_h && rows_pad > nb) GPX_HIP(hipMemsetAsync(H + nb * npad, 0, sizeof(double) * (rows_pad - nb) * npad, s));
    const dim3 grid((unsigned)(npad / EM_COLS), (unsigned)ygrid);
    const long npart = (long)(npad / EM_COLS);
    if (want_h)
        hipLaunchKernelGGL(exact_many_build_kernel<true>, grid, dim3(256), sizeof(double) * 2 * EM_COLS * d, s, x, xh, (long)n, (long)npad, d, U_dev,
                           Uh_dev, (long)nb, w_dev, dinv_diag_dev, sgn_dev, beta, v, vt, nc1, H, mpart, npart);
    else
        hipLaunchKernelGGL(exact_many_build_kernel<false>, grid, dim3(256), sizeof(double) * EM_COLS * d, s, x, xh, (long)n, (long)npad, d, U_dev,
                           Uh_dev, (long)nb, w_dev, dinv_diag_dev, sgn_dev, beta, v, vt, nc1, H, mpart, npart);
    GPX_HIP(hipGetLastError());
    return 0;
}

// One workgroup per input, fixed order: mean_i = sum of its column-tile partials, S_i = 2 sum_j Y_ij H_ij (Y = H Lo^T: the diagonal of
// Lo carries half its weight, so twice the lower sum is the full quadratic form), var_i = (v + vt) - nc2 S_i - mean_i^2
// (UncertaintyPropagation.py:377).  out: [2][ldo] = mean | var; Y == nullptr: the means alone.
__global__ __launch_bounds__(256) void exact_many_finish_kernel(const double *__restrict__ Y, const double *__restrict__ H, long npad,
                                                               const double *__restrict__ mpart, long npart, double vplusvt, double nc2,
                                                               double *__restrict__ out, long ldo)
{
    __shared__ double ws[2][4];
    const long i = blockIdx.x;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double m = 0.0, s0 = 0.0, s1 = 0.0;
    for (long p = t; p < npart; p += 256) m += mpart[i * npart + p];
    if (Y) {
        const double *y = Y + i * npad, *hh = H + i * npad;
        for (long c = 2 * t; c < npad; c += 512) {
            const v2d a = *reinterpret_cast<const v2d *>(y + c), b = *reinterpret_cast<const v2d *>(hh + c);
            s0 = fma(a.x, b.x, s0);
            s1 = fma(a.y, b.y, s1);
        }
    }
    m = wave_sum(m);
    const double sv = wave_sum(s0 + s1);
    if (lane == 0) { ws[0][wave] = m; ws[1][wave] = sv; }
    __syncthreads();
    if (t == 0) {
        const double mean = (ws[0][0] + ws[0][1]) + (ws[0][2] + ws[0][3]);
        out[i] = mean;
        if (Y) {
            const double S = 2.0 * ((ws[1][0] + ws[1][1]) + (ws[1][2] + ws[1][3]));
            out[ldo + i] = vplusvt - nc2 * S - mean * mean;
        }
    }
}

int launch_exact_many_finish(const double *Y, const double *H, int64_t npad, const double *mpart, int64_t nb, double vplusvt, double nc2,
                             double *out, int64_t ldo, hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    ProfScope ps(prof, s, GPX_K_EXACT, (Y ? 2.0 : 0.0) * (double)nb * (double)npad + (double)nb * (double)(npad / EM_COLS));
    hipLaunchKernelGGL(exact_many_finish_kernel, dim3((unsigned)nb), dim3(256), 0, s, Y, H, (long)npad, mpart, (long)(npad / EM_COLS), vplusvt,
                       nc2, out, (long)ldo);
    GPX_HIP(hipGetLastError());
    return 0;
}
