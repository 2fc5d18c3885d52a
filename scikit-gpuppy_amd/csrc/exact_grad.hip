// exact_grad.hip -- the closed-form gradients of Girard's exact moments in u and in the diagonal of Sigma (gpx_propagate_exact_grad_many,
// propagate_api.hip).  On the factorisation of the batched Exact call (propagate.hip: L_ij / nc2 = h_i h_j E_ij, S = h^T M h,
// M = (Kinv - beta beta^T) o E, Lo = its lower half with the diagonal halved) and with b_j = A^-1 (u - x_j), A = Sigma + W^-1 / 2:
//   dh_j / du_k = -1/2 h_j b_jk,   dh_j / ds_k = 1/4 h_j b_jk^2,   dE_ij / ds_k = -1/8 E_ij (b_ik - b_jk)^2     (s_k = Sigma_kk)
// so with the rows  h,  p_k = h o b_.k,  c_k = h o b_.k^2  and  Y_r = Lo r  (x^T M y = x.Y_y + y.Y_x):
//   S = 2 h.Y_h,   G_k = p_k.Y_h + h.Y_pk = -dS/du_k,   Q_k = 1/2 (c_k.Y_h + h.Y_ck) + p_k.Y_pk = 2 dS/ds_k
//   dvar/du_k = nc2 G_k - 2 m dm/du_k,   dvar/ds_k = -nc2 (Q_k / 2 - w_k / (2 w_k s_k + 1) S) - 2 m dm/ds_k
// and for the mean m = sum_j beta_j l_j, l_j = F_j nc1 exp(-1/2 sum_k D_k a_jk^2), D_k = w_k / (1 + w_k s_k):
//   dm/du_k = -sum_j beta_j l_j D_k a_jk,   dm/ds_k = 1/2 sum_j beta_j l_j (D_k^2 a_jk^2 - D_k).
// Row layout: an input owns 2 d + 1 CONSECUTIVE rows of the slab -- 0: h, 1 + k: p_k, 1 + d + k: c_k -- so a single input is one padded
// product and a slab of inputs one launch of the triangular fp64 GEMM.
#include "common.h"

constexpr int EG_COLS = 64;
constexpr int EG_INPUTS = 16;

// A slab of inputs: the 2 d + 1 rows of each (WANT_H) and, per 64-column tile, the partials of the 2 d + 1 mean sums
//   mpart[(i (2 d + 1) + 0) npart + tile] = sum beta_j l_j,  [.. 1 + k ..] = dm/du_k,  [.. 1 + d + k ..] = dm/ds_k
// (wave shuffle, fixed order; the finish kernel adds the tiles).  The frame is exact_many_build_kernel's: a workgroup owns 64 columns and
// EG_INPUTS inputs, four per wave; the raw and the transformed inputs of its columns sit in LDS k-major (64 KB at d = 64: two workgroups
// per CU); u, uh and the run's constants are wave-uniform loads.  b_jk = sum_m Bm[k][m] (uh_m - xh_jm), Bm = 4 T^T diag(sgn) from the host
// (A^-1 / 4 = T^T diag(sgn) T): formed from the DIFFERENCES of the transformed coordinates, which are recomputed per k so that no lane
// holds d of them (no scratch at any d).
template <bool WANT_H>
__global__ __launch_bounds__(256, 2) void exact_grad_build_kernel(const double *__restrict__ x, const double *__restrict__ xh, long n, long npad,
                                                              int d, const double *__restrict__ U, const double *__restrict__ Uh, long nb,
                                                              const double *__restrict__ w, const double *__restrict__ dinv_diag,
                                                              const double *__restrict__ Dk, const double *__restrict__ sgn,
                                                              const double *__restrict__ Bm, const double *__restrict__ beta, double v,
                                                              double vt, double nc1, double *__restrict__ H, double *__restrict__ mpart,
                                                              long npart)
{
    extern __shared__ __attribute__((aligned(16))) double eg_smem[];
    double *x_s = eg_smem;                  // [d][64] raw inputs of the tile's columns
    double *xh_s = eg_smem + EG_COLS * d;   // [d][64] transformed ones (WANT_H)
    const int t = threadIdx.x;
    const long col0 = (long)blockIdx.x * EG_COLS;
    for (int e = t; e < EG_COLS * d; e += 256) {
        const int cc = e / d, k = e - cc * d;
        const long gc = col0 + cc;
        x_s[k * EG_COLS + cc] = (gc < n) ? x[gc * d + k] : 0.0;
        if constexpr (WANT_H) xh_s[k * EG_COLS + cc] = xh[gc * d + k];
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const long j = col0 + lane;
    const bool inb = j < n;
    const double bj = beta[j];
    const int nrow = 2 * d + 1;
    for (int q = 0; q < EG_INPUTS / 4; ++q) {
        const long i = (long)blockIdx.y * EG_INPUTS + 4 * q + wave;   // wave-uniform
        if (i >= nb) break;
        const double *u = U + i * d;
        double qw = 0.0, qd = 0.0, qa = 0.0;
        bool same = true;
        for (int k = 0; k < d; ++k) {          // the sums of exact_many_build_kernel, in its order: mean and h have that call's bits
            const double xv = x_s[k * EG_COLS + lane], uk = u[k];
            same = same && (xv == uk);
            const double ak = uk - xv;
            qw = fma(w[k] * ak, ak, qw);
            qd = fma(dinv_diag[k] * ak, ak, qd);
            if constexpr (WANT_H) {
                const double df = Uh[i * d + k] - xh_s[k * EG_COLS + lane];
                qa = fma(sgn[k] * df, df, qa);
            }
        }
        const double c = v * exp(-0.5 * qw);
        const double Ci = same ? c + vt : c;
        const double lm = inb ? Ci * nc1 * exp(0.5 * qd) : 0.0;
        const double bl = bj * lm;
        double *mp = mpart + (i * nrow) * npart + blockIdx.x;
        const double m = wave_sum(bl);
        if (lane == 0) mp[0] = m;
        double hv = 0.0;
        double *Hrow = nullptr;
        if constexpr (WANT_H) {
            hv = inb ? (same ? (v + vt) : v) * exp_nonpos(-qa) : 0.0;
            Hrow = H + (i * nrow) * npad + j;
            Hrow[0] = hv;
        }
        for (int k = 0; k < d; ++k) {
            const double ak = u[k] - x_s[k * EG_COLS + lane], Da = Dk[k] * ak;
            const double du = wave_sum(-bl * Da);
            const double ds = wave_sum(0.5 * bl * fma(Da, Da, -Dk[k]));
            if (lane == 0) {
                mp[(long)(1 + k) * npart] = du;
                mp[(long)(1 + d + k) * npart] = ds;
            }
            if constexpr (WANT_H) {
                double bk = 0.0;
                const double *Bk = Bm + k * d;
                for (int mm = 0; mm < d; ++mm) bk = fma(Bk[mm], Uh[i * d + mm] - xh_s[mm * EG_COLS + lane], bk);
                const double pk = hv * bk;
                Hrow[(long)(1 + k) * npad] = pk;
                Hrow[(long)(1 + d + k) * npad] = pk * bk;
            }
        }
    }
}

// H [rows_pad, npad]: rows [0, nb (2 d + 1)) written by the kernel (every column), the rest of the last 128-row tile cleared;
// mpart [nb (2 d + 1), npad / 64].  H == nullptr: the mean sums alone.
int launch_exact_grad_build(const double *x, const double *xh, int64_t n, int64_t npad, int d, const double *U_dev, const double *Uh_dev,
                            int64_t nb, int64_t rows_pad, const double *w_dev, const double *dinv_diag_dev, const double *Dk_dev,
                            const double *sgn_dev, const double *Bm_dev, const double *beta, double v, double vt, double nc1, double *H,
                            double *mpart, hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    const bool want_h = H != nullptr;
    const int64_t ygrid = (nb + EG_INPUTS - 1) / EG_INPUTS, rows = nb * (2 * d + 1);
    if (d < 1 || d > GPX_MAX_D || npad % EG_COLS || (want_h && rows > rows_pad) || ygrid > 65535) {
        gpx_set_error("exact_grad_build: bad block shape");
        return GPX_ERR_BAD_ARG;
    }
    // algorithmic flops per (input, column): the three sums and exponentials of the plain build, 12 per k for the mean sums, 3 d + 3 per k for b
    ProfScope ps(prof, s, GPX_K_EXACT, (double)nb * (double)npad * ((want_h ? 7.0 : 4.0) * d + (want_h ? 65.0 : 45.0) + 12.0 * d + (want_h ? (3.0 * d + 3.0) * d : 0.0)));
    if (want_h && rows_pad > rows) GPX_HIP(hipMemsetAsync(H + rows * npad, 0, sizeof(double) * (rows_pad - rows) * npad, s));
    const dim3 grid((unsigned)(npad / EG_COLS), (unsigned)ygrid);
    const long npart = (long)(npad / EG_COLS);
    if (want_h)
        hipLaunchKernelGGL(exact_grad_build_kernel<true>, grid, dim3(256), sizeof(double) * 2 * EG_COLS * d, s, x, xh, (long)n, (long)npad, d, U_dev,
                           Uh_dev, (long)nb, w_dev, dinv_diag_dev, Dk_dev, sgn_dev, Bm_dev, beta, v, vt, nc1, H, mpart, npart);
    else
        hipLaunchKernelGGL(exact_grad_build_kernel<false>, grid, dim3(256), sizeof(double) * EG_COLS * d, s, x, xh, (long)n, (long)npad, d, U_dev,
                           Uh_dev, (long)nb, w_dev, dinv_diag_dev, Dk_dev, sgn_dev, Bm_dev, beta, v, vt, nc1, H, mpart, npart);
    GPX_HIP(hipGetLastError());
    return 0;
}

// the sum of up to NV values per thread over the workgroup's 256 threads, in every thread: butterfly in the wave, then the four waves in
// the order (0 + 1) + (2 + 3).  ws is one of two alternating LDS blocks, so consecutive calls need one barrier each.
template <int NV>
static __device__ __forceinline__ void block_sums(double (&val)[NV], double (*ws)[4], int wave, int lane)
{
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        val[q] = wave_sum(val[q]);
        if (lane == 0) ws[q][wave] = val[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) val[q] = (ws[q][0] + ws[q][1]) + (ws[q][2] + ws[q][3]);
}

// One workgroup per input, fixed order.  First m (the column-tile partials) and S = 2 h.Y_h, then per k the two mean sums and the five row
// products p_k.Y_h, h.Y_pk, c_k.Y_h, h.Y_ck, p_k.Y_pk over the input's rows of H and Y (each of the 4 d rows p, c, Y_p, Y_c is read once;
// h and Y_h are read again per k, from cache).  out: [mean | var | dmean_du [, d] | dvar_du [, d] | dmean_ds [, d] | dvar_ds [, d]], each
// block ldo inputs long; the slab's input i is input o0 + i of the batch.  Y == nullptr: mean and its two gradients alone.
__global__ __launch_bounds__(256, 4) void exact_grad_finish_kernel(const double *__restrict__ Y, const double *__restrict__ H, long npad, int d,
                                                               const double *__restrict__ mpart, long npart, double vplusvt, double nc2,
                                                               const double *__restrict__ nq, double *__restrict__ out, long ldo, long o0)
{
    __shared__ double ws[2][7][4];
    const long i = blockIdx.x;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int nrow = 2 * d + 1;
    const double *mp = mpart + (i * nrow) * npart;
    const double *h0 = H + (i * nrow) * npad, *y0 = Y + (i * nrow) * npad;
    const long io = o0 + i;
    double *mean_o = out, *var_o = out + ldo, *dmu_o = var_o + ldo, *dvu_o = dmu_o + ldo * d, *dms_o = dvu_o + ldo * d, *dvs_o = dms_o + ldo * d;
    double a[2] = {0.0, 0.0};
    for (long p = t; p < npart; p += 256) a[0] += mp[p];
    if (Y) {
        double s0 = 0.0, s1 = 0.0;
        for (long c = 2 * t; c < npad; c += 512) {
            const v2d yy = *reinterpret_cast<const v2d *>(y0 + c), hh = *reinterpret_cast<const v2d *>(h0 + c);
            s0 = fma(yy.x, hh.x, s0);
            s1 = fma(yy.y, hh.y, s1);
        }
        a[1] = s0 + s1;
    }
    block_sums<2>(a, ws[0], wave, lane);
    const double m = a[0], S = 2.0 * a[1];
    if (t == 0) {
        mean_o[io] = m;
        if (Y) var_o[io] = vplusvt - nc2 * S - m * m;
    }
    for (int k = 0; k < d; ++k) {
        double r[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // dm/du_k, dm/ds_k, p.Y_h, h.Y_p, c.Y_h, h.Y_c, p.Y_p
        const double *mu = mp + (long)(1 + k) * npart, *ms = mp + (long)(1 + d + k) * npart;
        for (long p = t; p < npart; p += 256) { r[0] += mu[p]; r[1] += ms[p]; }
        if (Y) {
            const double *pk = h0 + (long)(1 + k) * npad, *ck = h0 + (long)(1 + d + k) * npad;
            const double *ypk = y0 + (long)(1 + k) * npad, *yck = y0 + (long)(1 + d + k) * npad;
            double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (long c = 2 * t; c < npad; c += 512) {
                const v2d hh = *reinterpret_cast<const v2d *>(h0 + c), yh = *reinterpret_cast<const v2d *>(y0 + c);
                const v2d pp = *reinterpret_cast<const v2d *>(pk + c), cc = *reinterpret_cast<const v2d *>(ck + c);
                const v2d yp = *reinterpret_cast<const v2d *>(ypk + c), yc = *reinterpret_cast<const v2d *>(yck + c);
                r[2] = fma(pp.x, yh.x, r[2]); e[0] = fma(pp.y, yh.y, e[0]);
                r[3] = fma(hh.x, yp.x, r[3]); e[1] = fma(hh.y, yp.y, e[1]);
                r[4] = fma(cc.x, yh.x, r[4]); e[2] = fma(cc.y, yh.y, e[2]);
                r[5] = fma(hh.x, yc.x, r[5]); e[3] = fma(hh.y, yc.y, e[3]);
                r[6] = fma(pp.x, yp.x, r[6]); e[4] = fma(pp.y, yp.y, e[4]);
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) r[2 + q] += e[q];
        }
        block_sums<7>(r, ws[(k + 1) & 1], wave, lane);
        if (t == 0) {
            dmu_o[io * d + k] = r[0];
            dms_o[io * d + k] = r[1];
            if (Y) {
                const double G = r[2] + r[3], Q = 0.5 * (r[4] + r[5]) + r[6];
                dvu_o[io * d + k] = nc2 * G - 2.0 * m * r[0];
                dvs_o[io * d + k] = -nc2 * (0.5 * Q - nq[k] * S) - 2.0 * m * r[1];
            }
        }
    }
}

int launch_exact_grad_finish(const double *Y, const double *H, int64_t npad, int d, const double *mpart, int64_t nb, double vplusvt, double nc2,
                             const double *nq_dev, double *out, int64_t ldo, int64_t o0, hipStream_t s, Profiler *prof)
{
    if (nb <= 0) return 0;
    ProfScope ps(prof, s, GPX_K_EXACT, (Y ? 2.0 + 10.0 * d : 0.0) * (double)nb * (double)npad + (double)nb * (2.0 * d + 1.0) * (double)(npad / EG_COLS));
    hipLaunchKernelGGL(exact_grad_finish_kernel, dim3((unsigned)nb), dim3(256), 0, s, Y, H, (long)npad, d, mpart, (long)(npad / EG_COLS), vplusvt,
                       nc2, nq_dev, out, (long)ldo, (long)o0);
    GPX_HIP(hipGetLastError());
    return 0;
}
