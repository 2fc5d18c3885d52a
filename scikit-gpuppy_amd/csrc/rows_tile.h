// rows_tile.h -- the frame of every build kernel of the batched row calls (propagate.hip: the Gaussian kernel, matern.hip: Matern), once.
//
// The vectors of MANY inputs u_b as the rows of a right-hand-side block Z (leading dimension npad) for the many-right-hand-side triangular
// solver.  With delta = x_i - u, wd = w . delta and q = wd . delta, an input owns rows_per_input(LAYOUT, d) rows (GPX_ROWS_*, include/gpx.h):
//   APPROX  [C, tr, J_1..J_d]             tr_i = tracedot(H_i, Sigma_b), full Sigma
//   DVH     [C, J_1..J_d, H_11..H_dd]     no Sigma
//   GRAD    [C, J_1..J_d]                 no Sigma (the rows of gpx_predict_grad)
// C_i carries +vt iff x_i == u_b elementwise.  A workgroup owns 128 columns (a lane two adjacent ones: 16-byte stores) and RT_INPUTS inputs,
// four per wave; the x tile sits in LDS k-major as in gram_tile.h; the input's u, w, Sigma are wave-uniform (scalar loads).  Radial factors
// once per (input, column); columns past n are zero in every row.  DR > 0: d <= DR, wd stays in registers; DR = 0: any d, from the LDS tile.
// The frame owns the staging, the wave -> input map, the q / equality pass, the C row, the J / H / tr loops and the stores; the per-thread
// arrays wd0 / wd1 stay plain locals of the frame (nll_grad_tile.h explains why).  What a kernel family computes comes in as a policy:
//   struct Policy {
//       double v, vt;                                                  // wave-uniform
//       static constexpr bool has_layout(int layout);                  // the family has the derivatives the layout needs
//       typedef ... in_ptr, out_ptr;                                   // const double * / double *, with or without __restrict__ (below)
//       static constexpr bool pin(int layout);                         // form w and the tests k < d anew per input (below)
//       struct Col {                                                   // the radial factors of one (input, column)
//           Col(const Policy &, bool in, double q);                    // in: the column lies below n
//           double kf() const;                                         // the C row, before +vt
//           double jfac() const;                                       // J_k = -wd_k jfac()
//           double hkk(double wd, double w_k) const;                   // H_kk
//           double tr(double s, double wdiag) const;                   // tr(H Sigma) from s = wd^T Sigma wd, wdiag = sum_k w_k Sigma_kk
//       };
//   };
// pin: held across a wave's inputs, w and the tests k < d cost scalar registers that the GRAD instantiations of the Matern policy do not
// have (predict_grad.hip explains); where a policy returns true the frame has them re-formed per input.
// in_ptr / out_ptr: on the inlined frame __restrict__ makes further wave-uniform loads (u, w) scalar ones.  The Matern instantiations are
// compiled with it; the Gaussian DR = 0 ones then run out of scalar registers and drop from 8 to 7 waves per SIMD, so the Gaussian policy
// leaves it out.  The values are the same either way.  Both keep every instantiation at the registers, spills and occupancy that the
// separate bodies had (tests/test_rows_model.py, tests/test_predict_grad_model.py).
#pragma once
#include "common.h"
#include "radial.h"   // GaussRadial, MaternRadial: the radial factors at q

constexpr int RT_COLS = 128;    // columns of one workgroup (64 lanes x 2 adjacent columns)
constexpr int RT_INPUTS = 16;   // inputs of one workgroup, four per wave

template <int DR, int LAYOUT, class Policy>
__device__ __forceinline__ void rows_build_tile(const Policy &pol, typename Policy::in_ptr x, long n, long npad, int d, typename Policy::in_ptr U,
                                                typename Policy::in_ptr Sigma, long sigma_stride, long nb, typename Policy::in_ptr w_in,
                                                typename Policy::out_ptr Z)
{
    typedef typename Policy::Col Col;
    constexpr bool DVH = LAYOUT == GPX_ROWS_DVH, TR = LAYOUT == GPX_ROWS_APPROX, PIN = Policy::pin(LAYOUT);
    static_assert(Policy::has_layout(LAYOUT), "the kernel family has no rows of this layout");
    const double *w = w_in;
    extern __shared__ __attribute__((aligned(16))) double rt_smem[];
    double *x_s = rt_smem;   // [d][128] raw inputs of the tile's columns, k-major
    const int t = threadIdx.x;
    const long col0 = (long)blockIdx.x * RT_COLS;
    for (int e = t; e < RT_COLS * d; e += 256) {
        const int c = e & (RT_COLS - 1), k = e >> 7;
        const long gc = col0 + c;
        x_s[k * RT_COLS + c] = (gc < n) ? x[gc * d + k] : 0.0;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const long c = col0 + 2 * lane;
    const bool in0 = c < n, in1 = c + 1 < n;
    const long nrow = rows_per_input(LAYOUT, d);
    const int jrow = TR ? 2 : 1;   // first row of J
    for (int j = 0; j < RT_INPUTS / 4; ++j) {
        const long b = (long)blockIdx.y * RT_INPUTS + 4 * j + wave;   // wave-uniform
        if (b >= nb) break;
        if constexpr (PIN) asm volatile("" : "+s"(w), "+s"(d));
        const double *u = U + b * d;
        double *zrow = Z + b * nrow * npad + c;
        double wd0[DR > 0 ? DR : 1], wd1[DR > 0 ? DR : 1];
        double q0 = 0.0, q1 = 0.0;
        bool same0 = true, same1 = true;
        if constexpr (DR > 0) {
#pragma unroll
            for (int k = 0; k < DR; ++k) {
                wd0[k] = 0.0; wd1[k] = 0.0;
                if (k < d) {
                    const v2d xv = *reinterpret_cast<const v2d *>(&x_s[k * RT_COLS + 2 * lane]);
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
            for (int k = 0; k < d; ++k) {
                const v2d xv = *reinterpret_cast<const v2d *>(&x_s[k * RT_COLS + 2 * lane]);
                const double uk = u[k], wk = w[k];
                const double d0 = xv.x - uk, d1 = xv.y - uk;
                same0 = same0 && (xv.x == uk);
                same1 = same1 && (xv.y == uk);
                q0 = fma(wk * d0, d0, q0);
                q1 = fma(wk * d1, d1, q1);
            }
        }
        const Col r0(pol, in0, q0), r1(pol, in1, q1);
        const double c0 = r0.kf(), c1 = r1.kf(), g0 = r0.jfac(), g1 = r1.jfac();
        v2d o;
        o.x = (in0 && same0) ? c0 + pol.vt : c0;
        o.y = (in1 && same1) ? c1 + pol.vt : c1;
        *reinterpret_cast<v2d *>(zrow) = o;
        const double *S = TR ? Sigma + b * sigma_stride : nullptr;
        double s0 = 0.0, s1 = 0.0, wdiag = 0.0;
        if constexpr (DR > 0) {
#pragma unroll
            for (int a = 0; a < DR; ++a) {
                if (a < d) {
                    v2d jk;
                    jk.x = -wd0[a] * g0; jk.y = -wd1[a] * g1;
                    *reinterpret_cast<v2d *>(zrow + (long)(jrow + a) * npad) = jk;
                    if constexpr (DVH) {
                        const double wa = w[a];
                        v2d hk;
                        hk.x = r0.hkk(wd0[a], wa); hk.y = r1.hkk(wd1[a], wa);
                        *reinterpret_cast<v2d *>(zrow + (long)(1 + d + a) * npad) = hk;
                    } else if constexpr (TR) {
                        double t0 = 0.0, t1 = 0.0;
#pragma unroll
                        for (int e = 0; e < DR; ++e)
                            if (e < d) {
                                const double sg = S[a * d + e];
                                t0 = fma(sg, wd0[e], t0);
                                t1 = fma(sg, wd1[e], t1);
                            }
                        s0 = fma(wd0[a], t0, s0);
                        s1 = fma(wd1[a], t1, s1);
                        wdiag = fma(w[a], S[a * d + a], wdiag);
                    }
                }
            }
        } else {
            if constexpr (PIN) asm volatile("" : "+s"(w), "+s"(d), "+s"(u));
            for (int a = 0; a < d; ++a) {
                const v2d xa = *reinterpret_cast<const v2d *>(&x_s[a * RT_COLS + 2 * lane]);
                const double wa = w[a], ua = u[a];
                const double a0 = wa * (xa.x - ua), a1 = wa * (xa.y - ua);
                v2d jk;
                jk.x = -a0 * g0; jk.y = -a1 * g1;
                *reinterpret_cast<v2d *>(zrow + (long)(jrow + a) * npad) = jk;
                if constexpr (DVH) {
                    v2d hk;
                    hk.x = r0.hkk(a0, wa); hk.y = r1.hkk(a1, wa);
                    *reinterpret_cast<v2d *>(zrow + (long)(1 + d + a) * npad) = hk;
                } else if constexpr (TR) {
                    double t0 = 0.0, t1 = 0.0;
                    for (int e = 0; e < d; ++e) {
                        const v2d xv = *reinterpret_cast<const v2d *>(&x_s[e * RT_COLS + 2 * lane]);
                        const double sg = S[a * d + e], ue = u[e], we = w[e];
                        t0 = fma(sg, we * (xv.x - ue), t0);
                        t1 = fma(sg, we * (xv.y - ue), t1);
                    }
                    s0 = fma(a0, t0, s0);
                    s1 = fma(a1, t1, s1);
                    wdiag = fma(wa, S[a * d + a], wdiag);
                }
            }
        }
        if constexpr (TR) {
            o.x = r0.tr(s0, wdiag);
            o.y = r1.tr(s1, wdiag);
            *reinterpret_cast<v2d *>(zrow + npad) = o;
        }
    }
}

// The Gaussian kernel: c = v exp(-q / 2) is every factor.  J_k = -wd_k c, H_kk = (wd_k^2 - w_k) c (the arithmetic of approx_build_kernel,
// propagate.hip), tr = c (wd^T Sigma wd - sum_k w_k Sigma_kk) (trace_kernel).
struct GaussRows {
    typedef const double *in_ptr;
    typedef double *out_ptr;
    double v, vt;
    static constexpr bool has_layout(int) { return true; }
    static constexpr bool pin(int) { return false; }
    struct Col {
        double c;
        __device__ __forceinline__ Col(const GaussRows &p, bool in, double q) : c(in ? GaussRadial(p.v, q).kf() : 0.0) {}
        __device__ __forceinline__ double kf() const { return c; }
        __device__ __forceinline__ double jfac() const { return c; }
        __device__ __forceinline__ double hkk(double wd, double wk) const { return (wd * wd - wk) * c; }
        __device__ __forceinline__ double tr(double s, double wdiag) const { return c * (s - wdiag); }
    };
};

// Matern, NU2 = 2 nu: with s = sqrt(2 nu q), e = v exp(-s) (MaternRadial)  C = kf(),  J_k = -wd_k g()  and, for nu = 5/2 alone (nu = 3/2
// has no Hessian at the origin), with f = (5/3) e and p = 1 + s
//   H_kl = f [5 wd_k wd_l - delta_kl w_k p],   tr(H Sigma) = f [5 wd^T Sigma wd - p sum_k w_k Sigma_kk].
template <int NU2>
struct MaternRows {
    typedef const double *__restrict__ in_ptr;
    typedef double *__restrict__ out_ptr;
    double v, vt;
    static constexpr bool has_layout(int layout) { return NU2 == 5 || layout == GPX_ROWS_GRAD; }
    static constexpr bool pin(int layout) { return layout == GPX_ROWS_GRAD; }
    struct Col {
        MaternRadial<NU2> r;
        __device__ __forceinline__ Col(const MaternRows &p, bool in, double q) : r(in ? p.v : 0.0, q) {}
        __device__ __forceinline__ double kf() const { return r.kf(); }
        __device__ __forceinline__ double jfac() const { return r.g(); }
        __device__ __forceinline__ double f() const { return (5.0 / 3.0) * r.e; }
        __device__ __forceinline__ double p() const { return 1.0 + r.s; }
        __device__ __forceinline__ double hkk(double wd, double wk) const { return f() * fma(5.0 * wd, wd, -wk * p()); }
        __device__ __forceinline__ double tr(double s, double wdiag) const { return f() * fma(5.0, s, -p() * wdiag); }
    };
};
