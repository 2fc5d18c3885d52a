// matern.hip -- MaternCovariance (ARD Matern, nu = 3/2 or 5/2) on the device: Gram / cross-covariance assembly, the one-pass likelihood
// gradient, for nu = 5/2 the right-hand-side blocks of the batched Approx and inverse propagation, and for either nu the rows [C, J_1..J_d]
// of the predictor's input gradients (gpx_predict_grad).
//
// theta = (log v, log vt, log w_1..d), GaussianCovariance's layout.  With delta = xi - xj, q = sum_k w_k delta_k^2 and s = sqrt(2 nu q)
//   nu = 5/2: Kf = v (1 + s + s^2 / 3) exp(-s)      nu = 3/2: Kf = v (1 + s) exp(-s)      K = Kf + (vt iff delta == 0 in every component).
// Every derivative is a polynomial in s times exp(-s) -- with G = (5/3) v (1 + s) exp(-s) (5/2) or 3 v exp(-s) (3/2)
//   d K / d log w_k = -1/2 w_k delta_k^2 G,      d Kf / d xi_k = -w_k delta_k G       (5/2: d^2 Kf / d xi_k d xi_l below)
// so nothing divides by s and delta = 0 gives exactly v: sqrt(0) = 0, exp_nonpos(0) = 1.  nu enters as NU2 = 2 nu (3 or 5), a template
// parameter.  The inputs are read RAW: equality is decided on max |delta|, which scaling by sqrt(w) would not preserve.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "gram_tile.h"
#include "nll_grad_tile.h"
#include "radial.h"   // MaternRadial: the radial factors at q, one sqrt and one exp for all of them
#include "rows_tile.h"

// what the deriv variant writes (the parameter's group; MD_W: its coordinate is a second argument)
enum { MD_V = 0, MD_VT = 1, MD_W = 2 };

// The pair policy of the Matern kernel on the raw inputs (the frame: gram_tile.h).  Per k and entry: the difference, max |delta| (the
// equality test) and one product into q with the wave-uniform w_k -- the Gaussian kernel's arithmetic plus one multiply; per entry one
// sqrt, one exp and the polynomial.  K_ij and K_ji are the same bits: delta changes sign and q is even in it operation by operation.
// The equality term is part of the entry, not of the frame's diagonal: a query may equal a training row anywhere.
// DERIV: d K / d theta_j instead of K -- kind (MD_*) and coordinate kd.
template <int NU2, bool DERIV>
struct MaternPair {
    const double *w;   // [d]
    int d;
    double v, vt;
    int kind, kd;
    // (q and max |delta| of a lane's 16 rows x 2 columns as vector values: PeriodicPair's State explains why)
    struct State { v16d acc0, acc1, m0, m1; double wk; v2d bk; };

    __device__ __forceinline__ void accumulate(State &st, const double *const (&arow)[16], const double *b_s, int lane, long, int) const
    {
        v16d &acc0 = st.acc0, &acc1 = st.acc1, &m0 = st.m0, &m1 = st.m1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0; acc1[r] = 0.0; m0[r] = 0.0; m1[r] = 0.0; }
        for (int k = 0; k < d; ++k) {
            const double wk = w[k];
            const v2d b = *reinterpret_cast<const v2d *>(&b_s[k * GT_COLS + 2 * lane]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double a = arow[r][k];
                const double e0 = a - b.x, e1 = a - b.y;
                m0[r] = fmax(m0[r], fabs(e0));
                m1[r] = fmax(m1[r], fabs(e1));
                acc0[r] = fma(wk * e0, e0, acc0[r]);
                acc1[r] = fma(wk * e1, e1, acc1[r]);
            }
        }
        if (DERIV) {
            st.wk = w[kd];
            st.bk = *reinterpret_cast<const v2d *>(&b_s[kd * GT_COLS + 2 * lane]);
        }
    }
    __device__ __forceinline__ double deriv_entry(double q, bool equal, double e, double wk) const
    {
        if (kind == MD_VT) return equal ? vt : 0.0;
        const MaternRadial<NU2> rad(v, q);
        if (kind == MD_V) return rad.kf();
        return -(0.5 * wk * e) * e * rad.g();
    }
    __device__ __forceinline__ v2d entry(const State &st, const double *const (&arow)[16], int r) const
    {
        v2d o;
        if (DERIV) {
            const double a = arow[r][kd];
            o.x = deriv_entry(st.acc0[r], st.m0[r] == 0.0, a - st.bk.x, st.wk);
            o.y = deriv_entry(st.acc1[r], st.m1[r] == 0.0, a - st.bk.y, st.wk);
        } else {
            o.x = MaternRadial<NU2>(v, st.acc0[r]).kf() + (st.m0[r] == 0.0 ? vt : 0.0);
            o.y = MaternRadial<NU2>(v, st.acc1[r]).kf() + (st.m1[r] == 0.0 ? vt : 0.0);
        }
        return o;
    }
};

template <int NU2, bool DERIV>
__global__ __launch_bounds__(256) void matern_gram_kernel(const double *__restrict__ xi, long n1, const double *__restrict__ xj, long n2, int d,
                                                         const double *__restrict__ w, double v, double vt, double add_diag, int lower_only,
                                                         int pad_mode, double *__restrict__ out, long ld, int kind, int kd)
{
    gram_tile<MaternPair<NU2, DERIV>, !DERIV>(MaternPair<NU2, DERIV>{w, d, v, vt, kind, kd}, xi, n1, xj, n2, d, add_diag, lower_only, pad_mode, out,
                                              ld);
}

// the padding contract of out: gram_launch_plan (gram_tile.h)
int launch_matern_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, const MaternData *md, double add_diag, int lower_only,
                       int pad_mode, double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad, hipStream_t s, Profiler *prof, int deriv)
{
    const int d = md->d;
    GramLaunch pl;
    if (!raw_gram_launch_plan(n1, n2, rows_pad, cols_pad, ld, d, lower_only, pad_mode, deriv, 2 + d, &pl) || (md->nu2 != 3 && md->nu2 != 5)) {
        gpx_set_error("launch_matern_gram: bad shape (n1=%ld n2=%ld rows_pad=%ld cols_pad=%ld ld=%ld d=%d deriv=%d nu2=%d)", (long)n1, (long)n2,
                      (long)rows_pad, (long)cols_pad, (long)ld, d, deriv, md->nu2);
        return GPX_ERR_BAD_ARG;
    }
    ProfScope ps(prof, s, GPX_K_GRAM, pl.bytes);
    const double *w = md->par;
    const int kind = deriv < 2 ? deriv : MD_W, kd = deriv < 2 ? 0 : deriv - 2;
#define MATERN_GRAM(NU2, DERIV, diag)                                                                                                       \
    hipLaunchKernelGGL((matern_gram_kernel<NU2, DERIV>), pl.grid, dim3(256), pl.lds, s, xi, (long)n1, xj, (long)n2, d, w, md->v, md->vt, diag, \
                       pl.lower_only, pad_mode, out, (long)ld, kind, kd)
    if (deriv < 0) {
        if (md->nu2 == 5) MATERN_GRAM(5, false, add_diag);
        else MATERN_GRAM(3, false, add_diag);
    } else {
        if (md->nu2 == 5) MATERN_GRAM(5, true, 0.0);
        else MATERN_GRAM(3, true, 0.0);
    }
#undef MATERN_GRAM
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Gradient of the negative log likelihood: the one pass of nll_grad_tile.h with the radial factors Kf and G of q_ij and, per coordinate,
// the one sum A_k = sum M G delta_k^2, so that  g_0 = S_0 / 2,  g_1 = vt T / 2,  g_{2+k} = -w_k A_k / 4.
// ---------------------------------------------------------------------------------------------
template <int NU2>
struct MaternGrad {
    static constexpr int KC = MAT_KC, NA = 1, NC = MAT_NC;
    const double *w;   // [d]
    double v;
    struct Coord { double wk; };

    __device__ __forceinline__ Coord coord(int k) const { return {w[k]}; }
    __device__ __forceinline__ double add_q(const Coord &c, double e, double q) const { return fma(c.wk * e, e, q); }
    __device__ __forceinline__ double pair(double mij, double wgt, double q, bool equal, double &s0, double &t) const
    {
        const double m = mij * wgt;
        const MaternRadial<NU2> rad(v, q);
        s0 = fma(m, rad.kf(), s0);
        if (equal) t += m;
        return m * rad.g();
    }
    __device__ __forceinline__ void sweep(const Coord &, double wq, double e, double (&acc)[NC], int kk) const
    {
        acc[1 + kk] = fma(wq, e * e, acc[1 + kk]);
    }
};

template <int NU2>
__global__ __launch_bounds__(256) void matern_nll_grad_kernel(const double *__restrict__ Kinv, long ld, long n, long npad, int d,
                                                             const double *__restrict__ alpha, const double *__restrict__ x,
                                                             const double *__restrict__ xT, const double *__restrict__ w, double v,
                                                             double *__restrict__ partial)
{
    nll_grad_tile(MaternGrad<NU2>{w, v}, Kinv, ld, n, npad, d, alpha, x, xT, partial);
}

int launch_matern_nll_grad(const double *Kinv, int64_t ld, int64_t n, int64_t npad, const MaternData *md, const double *alpha, double *partial,
                           hipStream_t s)
{
    const dim3 grid((unsigned)(npad / 8), (unsigned)((md->d + MAT_KC - 1) / MAT_KC));
    hipLaunchKernelGGL(md->nu2 == 5 ? matern_nll_grad_kernel<5> : matern_nll_grad_kernel<3>, grid, dim3(256), 0, s, Kinv, (long)ld, (long)n, (long)npad,
                       md->d, alpha, (const double *)md->x, (const double *)md->xT, (const double *)md->par, md->v, partial);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The build kernels of the batched row calls on the Matern kernel: the frame of rows_tile.h with the MaternRows<NU2> policy.
// matern52_build_many_kernel<DR, DVH> (nu = 5/2): the APPROX rows [C, tr, J_1..J_d] or, DVH = true, the DVH rows [C, J_1..J_d, H_11..H_dd];
// matern_grad_build_many_kernel<DR, NU2>: the GRAD rows [C, J_1..J_d] of gpx_predict_grad, one derivative only, so nu = 3/2 as well.
// DR = 8: d <= 8; DR = 0: any d.  launch_rows_build (propagate.hip) launches them.
// ---------------------------------------------------------------------------------------------
template <int DR, bool DVH>
__global__ __launch_bounds__(256) void matern52_build_many_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                                 const double *__restrict__ U, const double *__restrict__ Sigma,
                                                                 long sigma_stride, long nb, const double *__restrict__ w, double v, double vt,
                                                                 double *__restrict__ Z)
{
    rows_build_tile<DR, DVH ? GPX_ROWS_DVH : GPX_ROWS_APPROX>(MaternRows<5>{v, vt}, x, n, npad, d, U, Sigma, sigma_stride, nb, w, Z);
}

template <int DR, int NU2>
__global__ __launch_bounds__(256) void matern_grad_build_many_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                                    const double *__restrict__ U, long nb, const double *__restrict__ w, double v,
                                                                    double vt, double *__restrict__ Z)
{
    rows_build_tile<DR, GPX_ROWS_GRAD>(MaternRows<NU2>{v, vt}, x, n, npad, d, U, nullptr, 0, nb, w, Z);
}

// this file's part of launch_rows_build's table: neither kernel where the family has no such rows (nu = 3/2: GPX_ROWS_GRAD alone)
RowsKernel matern_rows_kernel(int nu2, int layout, bool regs)
{
    if (layout == GPX_ROWS_GRAD && nu2 == 5) return {nullptr, regs ? matern_grad_build_many_kernel<8, 5> : matern_grad_build_many_kernel<0, 5>};
    if (layout == GPX_ROWS_GRAD && nu2 == 3) return {nullptr, regs ? matern_grad_build_many_kernel<8, 3> : matern_grad_build_many_kernel<0, 3>};
    if (layout == GPX_ROWS_DVH && nu2 == 5) return {regs ? matern52_build_many_kernel<8, true> : matern52_build_many_kernel<0, true>, nullptr};
    if (layout == GPX_ROWS_APPROX && nu2 == 5) return {regs ? matern52_build_many_kernel<8, false> : matern52_build_many_kernel<0, false>, nullptr};
    return {nullptr, nullptr};
}

// ---- parameters of a Matern model ------------------------------------------------------------------------------------------
int matern_parse(const double *theta, int d, int nu2, MaternData *out)
{
    if (nu2 != 3 && nu2 != 5) {
        gpx_set_error("matern kernel: nu2 = 2 nu = %d (3 or 5 supported)", nu2);
        return GPX_ERR_BAD_ARG;
    }
    out->nu2 = nu2;
    GPX_TRY(raw_parse_head("matern", theta, d, out, out->w));
    for (int k = 0; k < d; ++k)
        if (!(out->w[k] >= 0.0) || !isfinite(out->w[k])) {
            gpx_set_error("matern kernel: theta gives w[%d]=%g", k, out->w[k]);
            return GPX_ERR_BAD_ARG;
        }
    return 0;
}

// ---- C-ABI ---------------------------------------------------------------------------------------------------------
extern "C" int gpx_matern_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, int d, const double *theta, int nu2, int deriv,
                               double *out)
{
    GPX_TRY(raw_gram_args("gpx_matern_gram", xi, n1, xj, n2, out));
    MaternData md;
    GPX_TRY(matern_parse(theta, d, nu2, &md));
    if (deriv < -1 || deriv >= 2 + d) { gpx_set_error("gpx_matern_gram: deriv=%d (-1 .. %d)", deriv, 1 + d); return GPX_ERR_BAD_ARG; }
    return raw_gram(&md, xi, n1, xj, n2, deriv, out);
}

// d nll / d theta [2 + d] at the handle's theta
extern "C" int gpx_matern_nll_grad(gpx_handle *h, double *grad_out)
{
    CHECK_H(h);
    GPX_TRY(need_kind(h, KernelKind::Matern, "gpx_matern_nll_grad"));
    if (!grad_out) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(ensure_kinv(h));
    const MaternData *md = handle_matern(h);
    const int d = md->d;
    double o[(GPX_MAX_D / MAT_KC) * MAT_NC];
    GPX_TRY(raw_nll_grad_sums(h, MAT_KC, MAT_NC, o));
    std::vector<double> g(2 + d);
    g[0] = 0.5 * o[0];                       // d K / d theta_0 = Kf
    g[1] = 0.5 * md->vt * o[MAT_NC - 1];     // vt on equality
    for (int k = 0; k < d; ++k) g[2 + k] = -0.25 * md->w[k] * o[(k / MAT_KC) * MAT_NC + 1 + k % MAT_KC];   // -1/2 w_k delta_k^2 G
    GPX_HIP(hipMemcpy(grad_out, g.data(), sizeof(double) * (2 + d), hipMemcpyDefault));
    return 0;
}

// the fused propagation of a Matern handle: nu = 5/2 alone
static int need_matern52(const gpx_handle *h, const char *what)
{
    GPX_TRY(need_kind(h, KernelKind::Matern, what));
    if (handle_matern(h)->nu2 == 5) return 0;
    gpx_set_error("%s: nu = 3/2 has no Hessian at the origin: the fused propagation serves nu = 5/2 alone", what);
    return GPX_ERR_STATE;
}

// propagate_GA_many with cov = MaternCovariance(2.5): gpx_propagate_approx_many's loop on this kernel's right-hand sides
extern "C" int gpx_matern_propagate_approx_many(gpx_handle *h, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *mean,
                                                double *var, double *sigma2, double *rest)
{
    CHECK_H(h);
    GPX_TRY(need_matern52(h, "gpx_matern_propagate_approx_many"));
    return approx_many_run(h, handle_dim(h), U, Sigma, sigma_shared, b, mean, var, sigma2, rest, "gpx_matern_propagate_approx_many",
                           rows_build_of(h, GPX_ROWS_APPROX));
}

// get_best_solution_many's dvh (and sigma2) with cov = MaternCovariance(2.5): gpx_propagate_dvh_many's loop
extern "C" int gpx_matern_propagate_dvh_many(gpx_handle *h, const double *U, int64_t b, double *dvh_out, double *sigma2_out)
{
    CHECK_H(h);
    GPX_TRY(need_matern52(h, "gpx_matern_propagate_dvh_many"));
    return dvh_many_run(h, handle_dim(h), U, b, dvh_out, sigma2_out, "gpx_matern_propagate_dvh_many", rows_build_of(h, GPX_ROWS_DVH));
}
