// periodic.hip -- PeriodicCovariance on the device: Gram / cross-covariance assembly and the one-pass likelihood gradient.
//
// Replaces PeriodicCovariance.__call__ evaluated N1 x N2 times in Python by the base class's cov_matrix_ij
// (skgpuppy/Covariance.py:361-386 through :137-164) and the 2 + 3 d derivative matrices of Covariance._d_nll_d_theta
// (:266-282 with :399-433).  theta = (log v, log vt, log w_1..d, log p_1..d, log w2_1..d); with delta = xi - xj
//   q = 1/2 sum_k [ w_k delta_k^2 + w2_k sin^2(pi delta_k / p_k) ],   k(xi, xj) = v exp(-q) + (vt iff delta == 0 in every component).
// The periodic factor needs delta itself, so the inputs are NOT pre-scaled: w / 2, 1 / p and w2 / 2 are a block of 4 d
// wave-uniform constants read through the scalar cache.  sin(pi delta / p) comes from a reduced argument (periodic_math.h).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "gram_tile.h"
#include "nll_grad_tile.h"
#include "periodic_math.h"

// what the deriv variant writes (the parameter's group; its coordinate is a second argument)
enum { PD_V = 0, PD_VT = 1, PD_W = 2, PD_P = 3, PD_W2 = 4 };

// one entry of d K / d theta_j from Kf = v exp(-q) and the difference e of the parameter's coordinate (Covariance.py:417-433)
__device__ __forceinline__ double periodic_deriv_entry(int kind, double e, double kf, bool equal, double vt, double hk, double ih, double il,
                                                       double dscale)
{
    if (kind == PD_V) return kf;
    if (kind == PD_VT) return equal ? vt : 0.0;
    if (kind == PD_W) return -(hk * e) * e * kf;                      // hk = w / 2
    const double rr = periodic_reduce(e, ih, il), sn = sinpi_half(rr);
    if (kind == PD_P) return dscale * e * (sn * cospi_half(rr)) * kf;   // dscale = pi w2 / p
    return -(hk * sn) * sn * kf;                                      // hk = w2 / 2
}

// The pair policy of the periodic kernel on the RAW inputs (the frame: gram_tile.h).  Per k and entry: the difference, max |delta| (the
// equality test: delta == 0 in EVERY component, not q == 0, which a zero w or an underflowing delta^2 would fool), two products into q
// and one sin(pi r): 24 fp64 operations, so the kernel is bound by the fp64 VALU from d = 2 on, not by its 8 B / entry store.
// K_ij and K_ji are the same bits: delta changes sign, and every term of q is even in delta operation by operation.
// The equality term is part of the entry, not of the frame's diagonal: a query may equal a training row anywhere.
// DERIV: d K / d theta_j instead of K -- kind (PD_*) and coordinate kd select the factor on Kf = v exp(-q); dscale = pi w2 / p (PD_P).
template <bool DERIV>
struct PeriodicPair {
    const double *par;   // [4][d]: w / 2, fl(1 / p), its correction, w2 / 2
    int d;
    double v, vt;
    int kind, kd;
    double dscale;
    // q and max |delta| of a lane's 16 rows x 2 columns, each set of 16 as ONE vector value: as arrays inside this struct they are taken
    // apart into 64 scalars before the frame is inlined into the kernel, and the kernel then needs 172 VGPRs instead of 164 (two waves
    // per SIMD instead of three).  DERIV alone: the constants hk, ih, il of coordinate kd and the lane's two columns bk of it.
    struct State { v16d acc0, acc1, m0, m1; double hk, ih, il; v2d bk; };

    __device__ __forceinline__ void accumulate(State &st, const double *const (&arow)[16], const double *b_s, int lane, long, int) const
    {
        v16d &acc0 = st.acc0, &acc1 = st.acc1, &m0 = st.m0, &m1 = st.m1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0; acc1[r] = 0.0; m0[r] = 0.0; m1[r] = 0.0; }
        for (int k = 0; k < d; ++k) {
            const double hw = par[k], ih = par[d + k], il = par[2 * d + k], hw2 = par[3 * d + k];
            const v2d b = *reinterpret_cast<const v2d *>(&b_s[k * GT_COLS + 2 * lane]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double a = arow[r][k];
                const double e0 = a - b.x, e1 = a - b.y;
                m0[r] = fmax(m0[r], fabs(e0));
                m1[r] = fmax(m1[r], fabs(e1));
                acc0[r] = fma(hw * e0, e0, acc0[r]);
                acc1[r] = fma(hw * e1, e1, acc1[r]);
                const double s0 = sinpi_half(periodic_reduce(e0, ih, il)), s1 = sinpi_half(periodic_reduce(e1, ih, il));
                acc0[r] = fma(hw2 * s0, s0, acc0[r]);
                acc1[r] = fma(hw2 * s1, s1, acc1[r]);
            }
        }
        if (DERIV) {
            st.hk = par[(kind == PD_W2 ? 3 * d : 0) + kd]; st.ih = par[d + kd]; st.il = par[2 * d + kd];
            st.bk = *reinterpret_cast<const v2d *>(&b_s[kd * GT_COLS + 2 * lane]);
        }
    }
    __device__ __forceinline__ v2d entry(const State &st, const double *const (&arow)[16], int r) const
    {
        v2d o;
        if (DERIV) {
            const double a = arow[r][kd];
            o.x = periodic_deriv_entry(kind, a - st.bk.x, v * exp_nonpos(-st.acc0[r]), st.m0[r] == 0.0, vt, st.hk, st.ih, st.il, dscale);
            o.y = periodic_deriv_entry(kind, a - st.bk.y, v * exp_nonpos(-st.acc1[r]), st.m1[r] == 0.0, vt, st.hk, st.ih, st.il, dscale);
        } else {
            o.x = v * exp_nonpos(-st.acc0[r]) + (st.m0[r] == 0.0 ? vt : 0.0);
            o.y = v * exp_nonpos(-st.acc1[r]) + (st.m1[r] == 0.0 ? vt : 0.0);
        }
        return o;
    }
};

template <bool DERIV>
__global__ __launch_bounds__(256) void periodic_gram_kernel(const double *__restrict__ xi, long n1, const double *__restrict__ xj, long n2,
                                                           int d, const double *__restrict__ par, double v, double vt, double add_diag,
                                                           int lower_only, int pad_mode, double *__restrict__ out, long ld, int kind, int kd,
                                                           double dscale)
{
    gram_tile<PeriodicPair<DERIV>, !DERIV>(PeriodicPair<DERIV>{par, d, v, vt, kind, kd, dscale}, xi, n1, xj, n2, d, add_diag, lower_only,
                                           pad_mode, out, ld);
}

// the padding contract of out: gram_launch_plan (gram_tile.h)
int launch_periodic_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, const PeriodicData *pd, double add_diag,
                         int lower_only, int pad_mode, double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad, hipStream_t s,
                         Profiler *prof, int deriv)
{
    const int d = pd->d;
    GramLaunch pl;
    if (!raw_gram_launch_plan(n1, n2, rows_pad, cols_pad, ld, d, lower_only, pad_mode, deriv, 2 + 3 * d, &pl)) {
        gpx_set_error("launch_periodic_gram: bad shape (n1=%ld n2=%ld rows_pad=%ld cols_pad=%ld ld=%ld d=%d deriv=%d)", (long)n1, (long)n2,
                      (long)rows_pad, (long)cols_pad, (long)ld, d, deriv);
        return GPX_ERR_BAD_ARG;
    }
    ProfScope ps(prof, s, GPX_K_GRAM, pl.bytes);
    if (deriv < 0) {
        hipLaunchKernelGGL(periodic_gram_kernel<false>, pl.grid, dim3(256), pl.lds, s, xi, (long)n1, xj, (long)n2, d, (const double *)pd->par,
                           pd->v, pd->vt, add_diag, pl.lower_only, pad_mode, out, (long)ld, 0, 0, 0.0);
    } else {
        const int kind = deriv < 2 ? deriv : 2 + (deriv - 2) / d, kd = deriv < 2 ? 0 : (deriv - 2) % d;
        const double dscale = kind == PD_P ? M_PI * pd->w2[kd] / pd->p[kd] : 0.0;
        hipLaunchKernelGGL(periodic_gram_kernel<true>, pl.grid, dim3(256), pl.lds, s, xi, (long)n1, xj, (long)n2, d, (const double *)pd->par,
                           pd->v, pd->vt, 0.0, pl.lower_only, pad_mode, out, (long)ld, kind, kd, dscale);
    }
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Gradient of the negative log likelihood (Covariance._d_nll_d_theta, skgpuppy/Covariance.py:266-282, with
// PeriodicCovariance._d_cov_d_theta, :399-433): the one pass of nll_grad_tile.h with Kf_ij = v exp(-q_ij) and, per coordinate and with
// s, c = sin, cos(pi delta_k / p_k), the three sums
//   A_k = sum M Kf delta_k^2,  B_k = sum M Kf delta_k s c,  C_k = sum M Kf s^2
// so that
//   g_0 = S_0 / 2,  g_1 = vt T / 2,  g_{w_k} = -w_k A_k / 4,  g_{p_k} = (pi w2_k / p_k) B_k / 2,  g_{w2_k} = -w2_k C_k / 4.
// A sweep forms the sine and cosine of its own KC coordinates once more -- per pair d + KC sines and KC cosines, 3 KC + 2 accumulators,
// whatever d is.  From d = 9 on every sweep repeats q: 2 x the sines at d = 16, 4.5 x at d = 64.
// ---------------------------------------------------------------------------------------------
template <int KC_>
struct PeriodicGrad {
    static constexpr int KC = KC_, NA = 3, NC = NA * KC + 2;
    const double *par;   // [4][d]: w / 2, fl(1 / p), its correction, w2 / 2
    int d;
    double v;
    struct Coord { double hw, ih, il, hw2; };

    __device__ __forceinline__ Coord coord(int k) const { return {par[k], par[d + k], par[2 * d + k], par[3 * d + k]}; }
    __device__ __forceinline__ double add_q(const Coord &c, double e, double q) const
    {
        q = fma(c.hw * e, e, q);
        const double sn = sinpi_half(periodic_reduce(e, c.ih, c.il));
        return fma(c.hw2 * sn, sn, q);
    }
    __device__ __forceinline__ double pair(double mij, double wgt, double q, bool equal, double &s0, double &t) const
    {
        const double wq = mij * wgt * v * exp_nonpos(-q);
        s0 += wq;
        if (equal) t += mij * wgt;
        return wq;
    }
    __device__ __forceinline__ void sweep(const Coord &c, double wq, double e, double (&acc)[NC], int kk) const
    {
        const double rr = periodic_reduce(e, c.ih, c.il), sn = sinpi_half(rr), cs = cospi_half(rr);
        acc[1 + 3 * kk] = fma(wq, e * e, acc[1 + 3 * kk]);
        acc[2 + 3 * kk] = fma(wq, e * (sn * cs), acc[2 + 3 * kk]);
        acc[3 + 3 * kk] = fma(wq, sn * sn, acc[3 + 3 * kk]);
    }
};

template <int KC>
__global__ __launch_bounds__(256) void periodic_nll_grad_kernel(const double *__restrict__ Kinv, long ld, long n, long npad, int d,
                                                               const double *__restrict__ alpha, const double *__restrict__ x,
                                                               const double *__restrict__ xT, const double *__restrict__ par, double v,
                                                               double *__restrict__ partial)
{
    nll_grad_tile(PeriodicGrad<KC>{par, d, v}, Kinv, ld, n, npad, d, alpha, x, xT, partial);
}

int launch_periodic_nll_grad(const double *Kinv, int64_t ld, int64_t n, int64_t npad, const PeriodicData *pd, const double *alpha,
                             double *partial, hipStream_t s)
{
    const int sweeps = (pd->d + PER_KC - 1) / PER_KC;
    hipLaunchKernelGGL(periodic_nll_grad_kernel<PER_KC>, dim3((unsigned)(npad / 8), (unsigned)sweeps), dim3(256), 0, s, Kinv, (long)ld, (long)n,
                       (long)npad, pd->d, alpha, (const double *)pd->x, (const double *)pd->xT, (const double *)pd->par, pd->v, partial);
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- parameters of a periodic model ---------------------------------------------------------------------------
int periodic_parse(const double *theta, int d, PeriodicData *out)
{
    GPX_TRY(raw_parse_head("periodic", theta, d, out, out->w));
    for (int k = 0; k < d; ++k) {
        out->p[k] = exp(theta[2 + d + k]);
        out->w2[k] = exp(theta[2 + 2 * d + k]);
        if (!(out->w[k] >= 0.0) || !isfinite(out->w[k]) || !(out->p[k] > 0.0) || !isfinite(out->p[k]) || !(out->w2[k] >= 0.0) ||
            !isfinite(out->w2[k])) {
            gpx_set_error("periodic kernel: theta gives w[%d]=%g p[%d]=%g w2[%d]=%g", k, out->w[k], k, out->p[k], k, out->w2[k]);
            return GPX_ERR_BAD_ARG;
        }
    }
    return 0;
}

// ---- C-ABI: the stand-alone Gram --------------------------------------------------------------------------------
extern "C" int gpx_periodic_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, int d, const double *theta, int deriv,
                                 double *out)
{
    GPX_TRY(raw_gram_args("gpx_periodic_gram", xi, n1, xj, n2, out));
    PeriodicData pd;
    GPX_TRY(periodic_parse(theta, d, &pd));
    if (deriv < -1 || deriv >= 2 + 3 * d) { gpx_set_error("gpx_periodic_gram: deriv=%d (-1 .. %d)", deriv, 1 + 3 * d); return GPX_ERR_BAD_ARG; }
    return raw_gram(&pd, xi, n1, xj, n2, deriv, out);
}

// d nll / d theta [2 + 3 d] at the handle's theta
extern "C" int gpx_periodic_nll_grad(gpx_handle *h, double *grad_out)
{
    CHECK_H(h);
    GPX_TRY(need_kind(h, KernelKind::Periodic, "gpx_periodic_nll_grad"));
    if (!grad_out) { gpx_set_error("null argument"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(ensure_kinv(h));
    const PeriodicData *pd = handle_periodic(h);
    const int d = pd->d;
    double o[(GPX_MAX_D / PER_KC) * PER_NC];
    GPX_TRY(raw_nll_grad_sums(h, PER_KC, PER_NC, o));
    std::vector<double> g(2 + 3 * d);
    g[0] = 0.5 * o[0];                                        // dK/dtheta_0 = Kf                     (Covariance.py:417-419)
    g[1] = 0.5 * pd->vt * o[PER_NC - 1];                      // vt on equality                        (:420-422)
    for (int k = 0; k < d; ++k) {
        const double *ok = o + (k / PER_KC) * PER_NC + 1 + 3 * (k % PER_KC);
        g[2 + k] = -0.25 * pd->w[k] * ok[0];                  // -1/2 w_k delta_k^2 Kf                 (:423-425)
        g[2 + d + k] = 0.5 * (M_PI * pd->w2[k] / pd->p[k]) * ok[1];   // pi delta_k w2_k / p_k sin cos Kf   (:426-429)
        g[2 + 2 * d + k] = -0.25 * pd->w2[k] * ok[2];         // -1/2 w2_k sin^2 Kf                    (:430-433)
    }
    GPX_HIP(hipMemcpy(grad_out, g.data(), sizeof(double) * (2 + 3 * d), hipMemcpyDefault));
    return 0;
}
