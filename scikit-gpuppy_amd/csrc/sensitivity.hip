// sensitivity.hip -- first-order and total-effect Sobol indices of the predictor mean under independent Gaussian inputs
// (gpx_sensitivity_many; include/gpx.h carries the formulas).  No reference counterpart: the closest reference code is the nquad /
// Hermite-Gauss cross-checks of skgpuppy/UncertaintyPropagation.py:135-210.
//
// mu(x) = sum_i beta_i c_i(x) with the PLAIN kernel c_i(x) = v exp(-1/2 sum_k w_k (x_k - x_ik)^2): the +vt of the scalar kernel on
// elementwise equality is a measure-zero event under a continuous input and does not enter.  x_k ~ N(u_k, s_k) independent.  With
// a_ik = u_k - x_ik, om = w_k, sg = s_k every kernel factor has a Gaussian expectation:
//   m_ik     = E[factor k of c_i]      = (1 + om sg)^-1/2 exp(-1/2 om a_ik^2 / (1 + om sg))
//   E_k(i,j) = E[factor k of c_i c_j]  = (1 + 2 om sg)^-1/2 exp(-1/4 om (a_ik - a_jk)^2 - 1/4 om (a_ik + a_jk)^2 / (1 + 2 om sg))
// E_k is the header's  -A (a_i^2 + a_j^2) + B a_i a_j  with the square completed: both terms of the exponent are non-positive as written,
// so no rounding makes an exponent positive and the two large terms of the header's form (A (a_i^2 + a_j^2) against B a_i a_j at
// a_i ~ a_j, om sg large) never cancel.  With b_ij = v^2 beta_i beta_j:
//   mean    = v sum_i beta_i prod_k m_ik
//   V       = sum_ij b_ij (prod_k E_k - prod_k m_ik m_jk)
//   first_k = sum_ij b_ij (prod_{l != k} m_il m_jl) (E_k - m_ik m_jk)
//   total_k = sum_ij b_ij (prod_{l != k} E_l) (E_k - m_ik m_jk)
//
// THE FORM THAT SHIPPED is this difference form, every exponent non-positive, with everything that separates over (i, j) moved out of
// the pair pass -- not the ratio form E_k / m_k - 1 (its exponent is positive for a_i ~ a_j and overflows against an underflowed g_i g_j
// at a far input):
//   * a coordinate with s_k = 0 has E_k = m_ik m_jk identically.  It is INACTIVE: its factor exp(-1/2 w_k a_ik^2) is folded into the
//     point weight bw_i = v beta_i prod_inactive, its first_k / total_k are 0.0 exactly (never computed), and the pair pass runs over the
//     na active coordinates alone, compacted into slots 0..na-1.  All s = 0: no pair pass, V = 0.0.
//   * prod_k m_ik m_jk = g_i g_j and prod_{l != k} m_il m_jl = lo_ik lo_jk with g_i = exp(sum_l lm_il), lo_ik = exp(sum_l lm_il - lm_ik)
//     per point (lm = log m): the m side of a pair costs no exponential and no prefix / suffix product.
//   * the pair pass therefore evaluates exactly na exponentials per pair and sweep (the E_k).  Counted in the compiled loops: 26.25
//     vector instructions per pair and slot outside the sweep (6 of argument, 19 of exp_nonpos, 1 product), 43 per own slot plus 85 per
//     pair for the leave-one-out products of E and the accumulations: 429 a pair at d = 8.
// Build kernel: one launch per chunk of inputs, per (input, i) the slot-major a, m, lo, then g and bw; the mean's block partials go
// through launch_sum_columns.  Pair kernel: the frame of exact_sum_kernel / matern_nll_grad_kernel -- a workgroup owns SEN_R rows i in
// LDS, a lane owns column j read slot-major (coalesced), pairs j <= i with weight 2 / 1, heavy row blocks first; grid.y sweeps of SEN_KC
// slots (2 na + 1 accumulators do not fit in registers at na = 64): a sweep forms prod E over ALL active slots and accumulates V and
// the first / total sums of its own slots; grid.z = the chunk's inputs.  Partials go per block into scratch [row block][input, sweep,
// SEN_NC], then ONE launch_sum_columns per chunk.  No atomics; an input's arithmetic reads nothing of another input's and its sums run
// in a fixed order: the result does not depend on its place in the batch or on the chunking.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"

constexpr int SEN_KC = 8;                 // active slots per sweep
constexpr int SEN_NC = 2 * SEN_KC + 1;    // sums per sweep: V, first of the sweep's slots, total of the sweep's slots
constexpr int SEN_R = 8;                  // rows per workgroup
// the constants of one input (host, sens_constants): rows [d] each --
//   0 lmc_l = -1/2 log1p(om sg), 1 lma_l = 1/2 om / (1 + om sg), 2 slot_l (-1: inactive)     by coordinate l
//   3 c0_q = -1/2 log1p(2 om sg), 4 P_q = om / 4, 5 Q_q = om / 4 / (1 + 2 om sg)              by active slot q
// then na
constexpr int SEN_CROWS = 6;
static inline int64_t sens_cb_size(int d) { return (int64_t)SEN_CROWS * d + 2; }

// per (input z, point i): aT / mT / loT [z][slot][npad], g / bw [z][npad]; mpart [block][input] = the block's share of the mean
__global__ __launch_bounds__(256) void sens_build_kernel(const double *__restrict__ x, long n, long npad, int d, const double *__restrict__ U,
                                                         const double *__restrict__ cb, long cb_stride, const double *__restrict__ beta, double v,
                                                         double *__restrict__ aT, double *__restrict__ mT, double *__restrict__ loT,
                                                         double *__restrict__ g, double *__restrict__ bw, double *__restrict__ mpart)
{
    __shared__ double ws[4];
    const int t = threadIdx.x;
    const long z = blockIdx.y, i = (long)blockIdx.x * 256 + t;
    const double *c = cb + z * cb_stride, *u = U + z * d;
    const long base = z * (long)d * npad;
    double mine = 0.0;
    if (i < npad) {
        const bool real = i < n;
        double lall = 0.0, lact = 0.0;
        for (int l = 0; l < d; ++l) {
            const double a = real ? u[l] - x[i * d + l] : 0.0;
            const double lm = real ? fma(-c[d + l] * a, a, c[l]) : 0.0;
            lall += lm;
            if (c[2 * d + l] >= 0.0) lact += lm;
        }
        for (int l = 0; l < d; ++l) {
            const int q = (int)c[2 * d + l];
            if (q < 0) continue;
            const double a = real ? u[l] - x[i * d + l] : 0.0;
            const double lm = real ? fma(-c[d + l] * a, a, c[l]) : 0.0;
            aT[base + q * npad + i] = a;
            mT[base + q * npad + i] = exp_nonpos(lm);
            loT[base + q * npad + i] = exp_nonpos(fmin(lact - lm, 0.0));
        }
        const double b0 = real ? v * beta[i] : 0.0;
        g[z * npad + i] = exp_nonpos(lact);
        bw[z * npad + i] = b0 * exp_nonpos(fmin(lall - lact, 0.0));   // the inactive coordinates' plain kernel factors
        mine = b0 * exp_nonpos(lall);
    }
    mine = wave_sum(mine);
    if ((t & 63) == 0) ws[t >> 6] = mine;
    __syncthreads();
    if (t == 0) mpart[(long)blockIdx.x * gridDim.y + z] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// log E of one slot for the pair (a_i, a_j): both terms non-positive
static __device__ __forceinline__ double sens_log_e(double ai, double aj, double c0, double P, double Q)
{
    const double dm = ai - aj, sm = ai + aj;
    return fma(-Q * sm, sm, fma(-P * dm, dm, c0));
}

// partial [row block][ncols], ncols = inputs * sweeps * SEN_NC: this block's [V, first (SEN_KC), total (SEN_KC)] at (z * sweeps + y) * SEN_NC
template <bool TOTAL>
__global__ __launch_bounds__(256, 2) void sens_pair_kernel(const double *__restrict__ aT, const double *__restrict__ mT,
                                                           const double *__restrict__ loT, const double *__restrict__ g,
                                                           const double *__restrict__ bw, const double *__restrict__ cb, long cb_stride,
                                                           long n, long npad, int d, double *__restrict__ partial, long ncols)
{
#pragma clang fp contract(off)   // the TOTAL and the first-only instantiation must give V and first the same bits
    constexpr int R = SEN_R, KC = SEN_KC, NC = SEN_NC;
    __shared__ double as[R][GPX_MAX_D];       // a_i of the block's rows, by slot (broadcast reads)
    __shared__ double os[R][KC][2];           // m_i, lo_i of the sweep's own slots
    __shared__ double rs[R][2];               // g_i, bw_i
    __shared__ double red[4][NC];
    // what a lane carries from the slot loop into the row loop, parked in LDS (each lane reads its own words back) so that the row loop
    // stays rolled and its 8 exponentials in flight fit the register budget beside the 17 accumulators
    __shared__ double pe[R][256];             // prod E outside the sweep, per row
    __shared__ double oj[KC][3][256];         // a_j, m_j, lo_j of the sweep's own slots
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int rb = gridDim.x - 1 - blockIdx.x;
    const long i0 = (long)rb * R, z = blockIdx.z;
    const int sweeps = gridDim.y, y = blockIdx.y, k0 = y * KC;
    const double *c = cb + z * cb_stride;
    const int na = (int)c[SEN_CROWS * d];
    const double *c0 = c + 3 * d, *cP = c + 4 * d, *cQ = c + 5 * d;
    double *pout = partial + (long)rb * ncols + (z * sweeps + y) * NC;
    if (k0 >= na && y > 0) {                  // an input with fewer active slots than the chunk's widest: nothing in this sweep
        if (t < NC) pout[t] = 0.0;
        return;
    }
    const long base = z * (long)d * npad;
    const double *aZ = aT + base, *mZ = mT + base, *loZ = loT + base;
    for (int q = t; q < R * GPX_MAX_D; q += 256) {
        const int r = q / GPX_MAX_D, k = q - r * GPX_MAX_D;
        as[r][k] = (k < na) ? aZ[(long)k * npad + i0 + r] : 0.0;
    }
    if (t < R * KC) {
        const int r = t / KC, kk = t - r * KC;
        const bool own = k0 + kk < na;
        os[r][kk][0] = own ? mZ[(long)(k0 + kk) * npad + i0 + r] : 1.0;
        os[r][kk][1] = own ? loZ[(long)(k0 + kk) * npad + i0 + r] : 0.0;
    }
    if (t < R) { rs[t][0] = g[z * npad + i0 + t]; rs[t][1] = bw[z * npad + i0 + t]; }
    __syncthreads();

    double acc[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) acc[q] = 0.0;
    const int k1 = (k0 + KC < na) ? k0 + KC : na;
    const long jend = (i0 + R < n) ? i0 + R : n;
    for (long j = t; j < jend; j += 256) {
        // prod E over the slots outside the sweep, for the block's R rows at once
        double PE[R];
#pragma unroll
        for (int r = 0; r < R; ++r) PE[r] = 1.0;
        for (int q = 0; q < na; ++q) {
            if (q >= k0 && q < k1) continue;
            const double aj = aZ[(long)q * npad + j];
            const double c0q = c0[q], Pq = cP[q], Qq = cQ[q];
#pragma unroll
            for (int r = 0; r < R; ++r) PE[r] *= exp_nonpos(sens_log_e(as[r][q], aj, c0q, Pq, Qq));
        }
#pragma unroll
        for (int r = 0; r < R; ++r) pe[r][t] = PE[r];
#pragma unroll
        for (int kk = 0; kk < KC; ++kk)
            if (k0 + kk < na) {
                const long at = (long)(k0 + kk) * npad + j;
                oj[kk][0][t] = aZ[at];
                oj[kk][1][t] = mZ[at];
                oj[kk][2][t] = loZ[at];
            }
        const double gj = g[z * npad + j], bj = bw[z * npad + j];
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            const long i = i0 + r;
            const double wgt = (j < i) ? 2.0 : ((j == i) ? 1.0 : 0.0);
            const double b = (rs[r][1] * bj) * wgt;
            double E[KC], dl[KC];
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) {
                E[kk] = 1.0;
                dl[kk] = 0.0;
                if (k0 + kk < na) {
                    E[kk] = exp_nonpos(sens_log_e(as[r][k0 + kk], oj[kk][0][t], c0[k0 + kk], cP[k0 + kk], cQ[k0 + kk]));
                    dl[kk] = E[kk] - os[r][kk][0] * oj[kk][1][t];
                    acc[1 + kk] = fma(b * (os[r][kk][1] * oj[kk][2][t]), dl[kk], acc[1 + kk]);
                }
            }
            double pre = pe[r][t];
            if (TOTAL) {
                double suf[KC];               // suf[kk] = prod of the own E after kk
                suf[KC - 1] = 1.0;
#pragma unroll
                for (int kk = KC - 2; kk >= 0; --kk) suf[kk] = suf[kk + 1] * E[kk + 1];
#pragma unroll
                for (int kk = 0; kk < KC; ++kk) {
                    acc[1 + KC + kk] = fma(b * (pre * suf[kk]), dl[kk], acc[1 + KC + kk]);
                    pre *= E[kk];
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < KC; ++kk) pre *= E[kk];
            }
            acc[0] = fma(b, pre - rs[r][0] * gj, acc[0]);
        }
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const double s = wave_sum(acc[q]);
        if (lane == 0) red[wave][q] = s;
    }
    __syncthreads();
    if (t < NC) pout[t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// the host side of one input's constants; false: a negative or non-finite variance
static bool sens_constants(const double *w, const double *s, int d, double *c)
{
    int na = 0;
    for (int l = 0; l < d; ++l) {
        const double sg = s[l], om = w[l];
        if (!(sg >= 0.0) || !std::isfinite(sg)) return false;
        const double ws = om * sg;
        c[l] = -0.5 * log1p(ws);
        c[d + l] = 0.5 * om / (1.0 + ws);
        c[2 * d + l] = -1.0;
        if (sg > 0.0) {
            c[2 * d + l] = (double)na;
            c[3 * d + na] = -0.5 * log1p(2.0 * ws);
            c[4 * d + na] = 0.25 * om;
            c[5 * d + na] = 0.25 * om / (1.0 + 2.0 * ws);
            ++na;
        }
    }
    for (int q = na; q < d; ++q) c[3 * d + q] = c[4 * d + q] = c[5 * d + q] = 0.0;
    c[SEN_CROWS * d] = (double)na;
    c[SEN_CROWS * d + 1] = 0.0;
    return true;
}

static int64_t sens_env_count(const char *name, int64_t dflt)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    return end == e ? dflt : (int64_t)v;
}

// GPX_SENS_CHUNK (read at every call): the most inputs of a chunk; default: what 2^27 doubles (1 GiB) of per-point data hold, at most 4096
extern "C" int gpx_sensitivity_many(gpx_handle *h, const double *U, const double *S, int s_shared, int64_t b, double *mean, double *var_mean,
                                    double *first, double *total)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_sensitivity_many");   // the closed form is the ARD squared-exponential kernel's: names the kernel the handle holds
    if (b < 0 || (b > 0 && (!U || !S || !mean || !var_mean || !first))) { gpx_set_error("gpx_sensitivity_many: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (b == 0) return 0;
    const int d = h->d;
    const int64_t n = h->n, np = h->npad, cbs = sens_cb_size(d), ns = s_shared ? 1 : b;
    const bool want_total = total != nullptr;
    hipStream_t s = h->stream;

    // every variance is checked, and every input's constants formed, before the first launch
    std::vector<double> Sh, cbh, rm, rv, rf, rt, oh;
    std::vector<int> nah;
    try {
        Sh.resize((size_t)(ns * d));
        cbh.resize((size_t)(ns * cbs));
        nah.resize((size_t)ns);
        rm.resize((size_t)b);
        rv.assign((size_t)b, 0.0);
        rf.assign((size_t)(b * d), 0.0);
        if (want_total) rt.assign((size_t)(b * d), 0.0);
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_TRY(fetch_small(Sh.data(), S, Sh.size()));
    for (int64_t i = 0; i < ns; ++i) {
        if (!sens_constants(h->w, &Sh[(size_t)(i * d)], d, &cbh[(size_t)(i * cbs)])) {
            gpx_set_error("gpx_sensitivity_many: the variances of input %ld are not all finite and >= 0", (long)i);
            return GPX_ERR_BAD_ARG;
        }
        nah[(size_t)i] = (int)cbh[(size_t)(i * cbs + SEN_CROWS * d)];
    }

    const int64_t per = (3 * (int64_t)d + 2) * np, nrb = np / SEN_R, nbb = (np + 255) / 256;
    int64_t chunk = std::min<int64_t>(4096, std::max<int64_t>(1, ((int64_t)1 << 27) / per));
    const int64_t forced = sens_env_count("GPX_SENS_CHUNK", 0);
    if (forced > 0) chunk = std::min<int64_t>(forced, 4096);
    chunk = std::min(chunk, b);
    const int max_sweeps = (d + SEN_KC - 1) / SEN_KC;
    const int64_t max_cols = chunk * max_sweeps * SEN_NC;

    Scratch sc(s);
    double *pd = nullptr, *cbd = nullptr, *ud = nullptr, *part = nullptr, *mpart = nullptr, *od = nullptr;
    GPX_TRY(sc.take(&pd, chunk * per));
    GPX_TRY(sc.take(&cbd, ns * cbs));
    GPX_TRY(sc.take(&ud, chunk * d));
    GPX_TRY(sc.take(&part, nrb * max_cols));
    GPX_TRY(sc.take(&mpart, nbb * chunk));
    GPX_TRY(sc.take(&od, max_cols + chunk));
    try { oh.resize((size_t)(max_cols + chunk)); } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpyAsync(cbd, cbh.data(), sizeof(double) * cbh.size(), hipMemcpyHostToDevice, s));
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0);
        double *aT = pd, *mT = aT + bc * d * np, *loT = mT + bc * d * np, *g = loT + bc * d * np, *bw = g + bc * np;
        const double *cbc = s_shared ? cbd : cbd + b0 * cbs;
        const long cb_stride = s_shared ? 0 : (long)cbs;
        int na_max = 0;
        for (int64_t i = 0; i < bc; ++i) na_max = std::max(na_max, nah[(size_t)(s_shared ? 0 : b0 + i)]);
        const int sweeps = (na_max + SEN_KC - 1) / SEN_KC;
        const int64_t ncols = bc * sweeps * SEN_NC;
        GPX_HIP(hipMemcpyAsync(ud, U + b0 * d, sizeof(double) * bc * d, hipMemcpyDefault, s));
        {
            // the build is timed in the class of the N-fold builders' sums (GPX_K_QUAD), the pair pass in GPX_K_EXACT: tools/probe_sensitivity.py
            ProfScope ps(&h->prof, s, GPX_K_QUAD, (double)n * (double)bc * (60.0 * d + 60.0));
            hipLaunchKernelGGL(sens_build_kernel, dim3((unsigned)nbb, (unsigned)bc), dim3(256), 0, s, (const double *)h->x, (long)n, (long)np, d,
                               (const double *)ud, cbc, cb_stride, (const double *)h->alpha, h->v, aT, mT, loT, g, bw, mpart);
            GPX_HIP(hipGetLastError());
        }
        GPX_TRY(launch_sum_columns(mpart, nbb, (int)bc, od + ncols, s));
        if (sweeps > 0) {
            {
                // na exponentials per visited pair and sweep
                ProfScope ps(&h->prof, s, GPX_K_EXACT, 0.5 * (double)n * (double)n * (double)bc * sweeps * (25.0 * na_max + 40.0));
                const dim3 grid((unsigned)nrb, (unsigned)sweeps, (unsigned)bc);
                if (want_total)
                    hipLaunchKernelGGL(sens_pair_kernel<true>, grid, dim3(256), 0, s, (const double *)aT, (const double *)mT, (const double *)loT,
                                       (const double *)g, (const double *)bw, cbc, cb_stride, (long)n, (long)np, d, part, (long)ncols);
                else
                    hipLaunchKernelGGL(sens_pair_kernel<false>, grid, dim3(256), 0, s, (const double *)aT, (const double *)mT, (const double *)loT,
                                       (const double *)g, (const double *)bw, cbc, cb_stride, (long)n, (long)np, d, part, (long)ncols);
                GPX_HIP(hipGetLastError());
            }
            GPX_TRY(launch_sum_columns(part, nrb, (int)ncols, od, s));
        }
        GPX_HIP(hipMemcpyAsync(oh.data(), od, sizeof(double) * (ncols + bc), hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));        // one per chunk: the next chunk reuses od
        for (int64_t i = 0; i < bc; ++i) {
            const double *c = &cbh[(size_t)((s_shared ? 0 : b0 + i) * cbs)];
            const int na = nah[(size_t)(s_shared ? 0 : b0 + i)];
            rm[(size_t)(b0 + i)] = oh[(size_t)(ncols + i)];
            if (na == 0) continue;               // no uncertain coordinate: V, first and total stay 0.0
            const double *o = &oh[(size_t)(i * sweeps * SEN_NC)];
            rv[(size_t)(b0 + i)] = o[0];         // sweep 0's V (every sweep forms the same sum)
            for (int l = 0; l < d; ++l) {
                const int q = (int)c[2 * d + l];
                if (q < 0) continue;
                const double *oq = o + (q / SEN_KC) * SEN_NC;
                rf[(size_t)((b0 + i) * d + l)] = oq[1 + q % SEN_KC];
                if (want_total) rt[(size_t)((b0 + i) * d + l)] = oq[1 + SEN_KC + q % SEN_KC];
            }
        }
    }
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_sensitivity_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpy(mean, rm.data(), sizeof(double) * b, hipMemcpyDefault));
    GPX_HIP(hipMemcpy(var_mean, rv.data(), sizeof(double) * b, hipMemcpyDefault));
    GPX_HIP(hipMemcpy(first, rf.data(), sizeof(double) * b * d, hipMemcpyDefault));
    if (want_total) GPX_HIP(hipMemcpy(total, rt.data(), sizeof(double) * b * d, hipMemcpyDefault));
    return 0;
}
