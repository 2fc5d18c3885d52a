// sensitivity_box.hip -- the variance decomposition of the predictor mean, its moments and E[k^T K^-1 k] under independent UNIFORM inputs
// over a box (gpx_sensitivity_box_many; include/gpx.h carries the formulas).  No reference counterpart: the reference integrates with nquad
// (skgpuppy/UncertaintyPropagation.py:135-210).  Host frame, chunking and the pair frame are sensitivity.hip's; the per-slot factor is new.
//
// x_k ~ U(lo_k, hi_k) independent, L_k = hi_k - lo_k; mu(x) = sum_i beta_i c_i(x) with the PLAIN kernel c_i(x) = v exp(-1/2 sum_k w_k
// (x_k - x_ik)^2) (no +vt, as in sensitivity.hip).  D(A, B) = erf(B) - erf(A) (erf_diff.h).  For an active coordinate (L_k > 0), om = w_k:
//   m_ik     = sqrt(pi / (2 om)) / L_k D(sqrt(om / 2) (lo_k - x_ik), sqrt(om / 2) (hi_k - x_ik))                     E[factor k of c_i]
//   E_k(i,j) = exp(-1/4 om (x_ik - x_jk)^2) 1/2 sqrt(pi / om) / L_k D(sqrt(om) (lo_k - mid), sqrt(om) (hi_k - mid))   E[factor k of c_i c_j]
//              mid = (x_ik + x_jk) / 2
//   mean    = v sum_i beta_i prod_k m_ik
//   V       = sum_ij b_ij (prod_k E_k - prod_k m_ik m_jk)                     b_ij = v^2 beta_i beta_j
//   first_k = sum_ij b_ij (prod_{l != k} m_il m_jl) (E_k - m_ik m_jk)
//   total_k = sum_ij b_ij (prod_{l != k} E_l) (E_k - m_ik m_jk)
//   quad    = v^2 sum_ij Kinv_ij prod_k E_k                                   E[k(x)^T K^-1 k(x)]
// A coordinate with L_k = 0 is pinned at lo_k and INACTIVE as s_k = 0 is in sensitivity.hip: its factor exp(-1/2 w_k (lo_k - x_ik)^2) is
// folded into the point weights kw_i = v prod_inactive and bw_i = kw_i beta_i, its first_k / total_k are 0.0 exactly, and the pair pass
// runs over the na active coordinates, compacted into slots 0..na-1.
//
// WHAT DIFFERS FROM THE GAUSSIAN LAW.  m_ik and E_k are no exponentials of a sum: a point outside the box has them through erfc, down to
// exactly 0.0 from ~26.5 / sqrt(om) outside on, so nothing is kept in log form and nothing is divided:
//   * the build kernel stores, per (input, point, slot), the SCALED offset al = sqrt(om) (lo - x_ik): a pair's lower argument is the mean
//     (al_i + al_j) / 2 of two stored numbers and its exponent is -1/4 (al_i - al_j)^2, no multiply by sqrt(om) in the pair pass.  The upper
//     argument is NOT stored: D takes the lower argument and the scaled width h = sqrt(om) L, a constant of the slot formed from L itself
//     (erf_diff.h: the difference of two rounded offsets would lose the digits the narrow-box expansion keeps).  Then m_ik; and the
//     leave-one-out product lo_ik = prod_{l != k} m_il by a prefix pass and a
//     suffix pass over the slots (the thread reads its own m back); then g_i = prod m_ik, bw_i, kw_i and the mean's block partials.
//   * the pair kernel keeps sensitivity.hip's frame -- a workgroup owns SEN_R rows i in LDS, a lane owns column j read slot-major, pairs
//     j <= i with weight 2 / 1, heavy row blocks first, sweeps of SEN_KC slots on grid.y, inputs on grid.z -- but ONE rolled loop over all
//     slots evaluates the factor (one exp, one D, the product with 1/2 sqrt(pi / om) / L) per (row, slot): the erf / erfc bodies are
//     inlined once, not once per unrolled slot.  A slot outside the sweep multiplies into a running product, a slot of the sweep is parked
//     in LDS (each lane reads its own word back) for the unrolled prefix / suffix products and the 2 SEN_KC + 2 accumulations.
//   * QUAD (sweep 0 only) reads Kinv[i][j] with the lane on j, lower triangle, same weights; without it no K^-1 is read or needed.
// No atomics, fixed summation order: partials per block, one launch_sum_columns per chunk.
#include <cmath>
#include <cstring>

#include "common.h"
#include "erf_diff.h"

constexpr int BOX_NC = 2 * SEN_KC + 2;    // sums per sweep: V, first and total of the sweep's slots, quad (sweep 0)
// the constants of one input (host, box_constants): rows [d] each -- 0 slot_l (-1: inactive) by coordinate l; 1 sqrt(om), 2 1/2 sqrt(pi / om) / L,
// 3 sqrt(pi / (2 om)) / L, 4 the scaled width sqrt(om) L (the h of erf_diff: from L itself, never from two rounded offsets) by active slot q; then na
// (BOX_CROWS = 5 rows, box_cb_size: common.h, shared with sensitivity_box_second.hip)

// per (input z, point i): alT / mT / loT [z][slot][npad], g / bw / kw [z][npad]; mpart [block][input] = the block's share of the mean
__global__ __launch_bounds__(256) void box_build_kernel(const double *__restrict__ x, long n, long npad, int d, const double *__restrict__ lo_all,
                                                        long lo_stride, const double *__restrict__ w, const double *__restrict__ cb, long cb_stride,
                                                        const double *__restrict__ beta, double v, double *__restrict__ alT,
                                                        double *__restrict__ mT, double *__restrict__ loT,
                                                        double *__restrict__ g, double *__restrict__ bw, double *__restrict__ kw,
                                                        double *__restrict__ mpart)
{
    __shared__ double ws[4];
    const int t = threadIdx.x;
    const long z = blockIdx.y, i = (long)blockIdx.x * 256 + t;
    const double *c = cb + z * cb_stride, *lo = lo_all + z * lo_stride;
    const int na = (int)c[BOX_CROWS * d];
    const long base = z * (long)d * npad;
    double mine = 0.0;
    if (i < npad && i >= n) {                 // padding: a pair with such a row weighs 0.0, its factors are finite
        for (int q = 0; q < na; ++q) alT[base + q * npad + i] = mT[base + q * npad + i] = loT[base + q * npad + i] = 0.0;
        g[z * npad + i] = bw[z * npad + i] = kw[z * npad + i] = 0.0;
    } else if (i < n) {
        double lin = 0.0, pre = 1.0;          // the pinned coordinates' exponent; prod of the m before the slot
        for (int l = 0; l < d; ++l) {
            const int q = (int)c[l];
            const double xl = x[i * d + l], dlo = lo[l] - xl;
            if (q < 0) { lin = fma(-0.5 * w[l] * dlo, dlo, lin); continue; }
            const double al = c[d + q] * dlo;
            const double m = c[3 * d + q] * erf_diff(al * 0.70710678118654752, c[4 * d + q] * 0.70710678118654752);
            alT[base + q * npad + i] = al;
            mT[base + q * npad + i] = m;
            loT[base + q * npad + i] = pre;
            pre *= m;
        }
        double suf = 1.0;                     // prod of the m after the slot: no division, an m that is 0.0 stays out of its own lo
        for (int q = na - 1; q >= 0; --q) {
            loT[base + q * npad + i] *= suf;
            suf *= mT[base + q * npad + i];
        }
        const double k0 = v * exp_nonpos(lin), b0 = k0 * beta[i];
        g[z * npad + i] = pre;
        kw[z * npad + i] = k0;
        bw[z * npad + i] = b0;
        mine = b0 * pre;
    }
    mine = wave_sum(mine);
    if ((t & 63) == 0) ws[t >> 6] = mine;
    __syncthreads();
    if (t == 0) mpart[(long)blockIdx.x * gridDim.y + z] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// E of one slot for the pair of points with scaled offsets al_i, al_j; ce = 1/2 sqrt(pi / om) / L, h = sqrt(om) L
static __device__ __forceinline__ double box_e(double ali, double alj, double ce, double h)
{
#pragma clang fp contract(off)
    const double dm = ali - alj;
    return (exp_nonpos(-0.25 * dm * dm) * ce) * erf_diff(0.5 * ali + 0.5 * alj, h);
}

// partial [row block][ncols], ncols = inputs * sweeps * BOX_NC: this block's [V, first (SEN_KC), total (SEN_KC), quad] at (z * sweeps + y) * BOX_NC
template <bool TOTAL, bool QUAD>
__global__ __launch_bounds__(256, 2) void box_pair_kernel(const double *__restrict__ alT,
                                                          const double *__restrict__ mT, const double *__restrict__ loT,
                                                          const double *__restrict__ g, const double *__restrict__ bw,
                                                          const double *__restrict__ kw, const double *__restrict__ cb, long cb_stride,
                                                          const double *__restrict__ Kinv, long ldk, long n, long npad, int d,
                                                          double *__restrict__ partial, long ncols)
{
#pragma clang fp contract(off)   // every instantiation must give the sums it shares with the others the same bits
    constexpr int R = SEN_R, KC = SEN_KC, NC = BOX_NC;
    __shared__ double als[R][GPX_MAX_D];      // al_i of the block's rows, by slot (broadcast reads)
    __shared__ double os[R][KC][2];           // m_i, lo_i of the sweep's own slots
    __shared__ double rs[R][3];               // g_i, bw_i, kw_i
    __shared__ double red[4][NC];
    __shared__ double oe[KC][256];            // E of the sweep's own slots for the row in hand: each lane parks and reads back its own words
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int rb = gridDim.x - 1 - blockIdx.x;
    const long i0 = (long)rb * R, z = blockIdx.z;
    const int sweeps = gridDim.y, y = blockIdx.y, k0 = y * KC;
    const double *c = cb + z * cb_stride;
    const int na = (int)c[BOX_CROWS * d];
    const double *ce = c + 2 * d, *hq = c + 4 * d;
    double *pout = partial + (long)rb * ncols + (z * sweeps + y) * NC;
    if (k0 >= na && y > 0) {                  // an input with fewer active slots than the chunk's widest: nothing in this sweep
        if (t < NC) pout[t] = 0.0;
        return;
    }
    const long base = z * (long)d * npad;
    const double *alZ = alT + base, *mZ = mT + base, *loZ = loT + base;
    for (int q = t; q < R * GPX_MAX_D; q += 256) {
        const int r = q / GPX_MAX_D, k = q - r * GPX_MAX_D;
        als[r][k] = (k < na) ? alZ[(long)k * npad + i0 + r] : 0.0;
    }
    if (t < R * KC) {
        const int r = t / KC, kk = t - r * KC;
        const bool own = k0 + kk < na;
        os[r][kk][0] = own ? mZ[(long)(k0 + kk) * npad + i0 + r] : 1.0;
        os[r][kk][1] = own ? loZ[(long)(k0 + kk) * npad + i0 + r] : 0.0;
    }
    if (t < R) { rs[t][0] = g[z * npad + i0 + t]; rs[t][1] = bw[z * npad + i0 + t]; rs[t][2] = kw[z * npad + i0 + t]; }
    __syncthreads();

    double acc[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) acc[q] = 0.0;
    const int k1 = (k0 + KC < na) ? k0 + KC : na;
    const long jend = (i0 + R < n) ? i0 + R : n;
    for (long j = t; j < jend; j += 256) {
        double mj[KC], lj[KC];                // m_j, lo_j of the sweep's own slots
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            const bool own = k0 + kk < na;
            mj[kk] = own ? mZ[(long)(k0 + kk) * npad + j] : 1.0;
            lj[kk] = own ? loZ[(long)(k0 + kk) * npad + j] : 0.0;
        }
        const double gj = g[z * npad + j], bj = bw[z * npad + j], kj = kw[z * npad + j];
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            const long i = i0 + r;
            const double wgt = (j < i) ? 2.0 : ((j == i) ? 1.0 : 0.0);
            const double b = (rs[r][1] * bj) * wgt;
            double pre = 1.0;                 // prod E over the slots outside the sweep
#pragma unroll 1
            for (int q = 0; q < na; ++q) {
                const long at = (long)q * npad + j;
                const double e = box_e(als[r][q], alZ[at], ce[q], hq[q]);
                if (q >= k0 && q < k1) oe[q - k0][t] = e;
                else pre *= e;
            }
            double E[KC], dl[KC];
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) {
                E[kk] = 1.0;
                dl[kk] = 0.0;
                if (k0 + kk < na) {
                    E[kk] = oe[kk][t];
                    dl[kk] = E[kk] - os[r][kk][0] * mj[kk];
                    acc[1 + kk] = fma(b * (os[r][kk][1] * lj[kk]), dl[kk], acc[1 + kk]);
                }
            }
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
            if (QUAD && y == 0) {
                const double kij = (i < n) ? Kinv[i * ldk + j] : 0.0;
                acc[NC - 1] = fma(((rs[r][2] * kj) * wgt) * kij, pre, acc[NC - 1]);
            }
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

// the host side of one input's constants; 0: fine, else the offending coordinate + 1 (lo > hi, a non-finite bound, or a width whose
// normalisers 1 / L are not finite)
int box_constants(const double *w, const double *lo, const double *hi, int d, double *c)
{
    int na = 0;
    for (int l = 0; l < d; ++l) {
        const double L = hi[l] - lo[l], om = w[l];
        if (!std::isfinite(lo[l]) || !std::isfinite(hi[l]) || !(L >= 0.0) || !std::isfinite(L)) return l + 1;
        c[l] = -1.0;
        if (L > 0.0) {
            c[l] = (double)na;
            c[d + na] = sqrt(om);
            c[2 * d + na] = 0.5 * sqrt(M_PI / om) / L;
            c[3 * d + na] = sqrt(M_PI / (2.0 * om)) / L;
            c[4 * d + na] = sqrt(om) * L;
            if (!std::isfinite(c[2 * d + na]) || !std::isfinite(c[3 * d + na])) return l + 1;
            ++na;
        }
    }
    for (int q = na; q < d; ++q) c[d + q] = c[2 * d + q] = c[3 * d + q] = c[4 * d + q] = 0.0;
    c[BOX_CROWS * d] = (double)na;
    c[BOX_CROWS * d + 1] = 0.0;
    return 0;
}

using BoxPairKernel = void (*)(const double *, const double *, const double *, const double *, const double *, const double *,
                               const double *, long, const double *, long, long, long, int, double *, long);

// Inputs run in chunks as in gpx_sensitivity_many (sens_chunk: GPX_SENS_CHUNK, read at every call)
extern "C" int gpx_sensitivity_box_many(gpx_handle *h, const double *lo, const double *hi, int box_shared, int64_t b, double *mean,
                                        double *var_mean, double *first, double *total, double *quad)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_sensitivity_box_many");   // the closed form is the ARD squared-exponential kernel's: names the kernel the handle holds
    if (b < 0 || (b > 0 && (!lo || !hi || !mean || !var_mean || !first))) { gpx_set_error("gpx_sensitivity_box_many: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (b == 0) return 0;
    const int d = h->d;
    const int64_t n = h->n, np = h->npad, cbs = box_cb_size(d), ns = box_shared ? 1 : b;
    const bool want_total = total != nullptr, want_quad = quad != nullptr;
    hipStream_t s = h->stream;

    // every box is checked, and every input's constants formed, before the first launch
    std::vector<double> loh, hih, cbh, rm, rv, rf, rt, rq, oh;
    std::vector<int> nah;
    try {
        loh.resize((size_t)(ns * d));
        hih.resize((size_t)(ns * d));
        cbh.resize((size_t)(ns * cbs));
        nah.resize((size_t)ns);
        rm.resize((size_t)b);
        rv.assign((size_t)b, 0.0);
        rf.assign((size_t)(b * d), 0.0);
        if (want_total) rt.assign((size_t)(b * d), 0.0);
        if (want_quad) rq.assign((size_t)b, 0.0);
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_box_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_TRY(fetch_small(loh.data(), lo, loh.size()));
    GPX_TRY(fetch_small(hih.data(), hi, hih.size()));
    for (int64_t i = 0; i < ns; ++i) {
        const int bad = box_constants(h->w, &loh[(size_t)(i * d)], &hih[(size_t)(i * d)], d, &cbh[(size_t)(i * cbs)]);
        if (bad) {
            gpx_set_error("gpx_sensitivity_box_many: the bounds of input %ld are not finite with lo <= hi and a representable width (coordinate %d)",
                          (long)i, bad - 1);
            return GPX_ERR_BAD_ARG;
        }
        nah[(size_t)i] = (int)cbh[(size_t)(i * cbs + BOX_CROWS * d)];
    }
    if (want_quad) GPX_TRY(ensure_kinv(h));   // a pseudo-input handle holds P there from the start

    const int64_t per = (3 * (int64_t)d + 3) * np, nrb = np / SEN_R, nbb = (np + 255) / 256;
    const int64_t chunk = sens_chunk(per, b);
    const int max_sweeps = std::max(1, (d + SEN_KC - 1) / SEN_KC);
    const int64_t max_cols = chunk * max_sweeps * BOX_NC;

    Scratch sc(s);
    double *pd = nullptr, *cbd = nullptr, *lod = nullptr, *part = nullptr, *mpart = nullptr, *od = nullptr;
    GPX_TRY(sc.take(&pd, chunk * per));
    GPX_TRY(sc.take(&cbd, ns * cbs));
    GPX_TRY(sc.take(&lod, chunk * d));
    GPX_TRY(sc.take(&part, nrb * max_cols));
    GPX_TRY(sc.take(&mpart, nbb * chunk));
    GPX_TRY(sc.take(&od, max_cols + chunk));
    try { oh.resize((size_t)(max_cols + chunk)); } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_box_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpyAsync(cbd, cbh.data(), sizeof(double) * cbh.size(), hipMemcpyHostToDevice, s));
    static const BoxPairKernel kernels[2][2] = {{box_pair_kernel<false, false>, box_pair_kernel<false, true>},
                                                {box_pair_kernel<true, false>, box_pair_kernel<true, true>}};
    const BoxPairKernel pair = kernels[want_total][want_quad];
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0);
        double *alT = pd, *mT = alT + bc * d * np, *loT = mT + bc * d * np, *g = loT + bc * d * np, *bw = g + bc * np,
               *kw = bw + bc * np;
        const double *cbc = box_shared ? cbd : cbd + b0 * cbs;
        const long cb_stride = box_shared ? 0 : (long)cbs, lo_stride = box_shared ? 0 : (long)d;
        int na_max = 0;
        for (int64_t i = 0; i < bc; ++i) na_max = std::max(na_max, nah[(size_t)(box_shared ? 0 : b0 + i)]);
        // all coordinates pinned: V, first and total are 0.0 and no pair pass runs -- unless quad is asked for (its product of E is then 1)
        const int sweeps = std::max((na_max + SEN_KC - 1) / SEN_KC, want_quad ? 1 : 0);
        const int64_t ncols = bc * sweeps * BOX_NC;
        // the chunk's lower bounds from the caller's pointer, host or device (hi enters through the constants alone)
        if (!box_shared || b0 == 0) GPX_HIP(hipMemcpyAsync(lod, lo + (box_shared ? 0 : b0 * d), sizeof(double) * (box_shared ? 1 : bc) * d, hipMemcpyDefault, s));
        {
            // timed in the classes of the Gaussian call: the build in GPX_K_QUAD, the pair pass in GPX_K_EXACT
            ProfScope ps(&h->prof, s, GPX_K_QUAD, (double)n * (double)bc * (300.0 * d + 60.0));
            hipLaunchKernelGGL(box_build_kernel, dim3((unsigned)nbb, (unsigned)bc), dim3(256), 0, s, (const double *)h->x, (long)n, (long)np, d,
                               (const double *)lod, lo_stride, (const double *)h->wdev, cbc, cb_stride, (const double *)h->alpha, h->v, alT, mT, loT, g, bw,
                               kw, mpart);
            GPX_HIP(hipGetLastError());
        }
        GPX_TRY(launch_sum_columns(mpart, nbb, (int)bc, od + ncols, s));
        if (sweeps > 0) {
            {
                // na factors (one exp, two erf or erfc) per visited pair and sweep
                ProfScope ps(&h->prof, s, GPX_K_EXACT, 0.5 * (double)n * (double)n * (double)bc * sweeps * (300.0 * na_max + 40.0));
                hipLaunchKernelGGL(pair, dim3((unsigned)nrb, (unsigned)sweeps, (unsigned)bc), dim3(256), 0, s, (const double *)alT,
                                   (const double *)mT, (const double *)loT, (const double *)g, (const double *)bw,
                                   (const double *)kw, cbc, cb_stride, (const double *)h->Kinv, (long)np, (long)n, (long)np, d, part, (long)ncols);
                GPX_HIP(hipGetLastError());
            }
            GPX_TRY(launch_sum_columns(part, nrb, (int)ncols, od, s));
        }
        GPX_HIP(hipMemcpyAsync(oh.data(), od, sizeof(double) * (ncols + bc), hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));        // one per chunk: the next chunk reuses od
        for (int64_t i = 0; i < bc; ++i) {
            const double *c = &cbh[(size_t)((box_shared ? 0 : b0 + i) * cbs)];
            const int na = nah[(size_t)(box_shared ? 0 : b0 + i)];
            rm[(size_t)(b0 + i)] = oh[(size_t)(ncols + i)];
            if (sweeps == 0) continue;
            const double *o = &oh[(size_t)(i * sweeps * BOX_NC)];
            if (want_quad) rq[(size_t)(b0 + i)] = o[BOX_NC - 1];
            if (na == 0) continue;               // no uncertain coordinate: V, first and total stay 0.0
            rv[(size_t)(b0 + i)] = o[0];         // sweep 0's V (every sweep forms the same sum)
            for (int l = 0; l < d; ++l) {
                const int q = (int)c[l];
                if (q < 0) continue;
                const double *oq = o + (q / SEN_KC) * BOX_NC;
                rf[(size_t)((b0 + i) * d + l)] = oq[1 + q % SEN_KC];
                if (want_total) rt[(size_t)((b0 + i) * d + l)] = oq[1 + SEN_KC + q % SEN_KC];
            }
        }
    }
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_sensitivity_box_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpy(mean, rm.data(), sizeof(double) * b, hipMemcpyDefault));
    GPX_HIP(hipMemcpy(var_mean, rv.data(), sizeof(double) * b, hipMemcpyDefault));
    GPX_HIP(hipMemcpy(first, rf.data(), sizeof(double) * b * d, hipMemcpyDefault));
    if (want_total) GPX_HIP(hipMemcpy(total, rt.data(), sizeof(double) * b * d, hipMemcpyDefault));
    if (want_quad) GPX_HIP(hipMemcpy(quad, rq.data(), sizeof(double) * b, hipMemcpyDefault));
    return 0;
}
