// sensitivity_second.hip -- the second-order (pair interaction) Sobol terms of the predictor mean under independent Gaussian inputs, on
// v_mfma_f64_16x16x4_f64 (gpx_sensitivity_second_many; include/gpx.h carries the formulas).  No reference counterpart.
//
// Notation of sensitivity.hip: a_ik = u_k - x_ik, lm_ik = log m_ik, E_k(i,j), b_ij = v^2 beta_i beta_j, pairs j <= i with weight 2 / 1,
// the coordinates with s_k > 0 compacted into slots 0..na-1, the others folded into the point weight bw_i.  For k != l
//   second_kl = sum_ij b_ij (prod_{q != k,l} m_iq m_jq) (E_k - m_ik m_jk) (E_l - m_il m_jl)  =  V^closed_{kl} - first_k - first_l,
// the variance of the ANOVA term in (x_k, x_l).  All na (na - 1) / 2 of these sums are the Gram matrix of na vectors indexed by the pairs
// (i, j): a na x na x N^2 product, which the matrix core does.
//
// THE FORM THAT SHIPPED keeps every exponent non-positive.  The leave-two-out product separates as h_ik h_il with
// h_ik = exp(1/2 lact_i - lm_ik), lact_i = sum of lm over the active slots -- but h_ik alone overflows for a point far from u in coordinate
// k only, and is never formed.  Per (pair, slot) cell
//   dh_k(i,j) = h_ik h_jk (E_k - m_ik m_jk) = exp(e1) - sg_i sg_j,   sg_i = exp(hl_i), hl_i = 1/2 lact_i            (per point)
//   e1 = hl_i + hl_j + (lE_k - lm_ik - lm_jk)
//   lE_k - lm_ik - lm_jk = cc + cD (a_i - a_j)^2 + cS (a_i + a_j)^2        with, ws = om sg,
//       cc = log1p(ws) - 1/2 log1p(2 ws),  cD = -1/4 om ws / (1 + ws) <= 0,  cS = 1/4 om ws / ((1 + ws)(1 + 2 ws)) >= 0
//   (from lE_k = c0 - P dm^2 - Q sm^2, lm_i + lm_j = 2 lmc - lma (dm^2 + sm^2) / 2: ONE quadratic form with host-side coefficients, not a
//   difference of two evaluated logs), and second_kl = sum_pairs (wgt bw_i bw_j dh_k) dh_l.
// Sign of e1: Cauchy-Schwarz on E[f_i f_j] gives E_k(i,j)^2 <= E_k(i,i) E_k(j,j); the factor f lies in [0, 1], so f^2 <= f and
// E_k(i,i) <= m_ik; hence lE_k <= 1/2 (lm_ik + lm_jk) and e1 <= 1/2 sum_{q != k} (lm_iq + lm_jq) <= 0 ALWAYS: exp_nonpos(fmin(e1, 0.0)) is
// exact in intent, as the build kernel of sensitivity.hip does for lo.
// Rounding: where |1/2 lact_i - lm_ik| is large (a point far in coordinate k alone) the positive cS term cancels against hl_i + hl_j and
// the k cell carries a relative error of about that magnitude times u.  Every partner cell l != k of the same pair is then below
// exp(-that magnitude) (its e1 keeps lm_ik): the product is far under the rule's floor on the scale of the sum.
//
// Build kernel: per (input, point) POINT-major a [npad][W], W = 16 ceil(d / 16) (the slots of a point are consecutive, zero padded: four
// points x 16 slots is one 512-byte wave load), and hl, sg, bw [npad].  The slot compaction and the s = 0 folding are sens_constants'.
// Pair kernel: a workgroup owns S2_R rows i in LDS, its four waves walk the columns j <= i, 4 PACK at a time; lane (k = lane % 16,
// p = lane / 16) owns slot k of pair (i, j + p), keeps a_jk, hl_j, sg_j, bw_j in registers across the rows and reads the row side from LDS
// (16 addresses broadcast four ways).  ONE exponential per lane and block of 16 slots.  Its wgt bw_i bw_j dh_k is the A operand
// [row = lane % 16][kk = lane / 16], its dh_k the B operand [kk = lane / 16][col = lane % 16] of the same MFMA (the layouts of leaf.h /
// gemm.hip: the accumulator's entry r of a lane is D[4 r + lane / 16][lane % 16]): no data moves between lanes.  The accumulator's
// off-diagonal entries are second_kl, its diagonal is dropped.
//   na > 16: NB = ceil(na / 16) blocks, NB (NB + 1) / 2 accumulators (A from block al, B from block be >= al).
//   na <= 8 / <= 4: PACK = 2 / 4 pair groups share the 16 rows -- rows g SL .. g SL + SL - 1 (SL = 16 / PACK) are the pairs j + 4 g .. j + 4 g + 3;
//   the PACK diagonal SL x SL blocks are kept and added in the order of g (host), the cross blocks dropped.  na <= 1: no launch, zeros.
// The variant is chosen by an input's OWN na (a chunk's inputs are launched by variant through an index list), weights 0 and the zero bw
// of padded points mask the tail, the waves' accumulators go through LDS in a fixed order to partial [row block][input's columns], then
// ONE launch_sum_columns per chunk; the host scatters through the slot map.  No atomics: an input's result depends neither on its place
// in the batch nor on the chunking.
#include <cmath>
#include <cstring>

#include "common.h"

// S2_R rows per workgroup, the S2_NV variants (NB, PACK) and their column arithmetic: common.h (shared with sensitivity_box_second.hip)
constexpr int S2_CQ = 3 * GPX_MAX_D + 2;  // an input's pair constants: cc, cD, cS by active slot [GPX_MAX_D each], na, 0

// per (input z, point i): a [z][npad][W] by slot (zero from na on), pt [z][3][npad] = hl, sg, bw
__global__ __launch_bounds__(256) void sens2_build_kernel(const double *__restrict__ x, long n, long npad, int d, int W, const double *__restrict__ U,
                                                          const double *__restrict__ cb, long cb_stride, const double *__restrict__ beta, double v,
                                                          double *__restrict__ a2, double *__restrict__ pt)
{
    const long z = blockIdx.y, i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    const double *c = cb + z * cb_stride, *u = U + z * d;
    const int na = (int)c[SEN_CROWS * d];
    const bool real = i < n;
    double *row = a2 + (z * npad + i) * W;
    double lall = 0.0, lact = 0.0;
    for (int l = 0; l < d; ++l) {
        const double a = real ? u[l] - x[i * d + l] : 0.0;
        const double lm = real ? fma(-c[d + l] * a, a, c[l]) : 0.0;
        const int q = (int)c[2 * d + l];
        lall += lm;
        if (q >= 0) { lact += lm; row[q] = a; }
    }
    for (int q = na; q < W; ++q) row[q] = 0.0;
    const double hl = 0.5 * lact, b0 = real ? v * beta[i] : 0.0;
    double *p = pt + z * 3 * npad + i;
    p[0] = hl;
    p[npad] = exp_nonpos(hl);
    p[2 * npad] = b0 * exp_nonpos(fmin(lall - lact, 0.0));       // the inactive coordinates' plain kernel factors
}

// partial [row block][ncols]: this block's NACC accumulators at the input's column offset, entry a 256 + 64 r + lane = D_a[4 r + lane / 16][lane % 16]
template <int NB, int PACK>
__global__ __launch_bounds__(256, 2) void sens2_pair_kernel(const double *__restrict__ a2, const double *__restrict__ pt, const double *__restrict__ cq,
                                                            long cq_stride, const int *__restrict__ zl, long n, long npad, int W,
                                                            double *__restrict__ partial, long ncols)
{
#pragma clang fp contract(off)
    constexpr int R = S2_R, SL = 16 / PACK, CW = 4 * PACK, NACC = NB * (NB + 1) / 2, WB = 16 * NB;
    __shared__ double as[R][WB];              // a_i of the block's rows, by slot
    __shared__ double rs[R][4];               // hl_i, sg_i, bw_i
    __shared__ double red[4][256];
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int k = lane & 15, p = lane >> 4, slot = k % SL, grp = k / SL;
    const int rb = gridDim.x - 1 - blockIdx.x;                   // heavy row blocks first
    const long i0 = (long)rb * R;
    const long zi = zl[2 * blockIdx.z], co = zl[2 * blockIdx.z + 1];
    const double *c = cq + zi * cq_stride;
    const int na = (int)c[3 * GPX_MAX_D];
    const double *aZ = a2 + zi * npad * W, *pZ = pt + zi * 3 * npad;
    for (int q = t; q < R * WB; q += 256) {
        const int r = q / WB, kk = q - r * WB;
        as[r][kk] = aZ[(i0 + r) * W + kk];                       // i0 + r < npad: npad is a multiple of the 128-row tile
    }
    if (t < R) {
        rs[t][0] = pZ[i0 + t];
        rs[t][1] = pZ[npad + i0 + t];
        rs[t][2] = pZ[2 * npad + i0 + t];
    }
    __syncthreads();

    double cc[NB], cD[NB], cS[NB];
    bool ok[NB];
#pragma unroll
    for (int be = 0; be < NB; ++be) {
        const int q = 16 * be + slot;
        ok[be] = q < na;
        cc[be] = c[q];
        cD[be] = c[GPX_MAX_D + q];
        cS[be] = c[2 * GPX_MAX_D + q];
    }
    v4d acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = (v4d){0.0, 0.0, 0.0, 0.0};
    const long jend = (i0 + R < n) ? i0 + R : n;
    for (long j0 = (long)wave * CW; j0 < jend; j0 += 4 * CW) {
        const long col = j0 + 4 * grp + p;
        const bool in = col < npad;                              // no lane reads past npad
        double aj[NB];
#pragma unroll
        for (int be = 0; be < NB; ++be) aj[be] = in ? aZ[col * W + 16 * be + slot] : 0.0;
        const double hlj = in ? pZ[col] : 0.0, sgj = in ? pZ[npad + col] : 0.0, bwj = in ? pZ[2 * npad + col] : 0.0;
        const int rlo = (j0 > i0) ? (int)(j0 - i0) : 0;          // rows above it have no column of this step at or below the diagonal
        for (int r = rlo; r < R; ++r) {
            const long i = i0 + r;
            const double wgt = (col < i) ? 2.0 : ((col == i) ? 1.0 : 0.0);
            const double bb = (rs[r][2] * bwj) * wgt, ss = rs[r][1] * sgj, hh = rs[r][0] + hlj;
            double dh[NB];
#pragma unroll
            for (int be = 0; be < NB; ++be) {
                const double ai = as[r][16 * be + slot];
                const double dm = ai - aj[be], sm = ai + aj[be];
                const double e1 = hh + fma(cS[be] * sm, sm, fma(cD[be] * dm, dm, cc[be]));
                const double ex = exp_nonpos(fmin(e1, 0.0));
                dh[be] = ok[be] ? ex - ss : 0.0;
            }
#pragma unroll
            for (int be = 0; be < NB; ++be)
#pragma unroll
                for (int al = 0; al <= be; ++al)
                    acc[be * (be + 1) / 2 + al] = __builtin_amdgcn_mfma_f64_16x16x4f64(bb * dh[al], dh[be], acc[be * (be + 1) / 2 + al], 0, 0, 0);
        }
    }
    double *pout = partial + (long)rb * ncols + co;
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][64 * r + lane] = acc[q][r];
        __syncthreads();
        pout[256 * q + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
}

// cq <- the pair constants of one input from its variances (validated by sens_constants before)
static void sens2_constants(const double *w, const double *s, int d, double *cq)
{
    memset(cq, 0, sizeof(double) * S2_CQ);
    int na = 0;
    for (int l = 0; l < d; ++l) {
        if (!(s[l] > 0.0)) continue;
        const double om = w[l], ws = om * s[l];
        cq[na] = log1p(ws) - 0.5 * log1p(2.0 * ws);
        cq[GPX_MAX_D + na] = -0.25 * om * ws / (1.0 + ws);
        cq[2 * GPX_MAX_D + na] = 0.25 * om * ws / ((1.0 + ws) * (1.0 + 2.0 * ws));
        ++na;
    }
    cq[3 * GPX_MAX_D] = (double)na;
}

template <int NB, int PACK>
static void sens2_launch(dim3 grid, hipStream_t s, const double *a2, const double *pt, const double *cq, long cq_stride, const int *zl, long n,
                         long npad, int W, double *partial, long ncols)
{
    hipLaunchKernelGGL((sens2_pair_kernel<NB, PACK>), grid, dim3(256), 0, s, a2, pt, cq, cq_stride, zl, n, npad, W, partial, ncols);
}

// one input's [d, d] from its summed accumulators o [s2_cols(var)] through the slot map (row 2 of its sens_constants, row 0 of a box's)
void sens2_scatter(const double *o, int var, const double *slot_of, int d, double *out)
{
    const int pack = s2_pack(var), sl = 16 / pack;
    int coord[GPX_MAX_D];
    int na = 0;
    for (int l = 0; l < d; ++l)
        if (slot_of[l] >= 0.0) coord[(int)slot_of[l]] = l, ++na;
    auto entry = [](const double *acc, int row, int col) { return acc[64 * (row / 4) + 16 * (row % 4) + col]; };
    for (int qa = 0; qa < na; ++qa)
        for (int qb = qa + 1; qb < na; ++qb) {
            const int al = qa / 16, be = qb / 16;
            const double *acc = o + 256 * (be * (be + 1) / 2 + al);
            double val = 0.0;
            for (int g = 0; g < pack; ++g) val += entry(acc, g * sl + qa % 16, g * sl + qb % 16);   // pack == 1: the one entry
            out[coord[qa] * d + coord[qb]] = out[coord[qb] * d + coord[qa]] = val;
        }
}

extern "C" int gpx_sensitivity_second_many(gpx_handle *h, const double *U, const double *S, int s_shared, int64_t b, double *second)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_sensitivity_second_many");
    if (b < 0 || (b > 0 && (!U || !S || !second))) { gpx_set_error("gpx_sensitivity_second_many: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (b == 0) return 0;
    const int d = h->d, W = 16 * ((d + 15) / 16);
    const int64_t n = h->n, np = h->npad, cbs = sens_cb_size(d), ns = s_shared ? 1 : b;
    hipStream_t s = h->stream;

    // every variance is checked, and every input's constants and variant formed, before the first launch
    std::vector<double> Sh, cbh, cqh, res, oh;
    std::vector<int> var, zlh;
    try {
        Sh.resize((size_t)(ns * d));
        cbh.resize((size_t)(ns * cbs));
        cqh.resize((size_t)(ns * S2_CQ));
        var.resize((size_t)ns);
        zlh.resize((size_t)(2 * b));
        res.assign((size_t)(b * d * d), 0.0);
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_second_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_TRY(fetch_small(Sh.data(), S, Sh.size()));
    bool any = false;
    for (int64_t i = 0; i < ns; ++i) {
        if (!sens_constants(h->w, &Sh[(size_t)(i * d)], d, &cbh[(size_t)(i * cbs)])) {
            gpx_set_error("gpx_sensitivity_second_many: the variances of input %ld are not all finite and >= 0", (long)i);
            return GPX_ERR_BAD_ARG;
        }
        sens2_constants(h->w, &Sh[(size_t)(i * d)], d, &cqh[(size_t)(i * S2_CQ)]);
        var[(size_t)i] = s2_variant((int)cbh[(size_t)(i * cbs + SEN_CROWS * d)]);
        any = any || var[(size_t)i] >= 0;
    }
    if (!any) {                                  // no input has two uncertain coordinates: no launch, all zeros
        GPX_HIP(hipMemcpy(second, res.data(), sizeof(double) * b * d * d, hipMemcpyDefault));
        return 0;
    }

    const int64_t nrb = np / S2_R, nbb = (np + 255) / 256, max_cols1 = s2_cols(s2_variant(d));
    const int64_t per = ((int64_t)W + 3) * np + nrb * max_cols1;
    const int64_t chunk = sens_chunk(per, b);

    Scratch sc(s);
    double *a2 = nullptr, *pt = nullptr, *cbd = nullptr, *cqd = nullptr, *ud = nullptr, *part = nullptr, *od = nullptr;
    int *zld = nullptr;
    GPX_TRY(sc.take(&a2, chunk * W * np));
    GPX_TRY(sc.take(&pt, chunk * 3 * np));
    GPX_TRY(sc.take(&cbd, ns * cbs));
    GPX_TRY(sc.take(&cqd, ns * S2_CQ));
    GPX_TRY(sc.take(&ud, chunk * d));
    GPX_TRY(sc.take(&part, nrb * chunk * max_cols1));
    GPX_TRY(sc.take(&od, chunk * max_cols1));
    GPX_TRY(sc.take(&zld, 2 * b));
    try { oh.resize((size_t)(chunk * max_cols1)); } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_second_many: out of host memory"); return GPX_ERR_HIP; }
    // the index lists of every chunk: its inputs by variant, each (place in the chunk, first column of its accumulators)
    std::vector<int64_t> first_col((size_t)b, 0);
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0);
        int64_t at = 2 * b0, colsum = 0;
        for (int64_t i = 0; i < bc; ++i) { first_col[(size_t)(b0 + i)] = colsum; colsum += s2_cols(var[(size_t)(s_shared ? 0 : b0 + i)]); }
        for (int v = 0; v < S2_NV; ++v)
            for (int64_t i = 0; i < bc; ++i)
                if (var[(size_t)(s_shared ? 0 : b0 + i)] == v) { zlh[(size_t)at++] = (int)i; zlh[(size_t)at++] = (int)first_col[(size_t)(b0 + i)]; }
    }
    GPX_HIP(hipMemcpyAsync(cbd, cbh.data(), sizeof(double) * cbh.size(), hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(cqd, cqh.data(), sizeof(double) * cqh.size(), hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(zld, zlh.data(), sizeof(int) * zlh.size(), hipMemcpyHostToDevice, s));
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0);
        const double *cbc = s_shared ? cbd : cbd + b0 * cbs, *cqc = s_shared ? cqd : cqd + b0 * S2_CQ;
        int64_t cnt[S2_NV] = {0, 0, 0, 0, 0, 0}, ncols = 0, live = 0;
        for (int64_t i = 0; i < bc; ++i) {
            const int v = var[(size_t)(s_shared ? 0 : b0 + i)];
            if (v >= 0) { ++cnt[v]; ++live; ncols += s2_cols(v); }
        }
        if (live == 0) continue;                 // no input of the chunk has two uncertain coordinates: its rows stay 0.0
        GPX_HIP(hipMemcpyAsync(ud, U + b0 * d, sizeof(double) * bc * d, hipMemcpyDefault, s));
        {
            ProfScope ps(&h->prof, s, GPX_K_QUAD, (double)n * (double)bc * (40.0 * d + 60.0));
            hipLaunchKernelGGL(sens2_build_kernel, dim3((unsigned)nbb, (unsigned)bc), dim3(256), 0, s, (const double *)h->x, (long)n, (long)np, d, W,
                               (const double *)ud, cbc, s_shared ? 0L : (long)cbs, (const double *)h->alpha, h->v, a2, pt);
            GPX_HIP(hipGetLastError());
        }
        {
            // one exponential and NB (NB + 1) / 2 / NB matrix instructions per (pair, slot block) cell
            ProfScope ps(&h->prof, s, GPX_K_EXACT, 0.5 * (double)n * (double)n * (double)live * (35.0 * W));
            const int *zv = zld + 2 * b0;
            for (int v = 0; v < S2_NV; ++v) {
                if (cnt[v] == 0) continue;
                const dim3 grid((unsigned)nrb, 1, (unsigned)cnt[v]);
                const long cqs = s_shared ? 0L : (long)S2_CQ;
#define GPX_S2(NB, PACK) sens2_launch<NB, PACK>(grid, s, a2, pt, cqc, cqs, zv, (long)n, (long)np, W, part, (long)ncols)
                switch (v) {
                case 0: GPX_S2(1, 4); break;
                case 1: GPX_S2(1, 2); break;
                case 2: GPX_S2(1, 1); break;
                case 3: GPX_S2(2, 1); break;
                case 4: GPX_S2(3, 1); break;
                default: GPX_S2(4, 1); break;
                }
#undef GPX_S2
                GPX_HIP(hipGetLastError());
                zv += 2 * cnt[v];
            }
        }
        GPX_TRY(launch_sum_columns(part, nrb, (int)ncols, od, s));
        GPX_HIP(hipMemcpyAsync(oh.data(), od, sizeof(double) * ncols, hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));        // one per chunk: the next chunk reuses od
        for (int64_t i = 0; i < bc; ++i) {
            const int64_t si = s_shared ? 0 : b0 + i;
            if (var[(size_t)si] < 0) continue;
            sens2_scatter(&oh[(size_t)first_col[(size_t)(b0 + i)]], var[(size_t)si], &cbh[(size_t)(si * cbs + 2 * d)], d, &res[(size_t)((b0 + i) * d * d)]);
        }
    }
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_sensitivity_second_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpy(second, res.data(), sizeof(double) * b * d * d, hipMemcpyDefault));
    return 0;
}
