// sensitivity_box_second.hip -- the second-order (pair interaction) Sobol terms of the predictor mean under independent UNIFORM inputs
// over a box, on v_mfma_f64_16x16x4_f64 (gpx_sensitivity_box_second_many; include/gpx.h carries the formulas).  No reference counterpart.
//
// Notation of sensitivity_box.hip: x_k ~ U(lo_k, hi_k), L_k = hi_k - lo_k, the coordinates with L_k > 0 compacted into slots 0..na-1, the
// pinned ones folded into the point weight bw_i; per slot om = w_k, the scaled offset al_ik = sqrt(om) (lo_k - x_ik), the scaled width
// h_k = sqrt(om) L_k; m_ik = sqrt(pi / 2) / h_k D(al_ik / sqrt 2, h_k / sqrt 2), E_k(i,j) = exp(-1/4 (al_i - al_j)^2) 1/2 sqrt(pi) / h_k
// D((al_i + al_j) / 2, h_k), D(A, h) = erf(A + h) - erf(A).  For k != l
//   second_kl = sum_ij b_ij (prod_{q != k,l} m_iq m_jq) (E_k - m_ik m_jk) (E_l - m_il m_jl)  =  V^closed_{kl} - first_k - first_l,
// the Gram matrix of na vectors indexed by the pairs (i, j), as in sensitivity_second.hip -- whose frame (lane map, blocks, packing,
// reduction) this file takes; the cell and its numerics are new.
//
// THE FORM.  prod_{q != k,l} m_iq = h_ik h_il with h_ik = sqrt(prod_active m_iq) / m_ik: a division by m_ik, which sensitivity_box.hip
// never needs and which m_ik = 0.0 (a point ~26.5 / sqrt(om) outside the box) forbids in the linear domain.  So, HERE ALONE, m and E live
// as logarithms: lm_ik = lcm_k + logD(al_ik / sqrt 2, h_k / sqrt 2), lE_k(i,j) = lce_k - 1/4 (al_i - al_j)^2 + logD((al_i + al_j) / 2, h_k)
// with logD of log_erf_diff.h (finite where D underflows) and the host's lcm_k = log(sqrt(pi / 2) / h_k), lce_k = log(1/2 sqrt(pi) / h_k).
// Per (pair, slot) cell
//   dh_k(i,j) = h_ik h_jk (E_k - m_ik m_jk) = exp(e1) - sg_i sg_j,       hl_i = 1/2 sum_active lm_iq,  sg_i = exp(hl_i)       (per point)
//   e1 = gl_ik + gl_jk + lE_k(i,j),                                      gl_ik = hl_i - lm_ik                                (per point and slot)
// and second_kl = sum_pairs (wgt bw_i bw_j dh_k) dh_l.  h_ik = exp(gl_ik) alone overflows for a point far outside in coordinate k only
// and is never formed.
// Sign of e1, for ANY input law: f_i(x_k) in [0, 1] the kernel factor, m_ik = E[f_i], E_k(i,j) = E[f_i f_j].  Cauchy-Schwarz gives
// E_k(i,j)^2 <= E_k(i,i) E_k(j,j), and f^2 <= f gives E_k(i,i) <= m_ik; hence lE_k <= 1/2 (lm_ik + lm_jk) and
//   e1 <= hl_i + hl_j - 1/2 (lm_ik + lm_jk) = 1/2 sum_{q != k} (lm_iq + lm_jq) <= 0   ALWAYS.
// Rounding of fmin(e1, 0): the exact e1 is <= 0, so an evaluated e1 > 0 is positive by its rounding error alone and the clamp moves it
// by no more than that error; exp_nonpos(fmin(e1, 0.0)) is exact in intent.  Where |gl_ik| is large (a point far outside in coordinate k
// alone: gl ~ -1/2 lm_ik > 0 against lE_k ~ lm_ik < 0) the sum cancels and the k cell carries a relative error of about that magnitude
// times u; every partner cell l != k of the same pair keeps lm_ik in its e1 and is below exp(-that magnitude): the product is far
// under the rule's floor on the scale of the sum.  The logs of a narrow box carry u |log h| each (lcm, lce against the log h inside
// logD): 14 u at h = 1e-6.  log_erf_diff.h states what its bracket loses at the switch (128 u, as D itself).
// A box wholly outside the data: every lm ~ -450 or below, sg = 0.0, exp(e1) = 0.0: zeros, and no NaN since every log is finite.
//
// Build kernel: per (input, point) POINT-major al and gl [npad][W], W = 16 ceil(d / 16) (four points x 16 slots is one 512-byte wave
// load; zero from na on), and hl, sg, bw [npad]; lm is parked in gl's place until hl is known.  Slot map: box_constants' (common.h).
// Pair kernel: sens2_pair_kernel's frame.  A workgroup owns S2_R rows i in LDS, its four waves walk the columns j <= i, 4 PACK at a time;
// lane (k = lane % 16, p = lane / 16) owns slot k of pair (i, j + p).  Its wgt bw_i bw_j dh_k is the A operand, its dh_k the B operand of
// the same MFMA: no data moves between lanes.  Blocks (na > 16) and packing (na <= 8 / <= 4) as there.  WHAT DIFFERS: a cell is an erf
// / erfcx / log evaluation of several hundred instructions, so the NB blocks of a row are ONE ROLLED loop (the bodies are inlined once
// per instance, as box_pair_kernel does); the column side of a lane (al_j, gl_j by block) and the dh of the row in hand are parked in
// LDS words that only the owning lane reads back, never in a register array under a runtime index, and only the NB (NB + 1) / 2 MFMAs
// are unrolled.  A lane whose slot is past na skips the cell (dh = 0.0).
// Reduction, index list by variant, chunking, scatter: gpx_sensitivity_second_many's.  No atomics: an input's bits depend neither on its
// place in the batch nor on the chunking.
#include <cmath>
#include <cstring>

#include "common.h"
#include "log_erf_diff.h"

constexpr int BS_CQ = 3 * GPX_MAX_D + 2;  // an input's constants by active slot [GPX_MAX_D each]: lce, h, lcm; then na, 0

// per (input z, point i): al, gl [z][npad][W] by slot (zero from na on), pt [z][3][npad] = hl, sg, bw
__global__ __launch_bounds__(256) void box2_build_kernel(const double *__restrict__ x, long n, long npad, int d, int W,
                                                         const double *__restrict__ lo_all, long lo_stride, const double *__restrict__ w,
                                                         const double *__restrict__ cb, long cb_stride, const double *__restrict__ cq, long cq_stride,
                                                         const double *__restrict__ beta, double v, double *__restrict__ al2, double *__restrict__ gl2,
                                                         double *__restrict__ pt)
{
#pragma clang fp contract(off)
    const long z = blockIdx.y, i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    const double *c = cb + z * cb_stride, *q3 = cq + z * cq_stride, *lo = lo_all + z * lo_stride;
    const int na = (int)c[BOX_CROWS * d];
    const bool real = i < n;
    double *arow = al2 + (z * npad + i) * W, *grow = gl2 + (z * npad + i) * W;
    double lin = 0.0, lact = 0.0;             // the pinned coordinates' exponent; sum of lm over the active slots
    for (int l = 0; l < d; ++l) {
        const int q = (int)c[l];
        const double dlo = real ? lo[l] - x[i * d + l] : 0.0;
        if (q < 0) { lin = fma(-0.5 * w[l] * dlo, dlo, lin); continue; }
        const double al = c[d + q] * dlo;
        const double lm = real ? q3[2 * GPX_MAX_D + q] + log_erf_diff(al * 0.70710678118654752, c[4 * d + q] * 0.70710678118654752) : 0.0;
        arow[q] = al;
        grow[q] = lm;
        lact += lm;
    }
    const double hl = 0.5 * lact;
    for (int q = 0; q < na; ++q) grow[q] = hl - grow[q];        // the thread reads its own lm back
    for (int q = na; q < W; ++q) arow[q] = grow[q] = 0.0;
    double *p = pt + z * 3 * npad + i;
    p[0] = hl;
    p[npad] = exp_nonpos(fmin(hl, 0.0));
    p[2 * npad] = real ? (v * beta[i]) * exp_nonpos(lin) : 0.0;
}

// partial [row block][ncols]: this block's NACC accumulators at the input's column offset, entry a 256 + 64 r + lane = D_a[4 r + lane / 16][lane % 16]
template <int NB, int PACK>
__global__ __launch_bounds__(256, 2) void box2_pair_kernel(const double *__restrict__ al2, const double *__restrict__ gl2, const double *__restrict__ pt,
                                                           const double *__restrict__ cq, long cq_stride, const int *__restrict__ zl, long n, long npad,
                                                           int W, double *__restrict__ partial, long ncols)
{
#pragma clang fp contract(off)
    constexpr int R = S2_R, SL = 16 / PACK, CW = 4 * PACK, NACC = NB * (NB + 1) / 2, WB = 16 * NB;
    __shared__ double as[R][WB], gs[R][WB];   // al_i, gl_i of the block's rows, by slot
    __shared__ double rs[R][2];               // sg_i, bw_i
    __shared__ double ks[2][WB];              // lce, h by slot
    __shared__ double cj[NB][2][256];         // al_j, gl_j of a lane's column by block: each lane parks and reads back its own words
    __shared__ double od[NB][256];            // dh of the row in hand by block, likewise
    __shared__ double red[4][256];
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int k = lane & 15, p = lane >> 4, slot = k % SL, grp = k / SL;
    const int rb = gridDim.x - 1 - blockIdx.x;                   // heavy row blocks first
    const long i0 = (long)rb * R;
    const long zi = zl[2 * blockIdx.z], co = zl[2 * blockIdx.z + 1];
    const double *c = cq + zi * cq_stride;
    const int na = (int)c[3 * GPX_MAX_D];
    const double *aZ = al2 + zi * npad * W, *gZ = gl2 + zi * npad * W, *pZ = pt + zi * 3 * npad;
    for (int q = t; q < R * WB; q += 256) {
        const int r = q / WB, kk = q - r * WB;
        as[r][kk] = aZ[(i0 + r) * W + kk];                       // i0 + r < npad: npad is a multiple of the 128-row tile
        gs[r][kk] = gZ[(i0 + r) * W + kk];
    }
    if (t < R) {
        rs[t][0] = pZ[npad + i0 + t];
        rs[t][1] = pZ[2 * npad + i0 + t];
    }
    if (t < WB) {
        ks[0][t] = c[t];
        ks[1][t] = c[GPX_MAX_D + t];
    }
    __syncthreads();

    v4d acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = (v4d){0.0, 0.0, 0.0, 0.0};
    const long jend = (i0 + R < n) ? i0 + R : n;
    for (long j0 = (long)wave * CW; j0 < jend; j0 += 4 * CW) {
        const long col = j0 + 4 * grp + p;
        const bool in = col < npad;                              // no lane reads past npad
#pragma unroll 1
        for (int be = 0; be < NB; ++be) {
            cj[be][0][t] = in ? aZ[col * W + 16 * be + slot] : 0.0;
            cj[be][1][t] = in ? gZ[col * W + 16 * be + slot] : 0.0;
        }
        const double sgj = in ? pZ[npad + col] : 0.0, bwj = in ? pZ[2 * npad + col] : 0.0;
        const int rlo = (j0 > i0) ? (int)(j0 - i0) : 0;          // rows above it have no column of this step at or below the diagonal
#pragma unroll 1
        for (int r = rlo; r < R; ++r) {
#pragma unroll 1
            for (int be = 0; be < NB; ++be) {
                const int q = 16 * be + slot;
                double dh = 0.0;
                if (q < na) {
                    const double ai = as[r][q], aj = cj[be][0][t];
                    const double dm = ai - aj;
                    const double lE = (ks[0][q] - (0.25 * dm) * dm) + log_erf_diff(0.5 * ai + 0.5 * aj, ks[1][q]);
                    const double e1 = (gs[r][q] + cj[be][1][t]) + lE;
                    dh = exp_nonpos(fmin(e1, 0.0)) - rs[r][0] * sgj;
                }
                od[be][t] = dh;
            }
            const long i = i0 + r;                               // the pair's weight after the cells: nothing of it lives across them
            const double wgt = (col < i) ? 2.0 : ((col == i) ? 1.0 : 0.0);
            const double bb = (rs[r][1] * bwj) * wgt;
            double dv[NB];
#pragma unroll
            for (int be = 0; be < NB; ++be) dv[be] = od[be][t];
#pragma unroll
            for (int be = 0; be < NB; ++be)
#pragma unroll
                for (int al = 0; al <= be; ++al)
                    acc[be * (be + 1) / 2 + al] = __builtin_amdgcn_mfma_f64_16x16x4f64(bb * dv[al], dv[be], acc[be * (be + 1) / 2 + al], 0, 0, 0);
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

// cq <- the pair constants of one box from its box_constants c (validated there)
static void box2_constants(const double *c, int d, double *cq)
{
    memset(cq, 0, sizeof(double) * BS_CQ);
    const int na = (int)c[BOX_CROWS * d];
    for (int q = 0; q < na; ++q) {
        cq[q] = log(c[2 * d + q]);                               // lce = log(1/2 sqrt(pi / om) / L)
        cq[GPX_MAX_D + q] = c[4 * d + q];                        // h = sqrt(om) L, from L itself
        cq[2 * GPX_MAX_D + q] = log(c[3 * d + q]);               // lcm = log(sqrt(pi / (2 om)) / L)
    }
    cq[3 * GPX_MAX_D] = (double)na;
}

template <int NB, int PACK>
static void box2_launch(dim3 grid, hipStream_t s, const double *al2, const double *gl2, const double *pt, const double *cq, long cq_stride,
                        const int *zl, long n, long npad, int W, double *partial, long ncols)
{
    hipLaunchKernelGGL((box2_pair_kernel<NB, PACK>), grid, dim3(256), 0, s, al2, gl2, pt, cq, cq_stride, zl, n, npad, W, partial, ncols);
}

extern "C" int gpx_sensitivity_box_second_many(gpx_handle *h, const double *lo, const double *hi, int box_shared, int64_t b, double *second)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_sensitivity_box_second_many");
    if (b < 0 || (b > 0 && (!lo || !hi || !second))) { gpx_set_error("gpx_sensitivity_box_second_many: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (b == 0) return 0;
    const int d = h->d, W = 16 * ((d + 15) / 16);
    const int64_t n = h->n, np = h->npad, cbs = box_cb_size(d), ns = box_shared ? 1 : b;
    hipStream_t s = h->stream;

    // every box is checked, and every input's constants and variant formed, before the first launch
    std::vector<double> loh, hih, cbh, cqh, res, oh;
    std::vector<int> var, zlh;
    try {
        loh.resize((size_t)(ns * d));
        hih.resize((size_t)(ns * d));
        cbh.resize((size_t)(ns * cbs));
        cqh.resize((size_t)(ns * BS_CQ));
        var.resize((size_t)ns);
        zlh.resize((size_t)(2 * b));
        res.assign((size_t)(b * d * d), 0.0);
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_box_second_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_TRY(fetch_small(loh.data(), lo, loh.size()));
    GPX_TRY(fetch_small(hih.data(), hi, hih.size()));
    bool any = false;
    for (int64_t i = 0; i < ns; ++i) {
        const int bad = box_constants(h->w, &loh[(size_t)(i * d)], &hih[(size_t)(i * d)], d, &cbh[(size_t)(i * cbs)]);
        if (bad) {
            gpx_set_error("gpx_sensitivity_box_second_many: the bounds of input %ld are not finite with lo <= hi and a representable width (coordinate %d)",
                          (long)i, bad - 1);
            return GPX_ERR_BAD_ARG;
        }
        box2_constants(&cbh[(size_t)(i * cbs)], d, &cqh[(size_t)(i * BS_CQ)]);
        var[(size_t)i] = s2_variant((int)cbh[(size_t)(i * cbs + BOX_CROWS * d)]);
        any = any || var[(size_t)i] >= 0;
    }
    if (!any) {                                  // no input has two active coordinates: no launch, all zeros
        GPX_HIP(hipMemcpy(second, res.data(), sizeof(double) * b * d * d, hipMemcpyDefault));
        return 0;
    }

    const int64_t nrb = np / S2_R, nbb = (np + 255) / 256, max_cols1 = s2_cols(s2_variant(d));
    const int64_t per = (2 * (int64_t)W + 3) * np + nrb * max_cols1;
    const int64_t chunk = sens_chunk(per, b);

    Scratch sc(s);
    double *al2 = nullptr, *gl2 = nullptr, *pt = nullptr, *cbd = nullptr, *cqd = nullptr, *lod = nullptr, *part = nullptr, *od = nullptr;
    int *zld = nullptr;
    GPX_TRY(sc.take(&al2, chunk * W * np));
    GPX_TRY(sc.take(&gl2, chunk * W * np));
    GPX_TRY(sc.take(&pt, chunk * 3 * np));
    GPX_TRY(sc.take(&cbd, ns * cbs));
    GPX_TRY(sc.take(&cqd, ns * BS_CQ));
    GPX_TRY(sc.take(&lod, chunk * d));
    GPX_TRY(sc.take(&part, nrb * chunk * max_cols1));
    GPX_TRY(sc.take(&od, chunk * max_cols1));
    GPX_TRY(sc.take(&zld, 2 * b));
    try { oh.resize((size_t)(chunk * max_cols1)); } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_box_second_many: out of host memory"); return GPX_ERR_HIP; }
    // the index lists of every chunk: its inputs by variant, each (place in the chunk, first column of its accumulators)
    std::vector<int64_t> first_col((size_t)b, 0);
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0);
        int64_t at = 2 * b0, colsum = 0;
        for (int64_t i = 0; i < bc; ++i) { first_col[(size_t)(b0 + i)] = colsum; colsum += s2_cols(var[(size_t)(box_shared ? 0 : b0 + i)]); }
        for (int v = 0; v < S2_NV; ++v)
            for (int64_t i = 0; i < bc; ++i)
                if (var[(size_t)(box_shared ? 0 : b0 + i)] == v) { zlh[(size_t)at++] = (int)i; zlh[(size_t)at++] = (int)first_col[(size_t)(b0 + i)]; }
    }
    GPX_HIP(hipMemcpyAsync(cbd, cbh.data(), sizeof(double) * cbh.size(), hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(cqd, cqh.data(), sizeof(double) * cqh.size(), hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(zld, zlh.data(), sizeof(int) * zlh.size(), hipMemcpyHostToDevice, s));
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0);
        const double *cbc = box_shared ? cbd : cbd + b0 * cbs, *cqc = box_shared ? cqd : cqd + b0 * BS_CQ;
        const long cbst = box_shared ? 0L : (long)cbs, cqs = box_shared ? 0L : (long)BS_CQ, lo_stride = box_shared ? 0L : (long)d;
        int64_t cnt[S2_NV] = {0, 0, 0, 0, 0, 0}, ncols = 0, live = 0;
        for (int64_t i = 0; i < bc; ++i) {
            const int v = var[(size_t)(box_shared ? 0 : b0 + i)];
            if (v >= 0) { ++cnt[v]; ++live; ncols += s2_cols(v); }
        }
        if (live == 0) continue;                 // no input of the chunk has two active coordinates: its rows stay 0.0
        // the chunk's lower bounds from the caller's pointer, host or device (hi enters through the constants alone)
        GPX_HIP(hipMemcpyAsync(lod, lo + (box_shared ? 0 : b0 * d), sizeof(double) * (box_shared ? 1 : bc) * d, hipMemcpyDefault, s));
        {
            ProfScope ps(&h->prof, s, GPX_K_QUAD, (double)n * (double)bc * (300.0 * d + 60.0));
            hipLaunchKernelGGL(box2_build_kernel, dim3((unsigned)nbb, (unsigned)bc), dim3(256), 0, s, (const double *)h->x, (long)n, (long)np, d, W,
                               (const double *)lod, lo_stride, (const double *)h->wdev, cbc, cbst, cqc, cqs, (const double *)h->alpha, h->v, al2, gl2, pt);
            GPX_HIP(hipGetLastError());
        }
        {
            // one logD (erf / erfcx / log), one exponential and NB (NB + 1) / 2 / NB matrix instructions per (pair, slot block) cell
            ProfScope ps(&h->prof, s, GPX_K_EXACT, 0.5 * (double)n * (double)n * (double)live * (300.0 * W));
            const int *zv = zld + 2 * b0;
            for (int v = 0; v < S2_NV; ++v) {
                if (cnt[v] == 0) continue;
                const dim3 grid((unsigned)nrb, 1, (unsigned)cnt[v]);
#define GPX_B2(NB, PACK) box2_launch<NB, PACK>(grid, s, al2, gl2, pt, cqc, cqs, zv, (long)n, (long)np, W, part, (long)ncols)
                switch (v) {
                case 0: GPX_B2(1, 4); break;
                case 1: GPX_B2(1, 2); break;
                case 2: GPX_B2(1, 1); break;
                case 3: GPX_B2(2, 1); break;
                case 4: GPX_B2(3, 1); break;
                default: GPX_B2(4, 1); break;
                }
#undef GPX_B2
                GPX_HIP(hipGetLastError());
                zv += 2 * cnt[v];
            }
        }
        GPX_TRY(launch_sum_columns(part, nrb, (int)ncols, od, s));
        GPX_HIP(hipMemcpyAsync(oh.data(), od, sizeof(double) * ncols, hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));        // one per chunk: the next chunk reuses od
        for (int64_t i = 0; i < bc; ++i) {
            const int64_t si = box_shared ? 0 : b0 + i;
            if (var[(size_t)si] < 0) continue;
            sens2_scatter(&oh[(size_t)first_col[(size_t)(b0 + i)]], var[(size_t)si], &cbh[(size_t)(si * cbs)], d, &res[(size_t)((b0 + i) * d * d)]);
        }
    }
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_sensitivity_box_second_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpy(second, res.data(), sizeof(double) * b * d * d, hipMemcpyDefault));
    return 0;
}
