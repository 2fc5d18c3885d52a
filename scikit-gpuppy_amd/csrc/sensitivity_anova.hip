// sensitivity_anova.hip -- every term of the ANOVA decomposition of the predictor mean under independent Gaussian inputs, all interaction
// orders at once, on v_mfma_f64_16x16x4_f64 (gpx_sensitivity_anova_many; include/gpx.h carries the formulas).  No reference counterpart.
//
// Notation of sensitivity.hip: a_ik = u_k - x_ik, lm_ik = log m_ik, E_k(i,j), b_ij = v^2 beta_i beta_j, pairs j <= i with weight 2 / 1,
// the coordinates with s_k > 0 compacted into slots 0..na-1, the others folded into the point weight bw_i.  With, per pair and slot,
// M_q = exp(lm_iq) exp(lm_jq) and dE_q = E_q - M_q, the variance of the ANOVA component of mu in the slots S is
//   D_S = sum_ij b_ij prod_{q in S} dE_q prod_{q not in S} M_q                       for every non-empty S: 2^na - 1 sums.
// A term is a product over the slots, and a product over the slots splits over two HALVES of them: slots 0..ha-1 (ha = na / 2) and
// ha..na-1 (hb = na - ha <= 5).  With  PA_r = prod_{q < ha} (bit_q(r) ? dE_q : M_q)  and  PB_c = prod_{q < hb} (bit_q(c) ? dE_{ha+q} :
// M_{ha+q})  the term of mask r | c << ha is  sum_pairs (wgt bw_i bw_j PA_r) PB_c : ALL 2^na sums are one 2^ha x 2^hb x N^2 product, the
// pairs the contracted index, which the matrix core does.  na = 8 is one 16 x 16 accumulator.
//
// Every exponent is non-positive: E_q through the completed square of sensitivity.hip (sens_log_e), M_q from the per-point exp(lm_iq) of
// the build kernel.  No quotient, no h_ik, and no closed second moment the host would have to take mean^2 from: the device forms the D_S
// themselves, and what the host derives from them (closed indices, Shapley effects) are plain sums.
//
// Build kernel: per (input, point) POINT-major a [npad][AN_W] and em [npad][AN_W] = exp(lm_ik) by active slot, zero padded (AN_W = 16
// holds the ten slots the call serves), and the point weight bw [npad] = v beta_i times the inactive coordinates' plain kernel factors.
// Pair kernel: the frame of sens2_pair_kernel -- a workgroup owns S2_R rows i in LDS, its four waves walk the columns j <= i, CW at a
// time, weights 2 / 1 / 0 and the zero bw of padded points mask the tail, heavy row blocks first.  The cell:
//   1. lane (k = lane % 16, p = lane / 16) evaluates ONE exponential: E, M and dE of slot k % SL of the pair (i, j + 4 (k / SL) + p).
//      na <= 8: SL = 8, lanes 8..15 of a 16-lane row take a second group of four pairs (CW = 8, two matrix instructions a step, no lane
//      idle at na = 8); na = 9, 10: SL = 16, CW = 4.
//   2. EXCHANGE through a wave-private LDS strip [pair][slot][M, dE]: the lane writes its 16 bytes, then reads for each slot q of a half
//      the ONE word at [pair][q][bit_q(r)] -- the row or column bit picks the address, so the product over a half costs no select at all:
//      four loads and four multiplies for the low four slots of a half (the pair weight leads the A product; a slot the half lacks
//      reads a 1.0 parked in the pair's pad slot, so no branch on na splits the cell).  The strip belongs
//      to one wave, whose LDS operations execute in order: a wave-scope fence keeps the compiler from reordering, no barrier is executed;
//      rows alternate between two strips, so a row's write never waits for the row before it to be read.
//   3. A[r][p] = wgt bw_i bw_j PA_r (0.0 for r >= 2^ha), B[p][c] = PB_c (0.0 for c >= 2^hb): the operand layout of leaf.h / gemm.hip, the
//      accumulator's entry rr of a lane is D[4 rr + lane / 16][lane % 16].
//   More than 16 rows or columns (na = 9: 16 x 32, na = 10: 32 x 32): tile (ta, tb) has the FIFTH bit of the row or column fixed; the
//   product over the low four slots of the half is formed once and multiplied by the fifth slot's dE or M per tile (one 16-byte broadcast
//   load): TA TB accumulators.  Variants (TA, TB) = (1, 1) [na <= 8, two pair groups, one accumulator each], (1, 2) [9], (2, 2) [10].
// The variant is chosen by an input's OWN na (a chunk's inputs are launched by variant through an index list), the waves' accumulators go
// through LDS in a fixed order to partial [row block][input's columns], then ONE launch_sum_columns per chunk; the host adds the two pair
// groups in group order and scatters by mask.  No atomics: an input's bits depend neither on its place in the batch nor on the chunking.
#include <cmath>
#include <cstring>

#include "common.h"

constexpr int AN_W = 16;                  // slots per point in a and em (>= GPX_ANOVA_MAX_ACTIVE; one row is two 64-byte lines)
constexpr int AN_NV = 3;                  // variants (TA, TB): (1, 1), (1, 2), (2, 2)
static inline int an_variant(int na) { return na <= 0 ? -1 : (na <= 8 ? 0 : na - 8); }
static inline int an_cols(int var) { return var < 0 ? 0 : (var == 2 ? 1024 : 512); }   // (1, 1): the two pair groups' tiles

// per (input z, point i): a, em [z][npad][AN_W] by slot (zero from na on, and for a padded point), bw [z][npad]
__global__ __launch_bounds__(256) void anova_build_kernel(const double *__restrict__ x, long n, long npad, int d, const double *__restrict__ U,
                                                          const double *__restrict__ cb, long cb_stride, const double *__restrict__ beta, double v,
                                                          double *__restrict__ a2, double *__restrict__ em, double *__restrict__ bw)
{
    const long z = blockIdx.y, i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    const double *c = cb + z * cb_stride, *u = U + z * d;
    const bool real = i < n;
    double *ra = a2 + (z * npad + i) * AN_W, *re = em + (z * npad + i) * AN_W;
    for (int q = 0; q < AN_W; ++q) ra[q] = re[q] = 0.0;
    double lin = 0.0;                                            // log of the inactive coordinates' plain kernel factors: every term <= 0
    for (int l = 0; l < d; ++l) {
        const double a = real ? u[l] - x[i * d + l] : 0.0;
        const double lm = real ? fma(-c[d + l] * a, a, c[l]) : 0.0;
        const int q = (int)c[2 * d + l];
        if (q < 0) { lin += lm; continue; }
        ra[q] = a;
        re[q] = real ? exp_nonpos(lm) : 0.0;
    }
    bw[z * npad + i] = real ? (v * beta[i]) * exp_nonpos(lin) : 0.0;
}

// orders the wave's own LDS traffic for the compiler; the hardware executes one wave's LDS operations in order
static __device__ __forceinline__ void anova_strip_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// partial [row block][ncols]: this block's accumulators at the input's column offset, entry a 256 + 64 rr + lane = D_a[4 rr + lane / 16][lane % 16];
// a = the pair group for (1, 1), else the tile 2 ta + tb (TB == 2) of fifth bits (ta, tb)
template <int TA, int TB>
__global__ __launch_bounds__(256, 2) void anova_pair_kernel(const double *__restrict__ a2, const double *__restrict__ em, const double *__restrict__ bw,
                                                            const double *__restrict__ cb, long cb_stride, int d, const int *__restrict__ zl, long n,
                                                            long npad, double *__restrict__ partial, long ncols)
{
#pragma clang fp contract(off)
    constexpr int R = S2_R, PACK = (TA * TB == 1) ? 2 : 1, SL = 16 / PACK, CW = 4 * PACK, NACC = (PACK == 2) ? 2 : TA * TB;
    __shared__ double as[R][AN_W];            // a_i of the block's rows, by slot
    __shared__ double es[R][AN_W];            // exp(lm_i)
    __shared__ double rs[R];                  // bw_i
    __shared__ __attribute__((aligned(16))) double strip[2][4][CW][SL + 1][2];   // [row parity][wave][pair][slot] = (M, dE); a pair's
    // slots are padded by one: the four pairs of a step then read one slot's words from eight different banks (16 bytes apart modulo 128)
    __shared__ double red[4][256];
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int k = lane & 15, p = lane >> 4, slot = k % SL, grp = k / SL;
    const int rb = gridDim.x - 1 - blockIdx.x;                   // heavy row blocks first
    const long i0 = (long)rb * R;
    const long zi = zl[2 * blockIdx.z], co = zl[2 * blockIdx.z + 1];
    const double *c = cb + zi * cb_stride;
    const int na = (int)c[SEN_CROWS * d];
    const int ha = (TA * TB == 1) ? na / 2 : 4 + (TA - 1), hb = (TA * TB == 1) ? na - na / 2 : 5;   // (1, 2): 4 + 5, (2, 2): 5 + 5
    const int la = ha < 4 ? ha : 4, lb = hb < 4 ? hb : 4;       // the slots of a half that the 16 rows / columns index
    const double *aZ = a2 + zi * npad * AN_W, *eZ = em + zi * npad * AN_W, *bZ = bw + zi * npad;
    for (int q = t; q < R * AN_W; q += 256) {
        const int r = q / AN_W, kk = q - r * AN_W;
        as[r][kk] = aZ[(i0 + r) * AN_W + kk];                    // i0 + r < npad: npad is a multiple of the 128-row tile
        es[r][kk] = eZ[(i0 + r) * AN_W + kk];
    }
    if (t < R) rs[t] = bZ[i0 + t];
    if (t < 2 * 4 * CW) strip[t / (4 * CW)][(t / CW) % 4][t % CW][SL][0] = 1.0;   // the pad slot of every pair: the factor of a slot a half lacks
    __syncthreads();

    const bool own = slot < na;
    const double c0 = own ? c[3 * d + slot] : 0.0, cP = own ? c[4 * d + slot] : 0.0, cQ = own ? c[5 * d + slot] : 0.0;
    const bool rowlive = k < (1 << la), collive = k < (1 << lb);
    // the strip words this lane multiplies, as offsets in doubles from its pair: slot q of a half at 2 q + bit_q(k), and the pad slot's
    // 1.0 (exact) for a q the half does not have -- the cell is straight-line code with all its loads in flight at once, for every na
    int oa[4], ob[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        oa[q] = (q < la) ? 2 * q + ((k >> q) & 1) : 2 * SL;
        ob[q] = (q < lb) ? 2 * (ha + q) + ((k >> q) & 1) : 2 * SL;
    }
    const double *sbase = &strip[0][wave][0][0][0];
    constexpr int SPAR = 4 * CW * (SL + 1) * 2, SPAIR = (SL + 1) * 2;       // doubles per row parity, per pair
    v4d acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = (v4d){0.0, 0.0, 0.0, 0.0};
    const long jend = (i0 + R < n) ? i0 + R : n;
    for (long j0 = (long)wave * CW; j0 < jend; j0 += 4 * CW) {
        const long col = j0 + 4 * grp + p;                       // the pair this lane evaluates
        const bool in = col < npad;                              // no lane reads past npad
        const double aj = in ? aZ[col * AN_W + slot] : 0.0, ej = in ? eZ[col * AN_W + slot] : 0.0;
        double bj[PACK];                                         // the pairs this lane supplies operands for: j0 + 4 g + p
#pragma unroll
        for (int g = 0; g < PACK; ++g) bj[g] = (j0 + 4 * g + p < npad) ? bZ[j0 + 4 * g + p] : 0.0;
        const int rlo = (j0 > i0) ? (int)(j0 - i0) : 0;          // rows above it have no column of this step at or below the diagonal
        for (int r = rlo; r < R; ++r) {
            const long i = i0 + r;
            const double ai = as[r][slot];
            const double dm = ai - aj, sm = ai + aj;
            const double E = exp_nonpos(fma(-cQ * sm, sm, fma(-cP * dm, dm, c0)));     // sens_log_e of sensitivity.hip: both terms <= 0
            const double M = es[r][slot] * ej;
            strip[r & 1][wave][4 * grp + p][slot][0] = M;
            strip[r & 1][wave][4 * grp + p][slot][1] = E - M;
            anova_strip_fence();
            const double *sp = sbase + (r & 1) * SPAR;
#pragma unroll
            for (int g = 0; g < PACK; ++g) {
                const double *pr = sp + (4 * g + p) * SPAIR;
                const long cg = j0 + 4 * g + p;
                const double wgt = (cg < i) ? 2.0 : ((cg == i) ? 1.0 : 0.0);
                double A = rowlive ? (rs[r] * bj[g]) * wgt : 0.0, B = collive ? 1.0 : 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    A *= pr[oa[q]];
                    B *= pr[ob[q]];
                }
                if (TA * TB == 1) {
                    acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, B, acc[g], 0, 0, 0);
                } else {
                    // the fifth slot of a half: M for the tiles with its bit clear, dE for those with it set
                    double Af[TA] = {A}, Bf[TB] = {B};
                    if (TA == 2) { Af[0] = A * pr[2 * 4]; Af[TA - 1] = A * pr[2 * 4 + 1]; }
                    if (TB == 2) { Bf[0] = B * pr[2 * (ha + 4)]; Bf[TB - 1] = B * pr[2 * (ha + 4) + 1]; }
#pragma unroll
                    for (int ta = 0; ta < TA; ++ta)
#pragma unroll
                        for (int tb = 0; tb < TB; ++tb)
                            acc[ta * TB + tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(Af[ta], Bf[tb], acc[ta * TB + tb], 0, 0, 0);
                }
            }
        }
    }
    double *pout = partial + (long)rb * ncols + co;
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) red[wave][64 * rr + lane] = acc[q][rr];
        __syncthreads();
        pout[256 * q + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
}

template <int TA, int TB>
static void anova_launch(dim3 grid, hipStream_t s, const double *a2, const double *em, const double *bw, const double *cb, long cb_stride, int d,
                         const int *zl, long n, long npad, double *partial, long ncols)
{
    hipLaunchKernelGGL((anova_pair_kernel<TA, TB>), grid, dim3(256), 0, s, a2, em, bw, cb, cb_stride, d, zl, n, npad, partial, ncols);
}

// one input's terms [2^na] by mask from its summed accumulators o [an_cols(var)]; entry 0 (sum b_ij prod M) is written as 0.0
static void anova_scatter(const double *o, int var, int na, double *terms)
{
    const int ha = na / 2;
    auto entry = [](const double *acc, int row, int col) { return acc[64 * (row / 4) + 16 * (row % 4) + col]; };
    terms[0] = 0.0;
    for (int mask = 1; mask < (1 << na); ++mask) {
        const int row = mask & ((1 << ha) - 1), col = mask >> ha;
        if (var == 0) terms[mask] = entry(o, row, col) + entry(o + 256, row, col);       // the two pair groups, in group order
        else terms[mask] = entry(o + 256 * ((row >> 4) * 2 + (col >> 4)), row & 15, col & 15);
    }
}

extern "C" int gpx_sensitivity_anova_many(gpx_handle *h, const double *U, const double *S, int s_shared, int64_t b, double *terms, int64_t tstride)
{
    CHECK_H_PSEUDO_OK(h);                     // reads (x, alpha, v, w) alone
    NEED_KERNEL(h, "gpx_sensitivity_anova_many");
    if (b < 0 || (b > 0 && (!U || !S || !terms))) { gpx_set_error("gpx_sensitivity_anova_many: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (b == 0) return 0;
    const int d = h->d;
    const int64_t n = h->n, np = h->npad, cbs = sens_cb_size(d), ns = s_shared ? 1 : b;
    hipStream_t s = h->stream;

    // every variance, active count and stride is checked, and every input's constants and variant formed, before the first launch
    std::vector<double> Sh, cbh, res, oh;
    std::vector<int> nah, zlh;
    try {
        Sh.resize((size_t)(ns * d));
        cbh.resize((size_t)(ns * cbs));
        nah.resize((size_t)ns);
        zlh.resize((size_t)(2 * b));
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_anova_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_TRY(fetch_small(Sh.data(), S, Sh.size()));
    int max_var = -1;
    for (int64_t i = 0; i < ns; ++i) {
        if (!sens_constants(h->w, &Sh[(size_t)(i * d)], d, &cbh[(size_t)(i * cbs)])) {
            gpx_set_error("gpx_sensitivity_anova_many: the variances of input %ld are not all finite and >= 0", (long)i);
            return GPX_ERR_BAD_ARG;
        }
        const int na = nah[(size_t)i] = (int)cbh[(size_t)(i * cbs + SEN_CROWS * d)];
        if (na > GPX_ANOVA_MAX_ACTIVE) {
            gpx_set_error("gpx_sensitivity_anova_many: input %ld has %d uncertain coordinates, more than GPX_ANOVA_MAX_ACTIVE = %d", (long)i, na,
                          GPX_ANOVA_MAX_ACTIVE);
            return GPX_ERR_BAD_ARG;
        }
        if (tstride < ((int64_t)1 << na)) {
            gpx_set_error("gpx_sensitivity_anova_many: tstride = %ld is less than the 2^%d terms of input %ld", (long)tstride, na, (long)i);
            return GPX_ERR_BAD_ARG;
        }
        max_var = std::max(max_var, an_variant(na));
    }
    try { res.assign((size_t)(b * tstride), 0.0); } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_anova_many: out of host memory"); return GPX_ERR_HIP; }
    if (max_var < 0) {                           // no input has an uncertain coordinate: no launch, all zeros
        GPX_HIP(hipMemcpy(terms, res.data(), sizeof(double) * b * tstride, hipMemcpyDefault));
        return 0;
    }
    auto var_of = [&](int64_t i) { return an_variant(nah[(size_t)(s_shared ? 0 : i)]); };

    const int64_t nrb = np / S2_R, nbb = (np + 255) / 256, max_cols1 = an_cols(max_var);
    const int64_t per = (2 * (int64_t)AN_W + 1) * np + nrb * max_cols1;
    const int64_t chunk = sens_chunk(per, b);

    Scratch sc(s);
    double *a2 = nullptr, *em = nullptr, *bw = nullptr, *cbd = nullptr, *ud = nullptr, *part = nullptr, *od = nullptr;
    int *zld = nullptr;
    GPX_TRY(sc.take(&a2, chunk * AN_W * np));
    GPX_TRY(sc.take(&em, chunk * AN_W * np));
    GPX_TRY(sc.take(&bw, chunk * np));
    GPX_TRY(sc.take(&cbd, ns * cbs));
    GPX_TRY(sc.take(&ud, chunk * d));
    GPX_TRY(sc.take(&part, nrb * chunk * max_cols1));
    GPX_TRY(sc.take(&od, chunk * max_cols1));
    GPX_TRY(sc.take(&zld, 2 * b));
    try { oh.resize((size_t)(chunk * max_cols1)); } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_anova_many: out of host memory"); return GPX_ERR_HIP; }
    // the index lists of every chunk: its inputs by variant, each (place in the chunk, first column of its accumulators)
    std::vector<int64_t> first_col((size_t)b, 0);
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0);
        int64_t at = 2 * b0, colsum = 0;
        for (int64_t i = 0; i < bc; ++i) { first_col[(size_t)(b0 + i)] = colsum; colsum += an_cols(var_of(b0 + i)); }
        for (int v = 0; v < AN_NV; ++v)
            for (int64_t i = 0; i < bc; ++i)
                if (var_of(b0 + i) == v) { zlh[(size_t)at++] = (int)i; zlh[(size_t)at++] = (int)first_col[(size_t)(b0 + i)]; }
    }
    GPX_HIP(hipMemcpyAsync(cbd, cbh.data(), sizeof(double) * cbh.size(), hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(zld, zlh.data(), sizeof(int) * zlh.size(), hipMemcpyHostToDevice, s));
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0);
        const double *cbc = s_shared ? cbd : cbd + b0 * cbs;
        const long cb_stride = s_shared ? 0L : (long)cbs;
        int64_t cnt[AN_NV] = {0, 0, 0}, ncols = 0, live = 0;
        for (int64_t i = 0; i < bc; ++i) {
            const int v = var_of(b0 + i);
            if (v >= 0) { ++cnt[v]; ++live; ncols += an_cols(v); }
        }
        if (live == 0) continue;                 // no input of the chunk has an uncertain coordinate: its rows stay 0.0
        GPX_HIP(hipMemcpyAsync(ud, U + b0 * d, sizeof(double) * bc * d, hipMemcpyDefault, s));
        {
            ProfScope ps(&h->prof, s, GPX_K_QUAD, (double)n * (double)bc * (40.0 * d + 60.0));
            hipLaunchKernelGGL(anova_build_kernel, dim3((unsigned)nbb, (unsigned)bc), dim3(256), 0, s, (const double *)h->x, (long)n, (long)np, d,
                               (const double *)ud, cbc, cb_stride, (const double *)h->alpha, h->v, a2, em, bw);
            GPX_HIP(hipGetLastError());
        }
        {
            // one exponential per (pair, slot of the 16-lane row) cell, the exchange, and the halves' products
            ProfScope ps(&h->prof, s, GPX_K_EXACT, 0.5 * (double)n * (double)n * (double)live * (60.0 * AN_W));
            const int *zv = zld + 2 * b0;
            for (int v = 0; v < AN_NV; ++v) {
                if (cnt[v] == 0) continue;
                const dim3 grid((unsigned)nrb, 1, (unsigned)cnt[v]);
#define GPX_AN(TA, TB) anova_launch<TA, TB>(grid, s, a2, em, bw, cbc, cb_stride, d, zv, (long)n, (long)np, part, (long)ncols)
                switch (v) {
                case 0: GPX_AN(1, 1); break;
                case 1: GPX_AN(1, 2); break;
                default: GPX_AN(2, 2); break;
                }
#undef GPX_AN
                GPX_HIP(hipGetLastError());
                zv += 2 * cnt[v];
            }
        }
        GPX_TRY(launch_sum_columns(part, nrb, (int)ncols, od, s));
        GPX_HIP(hipMemcpyAsync(oh.data(), od, sizeof(double) * ncols, hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));        // one per chunk: the next chunk reuses od
        for (int64_t i = 0; i < bc; ++i)
            if (var_of(b0 + i) >= 0)
                anova_scatter(&oh[(size_t)first_col[(size_t)(b0 + i)]], var_of(b0 + i), nah[(size_t)(s_shared ? 0 : b0 + i)], &res[(size_t)((b0 + i) * tstride)]);
    }
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_sensitivity_anova_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpy(terms, res.data(), sizeof(double) * b * tstride, hipMemcpyDefault));
    return 0;
}
