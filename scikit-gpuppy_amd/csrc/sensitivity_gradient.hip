// sensitivity_gradient.hip -- the active-subspace matrix of the GP under independent Gaussian inputs: E[grad mu], E[grad mu grad mu^T] and
// E[Cov grad f], on v_mfma_f64_16x16x4_f64 (gpx_sensitivity_gradient_many; include/gpx.h carries the formulas).  No reference counterpart;
// the closed form is Wycoff, Binois and Wild, "Sequential learning of active subspaces" (2021).
//
// x_k ~ N(u_k, s_k) independent, mu(x) = sum_i beta_i c_i(x), c_i the PLAIN kernel (no +vt, as in sensitivity.hip).  Per coordinate k, with
// a_i = x_ik - u_k, om = w_k, sg = s_k, rho_k = om sg / (1 + 2 om sg), tau_k = sg / (1 + 2 om sg):
//   G_ij     = v^2 exp(sum_k lE_k(i,j)),  lE_k = -1/2 log1p(2 om sg) - 1/4 om (a_i - a_j)^2 - 1/4 om (a_i + a_j)^2 / (1 + 2 om sg)
//   p_k(i,j) = om (rho_k (a_i + a_j) - a_i),  q_k(i,j) = om (rho_k (a_i + a_j) - a_j) = p_k(j,i)
//   J_ij,kl  = G_ij (p_k q_l + delta_kl om^2 tau_k)
//   cmean_kl = sum_ij beta_i beta_j J_ij,kl,   cpost_kl = delta_kl v w_k - sum_ij Kinv_ij J_ij,kl
//   gmean_k  = v sum_i beta_i exp(sum_l lm_il) om a_i / (1 + om sg)
// ONE exponential a pair of training points, every term of its exponent non-positive (the completed square: exp_nonpos is exact in
// intent); the coordinates enter through the two LINEAR factors p and q, and their outer product is what the matrix core forms.  A
// coordinate with s_k = 0 is no special case (rho = tau = 0): there is no slot compaction, slot = coordinate.
//
// Over the pairs j <= i a pair below the diagonal contributes p q^T + q p^T, a diagonal pair p p^T.  The kernel accumulates
//   D = sum_{j <= i} wgt W_ij G_ij p q^T,  g = sum_{j <= i} wgt W_ij G_ij,   wgt = 1 below the diagonal, 1/2 on it, W = beta beta^T or Kinv
// and the host forms D + D^T + delta_kl 2 g om^2 tau_k: symmetric to the bit (one addition serves both entries).
//
// Build kernel: per (input, point) POINT-major a [npad][W], W = 16 NB, NB = ceil(d / 16), zero padded (four points x 16 slots is one
// 512-byte wave load), bw_i = v beta_i (0.0 for a padded point), and gmean's block partials, summed in fixed order.
// Pair kernel: a workgroup owns GR_R = 16 rows i in LDS (row stride 16 NB + 1 words: the 16 rows of phase 1 fall into 16 bank pairs), its
// four waves walk the columns j <= i four at a time.  A wave's step covers 16 rows x 4 columns = 64 pairs in two phases:
//   PHASE 1  lane (r = lane % 16, p = lane / 16) owns the PAIR (i0 + r, j + p): it loops over the coordinates for the exponent -- a_ik
//            from LDS, a_jk from lane k of its own 16-lane DPP row (row_newbcast of the register phase 2 keeps), the constants uniform --
//            evaluates the one exp_nonpos and forms wB = wgt bw_i bw_j ex and, in the cpost instance, wK = wgt v^2 Kinv_ij ex (the
//            element of K^-1 is loaded here, lower half only, 4 consecutive words a row).  wB and wK also enter the scalar sums g.
//   PHASE 2  for each of the 16 rows, lane (k = lane % 16, p) owns COORDINATE k of pair (row, j + p): p_k = cm a_ik + cr a_jk and
//            q_k = cr a_ik + cm a_jk (cr = om rho, cm = cr - om) as ONE addition each -- the row's shares cm a_ik, cr a_ik lie in
//            LDS (16 addresses broadcast four ways), the column's are formed once a step and kept in registers across the rows --
//            the row's pair weight from lane (row, p) by row_newbcast, then D += (w p) q^T: A = [row = lane % 16 -> k][kk = lane / 16 ->
//            pair], B = [kk][col -> l], the layouts of sensitivity_second.hip.  The cpost instance issues a second MFMA with the same B
//            into a second accumulator.
//   No data goes through LDS between the phases.
// d > 16: D is not symmetric, so NB^2 accumulators a weight.  NB = 2 keeps all four (and eight with cpost) in one workgroup; NB = 3, 4
// sweep the column blocks over grid.y (SWEEP: NB accumulators a weight and workgroup, phase 1 repeated per sweep) so that no instance
// needs scratch.  The waves' accumulators go through LDS in a fixed order to partial [row block][input's columns], then ONE
// launch_sum_columns per chunk.  No atomics: an input's result depends neither on its place in the batch nor on the chunking, and the
// beta sums have the same bits with and without cpost (the same instructions in the same order, contraction off).
#include <cmath>
#include <cstring>

#include "common.h"

constexpr int GR_R = 16;                        // rows per workgroup
// an input's constants by coordinate (zero from d on), rows [GPX_MAX_D] each: 0 cD = -om / 4, 1 cS = -om / 4 / (1 + 2 om sg),
// 2 cR = om rho, 3 om, 4 gm = om / (1 + om sg), 5 dg = om^2 tau; then c0 = -1/2 sum log1p(2 om sg), 0
constexpr int GR_CROWS = 6;
constexpr int GR_CQ = GR_CROWS * GPX_MAX_D + 2;
static inline int64_t gr_cols(int nb, int nw) { return (int64_t)nw * (256 * nb * nb + 1); }   // an input's columns: NW NB^2 accumulators, NW scalars

// lane J of the caller's own 16-lane row (the fp64 DPP of leaf.h; s_nop 1: a DPP read needs two wait states behind the VALU write of its source)
template <int J> static __device__ __forceinline__ double gr_row_bcast(double v)
{
    double r;
    asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(J));
    return r;
}
// the same behind an earlier gr_row_bcast of the same source: the volatile statements keep their order, so the wait states have passed
template <int J> static __device__ __forceinline__ double gr_row_bcast_again(double v)
{
    double r;
    asm volatile("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(J));
    return r;
}

// per (input z, point i): a [z][npad][W] by coordinate, bw [z][npad] = v beta_i; mpart [block][input][d] = the block's share of gmean
__global__ __launch_bounds__(256) void grad_build_kernel(const double *__restrict__ x, long n, long npad, int d, int W, const double *__restrict__ U,
                                                         const double *__restrict__ cb, long cb_stride, const double *__restrict__ cq, long cq_stride,
                                                         const double *__restrict__ beta, double v, double *__restrict__ a2, double *__restrict__ bw,
                                                         double *__restrict__ mpart)
{
    __shared__ double ws[4][GPX_MAX_D];
    const int t = threadIdx.x;
    const long z = blockIdx.y, i = (long)blockIdx.x * 256 + t;
    const bool live = i < npad, real = i < n;
    const double *c = cb + z * cb_stride, *gm = cq + z * cq_stride + 4 * GPX_MAX_D, *u = U + z * d;
    double lall = 0.0;
    if (live) {
        double *row = a2 + (z * npad + i) * W;
        for (int l = 0; l < d; ++l) {
            const double a = real ? x[i * d + l] - u[l] : 0.0;
            row[l] = a;
            lall += real ? fma(-c[d + l] * a, a, c[l]) : 0.0;
        }
        for (int l = d; l < W; ++l) row[l] = 0.0;
    }
    const double b0 = real ? v * beta[i] : 0.0;
    if (live) bw[z * npad + i] = b0;
    const double m = b0 * exp_nonpos(lall);
    for (int l = 0; l < d; ++l) {                 // every lane takes part in the wave's sum
        const double a = real ? x[i * d + l] - u[l] : 0.0;
        const double s = wave_sum(m * (gm[l] * a));
        if ((t & 63) == 0) ws[t >> 6][l] = s;
    }
    __syncthreads();
    if (t < d) mpart[((long)blockIdx.x * gridDim.y + z) * d + t] = (ws[0][t] + ws[1][t]) + (ws[2][t] + ws[3][t]);
}

// four coordinates of the exponent of phase 1; K0 a literal: the DPP lane is an immediate
#define GR_E1(K)                                                            \
    {                                                                       \
        const double ajk = gr_row_bcast<K>(aj[be]), aik = as[r][16 * be + K]; \
        const double dm = aik - ajk, sm = aik + ajk;                        \
        e = fma(cD[16 * be + K] * dm, dm, e);                               \
        e = fma(cS[16 * be + K] * sm, sm, e);                               \
    }
#define GR_E4(K0)                                                           \
    if (16 * be + K0 < d) { GR_E1(K0) GR_E1(K0 + 1) GR_E1(K0 + 2) GR_E1(K0 + 3) }
// one row of phase 2
#define GR_ROW(ROW)                                                                                                         \
    {                                                                                                                       \
        const double wb = (ROW == 0) ? gr_row_bcast<ROW>(wB) : gr_row_bcast_again<ROW>(wB);                                 \
        double wk = 0.0;                                                                                                    \
        if (KINV) wk = (ROW == 0) ? gr_row_bcast<ROW>(wK) : gr_row_bcast_again<ROW>(wK);                                    \
        double pp[NB], qq[NC];                                                                                              \
        _Pragma("unroll") for (int be = 0; be < NB; ++be) {                                                                 \
            pp[be] = ap[ROW][16 * be + k] + pj[be];                                                                         \
            if (!SWEEP) qq[be % NC] = aq[ROW][16 * be + k] + qj[be];                                                        \
        }                                                                                                                   \
        if (SWEEP) qq[0] = aq[ROW][16 * be0 + k] + qjs;                                                                     \
        _Pragma("unroll") for (int al = 0; al < NB; ++al)                                                                   \
            _Pragma("unroll") for (int cb = 0; cb < NC; ++cb) {                                                             \
                accB[al * NC + cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(wb * pp[al], qq[cb], accB[al * NC + cb], 0, 0, 0); \
                if (KINV) accK[al * NC + cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(wk * pp[al], qq[cb], accK[al * NC + cb], 0, 0, 0); \
            }                                                                                                               \
    }

// partial [row block][ncols]: at the input's column offset the accumulators ((w NB + al) NB + be) 256 + 64 r + lane = D_w,al,be[4 r + lane / 16]
// [lane % 16] (w = 0 beta beta^T, 1 Kinv), then the NW scalars g_w (written by sweep 0)
template <int NB, bool SWEEP, bool KINV>
__global__ __launch_bounds__(256, 2) void grad_pair_kernel(const double *__restrict__ a2, const double *__restrict__ bw, const double *__restrict__ cq,
                                                           long cq_stride, const double *__restrict__ Kinv, long ldk, long n, long npad, int d, double v2,
                                                           double *__restrict__ partial, long ncols)
{
#pragma clang fp contract(off)   // the instances with and without K^-1 give the sums they share the same bits
    constexpr int R = GR_R, WB = 16 * NB, NC = SWEEP ? 1 : NB, NW = KINV ? 2 : 1, NACC = NB * NC;
    __shared__ double as[R][WB + 1];          // a_i of the block's rows, by coordinate
    __shared__ double ap[R][WB], aq[R][WB];   // the rows' shares of p and q: (om rho - om) a_i, om rho a_i
    __shared__ double rs[R];                  // bw_i
    __shared__ double red[4][256];
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int k = lane & 15, r = k, p = lane >> 4;
    const int rb = gridDim.x - 1 - blockIdx.x;                   // heavy row blocks first
    const int be0 = SWEEP ? (int)blockIdx.y : 0;                 // the column block of this sweep
    const long i0 = (long)rb * R, zi = blockIdx.z;
    const double *c = cq + zi * cq_stride, *cD = c, *cS = c + GPX_MAX_D;
    const double c0 = c[GR_CROWS * GPX_MAX_D];
    const double *aZ = a2 + zi * npad * WB, *bZ = bw + zi * npad;
    for (int q = t; q < R * WB; q += 256) {
        const int rr = q / WB, kk = q - rr * WB;
        const double a = aZ[(i0 + rr) * WB + kk];                // i0 + rr < npad: npad is a multiple of the 128-row tile
        as[rr][kk] = a;
        ap[rr][kk] = (c[2 * GPX_MAX_D + kk] - c[3 * GPX_MAX_D + kk]) * a;
        aq[rr][kk] = c[2 * GPX_MAX_D + kk] * a;
    }
    if (t < R) rs[t] = bZ[i0 + t];
    __syncthreads();

    double cr[NB], cm[NB];                                       // p = cm a_i + cr a_j, q = cr a_i + cm a_j: cr = om rho, cm = cr - om
#pragma unroll
    for (int be = 0; be < NB; ++be) {
        cr[be] = c[2 * GPX_MAX_D + 16 * be + k];
        cm[be] = cr[be] - c[3 * GPX_MAX_D + 16 * be + k];
    }
    const double cmq = c[2 * GPX_MAX_D + 16 * be0 + k] - c[3 * GPX_MAX_D + 16 * be0 + k];
    v4d accB[NACC], accK[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) accB[q] = accK[q] = (v4d){0.0, 0.0, 0.0, 0.0};
    double gB = 0.0, gK = 0.0;
    const long i = i0 + r;                                       // phase 1's row
    const double bwi = rs[r];
    const long jend = (i0 + R < n) ? i0 + R : n;
    for (long j0 = (long)wave * 4; j0 < jend; j0 += 16) {
        const long col = j0 + p;
        const bool in = col < npad;                              // no lane reads past npad
        double aj[NB];
#pragma unroll
        for (int be = 0; be < NB; ++be) aj[be] = in ? aZ[col * WB + 16 * be + k] : 0.0;
        double ajq = 0.0;
        if (SWEEP) ajq = in ? aZ[col * WB + 16 * be0 + k] : 0.0;
        const double bwj = in ? bZ[col] : 0.0;
        // phase 1: this lane's pair (i, col)
        const double wgt = (col < i) ? 1.0 : ((col == i) ? 0.5 : 0.0);
        double kij = 0.0;
        if (KINV) kij = (col <= i && i < n) ? Kinv[i * ldk + col] : 0.0;
        double e = c0;
#pragma unroll
        for (int be = 0; be < NB; ++be) { GR_E4(0) GR_E4(4) GR_E4(8) GR_E4(12) }
        const double ex = exp_nonpos(e);
        const double wB = ((bwi * bwj) * wgt) * ex;
        double wK = 0.0;
        gB += wB;
        if (KINV) { wK = ((v2 * kij) * wgt) * ex; gK += wK; }
        // phase 2: this lane's coordinate k of the pairs (row, col); the column's shares of p and q once a step
        double pj[NB], qj[NB];
#pragma unroll
        for (int be = 0; be < NB; ++be) { pj[be] = cr[be] * aj[be]; qj[be] = cm[be] * aj[be]; }
        const double qjs = cmq * ajq;
        GR_ROW(0) GR_ROW(1) GR_ROW(2) GR_ROW(3) GR_ROW(4) GR_ROW(5) GR_ROW(6) GR_ROW(7)
        GR_ROW(8) GR_ROW(9) GR_ROW(10) GR_ROW(11) GR_ROW(12) GR_ROW(13) GR_ROW(14) GR_ROW(15)
    }
    double *pout = partial + (long)rb * ncols + zi * (long)(NW * (256 * NB * NB + 1));
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int al = q / NC, be = be0 + q % NC;
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) red[wave][64 * rr + lane] = (w == 0) ? accB[q][rr] : accK[q][rr];
            __syncthreads();
            pout[256 * ((w * NB + al) * NB + be) + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        }
    gB = wave_sum(gB);
    if (KINV) gK = wave_sum(gK);
    __syncthreads();
    if (lane == 0) { red[wave][0] = gB; red[wave][1] = gK; }
    __syncthreads();
    if (be0 == 0 && t < NW) pout[256 * NW * NB * NB + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}
#undef GR_E1
#undef GR_E4
#undef GR_ROW

// cq <- the pair constants of one input from its variances (validated by sens_constants before)
static void grad_constants(const double *w, const double *s, int d, double *cq)
{
    memset(cq, 0, sizeof(double) * GR_CQ);
    double c0 = 0.0;
    for (int l = 0; l < d; ++l) {
        const double om = w[l], ws = om * s[l], den = 1.0 + 2.0 * ws;
        cq[l] = -0.25 * om;
        cq[GPX_MAX_D + l] = -0.25 * om / den;
        cq[2 * GPX_MAX_D + l] = om * (ws / den);
        cq[3 * GPX_MAX_D + l] = om;
        cq[4 * GPX_MAX_D + l] = om / (1.0 + ws);
        cq[5 * GPX_MAX_D + l] = om * om * (s[l] / den);
        c0 -= 0.5 * log1p(2.0 * ws);
    }
    cq[GR_CROWS * GPX_MAX_D] = c0;
}

template <int NB, bool SWEEP>
static void grad_launch(bool kinv, unsigned nrb, unsigned bc, hipStream_t s, const double *a2, const double *bw, const double *cq, long cq_stride,
                        const double *Kinv, long ldk, long n, long npad, int d, double v2, double *partial, long ncols)
{
    const dim3 grid(nrb, SWEEP ? NB : 1, bc);
    if (kinv) hipLaunchKernelGGL((grad_pair_kernel<NB, SWEEP, true>), grid, dim3(256), 0, s, a2, bw, cq, cq_stride, Kinv, ldk, n, npad, d, v2, partial, ncols);
    else hipLaunchKernelGGL((grad_pair_kernel<NB, SWEEP, false>), grid, dim3(256), 0, s, a2, bw, cq, cq_stride, Kinv, ldk, n, npad, d, v2, partial, ncols);
}

// out [d, d] = sign (D + D^T + diag(2 g dg)) + diag(add) from one weight's summed accumulators o [256 NB^2] and its scalar g
static void grad_assemble(const double *o, double g, int nb, int d, const double *dg, double sign, const double *add, double vscale, double *out)
{
    auto entry = [&](int kk, int ll) {
        const double *acc = o + 256 * ((kk / 16) * nb + ll / 16);
        const int row = kk % 16, col = ll % 16;
        return acc[64 * (row / 4) + 16 * (row % 4) + col];
    };
    for (int kk = 0; kk < d; ++kk)
        for (int ll = kk; ll < d; ++ll) {
            double val = entry(kk, ll) + entry(ll, kk);
            if (kk == ll) val += 2.0 * g * dg[kk];
            val = (add && kk == ll) ? vscale * add[kk] + sign * val : sign * val;
            out[kk * d + ll] = out[ll * d + kk] = val;
        }
}

// Inputs run in chunks as in gpx_sensitivity_second_many (sens_chunk: GPX_SENS_CHUNK, read at every call)
extern "C" int gpx_sensitivity_gradient_many(gpx_handle *h, const double *U, const double *S, int s_shared, int64_t b, double *gmean, double *cmean,
                                             double *cpost)
{
    CHECK_H_PSEUDO_OK(h);
    NEED_KERNEL(h, "gpx_sensitivity_gradient_many");
    if (b < 0 || (b > 0 && (!U || !S || !gmean || !cmean))) { gpx_set_error("gpx_sensitivity_gradient_many: bad arguments"); return GPX_ERR_BAD_ARG; }
    if (b == 0) return 0;
    const int d = h->d, NB = (d + 15) / 16, W = 16 * NB;
    const bool want_post = cpost != nullptr;
    const int NW = want_post ? 2 : 1;
    const int64_t n = h->n, np = h->npad, cbs = sens_cb_size(d), ns = s_shared ? 1 : b, ci = gr_cols(NB, NW), nacc = 256 * (int64_t)NB * NB;
    hipStream_t s = h->stream;

    // every variance is checked, and every input's constants formed, before the first launch
    std::vector<double> Sh, cbh, cqh, rg, rc, rp, oh;
    try {
        Sh.resize((size_t)(ns * d));
        cbh.resize((size_t)(ns * cbs));
        cqh.resize((size_t)(ns * GR_CQ));
        rg.resize((size_t)(b * d));
        rc.resize((size_t)(b * d * d));
        if (want_post) rp.resize((size_t)(b * d * d));
    } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_gradient_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_TRY(fetch_small(Sh.data(), S, Sh.size()));
    for (int64_t i = 0; i < ns; ++i) {
        if (!sens_constants(h->w, &Sh[(size_t)(i * d)], d, &cbh[(size_t)(i * cbs)])) {
            gpx_set_error("gpx_sensitivity_gradient_many: the variances of input %ld are not all finite and >= 0", (long)i);
            return GPX_ERR_BAD_ARG;
        }
        grad_constants(h->w, &Sh[(size_t)(i * d)], d, &cqh[(size_t)(i * GR_CQ)]);
    }
    if (want_post) GPX_TRY(ensure_kinv(h));   // a pseudo-input handle holds P there from the start

    const int64_t nrb = np / GR_R, nbb = (np + 255) / 256;
    const int64_t per = ((int64_t)W + 1) * np + nrb * ci + nbb * d;
    const int64_t chunk = sens_chunk(per, b);

    Scratch sc(s);
    double *a2 = nullptr, *bw = nullptr, *cbd = nullptr, *cqd = nullptr, *ud = nullptr, *part = nullptr, *mpart = nullptr, *od = nullptr;
    GPX_TRY(sc.take(&a2, chunk * W * np));
    GPX_TRY(sc.take(&bw, chunk * np));
    GPX_TRY(sc.take(&cbd, ns * cbs));
    GPX_TRY(sc.take(&cqd, ns * GR_CQ));
    GPX_TRY(sc.take(&ud, chunk * d));
    GPX_TRY(sc.take(&part, nrb * chunk * ci));
    GPX_TRY(sc.take(&mpart, nbb * chunk * d));
    GPX_TRY(sc.take(&od, chunk * (ci + d)));
    try { oh.resize((size_t)(chunk * (ci + d))); } catch (const std::bad_alloc &) { gpx_set_error("gpx_sensitivity_gradient_many: out of host memory"); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpyAsync(cbd, cbh.data(), sizeof(double) * cbh.size(), hipMemcpyHostToDevice, s));
    GPX_HIP(hipMemcpyAsync(cqd, cqh.data(), sizeof(double) * cqh.size(), hipMemcpyHostToDevice, s));
    for (int64_t b0 = 0; b0 < b; b0 += chunk) {
        const int64_t bc = std::min(chunk, b - b0), ncols = bc * ci;
        const double *cbc = s_shared ? cbd : cbd + b0 * cbs, *cqc = s_shared ? cqd : cqd + b0 * GR_CQ;
        const long cb_stride = s_shared ? 0L : (long)cbs, cq_stride = s_shared ? 0L : (long)GR_CQ;
        GPX_HIP(hipMemcpyAsync(ud, U + b0 * d, sizeof(double) * bc * d, hipMemcpyDefault, s));
        {
            // timed in the classes of the other sensitivity calls: the build in GPX_K_QUAD, the pair pass in GPX_K_EXACT
            ProfScope ps(&h->prof, s, GPX_K_QUAD, (double)n * (double)bc * (50.0 * d + 60.0));
            hipLaunchKernelGGL(grad_build_kernel, dim3((unsigned)nbb, (unsigned)bc), dim3(256), 0, s, (const double *)h->x, (long)n, (long)np, d, W,
                               (const double *)ud, cbc, cb_stride, cqc, cq_stride, (const double *)h->alpha, h->v, a2, bw, mpart);
            GPX_HIP(hipGetLastError());
        }
        GPX_TRY(launch_sum_columns(mpart, nbb, (int)(bc * d), od + ncols, s));
        {
            // per pair: 6 d operations of the exponent, one exponential, and 2 NB^2 NW matrix instructions of 16 x 16 x 4 per 4 pairs
            ProfScope ps(&h->prof, s, GPX_K_EXACT, 0.5 * (double)n * (double)n * (double)bc * (6.0 * d + 40.0 + 512.0 * NB * NB * NW));
            const double v2 = h->v * h->v;
#define GPX_GR(NB_, SWEEP_) grad_launch<NB_, SWEEP_>(want_post, (unsigned)nrb, (unsigned)bc, s, a2, bw, cqc, cq_stride, h->Kinv, (long)np, (long)n, (long)np, d, v2, part, (long)ncols)
            switch (NB) {
            case 1: GPX_GR(1, false); break;
            case 2: GPX_GR(2, false); break;
            case 3: GPX_GR(3, true); break;
            default: GPX_GR(4, true); break;
            }
#undef GPX_GR
            GPX_HIP(hipGetLastError());
        }
        GPX_TRY(launch_sum_columns(part, nrb, (int)ncols, od, s));
        GPX_HIP(hipMemcpyAsync(oh.data(), od, sizeof(double) * (ncols + bc * d), hipMemcpyDeviceToHost, s));
        GPX_HIP(hipStreamSynchronize(s));        // one per chunk: the next chunk reuses od
        for (int64_t i = 0; i < bc; ++i) {
            const double *o = &oh[(size_t)(i * ci)], *dg = &cqh[(size_t)((s_shared ? 0 : b0 + i) * GR_CQ + 5 * GPX_MAX_D)];
            memcpy(&rg[(size_t)((b0 + i) * d)], &oh[(size_t)(ncols + i * d)], sizeof(double) * d);
            grad_assemble(o, o[NW * nacc], NB, d, dg, 1.0, nullptr, 0.0, &rc[(size_t)((b0 + i) * d * d)]);
            if (want_post) grad_assemble(o + nacc, o[NW * nacc + 1], NB, d, dg, -1.0, h->w, h->v, &rp[(size_t)((b0 + i) * d * d)]);
        }
    }
    const hipError_t e = sc.wait_and_free();
    if (e != hipSuccess) { gpx_set_error("gpx_sensitivity_gradient_many: %s", hipGetErrorString(e)); return GPX_ERR_HIP; }
    GPX_HIP(hipMemcpy(gmean, rg.data(), sizeof(double) * b * d, hipMemcpyDefault));
    GPX_HIP(hipMemcpy(cmean, rc.data(), sizeof(double) * b * d * d, hipMemcpyDefault));
    if (want_post) GPX_HIP(hipMemcpy(cpost, rp.data(), sizeof(double) * b * d * d, hipMemcpyDefault));
    return 0;
}
