// gram.hip -- ARD squared-exponential Gram / cross-covariance assembly for gfx950.
//
// Replaces GaussianCovariance.cov_matrix_ij / cov_matrix (skgpuppy/Covariance.py:461-483): the reference
// expands ||a||^2 + ||b||^2 - 2ab through a GEMM and three N1 x N2 np.tile temporaries; here each
// output is produced once from direct differences of sqrt(w)-scaled inputs staged in LDS, with the
// exp, the v scale, the +vt diagonal and the tile padding fused, and written with 16-byte coalesced
// stores.  The inner dimension d (2..64) is far too short for MFMA: the kernel is bound by the
// 8 B/element HBM store and the fp64 exp, not by a contraction.
#include "common.h"
#include "gram_tile.h"

__global__ __launch_bounds__(256) void scale_rows_kernel(const double *__restrict__ x, long n, long npad, int d,
                                                        const double *__restrict__ sw, double *__restrict__ out,
                                                        const double *__restrict__ origin)
{
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = npad * d;
    if (e >= total) return;
    long i = e / d;
    int k = (int)(e - i * d);
    out[e] = (i < n) ? (origin ? x[e] - origin[k] : x[e]) * sw[k] : 0.0;
}

// The pair policy of the ARD squared exponential on inputs scaled by sqrt(w): acc = sum_k (a_k - b_k)^2, entry = v exp(-acc / 2) colscale.
// The rows' inputs are WAVE-UNIFORM (a wave owns 16 rows, a lane two columns): they are read straight from global memory through
// the scalar cache into SGPRs -- as LDS broadcasts (rounds 1-3) the 16 reads per k and wave made the LDS pipe, not the fp64 VALU,
// the bound of the difference loop (4 waves x 16 x 4 cycles against 32 x 4 VALU cycles per SIMD and k): d = 16 ran at 3.1 TB/s.
struct GaussPair {
    double v;
    // optional factor per COLUMN (SPGP: W^T = (Lambda^-1/2 K_NM)^T is generated as the Gram matrix K_MN with its columns scaled, instead
    // of transposing a stored K_NM: spgp.hip); columns past n2 are padding and written as such by the frame
    const double *colscale;
    long n2;
    struct State { double acc0[16], acc1[16]; v2d cs; };

    __device__ __forceinline__ void accumulate(State &st, const double *const (&arow)[16], const double *b_s, int lane, long gc, int d) const
    {
        double (&acc0)[16] = st.acc0, (&acc1)[16] = st.acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0; acc1[r] = 0.0; }
        int k = 0;
        for (; k + 2 <= d; k += 2) {
            const v2d b0 = *reinterpret_cast<const v2d *>(&b_s[k * GT_COLS + 2 * lane]);
            const v2d b1 = *reinterpret_cast<const v2d *>(&b_s[(k + 1) * GT_COLS + 2 * lane]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double a0 = arow[r][k], a1 = arow[r][k + 1];
                double e0 = a0 - b0.x, e1 = a0 - b0.y;
                acc0[r] = fma(e0, e0, acc0[r]);
                acc1[r] = fma(e1, e1, acc1[r]);
                e0 = a1 - b1.x; e1 = a1 - b1.y;
                acc0[r] = fma(e0, e0, acc0[r]);
                acc1[r] = fma(e1, e1, acc1[r]);
            }
        }
        if (k < d) {
            const v2d b = *reinterpret_cast<const v2d *>(&b_s[k * GT_COLS + 2 * lane]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double a = arow[r][k];
                const double d0 = a - b.x, d1 = a - b.y;
                acc0[r] = fma(d0, d0, acc0[r]);
                acc1[r] = fma(d1, d1, acc1[r]);
            }
        }
        st.cs = (v2d){1.0, 1.0};
        if (colscale) { st.cs.x = gc < n2 ? colscale[gc] : 0.0; st.cs.y = gc + 1 < n2 ? colscale[gc + 1] : 0.0; }
    }
    __device__ __forceinline__ v2d entry(const State &st, const double *const (&)[16], int r) const
    {
        v2d o;
        o.x = v * exp_nonpos(-0.5 * st.acc0[r]) * st.cs.x;
        o.y = v * exp_nonpos(-0.5 * st.acc1[r]) * st.cs.y;
        return o;
    }
};

__global__ __launch_bounds__(256) void gram_kernel(const double *__restrict__ xi, long n1,
                                                  const double *__restrict__ xj, long n2, int d, double v,
                                                  double add_diag, int lower_only, int pad_mode,
                                                  double *__restrict__ out, long ld, const double *__restrict__ colscale)
{
    gram_tile(GaussPair{v, colscale, n2}, xi, n1, xj, n2, d, add_diag, lower_only, pad_mode, out, ld);
}

int launch_scale_rows(const double *x, int64_t n, int64_t npad, int d, const double *sw_dev, double *out, hipStream_t s, const double *origin_dev)
{
    long total = npad * d;
    if (total == 0) return 0;
    int blocks = (int)((total + 255) / 256);
    hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks), dim3(256), 0, s, x, (long)n, (long)npad, d, sw_dev, out, origin_dev);
    GPX_HIP(hipGetLastError());
    return 0;
}

// xi_w / xj_w: inputs already scaled by sqrt(w); the padding contract of out: gram_launch_plan (gram_tile.h)
int launch_gram(const double *xi_w, int64_t n1, const double *xj_w, int64_t n2, int d, double v, double add_diag,
                int lower_only, int pad_mode, double *out, int64_t ld, int64_t rows_pad, int64_t cols_pad,
                hipStream_t s, Profiler *prof, const double *colscale)
{
    GramLaunch pl;
    if (!gram_launch_plan(rows_pad, cols_pad, ld, d, lower_only, &pl)) {
        gpx_set_error("launch_gram: bad padding (rows_pad=%ld cols_pad=%ld ld=%ld d=%d)", (long)rows_pad, (long)cols_pad, (long)ld, d);
        return GPX_ERR_BAD_ARG;
    }
    if (rows_pad == 0 || cols_pad == 0) return 0;
    ProfScope ps(prof, s, GPX_K_GRAM, pl.bytes);
    hipLaunchKernelGGL(gram_kernel, pl.grid, dim3(256), pl.lds, s, xi_w, (long)n1, xj_w, (long)n2, d, v, add_diag,
                       pl.lower_only, pad_mode, out, (long)ld, colscale);
    GPX_HIP(hipGetLastError());
    return 0;
}
