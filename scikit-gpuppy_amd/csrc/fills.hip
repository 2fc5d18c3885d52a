// fills.hip -- small reductions and fills shared across the library (declared in common.h): log-determinant from a factor's diagonal,
// the row sums of a prediction, identity fill, lower-to-upper mirror.
#include "common.h"

// logdet K = 2 sum_i log L_ii over the n real rows; single block, fixed order -> deterministic
__global__ __launch_bounds__(256) void logdet_kernel(const double *diagL, long n, double *out)
{
    __shared__ double ws[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) s += log(diagL[i]);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = 2.0 * (ws[0] + ws[1] + ws[2] + ws[3]);
}

int launch_logdet(const double *diagL, int64_t n, double *out_dev, hipStream_t s)
{
    hipLaunchKernelGGL(logdet_kernel, dim3(1), dim3(256), 0, s, diagL, (long)n, out_dev);
    GPX_HIP(hipGetLastError());
    return 0;
}

// mean_m = sum_n Z[m][n] y[n];  var_m = (v+vt) - sum_n Z[m][n]^2 ; one wave per row, 16-byte loads
__global__ __launch_bounds__(256) void predict_reduce_kernel(const double *__restrict__ Z, long ldz, long m, long npad,
                                                            const double *__restrict__ y, double vplusvt,
                                                            double *__restrict__ mean, double *__restrict__ var, const double *__restrict__ kdiag)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const int lane = threadIdx.x & 63;
    const double *zr = Z + row * ldz;
    double sm = 0.0, sq = 0.0;
    for (long c = 2 * lane; c < npad; c += 128) {
        const v2d z = *reinterpret_cast<const v2d *>(zr + c);
        const v2d yy = *reinterpret_cast<const v2d *>(y + c);
        sm = fma(z.x, yy.x, sm);
        sm = fma(z.y, yy.y, sm);
        sq = fma(z.x, z.x, sq);
        sq = fma(z.y, z.y, sq);
    }
    sm = wave_sum(sm);
    sq = wave_sum(sq);
    if (lane == 0) {
        mean[row] = sm;
        var[row] = (kdiag ? kdiag[row] : vplusvt) - sq;   // kdiag: the operator's own prior variances (gpx_predict_kv)
    }
}

int launch_predict_reduce(const double *Z, int64_t ldz, int64_t m, int64_t npad, const double *y, double vplusvt,
                          double *mean, double *var, hipStream_t s, Profiler *prof, const double *kdiag)
{
    if (m <= 0) return 0;
    ProfScope ps(prof, s, GPX_K_REDUCE, 8.0 * (double)m * (double)npad);
    hipLaunchKernelGGL(predict_reduce_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s, Z, (long)ldz, (long)m,
                       (long)npad, y, vplusvt, mean, var, kdiag);
    GPX_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void set_identity_kernel(double *Z, long ld, long n)
{
    const long row = blockIdx.x;
    const long c = ((long)blockIdx.y * 256 + threadIdx.x) * 2;
    if (c >= n) return;
    v2d o;
    o.x = (c == row) ? 1.0 : 0.0;
    o.y = (c + 1 == row) ? 1.0 : 0.0;
    *reinterpret_cast<v2d *>(Z + row * ld + c) = o;
}

int launch_set_identity(double *Z, int64_t ld, int64_t n, hipStream_t s)
{
    if (n <= 0) return 0;
    dim3 grid((unsigned)n, (unsigned)((n / 2 + 255) / 256));
    hipLaunchKernelGGL(set_identity_kernel, grid, dim3(256), 0, s, Z, (long)ld, (long)n);
    GPX_HIP(hipGetLastError());
    return 0;
}

// copy the strict lower triangle onto the upper one (A[j][i] = A[i][j], i > j), 32x32 LDS transposes
__global__ __launch_bounds__(256) void symmetrize_lower_kernel(double *A, long ld, long n)
{
    __shared__ double tile[32][33];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj > bi) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const long i = (long)bi * 32 + r, j = (long)bj * 32 + tx;
        tile[r][tx] = (i < n && j < n) ? A[i * ld + j] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long j = (long)bj * 32 + r, i = (long)bi * 32 + tx;   // write A[j][i] = tile[i-local][j-local]
        if (i < n && j < n && i > j) A[j * ld + i] = tile[tx][r];
    }
}

int launch_symmetrize_lower(double *A, int64_t ld, int64_t n, hipStream_t s)
{
    if (n <= 0) return 0;
    const unsigned nb = (unsigned)((n + 31) / 32);
    hipLaunchKernelGGL(symmetrize_lower_kernel, dim3(nb, nb), dim3(256), 0, s, A, (long)ld, (long)n);
    GPX_HIP(hipGetLastError());
    return 0;
}
