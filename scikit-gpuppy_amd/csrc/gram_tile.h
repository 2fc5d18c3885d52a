// gram_tile.h -- the block-tile frame of every Gram / cross-covariance kernel (gram.hip, periodic.hip, matern.hip), once.
//
// A block of 256 threads owns a 64 x 128 tile of out: the column tile of xj sits k-major in LDS, a wave's 16 rows of xi are wave-uniform
// (scalar loads), a lane owns two adjacent columns and stores 16 bytes.  The frame owns the tile decode, the staging, the row pointers,
// the interior fast path and the diagonal / padding epilogue; what a kernel family computes per coordinate and pair comes in as a pair
// policy:
//   struct Pair {
//       struct State;                                                        // per-entry sums of a lane's 16 rows x 2 columns
//       void accumulate(State &, arow, b_s, lane, gc, d) const;              // the sum over the d coordinates
//       v2d entry(const State &, arow, r) const;                             // row r's two entries, before add_diag and the padding
//   };
// arow[r]: row r's inputs (wave-uniform pointers), b_s [d][128]: the staged column tile, gc: the lane's first column.
#pragma once
#include "common.h"

constexpr int GT_ROWS = 64;    // rows of one block tile (4 waves x 16 rows)
constexpr int GT_COLS = 128;   // columns of one block tile (64 lanes x 2 adjacent columns)
enum { PAD_NONE = 0, PAD_ZERO = 1, PAD_IDENT = 2 };
typedef double v16d __attribute__((ext_vector_type(16)));   // one value per row of a lane

// lower_only: 0 = every tile, 1 = a 2-D grid whose tiles above the diagonal retire at once, 2 = the 1-D grid of gram_launch_plan.
// DIAG = false: a matrix without a diagonal term (a derivative): add_diag is never added -- not even as + 0.0, which would turn an
// entry of -0.0 on the diagonal into +0.0 --, PAD_IDENT has no meaning (the launcher refuses it) and there is one epilogue only.
template <class Pair, bool DIAG = true>
__device__ __forceinline__ void gram_tile(const Pair &pair, const double *__restrict__ xi, long n1, const double *__restrict__ xj, long n2, int d,
                                          double add_diag, int lower_only, int pad_mode, double *__restrict__ out, long ld)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double *b_s = smem;               // [d][128]  columns of xj, k-major so a lane reads 2 adjacent columns

    long ry = blockIdx.y, cx = blockIdx.x;
    if (lower_only == 2) {
        // 1-D grid over the tiles that touch the lower triangle only (a square launch: rounds 1-4 dispatched the full grid and retired
        // half of it at once).  Row tile ry (64 rows) needs the column tiles cx <= ry / 2 (128 columns): the row pairs (2m, 2m + 1) hold
        // m + 1 tiles each, m (m + 1) tiles lie before pair m.
        const long lid = blockIdx.x;
        long m = (long)((sqrt(4.0 * (double)lid + 1.0) - 1.0) * 0.5);
        while (m * (m + 1) > lid) --m;
        while ((m + 1) * (m + 2) <= lid) ++m;
        const long rem = lid - m * (m + 1);
        ry = 2 * m + (rem > m ? 1 : 0);
        cx = rem > m ? rem - (m + 1) : rem;
    }
    const long row0 = ry * GT_ROWS;
    const long col0 = cx * GT_COLS;
    if (lower_only && col0 > row0 + (GT_ROWS - 1)) return;   // tile entirely above the diagonal (2-D grid of a non-square lower launch)

    const int t = threadIdx.x;
    for (int e = t; e < GT_COLS * d; e += 256) {
        int c = e & (GT_COLS - 1), k = e >> 7;
        long gc = col0 + c;
        b_s[k * GT_COLS + c] = (gc < n2) ? xj[gc * d + k] : 0.0;
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    // rows past n1 (padding) read the last real row: their outputs are overwritten below
    const long rbase = row0 + wave * 16;
    const double *arow[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) arow[r] = xi + (rbase + r < n1 ? rbase + r : n1 - 1) * d;
    const long gc = col0 + 2 * lane;
    typename Pair::State st;
    pair.accumulate(st, arow, b_s, lane, gc, d);

    // a tile that touches neither the diagonal nor the padding (all but a few per mille of them) skips the per-entry tests of those two
    if (DIAG && row0 + GT_ROWS <= n1 && col0 + GT_COLS <= n2 && (col0 >= row0 + GT_ROWS || col0 + GT_COLS <= row0)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) *reinterpret_cast<v2d *>(&out[(rbase + r) * ld + gc]) = pair.entry(st, arow, r);
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long gr = rbase + r;
        v2d o = pair.entry(st, arow, r);
        if (DIAG) {
            if (gr == gc) o.x += add_diag;
            if (gr == gc + 1) o.y += add_diag;
        }
        if (pad_mode != PAD_NONE) {
            if (gr >= n1 || gc >= n2) o.x = (DIAG && pad_mode == PAD_IDENT && gr == gc) ? 1.0 : 0.0;
            if (gr >= n1 || gc + 1 >= n2) o.y = (DIAG && pad_mode == PAD_IDENT && gr == gc + 1) ? 1.0 : 0.0;
        }
        *reinterpret_cast<v2d *>(&out[gr * ld + gc]) = o;
    }
}

// What a launcher derives from the padded shape: out must hold rows_pad x ld doubles with rows_pad % 64 == 0, cols_pad % 128 == 0,
// ld >= cols_pad, ld even and out 16-byte aligned (false: it does not).  A square lower launch over whole row pairs takes the 1-D grid
// of the tiles that touch the lower triangle (lower_only = 2).
struct GramLaunch {
    dim3 grid;
    size_t lds = 0;
    int lower_only = 0;
    double bytes = 0;   // stored, for the profiler
};
static inline bool gram_launch_plan(int64_t rows_pad, int64_t cols_pad, int64_t ld, int d, int lower_only, GramLaunch *pl)
{
    if (rows_pad % GT_ROWS || cols_pad % GT_COLS || ld < cols_pad || (ld & 1) || d < 1 || d > GPX_MAX_D) return false;
    pl->grid = dim3((unsigned)(cols_pad / GT_COLS), (unsigned)(rows_pad / GT_ROWS));
    pl->lds = (size_t)GT_COLS * d * sizeof(double);
    pl->lower_only = lower_only;
    pl->bytes = 8.0 * (lower_only ? 0.5 * (double)rows_pad * (double)cols_pad : (double)rows_pad * (double)cols_pad);
    if (lower_only && rows_pad == cols_pad && rows_pad % (2 * GT_ROWS) == 0) {
        const int64_t m = rows_pad / (2 * GT_ROWS);           // row pairs: pair m holds 2 (m + 1) tiles
        pl->grid = dim3((unsigned)(m * (m + 1)), 1);
        pl->lower_only = 2;
    }
    return true;
}
// the plan of a raw-input kernel's launcher (periodic.hip, matern.hip), which also writes d K / d theta_deriv, deriv in [0, nderiv); -1:
// K itself.  A derivative has no diagonal term: identity padding would have no meaning for it, and no caller asks for it.
static inline bool raw_gram_launch_plan(int64_t n1, int64_t n2, int64_t rows_pad, int64_t cols_pad, int64_t ld, int d, int lower_only, int pad_mode,
                                        int deriv, int nderiv, GramLaunch *pl)
{
    return gram_launch_plan(rows_pad, cols_pad, ld, d, lower_only, pl) && n1 >= 1 && n2 >= 1 && n1 <= rows_pad && n2 <= cols_pad && deriv >= -1 &&
           deriv < nderiv && !(deriv >= 0 && pad_mode == PAD_IDENT);
}
