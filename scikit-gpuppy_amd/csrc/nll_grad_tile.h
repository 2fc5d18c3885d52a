// nll_grad_tile.h -- the frame of the one-pass likelihood gradient of every raw-input kernel (periodic.hip, matern.hip), once.
//
// ONE pass over the j <= i half of K^-1 recomputes the kernel's factors on the fly and accumulates, with M_ij = Kinv_ij - a_i a_j, the
// sum S_0 = sum M Kf, per coordinate k the policy's NA weighted sums, and T = sum over the pairs with x_i == x_j of M (T = tr Kinv - a.a
// without duplicate rows).  The sums of all d coordinates do not fit in registers at d = 64: grid.y sweeps of KC coordinates each.  A
// sweep forms q over ALL d coordinates (a runtime loop: no coordinate beyond d is ever evaluated, no per-thread array is indexed by it),
// then the weighted terms of its own KC coordinates -- from d = KC + 1 on every sweep repeats q.
// A block of 256 threads owns 8 rows (x and alpha in LDS); the blocks run from the last row block, the longest, to the first.  A lane owns
// a column j and reads it from the k-major copy xT [d, npad] of the inputs (coalesced).  live: the pair lies in the lower half and below
// n; an off-diagonal pair counts twice (wgt).  Equality is decided on max |delta| over every component, not on q == 0, which a zero
// weight or an underflowing delta^2 would fool.
// partial[sweep][block][NC], NC = NA KC + 2: [0] = S_0, [1 + NA kk ..] = the sums of coordinate sweep KC + kk, [NC - 1] = T.
//
// What a kernel family computes comes in as a policy (the per-thread arrays stay plain locals of the frame: inside a struct they have
// cost registers, gram_tile.h / PeriodicPair::State):
//   struct Policy {
//       static constexpr int KC, NA, NC = NA * KC + 2;
//       struct Coord;                                                         // the wave-uniform constants of one coordinate
//       Coord coord(int k) const;
//       double add_q(const Coord &, double e, double q) const;                // q plus coordinate k's term at the difference e
//       double pair(double mij, double wgt, double q, bool equal, double &s0, double &t) const;
//                                          // a finished pair: adds to S_0 and (where equal) to T, returns the weight wq of its sweep terms
//       void sweep(const Coord &, double wq, double e, double (&acc)[NC], int kk) const;   // adds to acc[1 + NA kk ..]
//   };
#pragma once
#include "common.h"

template <class Policy>
__device__ __forceinline__ void nll_grad_tile(const Policy &pol, const double *__restrict__ Kinv, long ld, long n, long npad, int d,
                                              const double *__restrict__ alpha, const double *__restrict__ x, const double *__restrict__ xT,
                                              double *__restrict__ partial)
{
    constexpr int R = 8, KC = Policy::KC, NC = Policy::NC;
    __shared__ double xs[R][GPX_MAX_D];
    __shared__ double as[R];
    __shared__ double red[4][NC];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int rb = gridDim.x - 1 - blockIdx.x;
    const long i0 = (long)rb * R;
    const int k0 = blockIdx.y * KC;
    for (int q = t; q < R * GPX_MAX_D; q += 256) {
        const int r = q / GPX_MAX_D, k = q - r * GPX_MAX_D;
        xs[r][k] = (k < d && i0 + r < n) ? x[(i0 + r) * d + k] : 0.0;
    }
    if (t < R) as[t] = alpha[i0 + t];
    __syncthreads();
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    for (long j = t; j < i0 + R && j < n; j += 256) {
        const double aj = alpha[j];
        double q[R], mx[R], wq[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { q[r] = 0.0; mx[r] = 0.0; }
        for (int k = 0; k < d; ++k) {
            const typename Policy::Coord ck = pol.coord(k);
            const double xjk = xT[(long)k * npad + j];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double e = xs[r][k] - xjk;
                mx[r] = fmax(mx[r], fabs(e));
                q[r] = pol.add_q(ck, e, q[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const long i = i0 + r;
            const bool live = i < n && j <= i;
            const double mij = live ? Kinv[i * ld + j] - as[r] * aj : 0.0;
            wq[r] = pol.pair(mij, (j < i) ? 2.0 : 1.0, q[r], live && mx[r] == 0.0, acc[0], acc[NC - 1]);
        }
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            const int k = k0 + kk;
            if (k < d) {
                const typename Policy::Coord ck = pol.coord(k);
                const double xjk = xT[(long)k * npad + j];
#pragma unroll
                for (int r = 0; r < R; ++r) pol.sweep(ck, wq[r], xs[r][k] - xjk, acc, kk);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double s = wave_sum(acc[c]);
        if (lane == 0) red[wave][c] = s;
    }
    __syncthreads();
    if (t < NC) partial[((long)blockIdx.y * gridDim.x + rb) * NC + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}
