// radial.h -- the radial factors of the stationary ARD kernels at q = sum_k w_k delta_k^2, one copy for every kernel that needs them
// (matern.hip: Gram, likelihood gradient; rows_tile.h: the right-hand-side blocks; predict_grad.hip: the predictor's input gradient).
//   kf(): the noise-free kernel      g(): d kf / d delta_k = -w_k delta_k g()
#pragma once
#include "common.h"

// Matern, NU2 = 2 nu (3 or 5): s = sqrt(2 nu q); one sqrt and one exp serve all factors
template <int NU2>
struct MaternRadial {
    double s, e;   // sqrt(2 nu q), v exp(-s)
    __device__ __forceinline__ MaternRadial(double v, double q) : s(sqrt((double)NU2 * q)), e(v * exp_nonpos(-s)) {}
    __device__ __forceinline__ double kf() const { return NU2 == 5 ? e * fma(s, fma(s, 1.0 / 3.0, 1.0), 1.0) : e * (1.0 + s); }
    __device__ __forceinline__ double g() const { return NU2 == 5 ? (5.0 / 3.0) * e * (1.0 + s) : 3.0 * e; }
};

// the Gaussian kernel in the same shape: c = v exp(-q / 2) is its own g (GaussRows of rows_tile.h forms its one factor through it)
struct GaussRadial {
    double e;
    __device__ __forceinline__ GaussRadial(double v, double q) : e(v * exp(-0.5 * q)) {}
    __device__ __forceinline__ double kf() const { return e; }
    __device__ __forceinline__ double g() const { return e; }
};

// NU2 = 0: the Gaussian kernel
template <int NU2> struct RadialOf { typedef MaternRadial<NU2> type; };
template <> struct RadialOf<0> { typedef GaussRadial type; };
