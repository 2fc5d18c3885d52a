// erf_diff.h -- D(A, h) = erf(A + h) - erf(A) for h >= 0 without cancellation (host and device; fp64 erf / erfc / exp of the math library).
// The expectation of a squared-exponential kernel factor under a uniform input is such a difference (sensitivity_box.hip).
//
// Written as erf(B) - erf(A) the difference loses everything once both values round to +-1 (both arguments beyond ~6 on one side: every
// training point outside the box), and log10(1 / h) digits for a narrow interval h = B - A.  Three cases:
//   * both arguments on one side of 0: erfc(A) - erfc(B) for A >= 0, erfc(-B) - erfc(-A) for B <= 0.  erfc keeps its relative accuracy
//     down to underflow (argument ~26.5: the result is then 0.0); what cancels is erfc(A) / D ~ 1 / (2 h max(1, |c|)), c = (A + B) / 2.
//   * opposite signs: erf(B) - erf(A) = erf(B) + erf(|A|), a sum of magnitudes.
//   * a narrow interval, h max(1, |c|) < 2^-8: the midpoint expansion, even orders only,
//       D = 2 / sqrt(pi) e^{-c^2} h sum_{n even} H_n(c) (h / 2)^n / (n + 1)!  =  2 / sqrt(pi) e^{-c^2} h (1 + H_2(c) h^2 / 24 + H_4(c) h^4 / 1920 + ...)
//     with the Hermite polynomials H_2 = 4 c^2 - 2, H_4 = 16 c^4 - 48 c^2 + 12.  Two correction terms: the first one left out is
//     H_6(c) h^6 / 322560, H_6 = 64 c^6 - 480 c^4 + 720 c^2 - 120, so with t = h max(1, |c|) it is at most (64 + 480 + 720 + 120) t^6 /
//     322560 = 4.3e-3 t^6 = 1.5e-17 at t = 2^-8: under u = 1.1e-16 at the switch (the later terms fall by t^2 / 50 each), where the two
//     cases above have lost 1 / (2 t) = 128 u.
// The narrow test comes FIRST in the code: the first two cases and the second between them cover every (A, B).
// THE WIDTH IS AN ARGUMENT, not B - A: the callers' A and B are rounded offsets of magnitude |A|, so B - A carries u |A| / h -- the very
// log10(1 / h) digits the expansion is there to keep, and 0 for a box narrower than the spacing of doubles at A.  h comes from the box's
// width alone (sqrt(om) L, relative error u); the expansion's midpoint is A + h / 2, whose rounding moves D by 2 |c| u |A| relative, as it
// moves every other case.
#pragma once
#include <cmath>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

constexpr double ERF_DIFF_NARROW = 0.00390625;   // 2^-8

__host__ __device__ static inline double erf_diff(double A, double h)
{
#pragma clang fp contract(off)   // the same bits in every kernel instantiation that inlines it
    const double B = A + h, c = A + 0.5 * h;
    if (h * fmax(1.0, fabs(c)) < ERF_DIFF_NARROW) {
        const double c2 = c * c, h2 = h * h;
        const double H2 = 4.0 * c2 - 2.0, H4 = (16.0 * c2 - 48.0) * c2 + 12.0;
        const double s = 1.0 + h2 * (H2 * (1.0 / 24.0) + (H4 * (1.0 / 1920.0)) * h2);
        return (1.1283791670955126 * exp(-c2)) * (h * s);
    }
    if (A >= 0.0) return erfc(A) - erfc(B);
    if (B <= 0.0) return erfc(-B) - erfc(-A);
    return erf(B) - erf(A);
}
