// log_erf_diff.h -- log D(A, h), D(A, h) = erf(A + h) - erf(A) for h > 0, finite where D itself underflows to 0.0 (device only: fp64 erf,
// erfcx, exp, log of the device math library).  erf_diff.h gives D in the linear domain; the second-order terms under uniform inputs
// (sensitivity_box_second.hip) divide by the expectation of a kernel factor, which a point ~26.5 / sqrt(om) outside the box has as 0.0,
// and so keep it as a logarithm.
//
// The three cases and the switch are erf_diff.h's, the narrow test first; every case ends in ONE log of a bracket, added to a base:
//   * narrow, h max(1, |c|) < 2^-8, c = A + h / 2:  log(2 / sqrt(pi)) - c^2 + log(h s), s = 1 + H_2(c) h^2 / 24 + H_4(c) h^4 / 1920 the
//     series of erf_diff.h (written there as log h + log1p(s - 1); s - 1 <= 4e-6 here and h s is one rounding away from either).
//   * one-sided, A >= 0:  erfc(x) = exp(-x^2) erfcx(x) gives D = exp(-A^2) (erfcx(A) - exp(-h (2 A + h)) erfcx(A + h)), so
//       log D = -A^2 + log(erfcx(A) - exp(-h (2 A + h)) erfcx(A + h)).
//     erfcx falls like 1 / (x sqrt(pi)): no factor underflows, the exponent -h (2 A + h) is non-positive, and the bracket is positive.
//     A + h <= 0 is the mirror image D(A, h) = D(-(A + h), h).
//   * straddling, A < 0 < A + h:  log(erf(A + h) + erf(|A|)), a sum of magnitudes that is at least erf(2^-9).
// What cancels in the one-sided bracket, by erf_diff.h's accounting: with t = h max(1, |c|) the subtrahend is erfcx(A) (1 - 2 t + ...) for
// A >= 1 (exp(-2 A h) A / (A + h)) and erfcx(A) - 2 / sqrt(pi) h (1 + ...) for A < 1, so erfcx(A) / bracket ~ 1 / (2 t): at most 128 at
// the switch t = 2^-8, the same 128 u that erfc(A) - erfc(B) has lost there.  A relative error of the bracket is an ABSOLUTE error of
// log D, i.e. again a relative error of whatever exponential the logarithm ends in.  The base -A^2 carries u A^2 from the rounding of
// the product; the caller's A is a rounded offset anyway and moves log D by 2 |A| u |A| (erf_diff.h, last paragraph).
// THE WIDTH IS AN ARGUMENT, formed from the box's width itself and never from two rounded offsets (erf_diff.h).
// The result is clamped at -1e300: an offset beyond 1e150 (A^2 overflows) stays finite, so that sums and differences of such logs are
// no NaN; everything below about -745 means "0.0" to the caller's exponential.
#pragma once
#include "erf_diff.h"

static __device__ __forceinline__ double log_erf_diff(double A, double h)
{
#pragma clang fp contract(off)   // the same bits in the build and in every pair kernel instance
    const double B = A + h, c = A + 0.5 * h;
    double base, arg;
    if (h * fmax(1.0, fabs(c)) < ERF_DIFF_NARROW) {
        const double c2 = c * c, h2 = h * h;
        const double H2 = 4.0 * c2 - 2.0, H4 = (16.0 * c2 - 48.0) * c2 + 12.0;
        base = 0.12078223763524522 - c2;     // log(2 / sqrt(pi))
        arg = h * (1.0 + h2 * (H2 * (1.0 / 24.0) + (H4 * (1.0 / 1920.0)) * h2));
    } else if (A >= 0.0 || B <= 0.0) {
        const double a = (A >= 0.0) ? A : -B;
        base = -(a * a);
        arg = __ocml_erfcx_f64(a) - exp(-h * (2.0 * a + h)) * __ocml_erfcx_f64(a + h);
    } else {
        base = 0.0;
        arg = erf(B) + erf(-A);
    }
    return fmax(base + log(arg), -1e300);
}
