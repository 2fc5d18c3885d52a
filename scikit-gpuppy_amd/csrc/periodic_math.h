// periodic_math.h -- the periodic factor of PeriodicCovariance on a reduced argument (host and device: the host build is what
// the stand-alone accuracy check of tools/native/check_sinpi.cpp compiles).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define GPX_HD __host__ __device__ __forceinline__
#else
#define GPX_HD static inline
#endif

// r = delta / p - rint(delta / p), |r| <= 1/2, from delta and the two-term reciprocal 1/p = ih + il (ih = fl(1/p),
// il = fl((1 - ih p) ih): |1/p - ih - il| <= u^2 / p).  n = rint(fl(delta ih)) is an integer below 2^52 for every input the kernel is
// good for, delta ih - n is formed exactly by the fma and rounded once, delta il is a correction of relative size u: the reduced
// argument is off by at most u/2 |r| + 2 u^2 |delta / p|, so sin^2 carries no error that grows with |delta / p| (a single rounded
// reciprocal would leave pi u |delta / p| / 2 in it: 10 u at delta / p = 6.7).  Odd in delta, bit for bit: rint rounds ties to even.
GPX_HD double periodic_reduce(double delta, double ih, double il)
{
    const double n = rint(delta * ih);
    return fma(delta, il, fma(delta, ih, -n));
}

// sin(pi r) on |r| <= 1/2 in the style of exp_nonpos: r S(r^2), S the degree-11 Taylor polynomial of sin(pi r) / r in r^2 with pi
// folded into the coefficients (truncation: the next term is (pi/2)^25 / 25! = 5.2e-21 at r = 1/2).  Rounding: the series alternates
// with sum |terms| <= 2.3 |sin| on the interval; Horner in fma leaves at most 2.9 u |sin| (u = 2^-53; measured over 4e6 arguments and
// the interval's ends: tools/native/check_sinpi.cpp), so sin^2 = s s is within 6.1 u relatively and, as sin^2 <= 1, absolutely: what
// enters the kernel's exponent is w2 / 2 times that.  14 fp64 operations.
// Odd in r, bit for bit (the polynomial is even, the last product odd).
GPX_HD double sinpi_half(double r)
{
    const double s = r * r;
    double p = -0x1.7215f879e1ac9p-37;       // -pi^23 / 23!
    p = fma(p, s, 0x1.2877020d52cf0p-31);    //  pi^21 / 21!
    p = fma(p, s, -0x1.8a404211f9547p-26);   // -pi^19 / 19!
    p = fma(p, s, 0x1.aaec32af93359p-21);    //  pi^17 / 17!
    p = fma(p, s, -0x1.6fadb9f155744p-16);   // -pi^15 / 15!
    p = fma(p, s, 0x1.e8f434d018d63p-12);    //  pi^13 / 13!
    p = fma(p, s, -0x1.e3074fde8871fp-8);    // -pi^11 / 11!
    p = fma(p, s, 0x1.50783487ee782p-4);     //  pi^9 / 9!
    p = fma(p, s, -0x1.32d2cce62bd86p-1);    // -pi^7 / 7!
    p = fma(p, s, 0x1.466bc6775aae2p+1);     //  pi^5 / 5!
    p = fma(p, s, -0x1.4abbce625be53p+2);    // -pi^3 / 3!
    p = fma(p, s, 0x1.921fb54442d18p+1);     //  pi
    return p * r;
}

// cos(pi r) on |r| <= 1/2: the degree-11 Taylor polynomial in r^2 (truncation (pi/2)^24 / 24! = 8.2e-20).  It goes to 0 at |r| = 1/2,
// where the error is absolute: 2.4 u at most (measured, as above).  Only the derivative in log p uses it, as sin cos.  Even in r.
GPX_HD double cospi_half(double r)
{
    const double s = r * r;
    double p = -0x1.52ae4120fde27p-34;       // -pi^22 / 22!
    p = fma(p, s, 0x1.ef6e308d6d1c4p-29);    //  pi^20 / 20!
    p = fma(p, s, -0x1.2a0c591af8314p-23);   // -pi^18 / 18!
    p = fma(p, s, 0x1.20c62c2f2d7f5p-18);    //  pi^16 / 16!
    p = fma(p, s, -0x1.b6e24f44b128fp-14);   // -pi^14 / 14!
    p = fma(p, s, 0x1.f9d38a3763cc3p-10);    //  pi^12 / 12!
    p = fma(p, s, -0x1.a6d1f2a204a8cp-6);    // -pi^10 / 10!
    p = fma(p, s, 0x1.e1f506891babbp-3);     //  pi^8 / 8!
    p = fma(p, s, -0x1.55d3c7e3cbffap+0);    // -pi^6 / 6!
    p = fma(p, s, 0x1.03c1f081b5ac4p+2);     //  pi^4 / 4!
    p = fma(p, s, -0x1.3bd3cc9be45dep+2);    // -pi^2 / 2!
    return fma(p, s, 1.0);
}
