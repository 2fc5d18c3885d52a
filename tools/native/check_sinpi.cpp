// check_sinpi.cpp -- host check of csrc/periodic_math.h against long double: the reduced argument, sin(pi r), cos(pi r) and
// sin^2(pi delta / p) as the periodic kernels form them.  Prints the worst error of each in units of u = 2^-53.
//   g++ -O2 -std=c++17 -ffp-contract=off -o check_sinpi tools/native/check_sinpi.cpp && ./check_sinpi
// (also builds with -fsanitize=address,undefined: it is a stand-alone host program)
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../scikit-gpuppy_amd/csrc/periodic_math.h"

int main()
{
    const long double PI = 3.14159265358979323846264338327950288L, u = 0x1p-53L;
    std::mt19937_64 rng(1);
    std::uniform_real_distribution<double> ur(-0.5, 0.5), ud(-10.0, 10.0), up(1.5, 4.0);
    long double es = 0, ec = 0, e2 = 0, esym = 0;
    for (int i = 0; i < 4000000; ++i) {
        double r = ur(rng);
        if (i < 1000) r = (i % 2 ? 0.5 : -0.5) * (1.0 - i * 0x1p-53);   // the end of the interval
        const long double s = sinl(PI * r), c = cosl(PI * r);
        const long double ds = fabsl((long double)sinpi_half(r) - s) / (fabsl(s) * u + 1e-300L);
        const long double dc = fabsl((long double)cospi_half(r) - c) / u;
        if (ds > es) es = ds;
        if (dc > ec) ec = dc;
        if (sinpi_half(-r) != -sinpi_half(r) || cospi_half(-r) != cospi_half(r)) esym = 1;
        const double delta = ud(rng), p = up(rng), ih = 1.0 / p, il = fma(-ih, p, 1.0) * ih;
        const double rr = periodic_reduce(delta, ih, il), sn = sinpi_half(rr);
        const long double t = sinl(PI * ((long double)delta / (long double)p)), want = t * t;
        const long double d2 = fabsl((long double)(sn * sn) - want);
        if (d2 / u > e2) e2 = d2 / u;
        if (periodic_reduce(-delta, ih, il) != -rr) esym = 1;
    }
    // (sin^2 absolutely: the long double argument pi delta / p is itself only good to 2e-18, too coarse to judge a sine near zero relatively)
    printf("sin(pi r): %.2Lf u of the value   cos(pi r): %.2Lf u   sin^2(pi delta/p): %.2Lf u   symmetry %s\n", es, ec, e2,
           esym == 0 ? "exact" : "BROKEN");
    return (es < 3.0 && ec < 3.0 && e2 < 6.5 && esym == 0) ? 0 : 1;
}
