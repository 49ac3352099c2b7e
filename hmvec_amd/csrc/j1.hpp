// Device Bessel functions of the first kind, orders one and two, J1(x) and J2(x), in fp64 for gfx950.
//
// J1 restates the published algorithm of Cephes Math Library 2.8 `j1.c` (S. L. Moshier, 1984-2000) with its published
// coefficients, in the same form as j0.hpp:
//   * 0 <= x <= 5:  J1 = x (z - Z1)(z - Z2) RP(z) / RQ(z),  z = x^2, with Z1, Z2 the squares of the first two zeros of
//                   J1 beyond 0;
//   * x > 5:        the Hankel form  J1 = sqrt(2/(pi x)) [P1(x) cos(x - 3pi/4) - (5/x) Q1(x) sin(x - 3pi/4)]  with
//                   P1, Q1 rationals in 25/x^2.
// J1 is odd.
//
// J2 (the two-halo tangential shear's kernel) is the recurrence J2 = 2 J1(x)/x - J0(x) where it is
// well conditioned.  Below J2_SERIES_X the recurrence cancels (J2 ~ x^2/8 against J0 ~ 1), and J2 is the power series
//   J2 = sum_k (-1)^k (x/2)^(2k+2) / (k! (k+2)!),
// nested as (y/2)(1 - y/(1*3)(1 - y/(2*4)(1 - ...))), y = x^2/4; J2_SERIES_N terms leave a truncation below 1e-23
// relative at the threshold.  J2 is even.
#pragma once
#include <hip/hip_runtime.h>

#include "j0.hpp"

namespace hmg {

namespace j1c {
constexpr double RP[4] = {-8.99971225705559398224E8, 4.52228297998194034323E11, -7.27494245221818276015E13,
                          3.68295732863852883286E15};
constexpr double RQ[8] = {6.20836478118054335476E2,  2.56987256757748830383E5,  8.35146791431949253037E7,
                          2.21511595479792499675E10, 4.74914122079991414898E12, 7.84369607876235854894E14,
                          8.95222336184627338078E16, 5.32278620332680085395E18};   // leading coefficient 1 implied
constexpr double PP[7] = {7.62125616208173112003E-4, 7.31397056940917570436E-2, 1.12719608129684925192E0,
                          5.11207951146807644818E0,  8.42404590141772420927E0,  5.21451598682361504063E0,
                          1.00000000000000000254E0};
constexpr double PQ[7] = {5.71323128072548699714E-4, 6.88455908754495404082E-2, 1.10514232634061696926E0,
                          5.07386386128601488557E0,  8.39985554327604159757E0,  5.20982848682361821619E0,
                          9.99999999999999997461E-1};
constexpr double QP[8] = {5.10862594750176621635E-2, 4.98213872951233449420E0, 7.58238284132545283818E1,
                          3.66779609360150777800E2,  7.10856304998926107277E2, 5.97489612400613639965E2,
                          2.11688757100572135698E2,  2.52070205858023719784E1};
constexpr double QQ[7] = {7.42373277035675149943E1, 1.05644886038262816351E3, 4.98641058337653607651E3,
                          9.56231892404756170795E3, 7.99704160447350683650E3, 2.82619278517639096600E3,
                          3.36093607810698293419E2};   // leading coefficient 1 implied
constexpr double Z1 = 1.46819706421238932572E1;
constexpr double Z2 = 4.92184563216946036703E1;
constexpr double THPIO4 = 2.35619449019234492885;        // 3 pi / 4
}  // namespace j1c

__device__ __forceinline__ double bessel_j1(double x) {
    using namespace j1c;
    const double ax = fabs(x);
    double v;
    if (ax <= 5.0) {
        const double z = ax * ax;
        v = j0_poly(z, RP) / j0_poly1(z, RQ) * ax * (z - Z1) * (z - Z2);
    } else {
        const double w = 5.0 / ax;
        const double q = w * w;
        const double p = j0_poly(q, PP) / j0_poly(q, PQ);
        const double qq = j0_poly(q, QP) / j0_poly1(q, QQ);
        double s, c;
        sincos(ax - THPIO4, &s, &c);
        v = (p * c - w * qq * s) * j0c::SQ2OPI / sqrt(ax);
    }
    return x < 0.0 ? -v : v;
}

constexpr double J2_SERIES_X = 2.0;
constexpr int J2_SERIES_N = 12;

__device__ __forceinline__ double bessel_j2(double x) {
    x = fabs(x);
    if (x < J2_SERIES_X) {
        const double y = 0.25 * x * x;
        double a = 1.0;
#pragma unroll
        for (int k = J2_SERIES_N; k >= 1; --k) a = 1.0 - y * (1.0 / (k * (k + 2.0))) * a;
        return 0.5 * y * a;
    }
    return 2.0 * bessel_j1(x) / x - bessel_j0(x);
}

}  // namespace hmg
