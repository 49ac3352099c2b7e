// Device Bessel function of the first kind, order zero, J0(x), in fp64 for gfx950.
//
// The reference's two-halo lensing term calls scipy.special.j0 (hmvec/hmvec.py:599), a third-party routine not in the
// reference tree: Cephes Math Library 2.8 `j0.c` (S. L. Moshier, 1984-2000).  This is a restatement of that published
// algorithm with its published coefficients:
//   * 0 <= x <= 5:  J0 = (z - DR1)(z - DR2) RP(z) / RQ(z),  z = x^2, with DR1, DR2 the squares of the first two zeros
//                   of J0, so that the rational stays accurate in relative terms around them;
//   * x > 5:        the Hankel form  J0 = sqrt(2/(pi x)) [P0(x) cos(x - pi/4) - (5/x) Q0(x) sin(x - pi/4)]  with
//                   P0, Q0 rationals in 25/x^2.
// J0 is even: the argument is taken by absolute value.
#pragma once
#include <hip/hip_runtime.h>

namespace hmg {

namespace j0c {
constexpr double PP[7] = {7.96936729297347051624E-4, 8.28352392107440799803E-2, 1.23953371646414299388E0,
                          5.44725003058768775090E0,  8.74716500199817011941E0,  5.30324038235394892183E0,
                          9.99999999999999997821E-1};
constexpr double PQ[7] = {9.24408810558863637013E-4, 8.56288474354474431428E-2, 1.25352743901058953537E0,
                          5.47097740330417105182E0,  8.76190883237069594232E0,  5.30605288235394617618E0,
                          1.00000000000000000218E0};
constexpr double QP[8] = {-1.13663838898469149931E-2, -1.28252718670509318512E0, -1.95539544257735972385E1,
                          -9.32060152123768231369E1,  -1.77681167980488050595E2, -1.47077505154951170175E2,
                          -5.14105326766599330220E1,  -6.05014350600728481186E0};
constexpr double QQ[7] = {6.43178256118178023184E1, 8.56430025976980587198E2, 3.88240183605401609683E3,
                          7.24046774195652478189E3, 5.93072701187316984827E3, 2.06209331660327847417E3,
                          2.42005740240291393179E2};   // leading coefficient 1 implied
constexpr double RP[4] = {-4.79443220978201773821E9, 1.95617491946556577543E12, -2.49248344360967716204E14,
                          9.70862251047306323952E15};
constexpr double RQ[8] = {4.99563147152651017219E2,  1.73785401676374683123E5,  4.84409658339962045305E7,
                          1.11855537045356834862E10, 2.11277520115489217587E12, 3.10518229857422583814E14,
                          3.18121955943204943306E16, 1.71086294081043136091E18};   // leading coefficient 1 implied
constexpr double DR1 = 5.78318596294678452118E0;
constexpr double DR2 = 3.04712623436620863991E1;
constexpr double SQ2OPI = 7.9788456080286535587989E-1;   // sqrt(2/pi)
constexpr double PIO4 = 7.85398163397448309616E-1;
}  // namespace j0c

template <int N>
__device__ __forceinline__ double j0_poly(double x, const double (&c)[N]) {
    double a = c[0];
#pragma unroll
    for (int i = 1; i < N; ++i) a = a * x + c[i];
    return a;
}
template <int N>
__device__ __forceinline__ double j0_poly1(double x, const double (&c)[N]) {   // leading coefficient 1
    double a = x + c[0];
#pragma unroll
    for (int i = 1; i < N; ++i) a = a * x + c[i];
    return a;
}

__device__ __forceinline__ double bessel_j0(double x) {
    using namespace j0c;
    x = fabs(x);
    if (x <= 5.0) {
        const double z = x * x;
        return (z - DR1) * (z - DR2) * j0_poly(z, RP) / j0_poly1(z, RQ);
    }
    const double w = 5.0 / x;
    const double q = 25.0 / (x * x);
    const double p = j0_poly(q, PP) / j0_poly(q, PQ);
    const double qq = j0_poly(q, QP) / j0_poly1(q, QQ);
    double s, c;
    sincos(x - PIO4, &s, &c);
    return (p * c - w * qq * s) * SQ2OPI / sqrt(x);
}

}  // namespace hmg
