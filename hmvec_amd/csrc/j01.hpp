// J0(x) and J1(x) of one argument x >= 0 together, in fp64 for gfx950: the Hankel transforms of kernels/realspace.hpp
// need both at every node.  The algorithm and the coefficients are those of j0.hpp and j1.hpp (Cephes 2.8 j0.c / j1.c),
// taken from their tables; what is shared is the large-argument phase.  With chi = x - pi/4,
//   cos(x - 3 pi/4) = sin(chi),   sin(x - 3 pi/4) = -cos(chi)            (exact identities),
// so  J0 = sqrt(2/(pi x)) [P0 cos(chi) - (5/x) Q0 sin(chi)],   J1 = sqrt(2/(pi x)) [P1 sin(chi) + (5/x) Q1 cos(chi)]
// take ONE sincos and one 1/sqrt(x).  Accuracy: chi is x - pi/4 rounded once (half an ulp of x, as the two separate
// subtractions of j0.hpp and j1.hpp are), and its sine and cosine come from sincos_fast (sici.hpp: < 1 ulp of the result
// + 2e-16 absolute) below 2^30 and from the library's full-range reduction beyond; both are scaled by
// sqrt(2/(pi x)) <= 0.36 here, so the absolute error of J0 and J1 stays that of the Cephes forms (a few 1e-16) plus half
// an ulp of x radians of phase, which the callers' gates carry as their phase term.  Measured on the device against
// 50-digit arithmetic (tests/test_gpu_math_probe.py: zeros and their neighbours, both sides of 5 and of chi = 2^30, x to
// 1e15), with u = 2^-53 and s = 1 for J0, min(1, x) for J1: |error| <= 8 u s + [x > 5] sqrt(2/(pi x)) (spacing(x)/2 +
// 2e-16) everywhere; up to 5 the worst is 2.8 u (J0) and 1.7 u s (J1), above it the phase term is reached to 0.94 (J0)
// and 0.97 (J1).  bessel_j0, bessel_j1 and bessel_j2 of j0.hpp and j1.hpp meet the same bound on both signs.
#pragma once
#include "j1.hpp"
#include "sici.hpp"

namespace hmg {

__device__ __forceinline__ void bessel_j01(double x, double& j0, double& j1) {
    if (x <= 5.0) {
        const double z = x * x;
        j0 = (z - j0c::DR1) * (z - j0c::DR2) * j0_poly(z, j0c::RP) / j0_poly1(z, j0c::RQ);
        j1 = j0_poly(z, j1c::RP) / j0_poly1(z, j1c::RQ) * x * (z - j1c::Z1) * (z - j1c::Z2);
        return;
    }
    const double w = 5.0 / x;
    const double q = w * w;
    const double p0 = j0_poly(q, j0c::PP) / j0_poly(q, j0c::PQ);
    const double q0 = j0_poly(q, j0c::QP) / j0_poly1(q, j0c::QQ);
    const double p1 = j0_poly(q, j1c::PP) / j0_poly(q, j1c::PQ);
    const double q1 = j0_poly(q, j1c::QP) / j0_poly1(q, j1c::QQ);
    const double chi = x - j0c::PIO4;
    double s, c;
    if (chi < 0x1p30) sincos_fast(chi, s, c);
    else sincos(chi, &s, &c);
    const double amp = j0c::SQ2OPI / sqrt(x);
    j0 = (p0 * c - w * q0 * s) * amp;
    j1 = (p1 * s + w * q1 * c) * amp;
}

}  // namespace hmg
