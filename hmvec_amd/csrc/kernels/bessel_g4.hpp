// G_4(x) = int_0^x t J_4(t) dt = 4 + 8 J0 + x J1 - 24 J1/x  (-> x^6/2304), the antiderivative that vanishes at 0: the end
// terms of W_4 (F1 of kernels/hankel.hpp) and the order-4 bin-averaged weight (kernels/angcov.hpp,
// section 23).  Plain C++ with no kernels: both units include it, and tests/cpp/angcov_host.cpp builds it with a host
// compiler.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define HMG_HD_FN __host__ __device__ __forceinline__
#else
#define HMG_HD_FN inline
#endif

namespace hmg {

// Below this x G_4 comes from its power series in y = x^2/4,
//   G_4 = y^3/36 (1 - 3y/(4*1*5) (1 - 4y/(5*2*6) (1 - ...))),       ratio of terms k-1 -> k:  y (k+2) / ((k+3) k (k+4))
// nested through k = G4_SERIES_N; the choice of the switch and of the term count is analysed in kernels/hankel.hpp with
// F2's.  Both branches are evaluated and selected.
constexpr double G4_SERIES_X = 5.0;
constexpr int G4_SERIES_N = 15;

// G_4(x) given J0(x) and J1(x)
HMG_HD_FN double bessel_g4(double x, double j0, double j1) {
    const double y = 0.25 * x * x;
    double s = 1.0;
#pragma unroll
    for (int k = G4_SERIES_N; k >= 1; --k) s = std::fma(-y * ((k + 2.0) / ((k + 3.0) * k * (k + 4.0))), s, 1.0);
    const bool series = x < G4_SERIES_X;
    const double d = series ? 1.0 : x;            // (the closed form is not used below the switch)
    return series ? y * y * y * (1.0 / 36.0) * s : std::fma(x, j1, std::fma(8.0, j0, 4.0)) - 24.0 * j1 / d;
}

}  // namespace hmg
