// Even moments of a Gaussian on [0, 1],  M_n(t) = int_0^1 mu^(2n) exp(-t mu^2) dmu,  n = 0, 1, 2,  t >= 0, in fp64: what
// the Legendre multipoles l = 0, 2, 4 of a Gaussian-damped redshift-space spectrum are made of (kernels/rsd.hpp;
// DESIGN.md section 19).
//   * t < GM_SWITCH:  M_n = sum_j (-t)^j / (j! (2n + 2j + 1)),  j < GM_TERMS, in Horner form with explicit fma; t = 0
//     gives the leading coefficient 1 / (2n + 1).  The first term left out is below t^20 / (20! 41) < 1.1e-20.
//   * t >= GM_SWITCH: M_0 = sqrt(pi / 4t) erf(sqrt t),  M_{n+1} = ((2n + 1) M_n - exp(-t)) / (2t).  The recurrence loses
//     accuracy as t falls (M_n -> 1 / (2n + 1) is a difference of terms of size 1 / t): hence the series below the switch.
// Measured against 40-digit arithmetic (tests/test_rsd_cpu.py, host build): section 19.
// Plain C++: __host__ __device__ under hipcc, inline under a host compiler; no HIP include (tests/cpp/
// gauss_moments_host.cpp builds it with g++).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define HMG_GM_FN __host__ __device__ __forceinline__
#else
#define HMG_GM_FN inline
#endif

namespace hmg {

constexpr double GM_SWITCH = 1.0;
constexpr int GM_TERMS = 20;

namespace gm {
// 1 / j!, j = 0 .. 19
constexpr double RFACT[GM_TERMS] = {1.0,
                                    1.0,
                                    1.0 / 2.0,
                                    1.0 / 6.0,
                                    1.0 / 24.0,
                                    1.0 / 120.0,
                                    1.0 / 720.0,
                                    1.0 / 5040.0,
                                    1.0 / 40320.0,
                                    1.0 / 362880.0,
                                    1.0 / 3628800.0,
                                    1.0 / 39916800.0,
                                    1.0 / 479001600.0,
                                    1.0 / 6227020800.0,
                                    1.0 / 87178291200.0,
                                    1.0 / 1307674368000.0,
                                    1.0 / 20922789888000.0,
                                    1.0 / 355687428096000.0,
                                    1.0 / 6402373705728000.0,
                                    1.0 / 121645100408832000.0};

// the coefficient 1 / (j! (2N + 2j + 1)), a compile-time constant
template <int N, int J>
constexpr double COEF = RFACT[J] / (2 * N + 2 * J + 1);

// Horner steps J, J - 1, ..., 0 of sum_j COEF<N, j> y^j (unrolled by recursion: no loop, every coefficient a literal)
template <int N, int J>
HMG_GM_FN double horner(double p, double y) {
    if constexpr (J < 0) return p;
    else return horner<N, J - 1>(std::fma(p, y, COEF<N, J>), y);
}

// sum_j (-t)^j / (j! (2N + 2j + 1))
template <int N>
HMG_GM_FN double series(double t) {
    return horner<N, GM_TERMS - 2>(COEF<N, GM_TERMS - 1>, -t);
}
}  // namespace gm

// M_0, M_1, M_2 at t >= 0
HMG_GM_FN void gauss_moments(double t, double& m0, double& m1, double& m2) {
    if (t < GM_SWITCH) {
        m0 = gm::series<0>(t);
        m1 = gm::series<1>(t);
        m2 = gm::series<2>(t);
        return;
    }
    const double e = std::exp(-t), h = 0.5 / t;
    m0 = std::sqrt(0.78539816339744830962 / t) * std::erf(std::sqrt(t));
    m1 = (m0 - e) * h;
    m2 = std::fma(3.0, m1, -e) * h;
}

}  // namespace hmg
