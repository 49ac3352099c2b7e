// Spherical Bessel functions j_0 .. j_L at one argument x > 0 in fp64: what the non-Limber
// transfer functions are sums of.  Plain C++ with device qualifiers under hipcc: a host compiler builds it as it is.
//
// x >= L: upward.  j_0 = sin x / x, j_1 = (j_0 - cos x) / x (below SB_SERIES_X its series: the difference loses x^2),
//   j_{l+1} = (2l + 1)/x j_l - j_{l-1}: neutrally stable while l <= x.
// x <  L: Miller.  y_{N+1} = 0, y_N = 1 at the start order N = sb_start_order(L) - a function of L alone - and
//   y_{l-1} = (2l + 1)/x y_l - y_{l+1} down to l = 0: the minimal solution grows downwards, whatever the start holds of
//   the other one has died by l = L (N - L >= 24 + 9 L^(1/3): (j_N y_L)/(j_L y_N) < 1e-18 at the worst x, x = L).  When
//   |y| passes SB_BIG = 2^512 both values are multiplied by SB_TINY = 2^-512 - exact - and the count c of such rescalings
//   goes up; y_l is remembered with the count c_l at which it was formed.  At l = 0 the pair (y_0, y_1) carries the final
//   count c_0 and s = j_0 / y_0 or j_1 / y_1, whichever true value is larger in magnitude (never a zero of either), and
//   j_l = y_l s 2^(-512 (c_0 - c_l)), the powers applied one by one: a value below the fp64 range comes out as a
//   denormal and then as 0, never as NaN.
// Both walks take (2l + 1)/x from 1/x held as a pair (rh, rl = (1 - rh x) rh): fma(2l + 1, rh, (2l + 1) rl) is the
// quotient to within 1e-3 of a rounding, at the price of a multiplication, not of a division.  With a rounded 1/x alone every
// coefficient would be off by the same factor, the walk that of a neighbouring argument, and the error x 2^-54 times the
// envelope.  The step itself is ONE fma; nothing else is fused.  The walk is given
// twice: sb_all writes a column (the probe and the free function), the transfer kernel (kernels/nonlimber.hpp) steps
// sb_up / sb_down itself, a tile of l at a time - the same operations in the same order, the same bits.
// Below SB_XMIN = 1e-100 the step's factor would overflow: there j_0 = 1, j_1 = x / 3 and every higher order is 0 (the
// callers refuse such arguments; the branch keeps a stray one finite).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define HMG_SB_FN __host__ __device__ __forceinline__
#else
#define HMG_SB_FN inline
#endif

namespace hmg {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr double SB_BIG = 0x1p512, SB_TINY = 0x1p-512, SB_XMIN = 1e-100, SB_SERIES_X = 0.25;

// the start order of the downward walk: L + 24 + 9 ceil(L^(1/3)), in integers (the host and the device agree)
HMG_SB_FN int sb_start_order(int L) {
    int c = 0;
    while ((long long)c * c * c < L) ++c;
    return L + 24 + 9 * c;
}

// 1 / x as a pair, and (2l + 1)/x = sb_coef(2l + 1, r)
struct sb_recip {
    double h, l;
};
HMG_SB_FN sb_recip sb_recip_of(double x) {
    const double h = 1.0 / x;
    return sb_recip{h, std::fma(-h, x, 1.0) * h};
}
HMG_SB_FN double sb_coef(double t, const sb_recip& r) { return std::fma(t, r.h, t * r.l); }

// j_0 and j_1 at x >= SB_XMIN; rx = 1 / x
HMG_SB_FN void sb_j01(double x, double rx, double& j0, double& j1) {
    const double s = std::sin(x), c = std::cos(x);
    j0 = s * rx;
    const double x2 = x * x;
    const double ser = x * (1.0 / 3.0) * (1.0 - x2 * (1.0 / 10.0) * (1.0 - x2 * (1.0 / 28.0) * (1.0 - x2 * (1.0 / 54.0) *
                       (1.0 - x2 * (1.0 / 88.0) * (1.0 - x2 * (1.0 / 130.0))))));
    j1 = x < SB_SERIES_X ? ser : (j0 - c) * rx;
}

// upward: a = j_l, b = j_{l+1}
struct sb_up {
    double a, b;
};
HMG_SB_FN void sb_up_step(sb_up& u, int l, const sb_recip& r) {  // l -> l + 1
    const double n = std::fma(sb_coef(2.0 * l + 3.0, r), u.b, -u.a);
    u.a = u.b, u.b = n;
}

// downward: a = y_l, b = y_{l+1}, c rescalings so far
struct sb_down {
    double a, b;
    int c;
};
HMG_SB_FN sb_down sb_down_start() { return sb_down{1.0, 0.0, 0}; }
HMG_SB_FN void sb_down_step(sb_down& d, int l, const sb_recip& r) {   // l -> l - 1
    const double n = std::fma(sb_coef(2.0 * l + 1.0, r), d.a, -d.b);
    d.b = d.a, d.a = n;
    if (std::fabs(n) > SB_BIG) d.a *= SB_TINY, d.b *= SB_TINY, ++d.c;
}
// the scale s of a walk that has arrived at l = 0, from the true j_0, j_1
HMG_SB_FN double sb_down_scale(const sb_down& d, double j0, double j1) {
    return std::fabs(j0) >= std::fabs(j1) ? j0 / d.a : j1 / d.b;
}
// j_l of y_l formed at count c, the final count c0
HMG_SB_FN double sb_down_value(double y, int c, double s, int c0) {
    double v = y * s;
    for (int m = c0 - c; m > 0 && v != 0.0; --m) v *= SB_TINY;
    return v;
}

// j_0 .. j_L at x into out[l * stride]; N = sb_start_order(L)
HMG_SB_FN void sb_all(double x, int L, int N, double* out, size_t stride) {
    if (!(x >= SB_XMIN)) {
        for (int l = 0; l <= L; ++l) out[l * stride] = l == 0 ? 1.0 : l == 1 ? x * (1.0 / 3.0) : 0.0;
        return;
    }
    const sb_recip rx = sb_recip_of(x);
    double j0, j1;
    sb_j01(x, rx.h, j0, j1);
    if (x >= (double)L) {
        sb_up u{j0, j1};
        for (int l = 0; l <= L; ++l) {
            out[l * stride] = u.a;
            sb_up_step(u, l, rx);
        }
        return;
    }
    sb_down d = sb_down_start();
    for (int l = N; l > 0; --l) sb_down_step(d, l, rx);
    const double s = sb_down_scale(d, j0, j1);
    const int c0 = d.c;
    d = sb_down_start();
    for (int l = N; l > L; --l) sb_down_step(d, l, rx);
    for (int l = L; l >= 0; --l) {
        out[l * stride] = sb_down_value(d.a, d.c, s, c0);
        if (l > 0) sb_down_step(d, l, rx);
    }
}

}  // namespace hmg
