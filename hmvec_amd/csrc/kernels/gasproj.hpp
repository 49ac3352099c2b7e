// Projected profiles of the generalised NFW family f(x) = x^gamma (1 + x^alpha)^(-eta), truncated at xcut (DESIGN.md
// section 18): the line-of-sight projection F(s), its mean G(s) inside a disc, the excess G - F, and F convolved with a
// circular Gaussian.  The Battaglia gas density and pressure profiles are members of the family, so these kernels are
// behind HaloModel.gas_sigma_1h_profiles, gas_delta_sigma_1h_profiles, tau_1h_profiles and y_1h_profiles.  Compiled in
// gasproj.hip, a translation unit of its own (kept out of hmgrid.hip: extra instantiations there change the hot kernels'
// code).  All fp64 on the vector units, fixed summation order, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "../i0e.hpp"
#include "../rowdev.hpp"

namespace hmg {

// ---------------------------------------------------------------- node tables
// GNFW_N Gauss-Legendre nodes on [0, 1] serve both the line of sight (in t) and the inner sphere (in v); GNFW_NS nodes per
// segment serve the outer integral of the smoothing.  Built once on the host (gasproj.hip: build_gnfw_quad) and copied
// here before the first launch on a device.  The layout is also what hmg_gnfw_quad_table hands out.
constexpr int GNFW_N = 64;
constexpr int GNFW_NS = 32;                 // two segments: one outer node per lane of a wavefront
constexpr double GNFW_SMOOTH_RMAX = 10.0;   // Gaussian tail beyond 10 sigma: exp(-50) ~ 2e-22
struct GnfwQuad {
    double u[GNFW_N], w[GNFW_N];                        // nodes and weights on [0, 1]
    double v2[GNFW_N], lv2[GNFW_N], wv[GNFW_N];         // inner sphere, r = b v^2: v^2, ln v^2, 2 v w
    double sg[GNFW_NS], cg[GNFW_NS], wj[GNFW_NS];       // smoothing, g = sin^2(pi u / 2): g, 1 - g, w (pi/2) sin(pi u)
};
__constant__ GnfwQuad gnfw_quad;

// x^g (1 + x^alpha)^(-eta) from lr = ln x (and x itself for the alpha == 1 member): the row kernels' evaluation
template <bool A1>
__device__ __forceinline__ double gnfw_pow(double lr, double r, double al, double et, double g) {
    if constexpr (A1) return gnfw_rho_alpha1(lr, r, 1.0, et, g);
    else return gnfw_rho_fast(lr, 1.0, al, et, g);
}

// ---------------------------------------------------------------- line of sight, s < xcut
// l = s sinh t, r = s cosh t, t in [0, T], T = arcosh(xcut / s):
//     F(s) = 2 int_0^T f(r) r dt                                              (dl = r dt)
//     outer(s) = int_s^xcut r^2 f(r) (1 - sqrt(1 - s^2/r^2)) dr = s int_0^T f(r) r  r sinh t (1 - tanh t) dt.
// The integrands are analytic in t (nearest singularities at Im t = pi/2 and pi/alpha), so Gauss-Legendre in t converges
// spectrally even where T ~ 13 (s = 1e-3, xcut = 200).  With e1 = exp(-t), e2 = e1^2:
//     ln r = ln(s/2) + t + log1p(e2),   r = s (1 + e2) / (2 e1),   sinh t (1 - tanh t) = e1 (1 - e2) / (1 + e2),
// and f(r) r = exp((gamma + 1) ln r - eta log1p(r^alpha)): one short exp for e1, one short log, and the family's
// evaluation with gamma + 1.  T comes from xcut - s, so that it keeps its relative accuracy as s -> xcut.
// F = 2 (T sum): the factor 2 is applied last, so G - F may or may not be contracted to a fused multiply-add - the bits
// are the same.
template <bool MEAN, bool A1>
__device__ __forceinline__ void gnfw_los(double s, double xc, double al, double et, double ga, double& F, double& outer) {
    const double um1 = (xc - s) / s;
    const double T = log1p(um1 + sqrt(um1 * (um1 + 2.0)));
    const double l0 = log(s) - 0.693147180559945309417;
    double aF = 0.0, aO = 0.0;
#pragma unroll 2
    for (int i = 0; i < GNFW_N; ++i) {
        const double t = T * gnfw_quad.u[i];
        const double e1 = exp_fast<false>(-t), e2 = e1 * e1;
        const double lr = l0 + t + log1p_abs(e2);
        const double r = 0.5 * s * (1.0 + e2) * fm_rcp(e1);
        const double fr = gnfw_quad.w[i] * gnfw_pow<A1>(lr, r, al, et, ga + 1.0);
        aF += fr;
        if constexpr (MEAN) aO += fr * r * (e1 * (1.0 - e2) * fm_rcp(1.0 + e2));
    }
    F = 2.0 * (T * aF);
    outer = MEAN ? T * s * aO : 0.0;
}

// int_0^b r^2 f(r) dr with r = b v^2, which absorbs r^(2 + gamma): the integrand is v^(5 + 2 gamma) times a factor smooth
// in v^(2 alpha)
template <bool A1>
__device__ __forceinline__ double gnfw_inner(double b, double al, double et, double ga) {
    const double lb = log(b);
    double a = 0.0;
#pragma unroll 2
    for (int i = 0; i < GNFW_N; ++i)
        a += gnfw_quad.wv[i] * gnfw_pow<A1>(lb + gnfw_quad.lv2[i], b * gnfw_quad.v2[i], al, et, ga + 2.0);
    return b * a;
}

// F (kind 0), G (1) or G - F (2) at s.  G = M_cyl(s) / (pi s^2), M_cyl = 4 pi (int_0^min(s, xcut) r^2 f dr + outer(s)); for
// s >= xcut F is 0.0 and G is N / (pi s^2).  Every kind runs the same line-of-sight loop, so "excess" is "mean" minus
// "sigma" bit for bit.
template <bool A1>
__device__ __forceinline__ double gnfw_core(int kind, double s, double xc, double al, double et, double ga) {
    double F = 0.0, outer = 0.0;
    const bool inside = s < xc;
    if (inside) gnfw_los<true, A1>(s, xc, al, et, ga, F, outer);
    if (kind == 0) return F;
    const double G = 4.0 * (gnfw_inner<A1>(inside ? s : xc, al, et, ga) + outer) / (s * s);
    if (kind == 1) return G;
    {
#pragma clang fp contract(off)
        return G - F;
    }
}

// one thread per (row, radius); x has row stride xstride (0: one row shared by every profile).  general != 0 sends
// alpha == 1 rows through the general evaluation too (testing)
__global__ __launch_bounds__(256) void gnfw_projected_kernel(size_t total, int nr, int xstride, int kind, int general,
                                                            const double* __restrict__ alpha,
                                                            const double* __restrict__ eta,
                                                            const double* __restrict__ xcut, double gamma,
                                                            const double* __restrict__ x, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t h = i / nr, j = i % nr;
    const double al = alpha[h], et = eta[h], xc = xcut[h];
    const double s = x[h * xstride + j];
    out[i] = (al == 1.0 && !general) ? gnfw_core<true>(kind, s, xc, al, et, gamma)
                                     : gnfw_core<false>(kind, s, xc, al, et, gamma);
}

// ---------------------------------------------------------------- Gaussian smoothing of F
// F_sigma(s) = int_0^inf ds' (s'/sig^2) exp(-(s - s')^2 / 2 sig^2) I0e(s s'/sig^2) F(s'): the convolution of the projected
// profile with a circular Gaussian of width sig (a beam), which is also its average over Rayleigh-distributed centre
// offsets.  F vanishes beyond xcut and the Gaussian beyond GNFW_SMOOTH_RMAX sig, so the range is [a, b] =
// [max(0, s - 10 sig), min(xcut, s + 10 sig)], empty when s - 10 sig >= xcut (the result is then 0).  It is split at
// c = s (the peak) when s < b, else at its middle.  One wavefront per output: lanes 0-31 own the nodes of [a, c], lanes
// 32-63 those of [c, b], each segment mapped by s' = lo + (hi - lo) sin^2(pi u / 2), u Gauss-Legendre on [0, 1]: the nodes
// cluster quadratically at both ends of both segments, which takes the s'^(1 + gamma) cusp of F at s' -> 0 and its
// square-root edge at xcut (nodes in the upper half of a segment are formed from its upper end, so their distance to xcut is
// not a rounded difference).  Each lane evaluates F at its node through gnfw_los, the device function of the unsmoothed
// kernel; the wave reduces in a fixed xor-butterfly order: a repeated call is bit-identical.
template <bool A1>
__device__ __forceinline__ double gnfw_F(double s, double xc, double al, double et, double ga) {
    double F = 0.0, outer;
    if (s < xc) gnfw_los<false, A1>(s, xc, al, et, ga, F, outer);
    return F;
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void gnfw_smooth_kernel(size_t total, int nr, int xstride, int general,
                                                                 const double* __restrict__ alpha,
                                                                 const double* __restrict__ eta,
                                                                 const double* __restrict__ xcut, double gamma,
                                                                 const double* __restrict__ x,
                                                                 const double* __restrict__ sigma,
                                                                 double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const size_t o = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (o >= total) return;                        // wave-uniform: no barrier follows
    const size_t h = o / nr, j = o % nr;
    const double al = alpha[h], et = eta[h], xc = xcut[h], sig = sigma[h];
    const double s = x[h * xstride + j];
    const double a = fmax(0.0, s - GNFW_SMOOTH_RMAX * sig), b = fmin(xc, s + GNFW_SMOOTH_RMAX * sig);
    if (!(b > a)) {                                // wave-uniform
        if (lane == 0) out[o] = 0.0;
        return;
    }
    const double c = s < b ? s : 0.5 * (a + b);
    const int k = lane & (GNFW_NS - 1);
    const double lo = lane < GNFW_NS ? a : c, hi = lane < GNFW_NS ? c : b, len = hi - lo;
    const double sp = k < GNFW_NS / 2 ? lo + len * gnfw_quad.sg[k] : hi - len * gnfw_quad.cg[k];
    const double F = (al == 1.0 && !general) ? gnfw_F<true>(sp, xc, al, et, gamma) : gnfw_F<false>(sp, xc, al, et, gamma);
    const double is2 = 1.0 / (sig * sig), d = s - sp;
    double v = gnfw_quad.wj[k] * len * (sp * is2) * exp(-0.5 * d * d * is2) * bessel_i0e(s * sp * is2) * F;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) out[o] = v;
}

}  // namespace hmg
