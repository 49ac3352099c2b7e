// Cluster-lensing profiles of HaloModel (hmvec/hmvec.py:574-625): the projected NFW surface density, centred and
// miscentred, and the two-halo convergence; the excess surface density, centred and miscentred,
// and the two-halo tangential shear.  Compiled in lensing.hip,
// a translation unit of its own (kept out of hmgrid.hip: extra instantiations there change the hot kernels' code).
// One kernel template per family (centred, miscentred, two-halo), instantiated for Sigma / kappa and for Delta Sigma /
// gamma_t: each instantiation is checked by ISA diff to be the code of the kernel written out on its own.
#pragma once
#include <hip/hip_runtime.h>

#include "../j0.hpp"
#include "../j1.hpp"

namespace hmg {

// ---------------------------------------------------------------- centred Sigma (Wright & Brainerd 2000, eq. 11)
// Sigma(R) = 2 r_s delta_c rho_c f(x), x = R / r_s.  Near x = 1 the closed forms of both branches are a difference of
// two nearly equal terms divided by x^2 - 1.  In t = (1 - x) / (1 + x) (x < 1: t > 0, artanh branch; x > 1: t < 0,
// arctan branch) the two branches are one analytic function,
//     f = (1 + t)^2 sum_{n >= 0} (n + 1) t^n / ((2n + 1)(2n + 3)),
// (expand artanh(s)/s resp. arctan(s)/s in s^2 = |t|; 1 + x = 2 / (1 + t) makes the leading 1 cancel term by term),
// so |t| < LENS_SERIES_T takes the series: 16 terms leave a truncation below 0.1^16 / 64 of f(1) = 1/3.
constexpr double LENS_SERIES_T = 0.1;
constexpr int LENS_SERIES_N = 16;

__device__ __forceinline__ double nfw_sigma_shape(double x) {
    const double t = (1.0 - x) / (1.0 + x);
    if (fabs(t) < LENS_SERIES_T) {
        double a = 0.0;
#pragma unroll
        for (int n = LENS_SERIES_N - 1; n >= 0; --n) a = a * t + (double)(n + 1) / ((2.0 * n + 1.0) * (2.0 * n + 3.0));
        return (1.0 + t) * (1.0 + t) * a;
    }
    const double xm1xp1 = (x - 1.0) * (x + 1.0);
    if (x < 1.0) {
        // artanh(s), s = sqrt(t) = sqrt((1-x)/(1+x)), as log((1+s) / sqrt(1-s^2)) with 1 - s^2 = 2x/(1+x) formed
        // exactly: no 1 - s when s -> 1 (x -> 0)
        const double s = sqrt(t);
        const double ath = log1p(s) - 0.5 * log(2.0 * x / (1.0 + x));
        return (1.0 - 2.0 / sqrt(-xm1xp1) * ath) / xm1xp1;
    }
    return (1.0 - 2.0 / sqrt(xm1xp1) * atan(sqrt(-t))) / xm1xp1;
}

// ---------------------------------------------------------------- centred Delta Sigma (Wright & Brainerd 2000, eqs. 13-15)
// Mean Sigma inside x over A: g(x) = (2/x^2) [h(x) + ln(x/2)], h = 2/sqrt(1-x^2) artanh sqrt((1-x)/(1+x)) (x < 1),
// 2/sqrt(x^2-1) arctan sqrt((x-1)/(1+x)) (x > 1), h(1) = 1.  In the t of nfw_sigma_shape both branches are
// h = (1 + t) sum_{n >= 0} t^n / (2n + 1) (artanh(s)/s resp. arctan(s)/s in s^2 = |t|, and sqrt|1-x^2| = 2 sqrt|t|/(1+t)),
// taken for |t| < LENS_SERIES_T with the same 16 terms (truncation below 0.1^16 / 33).  For x < 1, h = arccosh(1/x)/q with
// q = sqrt(1-x^2), and h + ln(x/2) = O(x^2 ln x) loses 2 log10(1/x) digits as written.  With
// arccosh(1/x) = ln(2/x) + log1p(u), u = -x^2 / (2 (1 + q)), and 1/q - 1 = x^2 / (q (1 + q)):
//     g = 2 [ln(2/x) / (q (1 + q)) - (log1p(u)/u) / (2 q (1 + q))],
// a sum of two terms of opposite sign whose ratio stays above 1.6: no cancellation at any x < 1.
__device__ __forceinline__ double nfw_mean_sigma_shape(double x) {
    const double t = (1.0 - x) / (1.0 + x);
    if (fabs(t) < LENS_SERIES_T) {
        double a = 0.0;
#pragma unroll
        for (int n = LENS_SERIES_N - 1; n >= 0; --n) a = a * t + 1.0 / (2.0 * n + 1.0);
        return 2.0 * ((1.0 + t) * a + log(0.5 * x)) / (x * x);
    }
    if (x < 1.0) {
        const double q = sqrt((1.0 - x) * (1.0 + x));
        const double u = -x * x / (2.0 * (1.0 + q));
        const double l1pu = u == 0.0 ? 1.0 : log1p(u) / u;
        return 2.0 * (log(2.0 / x) / (q * (1.0 + q)) - l1pu / (2.0 * q * (1.0 + q)));
    }
    const double xm1xp1 = (x - 1.0) * (x + 1.0);
    return 2.0 * (2.0 / sqrt(xm1xp1) * atan(sqrt(-t)) + log(0.5 * x)) / (x * x);
}

__device__ __forceinline__ double nfw_sigma_amp(double rs, double dc, double rhoc) { return 2.0 * rs * dc * rhoc; }

// one thread per (halo, radius); rbins has row stride rstride (0: one row shared by every halo).  With A = 2 r_s delta_c
// rho_c it stores Sigma = A f(x), or with DELTA the excess Delta Sigma = A (g(x) - f(x))
template <bool DELTA>
__global__ void lensing_centred_kernel(size_t total, int nr, int rstride, const double* __restrict__ rs,
                                       const double* __restrict__ dc, const double* __restrict__ rhoc,
                                       const double* __restrict__ rbins, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t h = i / nr, j = i % nr;
    const double r_s = rs[h];
    const double x = rbins[h * rstride + j] / r_s;
    const double A = nfw_sigma_amp(r_s, dc[h], rhoc[h]);
    if constexpr (DELTA) out[i] = A * (nfw_mean_sigma_shape(x) - nfw_sigma_shape(x));
    else out[i] = A * nfw_sigma_shape(x);
}

// ---------------------------------------------------------------- miscentred Sigma (Rayleigh offsets)
// Sigma_off(R) = int_0^inf dR' (R'/s^2) exp(-R'^2 / 2 s^2) (1/pi) int_0^pi dphi Sigma(sqrt(R^2 + R'^2 - 2 R R' cos phi)).
// One wavefront per output.  The 64 lanes own 64 angular nodes: phi = pi w^3 (w Gauss-Legendre on [0,1]) clusters
// them at phi = 0, where the integrand has its log singularity for R' = R; the radius is formed as
// (R - R')^2 + 4 R R' sin^2(phi/2), which keeps the small distances near the singularity exact.  The 64 outer nodes are
// Gauss-Legendre in w on two segments split at p = min(R, Rmax), Rmax = LENS_OFF_RMAX s, each mapped by w^2 so that
// they cluster at the split point: R' = p (1 - w^2) on [0, p] and R' = p + (Rmax - p) w^2 on [p, Rmax] (the azimuthal
// average has a |R' - R| log |R' - R| kink there).  Lane l forms outer node l, and the loop over the outer nodes reads
// node i from lane i (v_readlane: wave-uniform, lands in SGPRs).  Every lane sums its 64 terms in node order, then the
// wave reduces in a fixed xor-butterfly order: a repeated call is bit-identical.
constexpr int LENS_QUAD_N = 64;            // angular nodes = outer nodes = wavefront width
constexpr double LENS_OFF_RMAX = 10.0;     // Rayleigh tail beyond 10 sigma: exp(-50) ~ 2e-22
struct LensQuad {
    double w_outer[LENS_QUAD_N / 2], wt_outer[LENS_QUAD_N / 2];    // Gauss-Legendre on [0,1], 32 nodes
    double s2_phi[LENS_QUAD_N], wt_phi[LENS_QUAD_N];               // sin^2(phi_j/2), weight of (1/pi) dphi at node j
};
// built once on the host (lensing.hip: upload_once) and copied here before the first launch on a device
__constant__ LensQuad lens_quad;

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const unsigned long long b = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, lane);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---------------------------------------------------------------- miscentred Delta Sigma (Rayleigh offsets)
// Delta Sigma_off(R) = Sigmabar_off(<R) - Sigma_off(R).  With the order of integration swapped, Sigmabar_off(<R) is the
// Rayleigh average over the offset d of the centred profile's mass in a disc of radius R centred at distance d, over
// pi R^2:
//     M_disc(R, d) = [d < R] M_cyl(R - d) + int_{|R-d|}^{R+d} 2 r Sigma(r) arccos((r^2 + d^2 - R^2) / (2 r d)) dr,
// M_cyl(r) = pi r^2 A g(r / r_s) the full rings inside the disc.  The arc integral is mapped by r = a - b cos psi,
// a = max(R, d), b = min(R, d), psi in [0, pi] (dr = b sin psi dpsi: no square-root endpoints), so r = e + 2 b sin^2(psi/2)
// with e = a - b exact.  Half the arc angle is atan2(sqrt(N), sqrt(D)) with N / D = (1 - c) / (1 + c) formed from psi
// (sp = sin^2(psi/2), cp = cos^2(psi/2)) as products of positive terms:
//     d <= R:  N = cp (e + b sp),       D = sp (a + b sp);
//     d >  R:  N = b^2 cp sp,           D = (e + b sp)(a + b sp).
// psi = pi u^2 (u Gauss-Legendre on [0, 1]) clusters the nodes at psi = 0, where Sigma's log singularity sits when d = R.
// The same wavefront, outer nodes and loop as Sigma_off: the 64 lanes own both the angular node of Sigma_off and the
// psi node of the disc mass, and each lane adds the full rings M_cyl(R - d_l) of its own outer node once.  Both sums
// reduce in the fixed xor-butterfly order.
struct LensDiscQuad {
    double sp[LENS_QUAD_N], cp[LENS_QUAD_N];   // sin^2(psi_j/2), cos^2(psi_j/2)
    double wt[LENS_QUAD_N];                    // weight of dpsi at node j, times sin(psi_j)
};
// built once on the host (lensing.hip: upload_once) and copied here before the first launch on a device
__constant__ LensDiscQuad lens_disc_quad;

// DISC false stores Sigma_off; true adds the disc mass (a second sum and butterfly) and stores Delta Sigma_off
template <int WAVES, bool DISC>
__global__ __launch_bounds__(64 * WAVES) void lensing_off_kernel(
    size_t total, int nr, int rstride, const double* __restrict__ rs,
    const double* __restrict__ dc, const double* __restrict__ rhoc, const double* __restrict__ rbins,
    const double* __restrict__ offsets, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const size_t o = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (o >= total) return;                        // wave-uniform: no barrier follows
    const size_t h = o / nr, j = o % nr;
    const double r_s = rs[h];
    const double A = nfw_sigma_amp(r_s, dc[h], rhoc[h]);
    const double R = rbins[h * rstride + j];
    const double sig = offsets[h];

    // outer node of this lane
    const double rmax = LENS_OFF_RMAX * sig;
    const double p = fmin(R, rmax);
    const int k = lane & (LENS_QUAD_N / 2 - 1);
    const double w = lens_quad.w_outer[k], ww = lens_quad.wt_outer[k];
    const double len = lane < LENS_QUAD_N / 2 ? p : rmax - p;
    const double ro = lane < LENS_QUAD_N / 2 ? p - p * w * w : p + len * w * w;
    const double inv2s2 = 0.5 / (sig * sig);
    const double wo = 2.0 * len * w * ww * (ro / (sig * sig)) * exp(-ro * ro * inv2s2);
    // angular node and (DISC) psi node of this lane
    const double s2 = lens_quad.s2_phi[lane];
    const double sp = DISC ? lens_disc_quad.sp[lane] : 0.0, cp = DISC ? lens_disc_quad.cp[lane] : 0.0;

    double acc = 0.0, arc = 0.0;
    for (int i = 0; i < LENS_QUAD_N; ++i) {
        const double roi = readlane_f64(ro, i), woi = readlane_f64(wo, i);
        const double d = R - roi;
        const double r = sqrt(d * d + 4.0 * R * roi * s2);
        acc += woi * nfw_sigma_shape(r / r_s);
        if constexpr (DISC) {
            const double a = fmax(R, roi), b = fmin(R, roi), e = a - b, bs = b * sp;
            const double rr = e + 2.0 * bs;
            const bool inside = roi <= R;              // wave-uniform
            const double num = inside ? cp * (e + bs) : b * b * cp * sp;
            const double den = inside ? sp * (a + bs) : (e + bs) * (a + bs);
            arc += woi * b * rr * atan2(sqrt(num), sqrt(den)) * nfw_sigma_shape(rr / r_s);
        }
    }
    if constexpr (DISC) {
        // 2 r Sigma(r) arccos(c) dr = 4 (b r f(r / r_s) atan2(...)) (sin psi dpsi) A; the full rings of this lane's node
        const double rin = R - ro;
        const double cyl = rin > 0.0 ? M_PI * rin * rin * nfw_mean_sigma_shape(rin / r_s) : 0.0;
        double v = lens_quad.wt_phi[lane] * acc;
        double m = 4.0 * lens_disc_quad.wt[lane] * arc + wo * cyl;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            v += __shfl_xor(v, s, 64);
            m += __shfl_xor(m, s, 64);
        }
        if (lane == 0) out[o] = A * (m / (M_PI * R * R) - v);
    } else {
        double v = lens_quad.wt_phi[lane] * acc;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
        if (lane == 0) out[o] = A * v;
    }
}

// ---------------------------------------------------------------- two-halo convergence and tangential shear
// out(z, M, theta) = b(z, M) pre(z) trapz_l[ P(z, k) J_ORDER(l theta) l / 2 pi ],  l = k chi(z), lmin < l < lmax:
// ORDER 0 is kappa_2h, pre(z) = rho_m(z) / (1+z)^3 / Sigma_crit(z) / D_A(z)^2 (hmvec/hmvec.py:598-625); ORDER 2 is
// gamma_t^2h (Oguri & Takada 2011).  One workgroup per (z, theta).  The
// k grid is increasing, so the selected l are one run of the grid and the trapezoid over them is the sum of the
// panels (i, i+1) whose two ends are both selected: each thread forms panels i = tid, tid + NT, ... in order and the
// workgroup reduces them in a fixed LDS tree.  Then b(z, M) = linear interpolation of bh[z, :] on ms (the search and
// expression of scipy's interp1d: first node >= M, clamped to [1, nm-1]) scales the sum for every M.
template <int ORDER>
__device__ __forceinline__ double bessel_j(double x) {
    static_assert(ORDER == 0 || ORDER == 2, "J0 or J2");
    if constexpr (ORDER == 0) return bessel_j0(x);
    else return bessel_j2(x);
}

template <int NT, int ORDER>
__global__ __launch_bounds__(NT) void lensing_2h_kernel(
    int nk, int ntheta, int nm, int nM, const double* __restrict__ ks, const double* __restrict__ chi,
    const double* __restrict__ pre, const double* __restrict__ Pzk, const double* __restrict__ thetas, double lmin,
    double lmax, const double* __restrict__ ms, const double* __restrict__ bh, const double* __restrict__ Ms,
    double* __restrict__ out) {
    __shared__ double red[NT];
    const int it = blockIdx.x, z = blockIdx.y, tid = threadIdx.x;
    const double th = thetas[it], c = chi[z];
    const double* P = Pzk + (size_t)z * nk;
    double acc = 0.0;
    for (int i = tid; i + 1 < nk; i += NT) {
        const double l0 = ks[i] * c, l1 = ks[i + 1] * c;
        if (l0 > lmin && l0 < lmax && l1 > lmin && l1 < lmax) {
            const double y0 = P[i] * bessel_j<ORDER>(l0 * th) * l0;
            const double y1 = P[i + 1] * bessel_j<ORDER>(l1 * th) * l1;
            acc += (l1 - l0) * (y0 + y1);
        }
    }
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double I = red[0] * pre[z] * (0.25 / M_PI);     // trapezoid's 1/2 and the integrand's 1/(2 pi)
    const double* b = bh + (size_t)z * nm;
    for (int m = tid; m < nM; m += NT) {
        const double M = Ms[m];
        int lo = 0, hi = nm;                               // first index with ms[idx] >= M
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ms[mid] < M) lo = mid + 1; else hi = mid;
        }
        const int idx = lo < 1 ? 1 : (lo > nm - 1 ? nm - 1 : lo);
        const double slope = (b[idx] - b[idx - 1]) / (ms[idx] - ms[idx - 1]);
        out[((size_t)z * ntheta + it) * nM + m] = (slope * (M - ms[idx - 1]) + b[idx - 1]) * I;
    }
}

}  // namespace hmg
