// Angular correlation functions of tabulated spectra: w(theta), gamma_t(theta), xi+-(theta).
// Compiled in angular.hip, a translation unit of its own: realspace.hip does not see these instantiations.
//
// Under the flat-sky Limber approximation with k = l / chi,
//   zeta_n(theta) = int l dl/(2 pi) C_l J_n(l theta) = sum_z zw_z W_n^(z)(R = chi_z theta),      n = 0, 2, 4,
// with W_n(R) = 1/(2 pi) int k P~ J_n(k R) dk the transform of section 14 (realspace.hpp) of the row at z, P~ linear in
// k^2 on each panel.  W_0 and W_2 are formed by realspace.hpp's device functions, operation for operation; the new order
// is summed by parts in the same way, x = k R:
//   2 pi W_4 = [P F1(x)]/R^2 - (2/R^4) sum_i B_i (F2(x_{i+1}) - F2(x_i)),
//   F1 = 4 + 8 J0 + x J1 - 24 J1/x            = int_0^x t J4        (-> x^6/2304),
//   F2 = 2 x^2 + 8 x J1 + x^2 J2 + 24 (J0 - 1) = int_0^x t F1        (-> x^8/18432),
// the antiderivatives that vanish at 0.  The 4 of F1 and the 2 x^2 of F2 cancel between the end term and the B-sum
// ((2/R^4) sum_i B_i 2 (x_{i+1}^2 - x_i^2) = 4 [P]/R^2); they are left in and telescope, as the 2 and the x^2 of H1 and
// H2 do: the series below the switch hold them implicitly, so taking them out of the closed forms alone would break the
// telescoping at the node where the branch changes, and taking them out of both would leave -2 x^2 to swamp x^8/18432.
#pragma once
#include "realspace.hpp"

namespace hmg {

constexpr int AG_THREADS = 256;
constexpr int AG_TILE = 4;                    // angles per workgroup
// Below this x F1 and F2 come from their power series in y = x^2/4,
//   F1 = y^3/36 (1 - 3y/(4*1*5) (1 - 4y/(5*2*6) (1 - ...))),       ratio of terms j-1 -> j:  y (j+2) / ((j+3) j (j+4))
//   F2 = y^4/72 (1 - 3y/(1*5*5) (1 - 4y/(2*6*6) (1 - ...))),                                 y (j+2) / (j (j+4)^2)
// nested through j = AG_SERIES_N.  The closed forms subtract terms of size 12 + 2x (F1) and 4 x^2 + 24 (F2) that leave
// x^6/2304 and x^8/18432: at x = 2 they lose 580 and 3000, at x = 4 8 and 34, at x = 5 3.4 and 9.4 - section 14's 12 is
// reached only near 5.  The series' first ratio is 0.15 y (F1) and 0.12 y (F2): up to y = 6.67 the terms fall from the
// first; at x = 5 (y = 6.25) the sums are 0.37 and 0.46 of the leading term against absolute term sums of 2.5 and 2.1 -
// a loss of 6.7 and 4.5, the same size as the closed forms' there, so neither side of the switch is worse than 12.
// At the switch the first omitted term (j = 16) is 1.1e-18 (F1) and below 1e-19 (F2) of the sum.  x = 5 is also where
// bessel_j01 changes from the rational to the asymptotic form.  Both branches are evaluated and selected.
constexpr double AG_SERIES_X = 5.0;
constexpr int AG_SERIES_N = 15;

// F2(x) given J0(x) and J1(x)
__device__ __forceinline__ double angular_f2(double x, double j0, double j1) {
    const double y = 0.25 * x * x;
    double s = 1.0;
#pragma unroll
    for (int j = AG_SERIES_N; j >= 1; --j) s = fma(-y * ((j + 2.0) / (j * (j + 4.0) * (j + 4.0))), s, 1.0);
    const double y2 = y * y;
    const double gc = x * fma(-x, j0, 2.0 * j1);                                   // x^2 J2
    return x < AG_SERIES_X ? y2 * y2 * (1.0 / 72.0) * s : fma(x, fma(8.0, j1, 2.0 * x), fma(24.0, j0 - 1.0, gc));
}

// F1(x) given J0(x) and J1(x): the end terms of W_4
__device__ __forceinline__ double angular_f1(double x, double j0, double j1) {
    const double y = 0.25 * x * x;
    double s = 1.0;
#pragma unroll
    for (int j = AG_SERIES_N; j >= 1; --j) s = fma(-y * ((j + 2.0) / ((j + 3.0) * j * (j + 4.0))), s, 1.0);
    const bool series = x < AG_SERIES_X;
    const double d = series ? 1.0 : x;            // (the closed form is not used below the switch)
    return series ? y * y * y * (1.0 / 36.0) * s : fma(x, j1, fma(8.0, j0, 4.0)) - 24.0 * j1 / d;
}

// The node functions of the orders this instantiation writes, from one J0/J1 pair
template <bool W0, bool W2, bool W4>
__device__ __forceinline__ void angular_node(double x, double& g, double& h2, double& f2) {
    double j0, j1;
    bessel_j01(x, j0, j1);
    if (W0 || W2) hankel_node_j<W0, W2>(x, j0, j1, g, h2);
    if (W4) f2 = angular_f2(x, j0, j1);
}

// outN[row, j] = W_N(R) of the row P[row, :] at R = fl(chis[row % nz] * thetas[j]), N = 0, 2, 4 (W0 / W2 / W4: which of
// them this instantiation writes).  Panel ownership, the carried node, the per-thread LDS word of each (output, angle),
// the fixed LDS tree and the explicit fma are hankel_transform_kernel's (realspace.hpp); what differs is the radius,
// which depends on the row, and the third output.  No atomics; a result depends on nk, ks, its row and its R alone and
// is the same bits on every call, alone or in a batch, with or without the other outputs; W_0 and W_2 are the bits
// hankel_transform_kernel gives at the radius R.
template <int NT, int TR, bool W0, bool W2, bool W4>
__global__ __launch_bounds__(NT) void angular_transform_kernel(int nz, int nk, int nth, const double* __restrict__ ks,
                                                               const double* __restrict__ P,
                                                               const double* __restrict__ chis,
                                                               const double* __restrict__ thetas,
                                                               double* __restrict__ out0, double* __restrict__ out2,
                                                               double* __restrict__ out4) {
    constexpr int S2 = W0 ? 1 : 0, S4 = S2 + (W2 ? 1 : 0), NO = S4 + (W4 ? 1 : 0);
    __shared__ double red[NO * TR][NT];
    const int row = blockIdx.x, j0 = blockIdx.y * TR, tid = threadIdx.x;
    const int nt = nth - j0 < TR ? nth - j0 : TR;           // angles of this tile (>= 1 by the launch geometry)
    const double* Pr = P + (size_t)row * nk;
    const double chi = chis[row % nz];
    const int np = nk - 1, c = (np - 1) / NT + 1;
    const int lo = tid * c < np ? tid * c : np, hi = lo + c < np ? lo + c : np;
#pragma unroll 1
    for (int t = 0; t < TR; ++t) {
        double s0 = 0.0, s2 = 0.0, s4 = 0.0;
        if (t < nt && lo < hi) {
            const double R = __dmul_rn(chi, thetas[j0 + t]);
            double a = ks[lo], Pa = Pr[lo], gl = 0.0, hl = 0.0, fl = 0.0;
            angular_node<W0, W2, W4>(a * R, gl, hl, fl);
#pragma unroll 1
            for (int i = lo; i < hi; ++i) {
                const double b = ks[i + 1], Pb = Pr[i + 1];
                double gr = 0.0, hr = 0.0, fr = 0.0;
                angular_node<W0, W2, W4>(b * R, gr, hr, fr);
                const double B = (Pb - Pa) / ((b - a) * (b + a));
                if (W0) s0 = fma(B, gr - gl, s0);
                if (W2) s2 = fma(B, hr - hl, s2);
                if (W4) s4 = fma(B, fr - fl, s4);
                a = b, Pa = Pb, gl = gr, hl = hr, fl = fr;
            }
        }
        if (W0) red[t][tid] = s0;
        if (W2) red[S2 * TR + t][tid] = s2;
        if (W4) red[S4 * TR + t][tid] = s4;
    }
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int t = 0; t < NO * TR; ++t) red[t][tid] += red[t][tid + s];
        }
        __syncthreads();
    }
    if (tid < nt) {
        const double R = __dmul_rn(chi, thetas[j0 + tid]), iR = 1.0 / R, iR2 = iR * iR, iR4 = iR2 * iR2;
        const double ka = ks[0], kb = ks[np], Pa = Pr[0], Pb = Pr[np];
        const size_t o = (size_t)row * nth + j0 + tid;
        double a0, a1, b0, b1;
        bessel_j01(ka * R, a0, a1);
        bessel_j01(kb * R, b0, b1);
        if (W0) {
            const double ends = fma(Pb * kb, b1, -(Pa * ka * a1));
            out0[o] = fma(-2.0 * iR4, red[tid][0], ends * iR) * (0.5 / M_PI);
        }
        if (W2) {
            const double ends = fma(Pb, hankel_h1(kb * R, b0, b1), -(Pa * hankel_h1(ka * R, a0, a1)));
            out2[o] = fma(-2.0 * iR4, red[S2 * TR + tid][0], ends * iR2) * (0.5 / M_PI);
        }
        if (W4) {
            const double ends = fma(Pb, angular_f1(kb * R, b0, b1), -(Pa * angular_f1(ka * R, a0, a1)));
            out4[o] = fma(-2.0 * iR4, red[S4 * TR + tid][0], ends * iR2) * (0.5 / M_PI);
        }
    }
}

// out[i, w, j] = sum_z zw[w, z] W[i nz + z, j]: one thread per output, one fma chain over z in index order from 0.0 (a
// single z of weight 1.0 returns W's bits: fma(1, W, 0) = W).  No atomics; the launch shape decides nothing.
__global__ __launch_bounds__(256) void angular_zsum_kernel(int nz, int nth, int nw, size_t total,
                                                           const double* __restrict__ zw,
                                                           const double* __restrict__ W, double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t j = e % nth, w = (e / nth) % nw, i = e / ((size_t)nth * nw);
    const double* Wi = W + (i * nz) * nth + j;
    const double* zr = zw + w * nz;
    double s = 0.0;
    for (int z = 0; z < nz; ++z) s = fma(zr[z], Wi[(size_t)z * nth], s);
    out[e] = s;
}

}  // namespace hmg
