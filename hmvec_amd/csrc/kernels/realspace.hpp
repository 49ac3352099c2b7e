// Correlation function xi(r) of a tabulated spectrum.  Compiled in realspace.hip, a translation
// unit of its own (kept out of the power-path units).
//
// With f_i = k_i P_i and f~ the piecewise-linear interpolant of f on [k_0, k_{nk-1}] (zero outside),
//   xi(r) = 1/(2 pi^2 r) int f~(k) sin(k r) dk,
// the integral taken exactly, panel by panel.  For a panel [a, b]: h = b - a, m = (a + b)/2, f_m = (f_a + f_b)/2,
// theta = r h / 2, and the panel integral is
//   h f_m sin(m r) S(theta) + (f_b - f_a) h^2 r / 12 cos(m r) G(theta),
//   S = sin(theta)/theta,  G = 3 (sin(theta) - theta cos(theta)) / theta^3      (both -> 1 as theta -> 0):
// the two terms are the even and the odd part of f~ about the panel's midpoint, so nothing cancels inside a panel.
#pragma once
#include "../j01.hpp"
#include "../sici.hpp"

namespace hmg {

constexpr int XI_THREADS = 256;
constexpr int XI_TILE = 4;                    // radii per workgroup
// Below this theta S and G come from their even power series.  The closed form of G subtracts two terms of size theta
// that leave theta^3/3: it loses a factor 3/theta^2 (12 at the switch, 3.6 bits), which the gate of section 13 has room
// for; the series truncated after theta^12 is off by less than theta^14/15! (S) and 48 theta^14/17! (G), 5e-17 and
// 9e-18 at the switch.  Both branches are evaluated and selected, so a wavefront does not diverge here.
constexpr double XI_SERIES_THETA = 0.5;

// sin and cos of x >= 0: the Cody-Waite route of sici.hpp (error < 1 ulp of the result + 2e-16) where it holds, the
// library's full-range reduction beyond
__device__ __forceinline__ void xi_sincos(double x, double& s, double& c) {
    if (x < 0x1p30) sincos_fast(x, s, c);
    else sincos(x, &s, &c);
}

// S(theta) and G(theta) for theta >= 0
__device__ __forceinline__ void xi_panel_factors(double th, double& S, double& G) {
    double s, c;
    xi_sincos(th, s, c);
    const double z = th * th;
    // S = sum_j (-1)^j z^j / (2j+1)!,  G = sum_j (-1)^j 3 (2j+2) z^j / (2j+3)!
    double ps = 1.0 / 6227020800.0;
    ps = fma(ps, z, -1.0 / 39916800.0);
    ps = fma(ps, z, 1.0 / 362880.0);
    ps = fma(ps, z, -1.0 / 5040.0);
    ps = fma(ps, z, 1.0 / 120.0);
    ps = fma(ps, z, -1.0 / 6.0);
    ps = fma(ps, z, 1.0);
    double pg = 1.0 / 31135104000.0;
    pg = fma(pg, z, -1.0 / 172972800.0);
    pg = fma(pg, z, 1.0 / 1330560.0);
    pg = fma(pg, z, -1.0 / 15120.0);
    pg = fma(pg, z, 1.0 / 280.0);
    pg = fma(pg, z, -1.0 / 10.0);
    pg = fma(pg, z, 1.0);
    const bool series = th < XI_SERIES_THETA;
    const double d = series ? 1.0 : th;           // (the closed forms are not used below the switch: no 0/0 at theta = 0)
    S = series ? ps : s / d;
    G = series ? pg : 3.0 * (s - d * c) / (d * d * d);
}

// out[row, j] = xi(rs[j]) of the row P[row, :] on the grid ks.  One workgroup per (row, tile of TR radii).  A thread owns
// the panels i = tid, tid + NT, ...: it forms h, m, f_m and f_b - f_a of a panel once, adds the panel's integral for
// every radius of the tile to its own LDS word of that radius (in panel order), and a fixed LDS tree sums the NT words
// of each radius.  No atomics; a result depends on nk, ks, its row and its radius alone - not on the other rows or
// radii of the launch - and is the same bits on every call.
template <int NT, int TR>
__global__ __launch_bounds__(NT) void xi_transform_kernel(int nk, int nr, const double* __restrict__ ks,
                                                          const double* __restrict__ P,
                                                          const double* __restrict__ rs, double* __restrict__ out) {
    __shared__ double red[TR][NT];
    const int row = blockIdx.x, j0 = blockIdx.y * TR, tid = threadIdx.x;
    const int nt = nr - j0 < TR ? nr - j0 : TR;             // radii of this tile (>= 1 by the launch geometry)
    const double* Pr = P + (size_t)row * nk;
#pragma unroll
    for (int t = 0; t < TR; ++t) red[t][tid] = 0.0;
    for (int i = tid; i + 1 < nk; i += NT) {
        const double a = ks[i], b = ks[i + 1];
        const double fa = a * Pr[i], fb = b * Pr[i + 1];
        const double h = b - a, m = 0.5 * (a + b), fm = 0.5 * (fa + fb), df = fb - fa;
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            const double r = rs[j0 + t], th = 0.5 * r * h;
            double sm, cm, S, G;
            xi_sincos(m * r, sm, cm);
            xi_panel_factors(th, S, G);
            red[t][tid] += h * (fm * sm * S + df * (th * (1.0 / 6.0)) * cm * G);      // h^2 r / 12 = h theta / 6
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int t = 0; t < TR; ++t) red[t][tid] += red[t][tid + s];
        }
        __syncthreads();
    }
    if (tid < nt) out[(size_t)row * nr + j0 + tid] = red[tid][0] * (0.5 / (M_PI * M_PI)) / rs[j0 + tid];
}

// ---------------------------------------------------------------------------------------------------------------------
// Hankel transforms of orders 0 and 2 of a tabulated spectrum: w_p, Sigma and Delta Sigma.
//
// With P~ the interpolant of P that is linear in k^2 on each panel of [k_0, k_{nk-1}] (zero outside),
// P~ = P_a + B (k^2 - a^2), B = (P_b - P_a) / ((b - a)(b + a)) on [a, b],
//   W_0(R) = 1/(2 pi) int k P~ J0(k R) dk,   W_2(R) = 1/(2 pi) int k P~ J2(k R) dk,
// the integrals exact.  Summed by parts (P~ is continuous, so the end terms of the panels telescope), x = k R:
//   2 pi W_0 = [P k J1(x)]/R   - (2/R^4) sum_i B_i (g(x_{i+1}) - g(x_i)),    g  = x^2 J2                 = int_0^x t^2 J1
//   2 pi W_2 = [P H1(x)]/R^2   - (2/R^4) sum_i B_i (H2(x_{i+1}) - H2(x_i)),  H1 = 2 (1 - J0) - x J1      = int_0^x t J2
//                                                                            H2 = x^2 - 2 x J1 - x^2 J2  = int_0^x t H1
// H1 and H2 are the antiderivatives that vanish at 0: no constant is left to cancel against the sum at small k R.
constexpr int HK_THREADS = 256;
constexpr int HK_TILE = 4;                    // radii per workgroup
// Below this x the node functions come from their power series in y = x^2/4,
//   g  = 2 y^2 (1 - y/(1*3) (1 - y/(2*4) (1 - ...))),                    ratio of terms j-1 -> j:  y / (j (j+2))
//   H1 = y^2/2 (1 - 2y/(1*9) (1 - 3y/(2*16) (1 - ...))),                                       y (j+1) / (j (j+2)^2)
//   H2 = y^3/3 (1 - 2y/(1*3*4) (1 - 3y/(2*4*5) (1 - ...))),                                    y (j+1) / (j (j+2) (j+3))
// nested through j = HK_SERIES_N.  The closed forms subtract terms of size x^2 that leave x^4/8 (g), x^4/32 (H1) and
// x^6/192 (H2): they lose 8/x^2, 16/x^2 and 192/x^4 - 2, 4 and 12 at the switch, what section 13 accepts for G.  A lower
// switch would cost digits as x^-2 and x^-4.  A higher one would cost them inside the series: up to y = 1 its terms fall
// from the first (the second is at most 1/3 of it), so nothing cancels; beyond, they grow before they fall.  At the
// switch the first omitted terms are 8.0e-18 (g), 1.2e-18 (H1) and 2.7e-19 (H2) of the leading one.  Both branches are
// evaluated and selected.
constexpr double HK_SERIES_X = 2.0;
constexpr int HK_SERIES_N = 10;

// g(x) = x^2 J2(x) and H2(x) given J0(x) and J1(x); the closed forms without a division: x^2 J2 = x (2 J1 - x J0)
template <bool W0, bool W2>
__device__ __forceinline__ void hankel_node_j(double x, double j0, double j1, double& g, double& h2) {
    const double y = 0.25 * x * x;
    const bool series = x < HK_SERIES_X;
    const double gc = x * fma(-x, j0, 2.0 * j1);
    double sg = 1.0, sh = 1.0;
#pragma unroll
    for (int j = HK_SERIES_N; j >= 1; --j) {
        if (W0) sg = fma(-y * (1.0 / (j * (j + 2.0))), sg, 1.0);
        if (W2) sh = fma(-y * ((j + 1.0) / (j * (j + 2.0) * (j + 3.0))), sh, 1.0);
    }
    g = series ? 2.0 * y * y * sg : gc;
    h2 = series ? y * y * y * (1.0 / 3.0) * sh : fma(x, fma(-2.0, j1, x), -gc);
}

// the same at a node whose J0 and J1 the caller does not need (the angular kernel of kernels/angular.hpp does)
template <bool W0, bool W2>
__device__ __forceinline__ void hankel_node(double x, double& g, double& h2) {
    double j0, j1;
    bessel_j01(x, j0, j1);
    hankel_node_j<W0, W2>(x, j0, j1, g, h2);
}

// H1(x) given J0(x) and J1(x): the end terms of W_2
__device__ __forceinline__ double hankel_h1(double x, double j0, double j1) {
    const double y = 0.25 * x * x;
    double s = 1.0;
#pragma unroll
    for (int j = HK_SERIES_N; j >= 1; --j) s = fma(-y * ((j + 1.0) / (j * (j + 2.0) * (j + 2.0))), s, 1.0);
    return x < HK_SERIES_X ? 0.5 * y * y * s : fma(-x, j1, 2.0 * (1.0 - j0));
}

// out0[row, j] = W_0(rs[j]) and out2[row, j] = W_2(rs[j]) of the row P[row, :] on the grid ks (W0 / W2: which of the two
// this instantiation writes).  One workgroup per (row, tile of TR radii).  A thread owns a contiguous run of
// c = ceil((nk-1)/NT) panels, i = tid c ... min((tid+1) c, nk-1) - 1 (the last owners' runs are short or empty): it
// evaluates the node functions once at the left end of its run and then once per panel, at the panel's right node, which
// it carries to the next panel as the left one - (nk-1) + (owners) evaluations per radius instead of 2 (nk-1).  The price
// is in the loads: a thread reads c + 1 consecutive ks and P values, so the 64 lanes of a load are c words apart
// (uncoalesced: 64 cache lines per wavefront load, re-used over the c steps of the run from L1); a row is at most 32 KB
// and comes from L2 once per tile.  The radii of a tile are taken one after the other (the run is re-read from L1), each
// partial sum goes to the thread's LDS word of that radius and output, and a fixed LDS tree sums the NT words.  The two
// end terms are formed by the thread that writes the result.  No atomics; a result depends on nk, ks, its row and its
// radius alone and is the same bits on every call, alone or in a batch, with or without the other output.
template <int NT, int TR, bool W0, bool W2>
__global__ __launch_bounds__(NT) void hankel_transform_kernel(int nk, int nr, const double* __restrict__ ks,
                                                              const double* __restrict__ P,
                                                              const double* __restrict__ rs, double* __restrict__ out0,
                                                              double* __restrict__ out2) {
    constexpr int NO = (W0 ? 1 : 0) + (W2 ? 1 : 0);
    __shared__ double red[NO * TR][NT];
    const int row = blockIdx.x, j0 = blockIdx.y * TR, tid = threadIdx.x;
    const int nt = nr - j0 < TR ? nr - j0 : TR;             // radii of this tile (>= 1 by the launch geometry)
    const double* Pr = P + (size_t)row * nk;
    const int np = nk - 1, c = (np - 1) / NT + 1;
    const int lo = tid * c < np ? tid * c : np, hi = lo + c < np ? lo + c : np;
#pragma unroll 1
    for (int t = 0; t < TR; ++t) {
        double s0 = 0.0, s2 = 0.0;
        if (t < nt && lo < hi) {
            const double R = rs[j0 + t];
            double a = ks[lo], Pa = Pr[lo], gl, hl;
            hankel_node<W0, W2>(a * R, gl, hl);
#pragma unroll 1
            for (int i = lo; i < hi; ++i) {
                const double b = ks[i + 1], Pb = Pr[i + 1];
                double gr, hr;
                hankel_node<W0, W2>(b * R, gr, hr);
                const double B = (Pb - Pa) / ((b - a) * (b + a));
                if (W0) s0 = fma(B, gr - gl, s0);
                if (W2) s2 = fma(B, hr - hl, s2);
                a = b, Pa = Pb, gl = gr, hl = hr;
            }
        }
        if (W0) red[t][tid] = s0;
        if (W2) red[(NO - 1) * TR + t][tid] = s2;
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
        const double R = rs[j0 + tid], iR = 1.0 / R, iR2 = iR * iR, iR4 = iR2 * iR2;
        const double ka = ks[0], kb = ks[np], Pa = Pr[0], Pb = Pr[np];
        double a0, a1, b0, b1;
        bessel_j01(ka * R, a0, a1);
        bessel_j01(kb * R, b0, b1);
        if (W0) {
            const double ends = fma(Pb * kb, b1, -(Pa * ka * a1));
            out0[(size_t)row * nr + j0 + tid] = fma(-2.0 * iR4, red[tid][0], ends * iR) * (0.5 / M_PI);
        }
        if (W2) {
            const double ends = fma(Pb, hankel_h1(kb * R, b0, b1), -(Pa * hankel_h1(ka * R, a0, a1)));
            out2[(size_t)row * nr + j0 + tid] = fma(-2.0 * iR4, red[(NO - 1) * TR + tid][0], ends * iR2) * (0.5 / M_PI);
        }
    }
}

}  // namespace hmg
