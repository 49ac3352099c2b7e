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

}  // namespace hmg
