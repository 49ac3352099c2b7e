// Correlation function xi(r) of a tabulated spectrum and redshift-space correlation multipoles
// xi_0, xi_2, xi_4(s) of tabulated multipole spectra (section 24).  One kernel serves both: xi(r) is its order 0 alone.
// Compiled in realspace.hip, the only unit that holds it.
//
// With f_i = k_i P_l,i and f~ the piecewise-linear interpolant of f on [k_0, k_{nk-1}] (zero outside),
//   xi_l(s) = i^l / (2 pi^2) int k f~(k) j_l(k s) dk,      l = 0, 2, 4,
// the integral taken exactly, panel by panel.
//
// Order 0, k j_0(k s) = sin(k s)/s:  xi(r) = 1/(2 pi^2 r) int f~(k) sin(k r) dk.  For a panel [a, b]: h = b - a,
// m = (a + b)/2, f_m = (f_a + f_b)/2, theta = r h / 2, and the panel integral is
//   h f_m sin(m r) S(theta) + (f_b - f_a) h^2 r / 12 cos(m r) G(theta),
//   S = sin(theta)/theta,  G = 3 (sin(theta) - theta cos(theta)) / theta^3      (both -> 1 as theta -> 0):
// the two terms are the even and the odd part of f~ about the panel's midpoint, so nothing cancels inside a panel.
//
// Orders 2 and 4 are summed by parts (f~ is continuous, so the end terms of adjacent panels telescope), x = k s,
// sigma_i = (f_{i+1} - f_i)/(k_{i+1} - k_i):
//   int k f~ j_l(k s) dk = [f A_l(k s)]/s^2 - (1/s^3) sum_i sigma_i (B_l(x_{i+1}) - B_l(x_i)),
//   A_2 = 2 + cos x - 3 sin x / x                                          = int_0^x t j_2    (-> x^4/60),
//   B_2 = 2 x + sin x - 3 Si(x)                                            = int_0^x A_2      (-> x^5/300),
//   A_4 = 8/3 - cos x + 10 sin x / x + 35 cos x / x^2 - 35 sin x / x^3     = int_0^x t j_4    (-> x^6/5670),
//   B_4 = 8 x/3 - sin x - (15/2) Si(x) + (35/2) (sin x - x cos x) / x^2    = int_0^x A_4      (-> x^7/39690),
// the antiderivatives that vanish at 0.  The 2 and 8/3 of A_l and the 2 x and 8 x/3 of B_l cancel between the end term
// and the sum ((1/s^3) sum_i sigma_i 2 (x_{i+1} - x_i) = 2 [f]/s^2); they are left in and telescope, as the smooth
// parts of kernels/hankel.hpp do: the series below the switch hold them implicitly, so taking them out of the closed
// forms alone would break the telescoping at the node where the branch changes, and taking them out of both would leave
// -2 x to swamp x^5/300.
#pragma once
#include "../sici.hpp"
#include "panels.hpp"

namespace hmg {

constexpr int XI_THREADS = 256;
constexpr int XI_TILE = 4;                    // separations per workgroup
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

// Below these x the functions of orders 2 and 4 come from their power series in y = x^2, nested,
//   A_l = x^(l+2)/((l+2)(2l+1)!!) (1 - r_1 (1 - r_2 (1 - ...))),     r_m = y (l+2m) / ((l+2m+2) 2m (2l+2m+1))
//   B_l = x^(l+3)/((l+2)(l+3)(2l+1)!!) (1 - r_1 (1 - ...)),          r_m = y (l+2m)(l+2m+1) / ((l+2m+2)(l+2m+3) 2m (2l+2m+1))
// through m = XP_SERIES_N.  The closed forms add terms of size 2 x + 3 Si (B_2) and 8 x/3 + 7.5 Si + 17.5/x (B_4) that
// leave x^5/300 and x^7/39690: B_2 loses 105 at x = 2, 21 at 3 and 7.3 at 4; B_4 loses 113 at x = 4, 30 at 5 and 11.7 at
// 6 (A_2: 2.6 at 4; A_4: 2.9 at 6) - the 12 that section 14 accepts is reached at 4 and at 6.  A higher switch costs
// digits inside the series: at x = 4 the series of B_2 and A_2 lose 3.0 and 4.6 (absolute term sum over the sum) and at
// x = 5 5.5 and 11; at x = 6 those of B_4 and A_4 lose 6.7 and 11.8 and at x = 7 13 and 30.  At the switch the first
// omitted term (m = 15 and m = 17) is below 1e-17 of the sum.  x = 4 is also where sici_fast changes from the
// rational in x^2 to the auxiliary functions.  Both branches are evaluated and selected.
constexpr double XP_SERIES_X2 = 4.0;
constexpr double XP_SERIES_X4 = 6.0;
constexpr int XP_SERIES_N2 = 14;
constexpr int XP_SERIES_N4 = 16;

// sin x, cos x, 1/x and Si(x) at a node, shared by both orders; below the order-2 switch, where no closed form is read,
// the reciprocal is that of 1 (no 0/0 at x = 0)
struct XpTrig { double s, c, r, si; };
__device__ __forceinline__ XpTrig xp_trig(const SiciTable* __restrict__ T, double x, bool want_si) {
    XpTrig t;
    xi_sincos(x, t.s, t.c);
    t.r = rcp_fast(x < XP_SERIES_X2 ? 1.0 : x);
    t.si = 0.0;
    if (want_si) {
        double ci;
        bool small;
        sici_fast(T, x, t.s, t.c, t.r * t.r, t.si, ci, small);
    }
    return t;
}

// B_2(x) and B_4(x): the node functions of the sums
template <bool X2, bool X4>
__device__ __forceinline__ void xp_node(const SiciTable* __restrict__ T, double x, double& b2, double& b4) {
    const XpTrig t = xp_trig(T, x, true);
    const double y = x * x;
    if (X2) {
        double s = 1.0;
#pragma unroll
        for (int m = XP_SERIES_N2; m >= 1; --m)
            s = fma(-y * ((2.0 + 2 * m) * (3.0 + 2 * m) / ((4.0 + 2 * m) * (5.0 + 2 * m) * (2.0 * m) * (5.0 + 2 * m))), s, 1.0);
        b2 = x < XP_SERIES_X2 ? x * y * y * (1.0 / 300.0) * s : fma(2.0, x, fma(-3.0, t.si, t.s));
    }
    if (X4) {
        double s = 1.0;
#pragma unroll
        for (int m = XP_SERIES_N4; m >= 1; --m)
            s = fma(-y * ((4.0 + 2 * m) * (5.0 + 2 * m) / ((6.0 + 2 * m) * (7.0 + 2 * m) * (2.0 * m) * (9.0 + 2 * m))), s, 1.0);
        const double osc = fma(17.5 * (t.r * t.r), fma(-x, t.c, t.s), fma(-7.5, t.si, -t.s));
        b4 = x < XP_SERIES_X4 ? x * y * y * y * (1.0 / 39690.0) * s : fma(8.0 / 3.0, x, osc);
    }
}

// A_2(x) and A_4(x): the end terms
template <bool X2, bool X4>
__device__ __forceinline__ void xp_ends(double x, double& a2, double& a4) {
    const XpTrig t = xp_trig(nullptr, x, false);
    const double y = x * x, sr = t.s * t.r;
    if (X2) {
        double s = 1.0;
#pragma unroll
        for (int m = XP_SERIES_N2; m >= 1; --m)
            s = fma(-y * ((2.0 + 2 * m) / ((4.0 + 2 * m) * (2.0 * m) * (5.0 + 2 * m))), s, 1.0);
        a2 = x < XP_SERIES_X2 ? y * y * (1.0 / 60.0) * s : fma(-3.0, sr, 2.0 + t.c);
    }
    if (X4) {
        double s = 1.0;
#pragma unroll
        for (int m = XP_SERIES_N4; m >= 1; --m)
            s = fma(-y * ((4.0 + 2 * m) / ((6.0 + 2 * m) * (2.0 * m) * (9.0 + 2 * m))), s, 1.0);
        a4 = x < XP_SERIES_X4 ? y * y * y * (1.0 / 5670.0) * s
                              : fma(35.0 * (t.r * t.r), t.c - sr, fma(10.0, sr, 8.0 / 3.0 - t.c));
    }
}

// outL[row, j] = xi_L(ss[j]) of the row PL[row row_stride + i node_stride], i < nk, on the grid ks, L = 0, 2, 4 (X0 / X2 /
// X4: which of them this instantiation writes; each order reads its own rows).  One workgroup per (row, tile of TR
// separations).  Order 0: a thread owns the panels tid, tid + NT, ...: it forms h, m, f_m and f_b - f_a of a panel once
// and adds the panel's closed-form integral for every separation of the tile to its LDS word of that separation, in
// panel order; hmg_xi_transform is this order alone on contiguous rows.  Orders 2 and 4: contiguous-run ownership
// (panels.hpp) - c = ceil((nk-1)/NT) panels per thread, the node functions once at the left end of the run and once per
// panel at the right node, carried; one sincos and one Si per node serve both orders.  One LDS word per (thread, output,
// separation), the fixed tree, explicit fma; the writing thread forms the end terms.  No atomics; a result depends on
// nk, ks, its row and its separation alone and is the same bits on every call, alone or in a batch, with or without the
// other outputs, from strided or contiguous rows.  UNIT: the launch promises node_stride == 1 (hmg_xi_transform), so
// that the two nodes of a panel come from one 16-byte load and no index is multiplied; the arithmetic is the same.
template <int NT, int TR, bool X0, bool X2, bool X4, bool UNIT = false>
__global__ __launch_bounds__(NT) void xi_multipole_kernel(int nk, int ns, const double* __restrict__ ks,
                                                          const double* __restrict__ P0, const double* __restrict__ P2,
                                                          const double* __restrict__ P4, long long row_stride,
                                                          long long node_stride_arg, const double* __restrict__ ss,
                                                          const SiciTable* __restrict__ T, double* __restrict__ out0,
                                                          double* __restrict__ out2, double* __restrict__ out4) {
    constexpr int S2 = X0 ? 1 : 0, S4 = S2 + (X2 ? 1 : 0), NO = S4 + (X4 ? 1 : 0);
    __shared__ double red[NO * TR][NT];
    const int row = blockIdx.x, j0 = blockIdx.y * TR, tid = threadIdx.x;
    const int nt = tile_count<TR>(ns, j0);
    const int np = nk - 1;
    const long long node_stride = UNIT ? 1 : node_stride_arg;
    if (X0) {
        const double* Pr = P0 + (size_t)row * row_stride;
#pragma unroll
        for (int t = 0; t < TR; ++t) red[t][tid] = 0.0;
        for (int i = tid; i + 1 < nk; i += NT) {
            const double a = ks[i], b = ks[i + 1];
            const size_t o = (size_t)i * node_stride;       // (one 64-bit product per panel, not one per node)
            const double fa = a * Pr[o], fb = b * Pr[o + node_stride];
            const double h = b - a, m = 0.5 * (a + b), fm = 0.5 * (fa + fb), df = fb - fa;
#pragma unroll 1
            for (int t = 0; t < nt; ++t) {
                const double r = ss[j0 + t], th = 0.5 * r * h;
                double sm, cm, S, G;
                xi_sincos(m * r, sm, cm);
                xi_panel_factors(th, S, G);
                red[t][tid] += h * (fm * sm * S + df * (th * (1.0 / 6.0)) * cm * G);      // h^2 r / 12 = h theta / 6
            }
        }
    }
    if (X2 || X4) {
        const double* Pr2 = X2 ? P2 + (size_t)row * row_stride : nullptr;
        const double* Pr4 = X4 ? P4 + (size_t)row * row_stride : nullptr;
        const PanelRun run = panel_run<NT>(tid, np);
#pragma unroll 1
        for (int t = 0; t < TR; ++t) {
            double s2 = 0.0, s4 = 0.0;
            if (t < nt && run.lo < run.hi) {
                const double s = ss[j0 + t];
                double a = ks[run.lo], fa2 = 0.0, fa4 = 0.0, bl2 = 0.0, bl4 = 0.0;
                if (X2) fa2 = a * Pr2[(size_t)run.lo * node_stride];
                if (X4) fa4 = a * Pr4[(size_t)run.lo * node_stride];
                xp_node<X2, X4>(T, a * s, bl2, bl4);
#pragma unroll 1
                for (int i = run.lo; i < run.hi; ++i) {
                    const double b = ks[i + 1], ih = 1.0 / (b - a);
                    double br2 = 0.0, br4 = 0.0;
                    xp_node<X2, X4>(T, b * s, br2, br4);
                    if (X2) {
                        const double fb = b * Pr2[(size_t)(i + 1) * node_stride];
                        s2 = fma((fb - fa2) * ih, br2 - bl2, s2);
                        fa2 = fb;
                    }
                    if (X4) {
                        const double fb = b * Pr4[(size_t)(i + 1) * node_stride];
                        s4 = fma((fb - fa4) * ih, br4 - bl4, s4);
                        fa4 = fb;
                    }
                    a = b, bl2 = br2, bl4 = br4;
                }
            }
            if (X2) red[S2 * TR + t][tid] = s2;
            if (X4) red[S4 * TR + t][tid] = s4;
        }
    }
    panel_tree_sum(red, tid);
    if (tid < nt) {
        const size_t o = (size_t)row * ns + j0 + tid;
        if (X0) out0[o] = red[tid][0] * (0.5 / (M_PI * M_PI)) / ss[j0 + tid];
        if (X2 || X4) {
            const double s = ss[j0 + tid], is = 1.0 / s, is2 = is * is, is3 = is2 * is;
            const double ka = ks[0], kb = ks[np];
            double aa2 = 0.0, aa4 = 0.0, ab2 = 0.0, ab4 = 0.0;
            xp_ends<X2, X4>(ka * s, aa2, aa4);
            xp_ends<X2, X4>(kb * s, ab2, ab4);
            if (X2) {
                const double* Pr = P2 + (size_t)row * row_stride;
                const double ends = fma(kb * Pr[(size_t)np * node_stride], ab2, -(ka * Pr[0] * aa2));
                out2[o] = fma(-is3, red[S2 * TR + tid][0], ends * is2) * (-0.5 / (M_PI * M_PI));
            }
            if (X4) {
                const double* Pr = P4 + (size_t)row * row_stride;
                const double ends = fma(kb * Pr[(size_t)np * node_stride], ab4, -(ka * Pr[0] * aa4));
                out4[o] = fma(-is3, red[S4 * TR + tid][0], ends * is2) * (0.5 / (M_PI * M_PI));
            }
        }
    }
}

}  // namespace hmg
