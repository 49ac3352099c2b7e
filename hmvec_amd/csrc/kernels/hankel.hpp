// Hankel transforms of orders 0, 2 and 4 of a tabulated spectrum: w_p, Sigma and Delta Sigma at given radii (DESIGN.md
// section 14) and w(theta), gamma_t(theta), xi+-(theta) at R = chi theta (section 22).  One kernel serves both; what
// differs between them is the rule that gives a row its radii.  Compiled in hankel.hip, the only unit that holds it.
//
// With P~ the interpolant of P that is linear in k^2 on each panel of [k_0, k_{nk-1}] (zero outside),
// P~ = P_a + B (k^2 - a^2), B = (P_b - P_a) / ((b - a)(b + a)) on [a, b],
//   W_n(R) = 1/(2 pi) int k P~ J_n(k R) dk,      n = 0, 2, 4,
// the integrals exact.  Summed by parts (P~ is continuous, so the end terms of the panels telescope), x = k R:
//   2 pi W_0 = [P k J1(x)]/R   - (2/R^4) sum_i B_i (g(x_{i+1}) - g(x_i)),    g  = x^2 J2                 = int_0^x t^2 J1
//   2 pi W_2 = [P H1(x)]/R^2   - (2/R^4) sum_i B_i (H2(x_{i+1}) - H2(x_i)),  H1 = 2 (1 - J0) - x J1      = int_0^x t J2
//                                                                            H2 = x^2 - 2 x J1 - x^2 J2  = int_0^x t H1
//   2 pi W_4 = [P F1(x)]/R^2   - (2/R^4) sum_i B_i (F2(x_{i+1}) - F2(x_i)),
//   F1 = 4 + 8 J0 + x J1 - 24 J1/x            = int_0^x t J4        (-> x^6/2304),
//   F2 = 2 x^2 + 8 x J1 + x^2 J2 + 24 (J0 - 1) = int_0^x t F1        (-> x^8/18432).
// H1, H2, F1 and F2 are the antiderivatives that vanish at 0: no constant is left to cancel against the sum at small k R.
// The 4 of F1 and the 2 x^2 of F2 cancel between the end term and the B-sum ((2/R^4) sum_i B_i 2 (x_{i+1}^2 - x_i^2) =
// 4 [P]/R^2); they are left in and telescope, as the 2 and the x^2 of H1 and H2 do: the series below the switch hold them
// implicitly, so taking them out of the closed forms alone would break the telescoping at the node where the branch
// changes, and taking them out of both would leave -2 x^2 to swamp x^8/18432.
//
// Under the flat-sky Limber approximation with k = l / chi, the angular statistics are
//   zeta_n(theta) = int l dl/(2 pi) C_l J_n(l theta) = sum_z zw_z W_n^(z)(R = chi_z theta),
// W_n^(z) the transform of the row at z; angular_zsum_kernel takes the sum over z.
#pragma once
#include "../j01.hpp"
#include "bessel_g4.hpp"
#include "panels.hpp"

namespace hmg {

constexpr int HK_THREADS = 256;
constexpr int HK_TILE = 4;                    // radii per workgroup
// Below this x g, H1 and H2 come from their power series in y = x^2/4,
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
// Below this x F1 (bessel_g4.hpp) and F2 come from their power series in y = x^2/4,
//   F1 = y^3/36 (1 - 3y/(4*1*5) (1 - 4y/(5*2*6) (1 - ...))),       ratio of terms j-1 -> j:  y (j+2) / ((j+3) j (j+4))
//   F2 = y^4/72 (1 - 3y/(1*5*5) (1 - 4y/(2*6*6) (1 - ...))),                                 y (j+2) / (j (j+4)^2)
// nested through j = AG_SERIES_N.  The closed forms subtract terms of size 12 + 2x (F1) and 4 x^2 + 24 (F2) that leave
// x^6/2304 and x^8/18432: at x = 2 they lose 580 and 3000, at x = 4 8 and 34, at x = 5 3.4 and 9.4 - section 14's 12 is
// reached only near 5.  The series' first ratio is 0.15 y (F1) and 0.12 y (F2): up to y = 6.67 the terms fall from the
// first; at x = 5 (y = 6.25) the sums are 0.37 and 0.46 of the leading term against absolute term sums of 2.5 and 2.1 -
// a loss of 6.7 and 4.5, the same size as the closed forms' there, so neither side of the switch is worse than 12.
// At the switch the first omitted term (j = 16) is 1.1e-18 (F1) and below 1e-19 (F2) of the sum.  x = 5 is also where
// bessel_j01 changes from the rational to the asymptotic form.  Both branches are evaluated and selected.
constexpr double AG_SERIES_X = G4_SERIES_X;
constexpr int AG_SERIES_N = G4_SERIES_N;

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

// H1(x) given J0(x) and J1(x): the end terms of W_2
__device__ __forceinline__ double hankel_h1(double x, double j0, double j1) {
    const double y = 0.25 * x * x;
    double s = 1.0;
#pragma unroll
    for (int j = HK_SERIES_N; j >= 1; --j) s = fma(-y * ((j + 1.0) / (j * (j + 2.0) * (j + 2.0))), s, 1.0);
    return x < HK_SERIES_X ? 0.5 * y * y * s : fma(-x, j1, 2.0 * (1.0 - j0));
}

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

// The node functions of the orders this instantiation writes, from one J0/J1 pair
template <bool W0, bool W2, bool W4>
__device__ __forceinline__ void angular_node(double x, double& g, double& h2, double& f2) {
    double j0, j1;
    bessel_j01(x, j0, j1);
    if (W0 || W2) hankel_node_j<W0, W2>(x, j0, j1, g, h2);
    if (W4) f2 = angular_f2(x, j0, j1);
}

// The radius rule of a launch, a compile-time policy: of_row(nz, ra, rb, row) gives the function j -> R of a row from the
// kernel's arguments.  (They are plain arguments, not members of a rule object passed by value: with the object the
// prologue's argument loads were split differently and the small launches measured 0.2 to 0.5 % slower, DESIGN.md
// section 22.)
struct PlainRadius {                              // R = ra[j], the same for every row (section 14); nz and rb are not read
    static __device__ auto of_row(int, const double* rs, const double*, int) {
        return [rs](int j) { return rs[j]; };
    }
};
struct ChiThetaRadius {                           // R = fl(chis[row % nz] * thetas[j]), rounded once (section 22)
    static __device__ auto of_row(int nz, const double* chis, const double* thetas, int row) {
        const double chi = chis[row % nz];
        return [chi, thetas](int j) { return __dmul_rn(chi, thetas[j]); };
    }
};

// outN[row, j] = W_N(R) of the row P[row, :] on the grid ks at the j-th of the row's nr radii, N = 0, 2, 4 (W0 / W2 / W4:
// which of them this instantiation writes).  One workgroup per (row, tile of TR radii).  A thread owns a contiguous run
// of c = ceil((nk-1)/NT) panels (panels.hpp): it evaluates the node functions once at the left end of its run and then
// once per panel, at the panel's right node, which it carries to the next panel as the left one - (nk-1) + (owners)
// evaluations per radius instead of 2 (nk-1).  The price is in the loads: a thread reads c + 1 consecutive ks and P
// values, so the 64 lanes of a load are c words apart (uncoalesced: 64 cache lines per wavefront load, re-used over the c
// steps of the run from L1); a row is at most 32 KB and comes from L2 once per tile.  The radii of a tile are taken one
// after the other (the run is re-read from L1), each partial sum goes to the thread's LDS word of that radius and output,
// and the fixed LDS tree sums the NT words.  The end terms are formed by the thread that writes the result.  No atomics; a
// result depends on nk, ks, its row and its R alone and is the same bits on every call, alone or in a batch, with or
// without the other outputs, under either radius rule.  nz, ra and rb are the rule's inputs: (-, rs, -) or (nz, chis,
// thetas).
template <int NT, int TR, bool W0, bool W2, bool W4, class Radius>
__global__ __launch_bounds__(NT) void angular_transform_kernel(int nz, int nk, int nr, const double* __restrict__ ks,
                                                               const double* __restrict__ P,
                                                               const double* __restrict__ ra,
                                                               const double* __restrict__ rb,
                                                               double* __restrict__ out0, double* __restrict__ out2,
                                                               double* __restrict__ out4) {
    constexpr int S2 = W0 ? 1 : 0, S4 = S2 + (W2 ? 1 : 0), NO = S4 + (W4 ? 1 : 0);
    __shared__ double red[NO * TR][NT];
    const int row = blockIdx.x, j0 = blockIdx.y * TR, tid = threadIdx.x;
    const int nt = tile_count<TR>(nr, j0);
    const double* Pr = P + (size_t)row * nk;
    const auto radius = Radius::of_row(nz, ra, rb, row);
    const int np = nk - 1;
    const PanelRun run = panel_run<NT>(tid, np);
#pragma unroll 1
    for (int t = 0; t < TR; ++t) {
        double s0 = 0.0, s2 = 0.0, s4 = 0.0;
        if (t < nt && run.lo < run.hi) {
            const double R = radius(j0 + t);
            double a = ks[run.lo], Pa = Pr[run.lo], gl = 0.0, hl = 0.0, fl = 0.0;
            angular_node<W0, W2, W4>(a * R, gl, hl, fl);
#pragma unroll 1
            for (int i = run.lo; i < run.hi; ++i) {
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
    panel_tree_sum(red, tid);
    if (tid < nt) {
        const double R = radius(j0 + tid), iR = 1.0 / R, iR2 = iR * iR, iR4 = iR2 * iR2;
        const double ka = ks[0], kb = ks[np], Pa = Pr[0], Pb = Pr[np];
        const size_t o = (size_t)row * nr + j0 + tid;
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
            const double ends = fma(Pb, bessel_g4(kb * R, b0, b1), -(Pa * bessel_g4(ka * R, a0, a1)));
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
