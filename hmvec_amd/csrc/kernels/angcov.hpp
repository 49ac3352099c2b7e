// Covariance of angular correlation functions: the bin-averaged Bessel weights, the Gaussian
// covariance of xi_mu^{ab}(theta_i) and the node weights that project an (l, l') matrix to real space.  Compiled in
// angcov.hip, a translation unit of its own.
//
// Flat sky, section 22's J_mu convention: xi_mu^{ab}(theta) = 1/(2 pi) int l dl J_mu(l theta) C^{ab}(l), mu = 0, 2, 4.
// Bin-averaged kernel of the annulus [a, b], 0 < a < b in radians:
//   K_mu(l; a, b) = 2 / ((b^2 - a^2) l^2) [F_mu(l b) - F_mu(l a)],
//   F_0(x) = x J1(x),   F_2(x) = -x J1(x) - 2 J0(x),   F_4(x) = (x - 24/x) J1(x) + 8 J0(x),
// the exact antiderivatives of x J_mu(x).  Only differences of F_mu enter, so what is evaluated is
//   G_mu(x) = F_mu(x) - F_mu(0) = int_0^x t J_mu(t) dt:   G_0 = x J1,  G_2 = 2 (1 - J0) - x J1,  G_4 = 4 + 8 J0 + x J1 - 24 J1/x,
// which start as x^2/2, x^4/32 and x^6/2304: the constants -2 and -4 of F_2 and F_4 never meet the small values they
// would swamp, and a gate in units of |G| is a gate relative to the integral itself.
//
// Spectra: C[f, g, n] symmetric in (f, g) at the nodes ells[n] (strictly increasing, >= 1), C(l) linear in l between
// nodes and zero outside; N[f] >= 0 a white noise level; the multipole sum runs over the integers
// L = {ceil(ells[0]), ..., floor(ells[-1])}.  A probe is (f, g, mu).  For P = (a, b, mu), Q = (c, d, nu), A = 4 pi fsky:
//   cov[P,i,Q,j] = 1/(2 pi A) sum_{l in L} l K_mu(l; bin i) K_nu(l; bin j) G_PQ(l)
//                + delta_ij delta_mu,nu (delta_ac delta_bd + delta_ad delta_bc) N_a N_b / (A pi (b_i^2 - a_i^2)),
//   G_PQ = C^^ac C^^bd + C^^ad C^^bc - NN,   C^^fg = C^fg + delta_fg N_f,   NN = (delta_ac delta_bd + delta_ad delta_bc) N_a N_b:
// the noise x noise product is a delta function in theta whose l sum does not converge; it is taken out of the sum and
// added in closed form (for mu != nu it is dropped: Cov(xi+, xi-) has no pure shape-noise term).
// Node weights: R_mu[i, n] = sum_{l in L} l K_mu(l; bin i) h_n(l), h_n the hat function of node n.
//
// The first part of this file is plain C++ (the F functions given J0 and J1): tests/cpp/angcov_host.cpp builds it with a
// host compiler.  The kernels follow under __HIPCC__.
#pragma once
#include "bessel_g4.hpp"

namespace hmg {

// Below these x G_2 and G_4 come from their power series in y = x^2/4,
//   G_2 = y^2/2  (1 - 2y/(1*3*3) (1 - 3y/(2*4*4) (1 - ...))),     ratio of terms k-1 -> k:  y (k+1) / (k (k+2)^2)
//   G_4 = y^3/36 (1 - 3y/(4*1*5) (1 - 4y/(5*2*6) (1 - ...))),                               y (k+2) / ((k+3) k (k+4))
// nested through k = AC_SERIES_N.  G_2's closed form subtracts x J1 from 2 (1 - J0): at x = 1 the two are 0.47 and 0.44
// and leave 0.030 (a loss of 30), at x = 2 a loss of 6.8, at x = 3 2.52 and 1.02 leave 1.50 (2.4).  Its series at x = 3
// (y = 2.25) has terms 2.53, 1.27, 0.27, ... against the sum 1.50 (2.7): the two sides meet at 3, and the first term
// left out there (k = 16) is below 1e-22 of the first.  G_4 is bessel_g4 (bessel_g4.hpp), the function that gives W_4
// its end terms, with its switch at 5 (losses 3.4 and 6.7 on the two sides) and its 15 nested terms; the analysis is
// section 22's.
constexpr double AC_SERIES_X2 = 3.0;
constexpr double AC_SERIES_X4 = G4_SERIES_X;
constexpr int AC_SERIES_N = 15;

HMG_HD_FN double angcov_g0(double x, double j0, double j1) { return x * j1; }

HMG_HD_FN double angcov_g2(double x, double j0, double j1) {
    const double y = 0.25 * x * x;
    double s = 1.0;
#pragma unroll
    for (int k = AC_SERIES_N; k >= 1; --k) s = std::fma(-y * ((k + 1.0) / (k * (k + 2.0) * (k + 2.0))), s, 1.0);
    return x < AC_SERIES_X2 ? y * y * 0.5 * s : std::fma(-x, j1, 2.0 * (1.0 - j0));
}

// G_mu by order index o = mu / 2
HMG_HD_FN double angcov_g(int o, double x, double j0, double j1) {
    return o == 0 ? angcov_g0(x, j0, j1) : o == 1 ? angcov_g2(x, j0, j1) : bessel_g4(x, j0, j1);
}

// K_mu(l; a, b) from G_mu at the two edges: pre = 2 / ((b - a)(b + a)), one division by l^2
HMG_HD_FN double angcov_weight(double ga, double gb, double pre, double l) { return (gb - ga) * (pre / (l * l)); }

}  // namespace hmg

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../../include/hmgrid.h"
#include "../j01.hpp"

namespace hmg {

// From here on a product is fused into a sum only where fma() is written: the bit-identities of this file (a value that
// does not depend on how a probe is spelled, cov[P,i,Q,j] == cov[Q,j,P,i]) rest on sums of products that are rounded
// term by term.  (HIP's __dmul_rn and __dadd_rn would not do: they are the plain operators compiled with contraction
// allowed, and a product and a sum that both allow it are fused after inlining.)
#pragma clang fp contract(off)

constexpr int AC_CHUNK = HMG_ANGCOV_CHUNK;    // multipoles per partial sum: fixed, so the order of summation depends on L alone
constexpr int AC_STAGE = 32;                  // multipoles staged in LDS at a time
constexpr int AC_TILE = HMG_ANGCOV_TILE;      // bins of each probe per workgroup
constexpr int AC_THREADS = 64;    // one wavefront; each thread owns a 4 x 4 register tile of (i, j)
static_assert(AC_CHUNK % AC_STAGE == 0 && AC_TILE == 32 && AC_THREADS == 64, "the tile maps below assume these");

// K[o][l, i] = K_mu(ells[l]; edges[i], edges[i + 1]) for the orders whose pointer is not NULL; K (nl, nt), bins fastest.
// One thread per multipole walks the nt + 1 edges once: J0 and J1 are evaluated once per (l, edge) and every G_mu of an
// edge serves the two bins that share it.  A value depends on its l and its two edges alone.
__global__ __launch_bounds__(256) void angcov_weights_kernel(int nl, int nt, const double* __restrict__ ells,
                                                             const double* __restrict__ edges, double* __restrict__ k0,
                                                             double* __restrict__ k2, double* __restrict__ k4) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nl) return;
    const double ell = ells[l];
    double a = edges[0], j0, j1;
    bessel_j01(ell * a, j0, j1);
    double g0 = angcov_g0(ell * a, j0, j1), g2 = angcov_g2(ell * a, j0, j1), g4 = bessel_g4(ell * a, j0, j1);
    const size_t row = (size_t)l * nt;
#pragma unroll 1
    for (int i = 0; i < nt; ++i) {
        const double b = edges[i + 1], x = ell * b;
        bessel_j01(x, j0, j1);
        const double h0 = angcov_g0(x, j0, j1), h2 = angcov_g2(x, j0, j1), h4 = bessel_g4(x, j0, j1);
        const double pre = 2.0 / ((b - a) * (b + a));
        if (k0) k0[row + i] = angcov_weight(g0, h0, pre, ell);
        if (k2) k2[row + i] = angcov_weight(g2, h2, pre, ell);
        if (k4) k4[row + i] = angcov_weight(g4, h4, pre, ell);
        a = b, g0 = h0, g2 = h2, g4 = h4;
    }
}

// The panel of the node table that holds l: the largest n <= nn - 2 with nodes[n] <= l, and t = (l - nodes[n]) / width.
// A node that is hit exactly gives t = 0 (t = 1 at the last one), and t c1 + (1 - t) c0 then returns the node's value.
__device__ __forceinline__ void angcov_panel(const double* __restrict__ nodes, int nn, double l, int& n, double& t) {
    int lo = 0, hi = nn - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (nodes[mid] <= l) lo = mid;
        else hi = mid - 1;
    }
    n = lo;
    t = (l - nodes[lo]) / (nodes[lo + 1] - nodes[lo]);
}

__device__ __forceinline__ double angcov_cl(const double* __restrict__ C, int nf, int nn, int f, int g, int n, double t) {
    const int lo = f < g ? f : g, hi = f < g ? g : f;          // C is symmetric: the (min, max) entry is the one read
    const double* c = C + ((size_t)lo * nf + hi) * nn + n;
    return fma(t, c[1], (1.0 - t) * c[0]);
}

// G_PQ(l) = C^^ac C^^bd + C^^ad C^^bc - NN with the noise products multiplied out, so that NN is never formed and
// C = 0 gives exactly 0.  Every parenthesis is a sum of two terms that the symmetries (a <-> b, c <-> d, P <-> Q) swap
// or keep: the value has the same bits however the probes are written.
__device__ __forceinline__ double angcov_gpq(const double* __restrict__ C, const double* __restrict__ N, int nf, int nn,
                                             int a, int b, int c, int d, int n, double t) {
    const double cac = angcov_cl(C, nf, nn, a, c, n, t), cbd = angcov_cl(C, nf, nn, b, d, n, t);
    const double cad = angcov_cl(C, nf, nn, a, d, n, t), cbc = angcov_cl(C, nf, nn, b, c, n, t);
    const double t1 = cac * cbd, t2 = cad * cbc;
    const double t3 = b == d ? N[b] * cac : 0.0, t4 = a == c ? N[a] * cbd : 0.0;
    const double t5 = b == c ? N[b] * cad : 0.0, t6 = a == d ? N[a] * cbc : 0.0;
    return (t1 + t2) + ((t3 + t4) + (t5 + t6));
}

// (P, Q), P <= Q, of the pair index p among np probes, rows of the upper triangle one after the other
__device__ __forceinline__ void angcov_pair(int p, int np, int& P, int& Q) {
    P = 0;
    while (p >= np - P) p -= np - P, ++P;
    Q = P + p;
}
__device__ __forceinline__ int angcov_pair_index(int P, int Q, int np) { return P * np - P * (P - 1) / 2 + (Q - P); }

// The order two probes are contracted in is decided by what they are, not by where they stand in the call:
// the key (order, smaller field, larger field).  -1 / 0 / 1.
__device__ __forceinline__ int angcov_compare(const int* __restrict__ probes, int P, int Q) {
    const int* p = probes + 3 * P;
    const int* q = probes + 3 * Q;
    const int plo = p[0] < p[1] ? p[0] : p[1], phi = p[0] < p[1] ? p[1] : p[0];
    const int qlo = q[0] < q[1] ? q[0] : q[1], qhi = q[0] < q[1] ? q[1] : q[0];
    if (p[2] != q[2]) return p[2] < q[2] ? -1 : 1;
    if (plo != qlo) return plo < qlo ? -1 : 1;
    if (phi != qhi) return phi < qhi ? -1 : 1;
    return 0;
}

// partial[pair, chunk, i, j] = sum over the chunk's multipoles, in order, of (l G_PQ(l) K_mu(l; i)) K_nu(l; j), with
// (mu, i) the bins of the pair's first probe by angcov_compare.  Grid (pairs, chunks, tiles^2); one wavefront per block.
// Per stage of AC_STAGE multipoles: l G_PQ(l) is interpolated from the node table into LDS, then the two K tiles are
// staged (the first already times l G) and every thread adds the stage to its 4 x 4 accumulators with one fma per
// element and multipole.  Multipoles past the chunk's end and bins past nt are staged as 0: fma(0, 0, s) = s.
// An accumulator sees its own two probes, its two bins and the chunk's multipoles in order, nothing else.
// CURVED: the measure is l + 1/2 instead of l, a probe's third entry names one of the four
// curved-sky kinds and k6 holds the fourth kind's weights (kernels/curvedsky.hpp); the flat form never reads k6.
template <bool CURVED>
__global__ __launch_bounds__(AC_THREADS) void angcov_gaussian_kernel(
    int nf, int nn, const double* __restrict__ nodes, const double* __restrict__ C, const double* __restrict__ N, int l0,
    int nl, int nt, int np, const int* __restrict__ probes, const double* __restrict__ k0, const double* __restrict__ k2,
    const double* __restrict__ k4, const double* __restrict__ k6, double* __restrict__ partial) {
    __shared__ double sw[AC_STAGE];
    __shared__ __attribute__((aligned(16))) double sa[AC_STAGE][AC_TILE];
    __shared__ __attribute__((aligned(16))) double sb[AC_STAGE][AC_TILE];
    const int tid = threadIdx.x, chunk = blockIdx.y, tiles = (nt - 1) / AC_TILE + 1;
    const int bi0 = (blockIdx.z / tiles) * AC_TILE, bj0 = (blockIdx.z % tiles) * AC_TILE;
    int P, Q;
    angcov_pair(blockIdx.x, np, P, Q);
    if (angcov_compare(probes, P, Q) > 0) {
        const int s = P;
        P = Q, Q = s;
    }
    const int a = probes[3 * P], b = probes[3 * P + 1], c = probes[3 * Q], d = probes[3 * Q + 1];
    const int oa = probes[3 * P + 2], ob = probes[3 * Q + 2];
    const double* ka = oa == 0 ? k0 : oa == 1 ? k2 : !CURVED || oa == 2 ? k4 : k6;
    const double* kb = ob == 0 ? k0 : ob == 1 ? k2 : !CURVED || ob == 2 ? k4 : k6;
    const int la = chunk * AC_CHUNK, lb = nl - la < AC_CHUNK ? nl : la + AC_CHUNK;
    const int ti = 4 * (tid / 8), tj = 4 * (tid % 8);
    double acc[4][4] = {};
#pragma unroll 1
    for (int s = la; s < lb; s += AC_STAGE) {
        __syncthreads();                                  // the previous stage has been read
        if (tid < AC_STAGE) {
            double w = 0.0;
            if (s + tid < lb) {
                const double l = (double)(l0 + s + tid);
                int n;
                double t;
                angcov_panel(nodes, nn, l, n, t);
                w = (CURVED ? l + 0.5 : l) * angcov_gpq(C, N, nf, nn, a, b, c, d, n, t);
            }
            sw[tid] = w;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < AC_STAGE * AC_TILE / AC_THREADS; ++r) {
            const int e = tid + AC_THREADS * r, ll = e / AC_TILE, i = e % AC_TILE, l = s + ll;
            const bool in = l < lb;
            const double va = in && bi0 + i < nt ? ka[(size_t)l * nt + bi0 + i] : 0.0;
            const double vb = in && bj0 + i < nt ? kb[(size_t)l * nt + bj0 + i] : 0.0;
            sa[ll][i] = va * sw[ll];
            sb[ll][i] = vb;
        }
        __syncthreads();
#pragma unroll 4
        for (int ll = 0; ll < AC_STAGE; ++ll) {
            double x[4], y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = sa[ll][ti + q], y[q] = sb[ll][tj + q];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(x[p], y[q], acc[p][q]);
        }
    }
    double* out = partial + ((size_t)blockIdx.x * gridDim.y + chunk) * nt * nt;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (bi0 + ti + p < nt && bj0 + tj + q < nt) out[(size_t)(bi0 + ti + p) * nt + bj0 + tj + q] = acc[p][q];
}

// cov[P, i, Q, j] = pref * (the chunks' partial sums added in chunk order from 0.0) + the closed-form noise term.
// One thread per element: it finds where its value lies in partial - the pair's block, oriented by angcov_compare, and
// for two probes of one key the (smaller bin, larger bin) entry - so cov[P,i,Q,j] and cov[Q,j,P,i] read the same words.
// CURVED: `edges` holds cos a_i - cos b_i per bin instead of the edges, and the noise term's denominator is
// area 2 pi (cos a_i - cos b_i).
template <bool CURVED>
__global__ __launch_bounds__(256) void angcov_combine_kernel(int nchunks, int nt, int np, size_t total,
                                                             const int* __restrict__ probes,
                                                             const double* __restrict__ N,
                                                             const double* __restrict__ edges, double pref,
                                                             double area_pi, const double* __restrict__ partial,
                                                             double* __restrict__ cov) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int j = e % nt, Q = (e / nt) % np, i = (e / ((size_t)nt * np)) % nt, P = e / ((size_t)nt * np * nt);
    const int cmp = angcov_compare(probes, P, Q);
    int bi = cmp <= 0 ? i : j, bj = cmp <= 0 ? j : i;             // bins of the first and of the second probe
    if (cmp == 0 && bi > bj) {
        const int s = bi;
        bi = bj, bj = s;
    }
    const int pair = P <= Q ? angcov_pair_index(P, Q, np) : angcov_pair_index(Q, P, np);
    const double* src = partial + (size_t)pair * nchunks * nt * nt + (size_t)bi * nt + bj;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s = s + src[(size_t)c * nt * nt];
    double noise = 0.0;
    const int* p = probes + 3 * P;
    const int* q = probes + 3 * Q;
    if (i == j && p[2] == q[2]) {
        const double cnt = (p[0] == q[0] && p[1] == q[1] ? 1.0 : 0.0) + (p[0] == q[1] && p[1] == q[0] ? 1.0 : 0.0);
        if (CURVED) {
            noise = (cnt * (N[p[0]] * N[p[1]])) / (area_pi * (2.0 * edges[i]));
        } else {
            const double ea = edges[i], eb = edges[i + 1];
            noise = (cnt * (N[p[0]] * N[p[1]])) / (area_pi * ((eb - ea) * (eb + ea)));
        }
    }
    cov[e] = fma(s, pref, noise);
}

// R[i, n] = scale * sum_{l in L} l K(l; bin i) h_n(l), h_n the hat function of node n: t on the panel below the node
// and 1 - t on the panel above, t and the panel as angcov_panel gives them.  One thread per (n, i) walks the node's own
// support in l order; the partial sum of every AC_CHUNK-aligned chunk of L starts at 0.0 and the chunks' sums are added
// in chunk order, the order of summation of the Gaussian contraction.  by_node: R is written (nn, nt), else (nt, nn).
// CURVED: the measure is l + 1/2.
template <bool CURVED>
__global__ __launch_bounds__(256) void angcov_node_weights_kernel(int nn, const double* __restrict__ nodes, int l0, int nl,
                                                                  int nt, const double* __restrict__ K, double scale,
                                                                  int by_node, double* __restrict__ R) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)nn * nt) return;
    const int i = e % nt, n = e / nt;
    const double en = nodes[n];
    // the integers of L strictly between the neighbouring nodes (the whole of L's end at the first and the last node)
    int lo = n > 0 ? (int)floor(nodes[n - 1]) + 1 : l0;
    int hi = n < nn - 1 ? (int)ceil(nodes[n + 1]) - 1 : l0 + nl - 1;
    lo = lo < l0 ? l0 : lo;
    hi = hi > l0 + nl - 1 ? l0 + nl - 1 : hi;
    double s = 0.0;
    for (int ca = (lo - l0) / AC_CHUNK * AC_CHUNK; lo <= hi && ca <= hi - l0; ca += AC_CHUNK) {
        const int a = ca + l0 < lo ? lo : ca + l0, b = ca + AC_CHUNK - 1 + l0 > hi ? hi : ca + AC_CHUNK - 1 + l0;
        double p = 0.0;
        for (int li = a; li <= b; ++li) {
            const double l = (double)li;
            const bool rising = l < en || n == nn - 1;
            const double e0 = rising ? nodes[n - (n > 0)] : en, e1 = rising ? en : nodes[n + 1];
            const double t = (l - e0) / (e1 - e0), h = rising ? t : 1.0 - t;
            p = fma((CURVED ? l + 0.5 : l) * h, K[(size_t)(li - l0) * nt + i], p);
        }
        s = s + p;
    }
    R[by_node ? (size_t)n * nt + i : (size_t)i * nn + n] = s * scale;
}

}  // namespace hmg
#endif
