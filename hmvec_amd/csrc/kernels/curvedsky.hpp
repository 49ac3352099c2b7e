// Curved-sky angular correlation functions: the bin-averaged Wigner-d weights and the shear
// factors of a node table.  Compiled in curvedsky.hip, a translation unit of its own; the contraction, its combine and
// the node weights are angcov.hpp's kernels with the measure l + 1/2 (instantiated in angcov.hip).
//
// Kinds 0 .. 3 = "w", "gammat", "xip", "xim": d^l = P_l, d^l_{0,2}, d^l_{2,2}, d^l_{2,-2} of theta.  With x = cos theta,
// s = sin^2(theta/2), t = 2 s = 1 - x, M = l (l + 1):
//   G_kind(l; theta) = int_0^theta sin(v) d_kind^l(v) dv,   K_kind(l; a, b) = [G(l; b) - G(l; a)] / (cos a - cos b),
// a spin-2 kind is 0 below l = 2.  What is carried along l, per angle (cs_state):
//   P_l;   E_l = (l + 1) D_l, D_l = P_{l+1} - P_l:   P_{l+1} = P_l + E_l / (l + 1),   E_{l+1} = E_l - (2l + 3) t P_{l+1};
//   P'_{l+1} = P'_{l-1} + (2l + 1) P_l.
// The recurrence in t never forms cos theta: at small l theta every term of it has one sign and D_l keeps a relative
// accuracy where the textbook recurrence in x loses 1 / (l^2 t).  On the chain are two dependent fma per l; the
// reciprocal 1 / (l + 1) is a per-l constant (cs_consts) that the kernel's lanes prepare side by side.
// Closed forms, in Q_l = int_x^1 P_l = -(D_l + D_{l-1}) / (2l + 1) (no cancellation at small l theta: both D have one sign):
//   G_w = Q_l
//   G_gammat = [2 (1 - x P_l) - (M + 2) Q_l] / sqrt(M (M - 2))
//   n G_xip = -(A + B),   n G_xim = 2 (M - 2) - (A - B),   n = M (M - 2) / 2,   a = l (l - 1) / 2,
//   A = -a (M + 2) Q_l - 2 a x P_l - (M + 2) P_{l-1} + 4 P'_l + 2 x P'_{l-1},   B = 2 (l^2 - l + 1) P_l - 2 x P'_l - 4 P'_{l-1}
// (the textbook antiderivative with its pair of O(l^3) terms folded into -a M Q_l by l (x P_l - P_{l-1}) = -M Q_l, and
// P'_l - x P'_{l-1} = l P_{l-1}, x P'_l - P'_{l-1} = l P_l).  The spin-2 forms subtract O(1 / M) constants and O(P / M)
// terms from each other and start as powers of M s: below CS_SWITCH_* in M s they come from the terminating
// hypergeometric series of the Jacobi polynomial instead, integrated term by term, c_k the coefficients of
// 2F1(2 - l, l + 3; c; s), ratio c_k / c_{k-1} = -(M - 2 - k (k + 3)) / (k (k + c - 1)):
//   G_xip = 2 s sum_k c_k s^k [1/(k+1) - 2 s/(k+2) + s^2/(k+3)]                         (c = 1, times (1 - s)^2)
//   G_gammat = sqrt(M (M - 2)) s^2 sum_k c_k s^k [1/(k+2) - s/(k+3)]                     (c = 3, times s (1 - s))
//   G_xim = M (M - 2)/12 s^3 sum_k c_k s^k / (k+3)                                        (c = 5, times s^2)
// nested through k = CS_SERIES_N; the brackets are positive, a series ends by itself at k = l - 2 (its ratio is an exact
// zero there), and M s plays the part of x^2/4 in section 23's series.  Losses (sum of |terms| over |sum|, the worst of
// l = 2 .. 20000 at the switch, in 60 digits): series xip 11.7, gammat 2.7, xim 6.6; closed forms xip 5.7, gammat 2.5,
// xim 3.4, falling with M s.  The first term left out at the switch is below 1e-18 of the first.
//
// The first part of this file is plain C++: tests/cpp/curvedsky_host.cpp builds it with a host compiler.  The kernels
// follow under __HIPCC__.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define HMG_CS_FN __host__ __device__ __forceinline__
#else
#define HMG_CS_FN inline
#endif

namespace hmg {

// a product is fused into a sum only where fma() is written, on the host and on the device alike
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

constexpr int CS_KINDS = 4;
constexpr double CS_SWITCH_2 = 2.25;          // xip, gammat: series below M s = 2.25 (l theta about 3)
constexpr double CS_SWITCH_4 = 6.25;          // xim: below 6.25 (l theta about 5)
constexpr int CS_SERIES_N = 15;

struct cs_state {
    double p, e, pm, dm, dp, dpm;             // P_l, E_l, P_{l-1}, D_{l-1}, P'_l, P'_{l-1}
};

// what depends on l alone
struct cs_consts {
    double r, i2, M, N4, root, iroot, inv_n, a;      // 1/(l+1), 1/(2l+1), l(l+1), M - 2, sqrt(M N4), its inverse, 2/(M N4), l(l-1)/2
};

HMG_CS_FN cs_consts cs_consts_of(double l) {
    cs_consts c;
    c.r = 1.0 / (l + 1.0);
    c.i2 = 1.0 / (2.0 * l + 1.0);
    c.M = l * (l + 1.0);
    c.N4 = c.M - 2.0;
    const double mn = l < 2.0 ? 1.0 : c.M * c.N4;          // (spin-2 kinds are not evaluated below l = 2)
    c.root = std::sqrt(mn);
    c.iroot = 1.0 / c.root;
    c.inv_n = 2.0 / mn;
    c.a = 0.5 * l * (l - 1.0);
    return c;
}

// the state at l = 0 for t = 2 sin^2(theta/2)
HMG_CS_FN cs_state cs_start(double t) { return cs_state{1.0, -t, 0.0, 0.0, 0.0, 0.0}; }

// l -> l + 1; r = 1 / (l + 1)
HMG_CS_FN void cs_step(cs_state& q, double l, double t, double r) {
    const double d = q.e * r;
    const double pn = std::fma(q.e, r, q.p);
    const double dpn = std::fma(2.0 * l + 1.0, q.p, q.dpm);
    q.e = std::fma(-((2.0 * l + 3.0) * t), pn, q.e);
    q.pm = q.p, q.dm = d, q.dpm = q.dp, q.dp = dpn, q.p = pn;
}

HMG_CS_FN double cs_q(const cs_state& q, const cs_consts& c) { return -(q.e * c.r + q.dm) * c.i2; }

HMG_CS_FN double cs_g_gammat(const cs_state& q, const cs_consts& c, double s, double x, double Q) {
    double h = 1.0 / (CS_SERIES_N + 2.0) - s * (1.0 / (CS_SERIES_N + 3.0));
#pragma unroll
    for (int k = CS_SERIES_N; k >= 1; --k)
        h = std::fma((-(c.N4 - k * (k + 3.0)) * (1.0 / (k * (k + 2.0)))) * s, h, 1.0 / (k + 1.0) - s * (1.0 / (k + 2.0)));
    const double closed = (2.0 * (1.0 - x * q.p) - (c.M + 2.0) * Q) * c.iroot;
    return c.M * s < CS_SWITCH_2 ? c.root * s * s * h : closed;
}

HMG_CS_FN void cs_ab(const cs_state& q, const cs_consts& c, double l, double x, double Q, double& A, double& B) {
    A = -(c.a * (c.M + 2.0)) * Q - (2.0 * c.a) * (x * q.p) - (c.M + 2.0) * q.pm + 4.0 * q.dp + 2.0 * (x * q.dpm);
    B = 2.0 * (l * l - l + 1.0) * q.p - 2.0 * (x * q.dp) - 4.0 * q.dpm;
}

HMG_CS_FN double cs_g_xip(const cs_consts& c, double s, double A, double B) {
    double h = 1.0 / (CS_SERIES_N + 1.0) - s * (2.0 / (CS_SERIES_N + 2.0) - s * (1.0 / (CS_SERIES_N + 3.0)));
#pragma unroll
    for (int k = CS_SERIES_N; k >= 1; --k)
        h = std::fma((-(c.N4 - k * (k + 3.0)) * (1.0 / (k * (double)k))) * s, h,
                     1.0 / k - s * (2.0 / (k + 1.0) - s * (1.0 / (k + 2.0))));
    return c.M * s < CS_SWITCH_2 ? 2.0 * s * h : (-A - B) * c.inv_n;
}

HMG_CS_FN double cs_g_xim(const cs_consts& c, double s, double A, double B) {
    double h = 1.0 / (CS_SERIES_N + 3.0);
#pragma unroll
    for (int k = CS_SERIES_N; k >= 1; --k)
        h = std::fma((-(c.N4 - k * (k + 3.0)) * (1.0 / (k * (k + 4.0)))) * s, h, 1.0 / (k + 2.0));
    return c.M * s < CS_SWITCH_4 ? (c.M * c.N4) * (1.0 / 12.0) * (s * s * s) * h : (2.0 * c.N4 - A + B) * c.inv_n;
}

// G of the four kinds at l >= 1 from the state at l; want: bit k set = kind k asked for (the others are left alone)
HMG_CS_FN void cs_g_all(const cs_state& q, const cs_consts& c, double l, double s, double x, int want, double* g) {
    const double Q = cs_q(q, c);
    const bool low = l < 2.0;
    if (want & 1) g[0] = Q;
    if (want & 2) g[1] = low ? 0.0 : cs_g_gammat(q, c, s, x, Q);
    if (want & 12) {
        double A, B;
        cs_ab(q, c, l, x, Q, A, B);
        if (want & 4) g[2] = low ? 0.0 : cs_g_xip(c, s, A, B);
        if (want & 8) g[3] = low ? 0.0 : cs_g_xim(c, s, A, B);
    }
}

// K from G at the two edges; pre = 1 / (cos a - cos b)
HMG_CS_FN double cs_weight(double ga, double gb, double pre) { return (gb - ga) * pre; }

// cos a - cos b without forming either cosine
HMG_CS_FN double cs_cosdiff(double a, double b) { return 2.0 * (std::sin(0.5 * (a + b)) * std::sin(0.5 * (b - a))); }

// the factor of one spin-2 leg of a kappa spectrum at the node l: sqrt((l + 2)(l - 1) / (l (l + 1)))
HMG_CS_FN double cs_shear_factor(double l) { return std::sqrt(((l + 2.0) * (l - 1.0)) / (l * (l + 1.0))); }

}  // namespace hmg

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace hmg {

#pragma clang fp contract(off)                // (again: the pragma ends with the namespace block it stands in)

constexpr int CS_THREADS = 64;                // one wavefront: CS_THREADS edges, CS_THREADS - 1 bins per workgroup
constexpr int CS_STAGE = 16;                  // multipoles per stage: their constants and their G's pass through LDS
constexpr int CS_SEGMENT = 256;               // multipoles of L per workgroup
static_assert(CS_SEGMENT % CS_STAGE == 0 && CS_STAGE <= CS_THREADS, "the stage maps below assume these");

// K[kind][l - l0, i] for the kinds whose pointer is not NULL, on l = l0 .. l0 + nl - 1 and the bins edges[i : i + 2];
// cosdiff[i] = cos edges[i] - cos edges[i + 1].  Grid (tiles of CS_THREADS - 1 bins, segments of CS_SEGMENT multipoles).
// One thread per edge: it walks the bare recurrence from l = 0 to the segment's first multipole (two fma on the chain,
// the reciprocals from LDS, where the lanes computed 64 of them side by side) and then, stage by stage, steps on, forms the
// G's of its edge and leaves them in LDS; after the barrier thread j reads edge j + 1's and writes bin j's weights, a
// row segment per multipole.  Every segment and every tile runs cs_step from l = 0 in the same order: a value depends
// on its l and its two edges alone.
__global__ __launch_bounds__(CS_THREADS) void curvedsky_weights_kernel(int l0, int nl, int nt,
                                                                       const double* __restrict__ edges,
                                                                       const double* __restrict__ cosdiff,
                                                                       double* __restrict__ kw, double* __restrict__ kg,
                                                                       double* __restrict__ kp, double* __restrict__ km) {
    __shared__ double sr[CS_THREADS];
    __shared__ cs_consts sc[CS_STAGE];
    __shared__ double sg[CS_KINDS][CS_STAGE][CS_THREADS];
    const int tid = threadIdx.x, bin = blockIdx.x * (CS_THREADS - 1) + tid;
    const int la = l0 + blockIdx.y * CS_SEGMENT, lb = la + CS_SEGMENT < l0 + nl ? la + CS_SEGMENT : l0 + nl;
    const int edge = bin <= nt ? bin : nt;                       // lanes past the last edge repeat it and write nothing
    const double sh = sin(0.5 * edges[edge]), s = sh * sh, t = 2.0 * s, x = 1.0 - t;
    const bool writes = tid < CS_THREADS - 1 && bin < nt;
    const double pre = writes ? 1.0 / cosdiff[bin] : 0.0;
    const int want = (kw ? 1 : 0) | (kg ? 2 : 0) | (kp ? 4 : 0) | (km ? 8 : 0);
    double* const out[CS_KINDS] = {kw, kg, kp, km};
    cs_state q = cs_start(t);
    // l = 0 .. la - 1: the walk.  A stage's reciprocals are read 16 at a time into registers ahead of the chain: read
    // one by one inside it, each step would wait out an LDS round trip.
#pragma unroll 1
    for (int l = 0; l < la; l += CS_THREADS) {
        __syncthreads();
        sr[tid] = 1.0 / (l + tid + 1.0);
        __syncthreads();
        const int n = la - l < CS_THREADS ? la - l : CS_THREADS;
        int ll = 0;
#pragma unroll 1
        for (; ll + 16 <= n; ll += 16) {
            double r[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) r[j] = sr[ll + j];
#pragma unroll
            for (int j = 0; j < 16; ++j) cs_step(q, (double)(l + ll + j), t, r[j]);
        }
#pragma unroll 1
        for (; ll < n; ++ll) cs_step(q, (double)(l + ll), t, sr[ll]);
    }
    // l = la .. lb - 1: the state is at l when G is formed, then steps
#pragma unroll 1
    for (int l = la; l < lb; l += CS_STAGE) {
        __syncthreads();                                         // the previous stage's G's have been read
        if (tid < CS_STAGE) sc[tid] = cs_consts_of((double)(l + tid));
        __syncthreads();
        const int n = lb - l < CS_STAGE ? lb - l : CS_STAGE;
#pragma unroll 1
        for (int ll = 0; ll < n; ++ll) {
            const cs_consts c = sc[ll];
            double g[CS_KINDS] = {0.0, 0.0, 0.0, 0.0};
            cs_g_all(q, c, (double)(l + ll), s, x, want, g);
#pragma unroll
            for (int k = 0; k < CS_KINDS; ++k) sg[k][ll][tid] = g[k];
            cs_step(q, (double)(l + ll), t, c.r);
        }
        __syncthreads();
        if (writes) {
#pragma unroll
            for (int k = 0; k < CS_KINDS; ++k) {
                if (!out[k]) continue;
#pragma unroll 4
                for (int ll = 0; ll < n; ++ll)
                    out[k][(size_t)(l + ll - l0) * nt + bin] = cs_weight(sg[k][ll][tid], sg[k][ll][tid + 1], pre);
            }
        }
    }
}

// C[f, g, n] *= f(nodes[n])^(number of spin-2 fields among f and g), f = cs_shear_factor: kappa spectra to E-mode spectra
__global__ __launch_bounds__(256) void curvedsky_scale_kernel(int nf, int nn, const double* __restrict__ nodes,
                                                              const int* __restrict__ spins, double* __restrict__ C) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)nf * nf * nn) return;
    const int n = e % nn, g = (e / nn) % nf, f = e / ((size_t)nn * nf);
    const bool sf = spins[f] == 2, sg = spins[g] == 2;
    if (!sf && !sg) return;
    const double l = nodes[n], fac = cs_shear_factor(l);
    // both legs: f^2 is the ratio itself, formed without the root, and the same for (f, g) and (g, f)
    C[e] = C[e] * (sf && sg ? ((l + 2.0) * (l - 1.0)) / (l * (l + 1.0)) : fac);
}

}  // namespace hmg
#endif
