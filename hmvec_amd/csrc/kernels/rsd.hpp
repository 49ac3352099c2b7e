// Redshift-space spectra of the dispersion halo model: the wedges P^s(k, mu) and the multipoles
// P_0, P_2, P_4 of one pair of tracers at nodes of the k grid.
//     species of a leg x at (z, m, k): (p0, h0) = (Nc/ngal (u_c or 1), alpha_c^2 / 2), (p1, h1) = (Ns/ngal u_s, alpha_s^2 / 2)
//                                      of an HOD;  p0 = 0, (p1, h1) = (m/rho_m0 u, alpha_m^2 / 2) of a matter name
//     w^s_x(mu)   = p0 E(h0) + p1 E(h1),   E(h) = exp(-h x^2 mu^2),  x = k sigma_s[z,m]
//     P1h[z,s,q]  = damp[s] sum_m wm nzm S^s,   S^s = w^s_a w^s_b, or of two HOD names the first name's
//                   2<NcNs>/ngal^2 u_c u_s E(h0) E(h1) + <Ns(Ns-1)>/ngal^2 u_s^2 E(h1)^2
//     I^s = sum_m wm nzm bh w^s,  V^s = sum_m wm nzm w^s,  J^s = (I^s + b) - C,  K^s = (V^s + 1) - C0
//     P2h[z,s,q]  = P_lin (J^s_a + f mu^2 K^s_a) (J^s_b + f mu^2 K^s_b)
//     Q_n[z,s]    = sum_m wm nzm sum_terms v M_n((h_i + h_j) x^2),  M_n of gauss_moments.hpp; the 1-halo multipoles are
//                   P_0 = Q_0, P_2 = 5/2 (3 Q_1 - Q_0), P_4 = 9/8 (35 Q_2 - 30 Q_1 + 3 Q_0), times damp[s]
// The form of a leg is kernels/leg_form.hpp's (device functions only); C, C0, b of a leg are the leg sums of sampled.hip.
// Included by rsd.hip alone (its own translation unit: the other units do not see these kernels).
#pragma once
#include "../gauss_moments.hpp"
#include "leg_form.hpp"

namespace hmg {

constexpr int RSD_THREADS = 256;    // samples per workgroup
constexpr int RSD_CHUNK = 128;      // mass bins staged through LDS at a time: 128 * 9 * 8 B = 9 KB
constexpr int RSD_NCF = 9;          // per bin: the four slot coefficients, the two HOD-HOD coefficients, wn, wn bh, sigma_s
constexpr int RSD_MU = 8;           // mu nodes per thread: 5 accumulators each stay in registers
constexpr int RSD_MAXMU = 32;       // mu nodes per call

struct RsdArgs {
    BisLeg a, b;
    const double *NcNs, *NsNsm1;    // of leg a (two HOD names: the first name's square term)
    int same, hh;                   // leg b is leg a; both are HODs
    double ha0, ha1, hb0, hb1;      // alpha^2 / 2 of the two slots of each leg
    HaloGrid g;
    const double *sigma;            // [nz][nm]
    const double *f;                // [nz]
    const int* kidx;                // [n] node of each sample
    const double* damp;             // [n] the factor of the 1-halo term
    const double* mus;              // [nmu]
    const double* wl;               // [3][nmu] (2l + 1) w_q L_l(mu_q)
    const double *legs_a, *legs_b;  // [3][nz] each: C, C0, b
    double* out;                    // wedges [2][nz][n][nmu]; multipoles [2][nz][n][3]
    double* parts;                  // wedges [4][nz][n][nmu] = (I_a, V_a, I_b, V_b); multipoles [3][nz][n] = Q_n; or NULL
    double* w2h;                    // multipoles: the 2-halo wedge [nz][n][nmu]
    int n, nmu;
};

// one thread per bin of the chunk: the coefficients of the slots, the weights and the dispersion into LDS
__device__ __forceinline__ void rsd_stage(const RsdArgs& A, int z, int m, double* c) {
    const size_t zm = (size_t)z * A.g.nm + m;
    double ca[3], cb[3], lowk, ngals;
    bis_leg_form(A.a, zm, z, A.g.ms[m], A.g.rho_m0, ca, lowk, ngals);
    c[0] = ca[0] + ca[2];                      // (one of the two is zero)
    c[1] = ca[1];
    if (A.same) {
        c[2] = c[0];
        c[3] = c[1];
    } else {
        bis_leg_form(A.b, zm, z, A.g.ms[m], A.g.rho_m0, cb, lowk, ngals);
        c[2] = cb[0] + cb[2];
        c[3] = cb[1];
    }
    c[4] = c[5] = 0.0;
    if (A.hh) {
        const double ng = A.a.ngal[z], ng2 = ng * ng;
        c[4] = 2.0 * A.NcNs[zm] / ng2;
        c[5] = A.NsNsm1[zm] / ng2;
    }
    const double wn = A.g.wm[m] * A.g.nzm[zm];
    c[6] = wn;
    c[7] = wn * A.g.bh[zm];
    c[8] = A.sigma[zm];
}

// the (at most four) tensor values of a bin at a node: u_c (1 without a central profile) and u_s (or u) of each leg;
// a tensor both legs name is loaded once
__device__ __forceinline__ void rsd_load(const RsdArgs& A, size_t at, double& ua0, double& ua1, double& ub0, double& ub1) {
    ua1 = A.a.prof[at];
    ua0 = A.a.cprof ? A.a.cprof[at] : 1.0;
    if (A.same) {
        ub0 = ua0;
        ub1 = ua1;
    } else {
        ub1 = A.b.prof == A.a.prof ? ua1 : A.b.prof[at];
        ub0 = !A.b.cprof ? 1.0 : A.b.cprof == A.a.cprof ? ua0 : A.b.cprof[at];
    }
}

// Wedges.  grid (blocks of RSD_THREADS samples, nz, chunks of RSD_MU nodes of mu), RSD_THREADS threads: thread s owns one
// sample of one redshift and RSD_MU nodes of mu, and walks the whole mass axis in order - no split over workgroups, no
// atomics: a result depends on its own (z, s, q), the tables and the tensors alone.  A wave's lanes are consecutive
// samples: with consecutive nodes their loads fall in one tensor row.  Per bin the tensor values are loaded once and
// the mu loop runs in registers; a Gaussian is evaluated once per distinct non-zero alpha (alpha = 0: the factor 1).
// ONEH = false leaves the 1-halo sum out and writes the 2-halo wedge to A.w2h (the multipoles' first step).
template <bool ONEH>
__global__ __launch_bounds__(RSD_THREADS) void rsd_wedge_kernel(RsdArgs A) {
    __shared__ double cf[RSD_CHUNK * RSD_NCF];
    const int tid = threadIdx.x, s = blockIdx.x * RSD_THREADS + tid, z = blockIdx.y, q0 = blockIdx.z * RSD_MU;
    const int nq = min(RSD_MU, A.nmu - q0);
    const bool live = s < A.n;
    const int id = live ? A.kidx[s] : 0;
    const double k = A.g.ks[id];
    const bool useA0 = A.a.kind == HMG_TRACER_HOD, useB0 = A.b.kind == HMG_TRACER_HOD;
    double mu2[RSD_MU], s1[RSD_MU], Ia[RSD_MU], Va[RSD_MU], Ib[RSD_MU], Vb[RSD_MU];
#pragma unroll
    for (int q = 0; q < RSD_MU; ++q) {
        const double mu = q < nq ? A.mus[q0 + q] : 0.0;
        mu2[q] = mu * mu;
        s1[q] = Ia[q] = Va[q] = Ib[q] = Vb[q] = 0.0;
    }
    for (int m0 = 0; m0 < A.g.nm; m0 += RSD_CHUNK) {
        const int mc = min(RSD_CHUNK, A.g.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed
        if (tid < mc) rsd_stage(A, z, m0 + tid, cf + tid * RSD_NCF);
        __syncthreads();
        if (!live) continue;
        const size_t at0 = ((size_t)z * A.g.nm + m0) * (size_t)A.g.nk + id;
        for (int ml = 0; ml < mc; ++ml) {
            const double* c = cf + ml * RSD_NCF;
            double ua0, ua1, ub0, ub1;
            rsd_load(A, at0 + (size_t)ml * A.g.nk, ua0, ua1, ub0, ub1);
            const double pa0 = c[0] * ua0, pa1 = c[1] * ua1, pb0 = c[2] * ub0, pb1 = c[3] * ub1;
            const double t0 = c[4] * ua0 * ua1, t1 = c[5] * ua1 * ua1;
            const double wn = c[6], wnb = c[7];
            const double x = k * c[8], x2 = x * x;
            const double ga0 = A.ha0 * x2, ga1 = A.ha1 * x2, gb0 = A.hb0 * x2, gb1 = A.hb1 * x2;
#pragma unroll
            for (int q = 0; q < RSD_MU; ++q) {
                if (q < nq) {
                    const double m2 = mu2[q];
                    const double Ea1 = A.ha1 != 0.0 ? exp(-(ga1 * m2)) : 1.0;
                    const double Ea0 = !useA0 || A.ha0 == 0.0 ? 1.0 : A.ha0 == A.ha1 ? Ea1 : exp(-(ga0 * m2));
                    const double wa = fma(pa1, Ea1, pa0 * Ea0);
                    Ia[q] = fma(wnb, wa, Ia[q]);
                    Va[q] = fma(wn, wa, Va[q]);
                    double wb = wa;
                    if (!A.same) {
                        const double Eb1 = A.hb1 == A.ha1 ? Ea1 : A.hb1 != 0.0 ? exp(-(gb1 * m2)) : 1.0;
                        const double Eb0 = !useB0 || A.hb0 == 0.0     ? 1.0
                                           : useA0 && A.hb0 == A.ha0 ? Ea0
                                           : A.hb0 == A.hb1          ? Eb1
                                                                     : exp(-(gb0 * m2));
                        wb = fma(pb1, Eb1, pb0 * Eb0);
                        Ib[q] = fma(wnb, wb, Ib[q]);
                        Vb[q] = fma(wn, wb, Vb[q]);
                    }
                    if (ONEH) {
                        const double S = A.hh ? fma(t1, Ea1 * Ea1, t0 * (Ea0 * Ea1)) : wa * wb;
                        s1[q] = fma(wn, S, s1[q]);
                    }
                }
            }
        }
    }
    if (!live) return;
    {   // the epilogue, every operation rounded by itself in the order of the definition
#pragma clang fp contract(off)
    const double Ca = A.legs_a[z], C0a = A.legs_a[A.g.nz + z], ba = A.legs_a[2 * A.g.nz + z];
    const double Cb = A.legs_b[z], C0b = A.legs_b[A.g.nz + z], bb = A.legs_b[2 * A.g.nz + z];
    const double P = A.g.Pzk[(size_t)z * A.g.nk + id], f = A.f[z];
    const size_t plane = (size_t)A.g.nz * A.n * A.nmu;
    const size_t o = ((size_t)z * A.n + s) * A.nmu + q0;
    const double damp = ONEH ? A.damp[s] : 0.0;
#pragma unroll
    for (int q = 0; q < RSD_MU; ++q) {
        if (q < nq) {
            const double ib = A.same ? Ia[q] : Ib[q], vb = A.same ? Va[q] : Vb[q];
            const double Ja = (Ia[q] + ba) - Ca, Ka = (Va[q] + 1.0) - C0a;
            const double Jb = (ib + bb) - Cb, Kb = (vb + 1.0) - C0b;
            const double fm = f * mu2[q];
            const double ta = Ja + fm * Ka, tb = Jb + fm * Kb;
            const double p2 = P * ta * tb;
            if (ONEH) {
                A.out[o + q] = damp * s1[q];
                A.out[plane + o + q] = p2;
                if (A.parts) {
                    A.parts[o + q] = Ia[q];
                    A.parts[plane + o + q] = Va[q];
                    A.parts[2 * plane + o + q] = ib;
                    A.parts[3 * plane + o + q] = vb;
                }
            } else {
                A.w2h[o + q] = p2;
            }
        }
    }
    }
}

// Q_n += wn v M_n(t), n = 0, 1, 2
__device__ __forceinline__ void rsd_moments(double wv, double t, double& Q0, double& Q1, double& Q2) {
    double m0, m1, m2;
    gauss_moments(t, m0, m1, m2);
    Q0 = fma(wv, m0, Q0);
    Q1 = fma(wv, m1, Q1);
    Q2 = fma(wv, m2, Q2);
}

// One-halo multipoles, exact in mu.  grid (blocks of RSD_THREADS samples, nz), the walk of the wedge kernel with three
// accumulators: per bin the products of two species (two HOD names: the two terms of the first name) with their
// moments at t = (h_i + h_j) x^2.  The two mixed products of a pair of legs share a moment when their t are equal.
__global__ __launch_bounds__(RSD_THREADS) void rsd_multipole_kernel(RsdArgs A) {
    __shared__ double cf[RSD_CHUNK * RSD_NCF];
    const int tid = threadIdx.x, s = blockIdx.x * RSD_THREADS + tid, z = blockIdx.y;
    const bool live = s < A.n;
    const int id = live ? A.kidx[s] : 0;
    const double k = A.g.ks[id];
    const bool useA0 = A.a.kind == HMG_TRACER_HOD, useB0 = A.b.kind == HMG_TRACER_HOD;
    const double h00 = A.ha0 + A.hb0, h01 = A.ha0 + A.hb1, h10 = A.ha1 + A.hb0, h11 = A.ha1 + A.hb1;
    const bool mixed_alike = useA0 && useB0 && h01 == h10;
    double Q0 = 0.0, Q1 = 0.0, Q2 = 0.0;
    for (int m0 = 0; m0 < A.g.nm; m0 += RSD_CHUNK) {
        const int mc = min(RSD_CHUNK, A.g.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed
        if (tid < mc) rsd_stage(A, z, m0 + tid, cf + tid * RSD_NCF);
        __syncthreads();
        if (!live) continue;
        const size_t at0 = ((size_t)z * A.g.nm + m0) * (size_t)A.g.nk + id;
        for (int ml = 0; ml < mc; ++ml) {
            const double* c = cf + ml * RSD_NCF;
            double ua0, ua1, ub0, ub1;
            rsd_load(A, at0 + (size_t)ml * A.g.nk, ua0, ua1, ub0, ub1);
            const double wn = c[6];
            const double x = k * c[8], x2 = x * x;
            if (A.hh) {
                rsd_moments(wn * (c[4] * ua0 * ua1), (A.ha0 + A.ha1) * x2, Q0, Q1, Q2);
                rsd_moments(wn * (c[5] * ua1 * ua1), (A.ha1 + A.ha1) * x2, Q0, Q1, Q2);
            } else {
                const double pa0 = c[0] * ua0, pa1 = c[1] * ua1, pb0 = c[2] * ub0, pb1 = c[3] * ub1;
                rsd_moments(wn * (pa1 * pb1), h11 * x2, Q0, Q1, Q2);
                if (mixed_alike) {
                    rsd_moments(wn * fma(pa0, pb1, pa1 * pb0), h01 * x2, Q0, Q1, Q2);
                } else {
                    if (useA0) rsd_moments(wn * (pa0 * pb1), h01 * x2, Q0, Q1, Q2);
                    if (useB0) rsd_moments(wn * (pa1 * pb0), h10 * x2, Q0, Q1, Q2);
                }
                if (useA0 && useB0) rsd_moments(wn * (pa0 * pb0), h00 * x2, Q0, Q1, Q2);
            }
        }
    }
    if (!live) return;
    {   // the epilogue, every operation rounded by itself in the order of the definition
#pragma clang fp contract(off)
    const size_t zn = (size_t)A.g.nz * A.n, o = (size_t)z * A.n + s;
    const double damp = A.damp[s];
    const double p2 = 2.5 * (3.0 * Q1 - Q0);
    const double p4 = 1.125 * ((35.0 * Q2 - 30.0 * Q1) + 3.0 * Q0);
    A.out[3 * o] = damp * Q0;
    A.out[3 * o + 1] = damp * p2;
    A.out[3 * o + 2] = damp * p4;
    if (A.parts) {
        A.parts[o] = Q0;
        A.parts[zn + o] = Q1;
        A.parts[2 * zn + o] = Q2;
    }
    }
}

// Two-halo multipoles: the rule's sum over the nodes of mu, ascending, of the 2-halo wedge with the weights
// (2l + 1) w_q L_l(mu_q) the host tabulated.  One thread per (z, sample).
__global__ __launch_bounds__(256) void rsd_contract_kernel(RsdArgs A) {
    const size_t zn = (size_t)A.g.nz * A.n;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= zn) return;
    const double* w = A.w2h + e * A.nmu;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < A.nmu; ++q) {
        const double v = w[q];
#pragma unroll
        for (int l = 0; l < 3; ++l) acc[l] = fma(A.wl[l * A.nmu + q], v, acc[l]);
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) A.out[3 * (zn + e) + l] = acc[l];
}

// raises *bad (a plain store) if a sample's node is not on the grid; one thread per sample
__global__ __launch_bounds__(256) void rsd_check_kernel(int n, int nk, const int* __restrict__ kidx, int* __restrict__ bad) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    if (kidx[e] < 0 || kidx[e] >= nk) *bad = 1;
}

}  // namespace hmg
