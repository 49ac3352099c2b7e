// The CIB halo model: the luminosities L_c, L_s of every (frequency, z, m) and the contraction of
// an emissivity tracer a_f = L_c[f] + L_s[f] u over the mass axis for every pair of frequencies.  Kernels of the unit
// cib.hip only.
//
// ---- cib_luminosity_kernel: the order of the operations (tests/helpers/cib_model.py follows it line by line) ----------
// Host scalars of the call: norm = 1 / sqrt((2 pi) sigma2), inv2s2 = 1 / (2 sigma2), E0 = expm1(x0), KH = k_B / h in
// GHz / K, FOURPI = 4 pi, INV4PI = 1 / (4 pi).  fp contraction is off: every product and sum below rounds once.
//   per (f, z):   zp1 = 1 + z;   phi = pow(min(zp1, 1 + z_p), delta);   Td = T0 pow(zp1, alpha);   nu0 = (x0 KH) Td;
//                 r = (zp1 nu_f) / nu0;   theta = r < 1 ? pow(r, 3 + beta) (E0 / expm1(x0 r)) : pow(r, -gamma);
//                 A = (L0 phi) theta;     den = (FOURPI zp1) (chi chi)
//   Sigma(M):     d = log10(M) - log10 M_eff;   Sigma = (M norm) exp(-((d d) inv2s2))
//   a source M:   L = A Sigma(M);  it is masked where a cut is given and  L / den > S_cut[f]
//   central:      L_c = M >= M_min and not masked ? L INV4PI : 0
//   satellites:   hw = log(M / M_min);  node g:  x = hw t[g];  ms = M_min exp(x);  q = ms / M;
//                 N = (0.3 pow(q, -0.7)) exp(-(9.9 pow(q, 2.5)));   L = A Sigma(ms);
//                 term = masked ? 0 : (w[g] hw) (N (L INV4PI));     L_s = M > M_min ? sum_g term, g ascending : 0
// N and Sigma(ms) do not depend on the frequency: a node evaluates them once and forms the F terms from them.
// A wavefront owns one (z, m); lane g % 64 evaluates node g, the terms of 64 nodes go through LDS and lane f adds those
// of frequency f in ascending g - one chain per element, so an element depends on its own (f, z, m) only.
//
// ---- emission_power_kernel ---------------------------------------------------------------------------------------------
// A thread owns one column (a node of the k grid) at one redshift and one TILE of frequency pairs: the frequencies come
// in blocks of CIB_T, the tile (bi, bj), bi <= bj, holds the pairs f in block bi, g in block bj.  With w = wm nzm,
// u = u_s[z, m, k], t_f = L_s[f] u, a_f = L_c[f] + t_f and wt_f = w t_f, per mass bin, m ascending:
//     P[f][g] = fma(a_f, wt_g, fma(L_c[g], wt_f, P[f][g]))         (= w (L_c[f] t_g + L_c[g] t_f + t_f t_g), f <= g)
//     I[f]    = fma(a_f, w bh, I[f])                               (diagonal tiles)
//     X[p][f] = fma(a_f, (w c_p) prof_p, X[p][f])                  (diagonal tiles; c = m / rho_m0 or 1)
// Every accumulator is its own chain over m, the frequencies past F hold L_c = L_s = 0 and add exact zeros, and a pair is
// formed the same way in a diagonal and in an off-diagonal tile: an element does not depend on F, on the tile it falls
// in, or on the partners.  f is the frequency that comes first in the caller's list.
// 1-D grid as hodens_power_kernel's: the tiles of one (z, column tile) have consecutive ids on one XCD and find the
// tensor tile the first of them loaded in that XCD's L2.
#pragma once

namespace hmg {

constexpr int CIB_FMAX = HMG_CIB_FMAX;      // frequencies of a call, at most
constexpr int CIB_T = 4;                    // frequencies of a block: a tile holds up to CIB_T x CIB_T pairs
constexpr int CIB_KT = 256;                 // columns of a workgroup, at most
constexpr int CIB_LW = 4;                   // wavefronts (halos) of a workgroup of the luminosity kernel
constexpr int CIB_LS = CIB_FMAX + 1;        // doubles between the terms of two nodes in LDS (odd: no bank conflicts)
constexpr double CIB_KH = 20.836619123327576;         // k_B / h [GHz / K]
constexpr double CIB_FOURPI = 12.566370614359172;
constexpr double CIB_INV4PI = 0.07957747154594767;

struct CibLumArgs {
    int F, nz, nm, nsub;
    const double *nus, *zs, *ms, *chis;     // [F], [nz], [nm], [nz]
    const double *scut;                     // [F] or NULL
    const double *t, *w;                    // [nsub]
    double alpha, T0, beta, gamma, delta, zp, lMeff, Mmin, L0, x0;
    double norm, inv2s2, E0;
    double *Lc, *Ls;                        // [F][nz][nm]
};

__device__ __forceinline__ double cib_sigma(double M, const CibLumArgs& A) {
#pragma clang fp contract(off)
    const double d = log10(M) - A.lMeff;
    return (M * A.norm) * exp(-((d * d) * A.inv2s2));
}

__global__ __launch_bounds__(64 * CIB_LW) void cib_luminosity_kernel(CibLumArgs A) {
#pragma clang fp contract(off)
    __shared__ double sA[CIB_LW][CIB_FMAX], sC[CIB_LW][CIB_FMAX];
    __shared__ double st[CIB_LW][64 * CIB_LS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, F = A.F, nm = A.nm;
    const size_t total = (size_t)A.nz * nm;
    size_t e = (size_t)blockIdx.x * CIB_LW + wv;
    const bool inside = e < total;
    if (!inside) e = total - 1;                 // (a wavefront past the end works on the last halo and writes nothing)
    const int z = (int)(e / nm), m = (int)(e - (size_t)z * nm);
    const double zp1 = 1.0 + A.zs[z], M = A.ms[m], chi = A.chis[z];
    const double den = (CIB_FOURPI * zp1) * (chi * chi);
    const bool cut = A.scut != nullptr;
    if (lane < F) {
        const double phi = pow(fmin(zp1, 1.0 + A.zp), A.delta);
        const double Td = A.T0 * pow(zp1, A.alpha);
        const double nu0 = (A.x0 * CIB_KH) * Td;
        const double r = (zp1 * A.nus[lane]) / nu0;
        const double theta = r < 1.0 ? pow(r, 3.0 + A.beta) * (A.E0 / expm1(A.x0 * r)) : pow(r, -A.gamma);
        sA[wv][lane] = (A.L0 * phi) * theta;
        sC[wv][lane] = cut ? A.scut[lane] : 0.0;
    }
    __syncthreads();
    double lc = 0.0;
    if (lane < F && M >= A.Mmin) {
        const double L = sA[wv][lane] * cib_sigma(M, A);
        lc = (cut && L / den > sC[wv][lane]) ? 0.0 : L * CIB_INV4PI;
    }
    const double hw = log(M / A.Mmin);
    double acc = 0.0;
    for (int g0 = 0; g0 < A.nsub; g0 += 64) {
        const int g = g0 + lane;
        if (g < A.nsub) {
            const double x = hw * A.t[g];
            const double ms = A.Mmin * exp(x);
            const double q = ms / M;
            const double N = (0.3 * pow(q, -0.7)) * exp(-(9.9 * pow(q, 2.5)));
            const double sg = cib_sigma(ms, A);
            const double wg = A.w[g] * hw;
            double* o = &st[wv][lane * CIB_LS];
            for (int f = 0; f < F; ++f) {
                const double L = sA[wv][f] * sg;
                const bool masked = cut && L / den > sC[wv][f];
                o[f] = masked ? 0.0 : wg * (N * (L * CIB_INV4PI));
            }
        }
        __syncthreads();
        const int cnt = A.nsub - g0 < 64 ? A.nsub - g0 : 64;
        if (lane < F)
            for (int j = 0; j < cnt; ++j) acc += st[wv][j * CIB_LS + lane];
        __syncthreads();
    }
    if (inside && lane < F) {
        const size_t o = ((size_t)lane * A.nz + z) * nm + m;
        A.Lc[o] = lc;
        A.Ls[o] = M > A.Mmin ? acc : 0.0;
    }
}

// coef[nz][nm][Fpad][2] = (L_c, L_s), zeros in the frequencies F .. Fpad-1; side[nz][nm][4] = (w, w bh, w c_0, w c_1)
// with w = wm nzm and c_p = m / rho_m0 (matter), 1 (pressure) or 0 (no such partner).  One thread per (z, m).
struct EmissionPrepArgs {
    int F, Fpad, nz, nm, NP, kind[2];
    const double *Lc, *Ls, *nzm, *bh, *ms, *wm;
    double rho_m0;
    double *coef, *side;
};

__global__ __launch_bounds__(256) void emission_prep_kernel(EmissionPrepArgs A) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t plane = (size_t)A.nz * A.nm;
    if (e >= plane) return;
    const int m = (int)(e % A.nm);
    double* c = A.coef + e * A.Fpad * 2;
    for (int f = 0; f < A.Fpad; ++f) {
        c[2 * f] = f < A.F ? A.Lc[f * plane + e] : 0.0;
        c[2 * f + 1] = f < A.F ? A.Ls[f * plane + e] : 0.0;
    }
    const double w = A.wm[m] * A.nzm[e], r = A.ms[m] / A.rho_m0;
    double* s = A.side + 4 * e;
    s[0] = w;
    s[1] = w * A.bh[e];
    for (int p = 0; p < 2; ++p) s[2 + p] = p >= A.NP ? 0.0 : (A.kind[p] == HMG_TRACER_MATTER ? w * r : w);
}

// raises *bad (a plain store) if a column's node is off the k grid
__global__ __launch_bounds__(256) void emission_check_kernel(int n, int nk, const int* __restrict__ kidx, int* __restrict__ bad) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && (kidx[e] < 0 || kidx[e] >= nk)) *bad = 1;
}

struct EmissionArgs {
    int F, Fpad, nb, nz, nm, nk, n;
    int ngroups, ntiles;            // (z, column tile) groups; pair tiles = nb (nb + 1) / 2
    const double* us;               // [nz][nm][nk]
    const double* prof[2];          // the partners' tensors
    const double *coef, *side;
    const double* damp;             // [n]
    const int* kidx;                // [n] or NULL: column = node
    double *P1h, *I, *X1h;          // [npair][nz][n], [F][nz][n], [NP][F][nz][n]
};

// The coefficients and the side data of a mass bin have wave-uniform addresses and are read through the constant address
// space, so that every tile loads them through the scalar cache.  That address space promises that nothing writes the
// memory while this kernel runs, and it rests on one more fact: a kernel starts with its scalar cache invalidated, so
// a launch never sees lines an earlier launch left there.  Both hold here.  The two arrays are written by
// emission_prep_kernel only, a launch of its own on the same stream before this one, and the contraction writes its
// outputs only.  The block they live in (with_block) is reused from call to call, so another call's prepass may have
// written other values at the same addresses: it is the invalidation at every kernel's start, not the addresses being
// fresh, that makes the scalar loads see this call's values.
typedef const __attribute__((address_space(4))) double* cib_cptr;

template <int NP, bool DIAG>
__device__ __forceinline__ void emission_tile(const EmissionArgs& A, int z, int k, int col, bool live, int bi, int bj) {
#pragma clang fp contract(off)
    const int nm = A.nm;
    const size_t cstride = (size_t)A.Fpad * 2, row = (size_t)z * nm;
    const double* __restrict__ cfi = A.coef + row * cstride + (size_t)bi * CIB_T * 2;
    const double* __restrict__ cfj = A.coef + row * cstride + (size_t)bj * CIB_T * 2;
    const double* __restrict__ sd = A.side + row * 4;
    const double* __restrict__ pu = A.us + row * A.nk + k;
    const double* pp[2] = {NP > 0 ? A.prof[0] + row * A.nk + k : nullptr, NP > 1 ? A.prof[1] + row * A.nk + k : nullptr};
    const bool alias[2] = {NP > 0 && A.prof[0] == A.us, NP > 1 && A.prof[1] == A.us};       // (the tensor is loaded once)
    double P[CIB_T][CIB_T], I[CIB_T], X[2][CIB_T];
#pragma unroll
    for (int i = 0; i < CIB_T; ++i) {
        I[i] = X[0][i] = X[1][i] = 0.0;
#pragma unroll
        for (int g = 0; g < CIB_T; ++g) P[i][g] = 0.0;
    }
#pragma unroll 2
    for (int m = 0; m < nm; ++m) {
        const double u = pu[(size_t)m * A.nk];
        const cib_cptr q = (cib_cptr)(sd + 4 * (size_t)m);
        const cib_cptr ci = (cib_cptr)(cfi + (size_t)m * cstride);
        const cib_cptr cj = DIAG ? ci : (cib_cptr)(cfj + (size_t)m * cstride);
        const double w = q[0];
        double a[CIB_T], wti[CIB_T], wtj[CIB_T];
#pragma unroll
        for (int i = 0; i < CIB_T; ++i) {
            const double t = ci[2 * i + 1] * u;
            a[i] = ci[2 * i] + t;
            wti[i] = w * t;
            wtj[i] = DIAG ? wti[i] : w * (cj[2 * i + 1] * u);
        }
#pragma unroll
        for (int i = 0; i < CIB_T; ++i)
#pragma unroll
            for (int g = DIAG ? i : 0; g < CIB_T; ++g) P[i][g] = fma(a[i], wtj[g], fma(cj[2 * g], wti[i], P[i][g]));
        if (DIAG) {
            const double wb = q[1];
#pragma unroll
            for (int i = 0; i < CIB_T; ++i) I[i] = fma(a[i], wb, I[i]);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const double xp = q[2 + p] * (alias[p] ? u : pp[p][(size_t)m * A.nk]);
#pragma unroll
                for (int i = 0; i < CIB_T; ++i) X[p][i] = fma(a[i], xp, X[p][i]);
            }
        }
    }
    if (!live) return;
    const double D = A.damp[col];
    const size_t zc = (size_t)z * A.n + col, plane = (size_t)A.nz * A.n;
#pragma unroll
    for (int i = 0; i < CIB_T; ++i) {
        const int f = bi * CIB_T + i;
        if (f >= A.F) continue;
#pragma unroll
        for (int g = DIAG ? i : 0; g < CIB_T; ++g) {
            const int h = bj * CIB_T + g;
            if (h >= A.F) continue;
            const size_t pair = (size_t)f * A.F - (size_t)f * (f - 1) / 2 + (size_t)(h - f);
            A.P1h[pair * plane + zc] = D * P[i][g];
        }
        if (DIAG) {
            A.I[(size_t)f * plane + zc] = I[i];
#pragma unroll
            for (int p = 0; p < NP; ++p) A.X1h[((size_t)p * A.F + f) * plane + zc] = D * X[p][i];
        }
    }
}

template <int NP>
__global__ __launch_bounds__(CIB_KT) void emission_power_kernel(EmissionArgs A) {
    const int L = blockIdx.x, j = L >> 3;
    const int grp = (j / A.ntiles) * 8 + (L & 7);
    if (grp >= A.ngroups) return;
    int t = j % A.ntiles, bi = 0;
    while (t >= A.nb - bi) { t -= A.nb - bi; ++bi; }     // tile -> (bi, bj), bi <= bj, the diagonal tile of a block first
    const int bj = bi + t;
    const int nkt = (A.n + (int)blockDim.x - 1) / (int)blockDim.x;
    const int z = grp / nkt, kt = grp - z * nkt;
    const int col = kt * (int)blockDim.x + (int)threadIdx.x;
    const bool live = col < A.n;
    const int k = live ? (A.kidx ? A.kidx[col] : col) : 0;          // (a column past the end reads node 0)
    if (bi == bj) emission_tile<NP, true>(A, z, k, col, live, bi, bj);
    else emission_tile<0, false>(A, z, k, col, live, bi, bj);
}

}  // namespace hmg
