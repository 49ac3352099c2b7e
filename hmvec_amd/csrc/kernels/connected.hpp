// The 2-, 3- and 4-halo terms of the trispectrum of two spectra: the angle-averaged
// perturbation-theory matrices Pbar, Bbar, Tbar (pt_average_kernel) and the mixed three- and two-leg mass contraction with
// two free sample indices and its epilogue (connected_kernel).  Included by connected.hip alone (its own translation
// unit).  The forms of a leg's weight and of a spectrum's square term are kernels/leg_form.hpp and
// kernels/square_term.hpp; the leg prepass that leaves J, P, D and the z sum are sampled.hip's; the 1-halo term is
// trispectrum.hip's.
#pragma once
#include "../fastmath.hpp"
#include "leg_form.hpp"
#include "square_term.hpp"

namespace hmg {

constexpr int CON_MAXN = 256;       // samples per redshift
constexpr int CON_MAXR = 256;       // nodes of the angle rule
constexpr int CON_TILE = 32;        // samples per tile side
constexpr int CON_CHUNK = 16;       // mass bins staged through LDS at a time
constexpr int CON_THREADS = 256;    // 16 x 16 threads, a 2 x 2 register block each
constexpr int CON_NA = 5;           // staged arrays per side
constexpr int PT_THREADS = 256;
constexpr int PT_MAXNK = 8192;      // 2 nk + 4 nr doubles of dynamic LDS: 139,264 B of the CU's 160 KB at the limits

// ---------------------------------------------------------------------------------------------- perturbation theory
struct PtArgs {
    int nz, nk, n, nr;
    const double *ks, *Pzk;         // [nk], [nz][nk]
    const int* idx;                 // [nz][n]
    const double* frac;
    const double *mu, *omm, *opm, *w;   // [nr] the rule: mu, 1 - mu, 1 + mu, weights
    double *Pbar, *Bbar, *Tbar;     // [nz][n][n]
};

// F2(p, q; r) of section 16 (bis_F2 of kernels/bispectrum.hpp restated: that header holds its unit's kernels): the
// numerator of mu factored, the longer of (p, q) first.
__device__ __forceinline__ double con_F2(double p, double q, double r) {
    const double a = fmax(p, q), b = fmin(p, q);
    double mu = fma(-b, b, (r - a) * (r + a)) / (2.0 * a * b);
    mu = fmin(1.0, fmax(-1.0, mu));
    const double s = a / b + b / a;
    return fma(2.0 / 7.0 * mu, mu, fma(0.5 * mu, s, 5.0 / 7.0));
}

// plin_at: linear in (ln k, ln P) on the row's grid, continued beyond either end with the end panel's slope.  The panel
// is the last one whose left node is <= ln q (binary search), clamped to 0 .. nk - 2.
__device__ __forceinline__ double con_plin(const double* lnk, const double* lnP, int nk, double q) {
    const double lq = log_fast(q);
    int lo = 0, hi = nk - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (lnk[mid] <= lq) lo = mid; else hi = mid - 1;
    }
    const double x0 = lnk[lo], y0 = lnP[lo];
    const double t = (lq - x0) / (lnk[lo + 1] - x0);
    return exp_fast<true>(fma(t, lnP[lo + 1] - y0, y0));
}

// F3s(k, -k, k') from the recursion for F_n, G_n, symmetrised, the orderings whose partial sum k - k vanishes dropped:
//   54 F3s = 7 r mu F2(-k,k') + G2(-k,k') (k'/q-^2) [7 (k' - k mu) + 2 r (k' mu - k)]
//          - 7 r mu F2(k,k')  + G2(k,k')  (k'/q+^2) [7 (k' + k mu) - 2 r (k + k' mu)],      r = k'/k,
// mu the cosine between k and k', q-+ = |k' -+ k|.  The brackets are formed from k' - k and 1 -+ mu, not from mu.
__device__ __forceinline__ double con_F3s(double k, double kp, double mu, double omm, double opm, double qm2, double qp2) {
    const double s = k / kp + kp / k, h = 0.5 * mu * s, m2 = mu * mu;
    const double e2 = fma(2.0 / 7.0, m2, 5.0 / 7.0), g2 = fma(4.0 / 7.0, m2, 3.0 / 7.0);
    const double F2m = e2 - h, F2p = e2 + h, G2m = g2 - h, G2p = g2 + h;
    const double dk = kp - k, r = kp / k, a = 7.0 * r * mu;
    const double Am = fma(7.0, fma(k, omm, dk), 2.0 * r * (dk - kp * omm));
    const double Ap = fma(7.0, fma(k, opm, dk), -2.0 * r * fma(kp, opm, -dk));
    const double tm = fma(G2m * (kp / qm2), Am, a * F2m);
    const double tp = fma(G2p * (kp / qp2), Ap, -(a * F2p));
    return (tm + tp) * (1.0 / 54.0);
}

// grid (blocks of PT_THREADS pairs, nz), dynamic LDS (2 nk + 4 nr) doubles.  One thread per (z, i <= j): it orders the
// two sides by (k, P), so a result does not depend on where its samples stand in the table, walks the rule in node
// order and mirrors its three results.
__global__ __launch_bounds__(PT_THREADS) void pt_average_kernel(PtArgs A) {
    extern __shared__ double pt_lds[];
    double* lnk = pt_lds;
    double* lnP = lnk + A.nk;
    double* rmu = lnP + A.nk;
    double* romm = rmu + A.nr;
    double* ropm = romm + A.nr;
    double* rw = ropm + A.nr;
    const int z = blockIdx.y, n = A.n;
    for (int t = threadIdx.x; t < A.nk; t += PT_THREADS) {
        lnk[t] = log_fast(A.ks[t]);
        lnP[t] = log_fast(A.Pzk[(size_t)z * A.nk + t]);
    }
    for (int t = threadIdx.x; t < A.nr; t += PT_THREADS) {
        rmu[t] = A.mu[t]; romm[t] = A.omm[t]; ropm[t] = A.opm[t]; rw[t] = A.w[t];
    }
    __syncthreads();
    const int p = blockIdx.x * PT_THREADS + threadIdx.x;
    if (p >= n * (n + 1) / 2) return;
    int j = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
    while ((j + 1) * (j + 2) / 2 <= p) ++j;
    while (j * (j + 1) / 2 > p) --j;
    const int i = p - j * (j + 1) / 2;
    const double* P = A.Pzk + (size_t)z * A.nk;
    double k1, k2, P1, P2;
    {
        const size_t o = (size_t)z * n + i;
        const int id = A.idx[o];
        const double f = A.frac[o];
        k1 = bis_sample_k(A.ks, id, f);
        P1 = P[id];
        if (f != 0.0) P1 = fma(f, P[id + 1], (1.0 - f) * P1);
    }
    {
        const size_t o = (size_t)z * n + j;
        const int id = A.idx[o];
        const double f = A.frac[o];
        k2 = bis_sample_k(A.ks, id, f);
        P2 = P[id];
        if (f != 0.0) P2 = fma(f, P[id + 1], (1.0 - f) * P2);
    }
    const bool first = k1 > k2 || (k1 == k2 && P1 >= P2);
    const double ka = first ? k1 : k2, kb = first ? k2 : k1, Pa = first ? P1 : P2, Pb = first ? P2 : P1;
    const double d = ka - kb, d2 = d * d, c2 = 2.0 * ka * kb;
    const double PaPb = Pa * Pb, Fab_scale = 12.0 * Pa * PaPb, Fba_scale = 12.0 * Pb * PaPb;
    double pbar = 0.0, bbar = 0.0, tbar = 0.0;
    for (int t = 0; t < A.nr; ++t) {
        const double mu = rmu[t], omm = romm[t], opm = ropm[t], w = rw[t];
        const double qm2 = fma(c2, omm, d2), qp2 = fma(c2, opm, d2);
        const double qm = sqrt(qm2), qp = sqrt(qp2);
        const double Pm = con_plin(lnk, lnP, A.nk, qm), Pp = con_plin(lnk, lnP, A.nk, qp);
        const double f1p = con_F2(qp, kb, ka), f2p = con_F2(qp, ka, kb);
        const double f1m = con_F2(qm, kb, ka), f2m = con_F2(qm, ka, kb);
        const double up = fma(f1p, Pb, f2p * Pa), um = fma(f1m, Pb, f2m * Pa);
        const double B = 2.0 * fma(con_F2(ka, kb, qp), PaPb, Pp * up);
        const double F3 = fma(con_F3s(ka, kb, mu, omm, opm, qm2, qp2), Fab_scale,
                              con_F3s(kb, ka, mu, omm, opm, qm2, qp2) * Fba_scale);
        const double T = fma(4.0 * Pp * up, up, fma(4.0 * Pm * um, um, F3));
        pbar = fma(w, Pp, pbar);
        bbar = fma(w, B, bbar);
        tbar = fma(w, T, tbar);
    }
    const size_t e = ((size_t)z * n + i) * n + j, m = ((size_t)z * n + j) * n + i;
    A.Pbar[e] = pbar; A.Bbar[e] = bbar; A.Tbar[e] = tbar;
    A.Pbar[m] = pbar; A.Bbar[m] = bbar; A.Tbar[m] = tbar;
}

// ---------------------------------------------------------------------------------------------- the mass contraction
struct ConArgs {
    BisLeg la, lb, lc, ld;          // the legs a, b (at sample i) and c, d (at sample j)
    TriSide ab, cd;                 // the square terms of the two spectra
    BisLeg h;                       // the request's one HOD (prof = u_s, cprof = u_c or NULL); read where a flag is set
    const double *NcNs, *NsNsm1;    // its second moments [nz][nm]
    int hod_ac, hod_ad, hod_bc, hod_bd;   // the pair (x, y) is twice that HOD: the two-wavenumber pair term
    HaloGrid g;
    SampleTable s;
    const double *Ja, *Jb, *Jc, *Jd;      // [nz][n] the brackets of the prepass
    const double *Ps, *Ds;                // [nz][n] sampled P_lin, damping factor
    const double *Pbar, *Bbar, *Tbar;     // [nz][n][n]
    double* T;                      // [5][nz][n][n]; plane 0 (the 1-halo term) is not written here
};

__device__ __forceinline__ double con_interp(const double* p, size_t at, double f) {
    double v = p[at];
    if (f != 0.0) v = fma(f, p[at + 1], (1.0 - f) * v);
    return v;
}

// Stage one side of the chunk: dst[(arr CON_CHUNK + ml) CON_TILE + il], arr 0, 1 the two legs' weights, 2 the square
// term of their spectrum, 3, 4 the HOD's profiles - (u_c, u_s) on the i side, (cN u_s, cN u_c + cS u_s) on the j side, so
// that the pair term is u_c(i) [cN u_s(j)] + u_s(i) [cN u_c(j) + cS u_s(j)].  A thread's sample il = tid % 32 is the
// same for all of its elements.
template <bool JSIDE>
__device__ __forceinline__ void con_stage(const ConArgs& A, const BisLeg& L1, const BisLeg& L2, const TriSide& S,
                                          const double* cf1, const double* cf2, const double* cfS, const double* sCN,
                                          const double* sCS, double* dst, bool anyhod, int z, int m0, int mc, bool live,
                                          int id, double f) {
    const int il = threadIdx.x & (CON_TILE - 1), grp = threadIdx.x / CON_TILE;
    for (int ml = grp; ml < mc; ml += CON_THREADS / CON_TILE) {
        double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
        if (live) {
            const size_t at = ((size_t)z * A.g.nm + (m0 + ml)) * (size_t)A.g.nk + id;
            v0 = bis_leg_at(L1, cf1 + 3 * ml, at, f);
            v1 = bis_leg_at(L2, cf2 + 3 * ml, at, f);
            const double* x1 = cfS + ml * (2 * TRI_NC);
            const double* x2 = x1 + TRI_NC;
            v2 = tri_square_at(S, x1, x2, at);
            if (f != 0.0) v2 = fma(f, tri_square_at(S, x1, x2, at + 1), (1.0 - f) * v2);
            if (anyhod) {
                const double us = con_interp(A.h.prof, at, f);
                const double uc = A.h.cprof ? con_interp(A.h.cprof, at, f) : 1.0;
                if (JSIDE) { v3 = sCN[ml] * us; v4 = fma(sCN[ml], uc, sCS[ml] * us); }
                else { v3 = uc; v4 = us; }
            }
        }
        dst[(0 * CON_CHUNK + ml) * CON_TILE + il] = v0;
        dst[(1 * CON_CHUNK + ml) * CON_TILE + il] = v1;
        dst[(2 * CON_CHUNK + ml) * CON_TILE + il] = v2;
        dst[(3 * CON_CHUNK + ml) * CON_TILE + il] = v3;
        dst[(4 * CON_CHUNK + ml) * CON_TILE + il] = v4;
    }
}

// grid (tiles of j, tiles of i, nz), CON_THREADS threads, a 2 x 2 register block per thread: eight bias-weighted sums per
// element, 32 fp64 accumulators per thread.  A workgroup walks the whole mass axis itself, in order, in chunks staged
// through LDS: no split over workgroups, no atomics - an element depends on its own (z, i, j), the tables and the tensors
// alone.  The weight wm nzm bh multiplies the product of the two sides; scales and damping multiply finished sums.
__global__ __launch_bounds__(CON_THREADS) void connected_kernel(ConArgs A) {
    __shared__ __align__(16) double sI[CON_NA * CON_CHUNK * CON_TILE], sJ[CON_NA * CON_CHUNK * CON_TILE];
    __shared__ double cfL[4 * CON_CHUNK * 3], cfS[2 * CON_CHUNK * 2 * TRI_NC];
    __shared__ double sWb[CON_CHUNK], sCN[CON_CHUNK], sCS[CON_CHUNK];
    const int tid = threadIdx.x;
    const int z = blockIdx.z, i0 = blockIdx.y * CON_TILE, j0 = blockIdx.x * CON_TILE;
    const int tx = tid & 15, ty = tid >> 4;
    const int n = A.s.n;
    const int il = tid & (CON_TILE - 1);
    const bool liveI = i0 + il < n, liveJ = j0 + il < n;
    int idI = 0, idJ = 0;
    double fI = 0.0, fJ = 0.0;
    if (liveI) { const size_t o = (size_t)z * n + i0 + il; idI = A.s.idx[o]; fI = A.s.frac[o]; }
    if (liveJ) { const size_t o = (size_t)z * n + j0 + il; idJ = A.s.idx[o]; fJ = A.s.frac[o]; }
    const bool anyhod = A.hod_ac || A.hod_ad || A.hod_bc || A.hod_bd;

    double acc[8][2][2];
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[q][r][0] = acc[q][r][1] = 0.0;

    for (int m0 = 0; m0 < A.g.nm; m0 += CON_CHUNK) {
        const int mc = min(CON_CHUNK, A.g.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed
        if (tid < 6 * CON_CHUNK) {             // the coefficient rows of the chunk: one thread per (form, m)
            const int ml = tid & (CON_CHUNK - 1), which = tid / CON_CHUNK;
            if (ml < mc) {
                const size_t zm = (size_t)z * A.g.nm + m0 + ml;
                const double mass = A.g.ms[m0 + ml];
                double lowk, ngals;
                double* cl = cfL + (which * CON_CHUNK + ml) * 3;
                if (which == 0) bis_leg_form(A.la, zm, z, mass, A.g.rho_m0, cl, lowk, ngals);
                else if (which == 1) bis_leg_form(A.lb, zm, z, mass, A.g.rho_m0, cl, lowk, ngals);
                else if (which == 2) bis_leg_form(A.lc, zm, z, mass, A.g.rho_m0, cl, lowk, ngals);
                else if (which == 3) bis_leg_form(A.ld, zm, z, mass, A.g.rho_m0, cl, lowk, ngals);
                else if (which == 4) {
                    double* x = cfS + ml * (2 * TRI_NC);
                    tri_square_forms(A.ab, zm, z, mass, A.g.rho_m0, x, x + TRI_NC);
                    sWb[ml] = A.g.wm[m0 + ml] * A.g.nzm[zm] * A.g.bh[zm];
                } else {
                    double* x = cfS + (CON_CHUNK + ml) * (2 * TRI_NC);
                    tri_square_forms(A.cd, zm, z, mass, A.g.rho_m0, x, x + TRI_NC);
                    double cn = 0.0, cs = 0.0;
                    if (anyhod) {
                        const double ng = A.h.ngal[z], ng2 = ng * ng;
                        cn = A.NcNs[zm] / ng2;
                        cs = A.NsNsm1[zm] / ng2;
                    }
                    sCN[ml] = cn;
                    sCS[ml] = cs;
                }
            }
        }
        __syncthreads();
        con_stage<false>(A, A.la, A.lb, A.ab, cfL, cfL + CON_CHUNK * 3, cfS, sCN, sCS, sI, anyhod, z, m0, mc, liveI, idI, fI);
        con_stage<true>(A, A.lc, A.ld, A.cd, cfL + 2 * CON_CHUNK * 3, cfL + 3 * CON_CHUNK * 3,
                        cfS + CON_CHUNK * 2 * TRI_NC, sCN, sCS, sJ, anyhod, z, m0, mc, liveJ, idJ, fJ);
        __syncthreads();
#pragma unroll 2
        for (int ml = 0; ml < mc; ++ml) {
            const double wb = sWb[ml];
            double2 vi[CON_NA], vj[CON_NA];
#pragma unroll
            for (int a = 0; a < CON_NA; ++a) {
                vi[a] = *reinterpret_cast<const double2*>(&sI[(a * CON_CHUNK + ml) * CON_TILE + ty * 2]);
                vj[a] = *reinterpret_cast<const double2*>(&sJ[(a * CON_CHUNK + ml) * CON_TILE + tx * 2]);
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const double wa = r ? vi[0].y : vi[0].x, wbl = r ? vi[1].y : vi[1].x, Sab = r ? vi[2].y : vi[2].x;
                const double uci = r ? vi[3].y : vi[3].x, usi = r ? vi[4].y : vi[4].x;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const double wc = c ? vj[0].y : vj[0].x, wd = c ? vj[1].y : vj[1].x, Scd = c ? vj[2].y : vj[2].x;
                    const double usn = c ? vj[3].y : vj[3].x, mix = c ? vj[4].y : vj[4].x;
                    const double pair = fma(uci, usn, usi * mix);
                    acc[0][r][c] = fma(wa * Scd, wb, acc[0][r][c]);
                    acc[1][r][c] = fma(wbl * Scd, wb, acc[1][r][c]);
                    acc[2][r][c] = fma(wc * Sab, wb, acc[2][r][c]);
                    acc[3][r][c] = fma(wd * Sab, wb, acc[3][r][c]);
                    acc[4][r][c] = fma(A.hod_ac ? pair : wa * wc, wb, acc[4][r][c]);
                    acc[5][r][c] = fma(A.hod_ad ? pair : wa * wd, wb, acc[5][r][c]);
                    acc[6][r][c] = fma(A.hod_bc ? pair : wbl * wc, wb, acc[6][r][c]);
                    acc[7][r][c] = fma(A.hod_bd ? pair : wbl * wd, wb, acc[7][r][c]);
                }
            }
        }
    }

    const size_t zn = (size_t)z * n, plane = (size_t)A.g.nz * n * n;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = i0 + ty * 2 + r;
        if (i >= n) continue;
        const double Ja = A.Ja[zn + i], Jb = A.Jb[zn + i], Pi = A.Ps[zn + i], Di = A.Ds[zn + i], sci = A.s.scale[zn + i];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int j = j0 + tx * 2 + c;
            if (j >= n) continue;
            const double Jc = A.Jc[zn + j], Jd = A.Jd[zn + j], Pj = A.Ps[zn + j], Dj = A.Ds[zn + j];
            const double sig = sci * A.s.scale[zn + j], DD = Di * Dj;
            const size_t e = (zn + i) * n + j;
            const double Iacd = acc[0][r][c], Ibcd = acc[1][r][c], Icab = acc[2][r][c], Idab = acc[3][r][c];
            const double Iac = acc[4][r][c], Iad = acc[5][r][c], Ibc = acc[6][r][c], Ibd = acc[7][r][c];
            const double t13 = fma(Pi, fma(Ja, Ibcd, Jb * Iacd), Pj * fma(Jc, Idab, Jd * Icab));
            const double t22 = A.Pbar[e] * fma(Iac, Ibd, Iad * Ibc);
            const double t3 = A.Bbar[e] * fma(Iac, Jb * Jd, fma(Ibd, Ja * Jc, fma(Iad, Jb * Jc, Ibc * (Ja * Jd))));
            const double t4 = A.Tbar[e] * ((Ja * Jb) * (Jc * Jd));
            A.T[plane + e] = sig * (DD * t13);
            A.T[2 * plane + e] = sig * ((DD * DD) * t22);
            A.T[3 * plane + e] = sig * (DD * t3);
            A.T[4 * plane + e] = sig * t4;
        }
    }
}

}  // namespace hmg
