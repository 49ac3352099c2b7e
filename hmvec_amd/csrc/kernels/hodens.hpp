// HOD parameter ensembles: P_gg and P_gm of S parameter sets against one mass function and one pair of profile tensors
// (DESIGN.md section 21).  Kernels of the unit hodens.hip only.  Needs rowdev.hpp (wave_sum) before it.
//
// Coefficient block, written by hodens_occ_kernel and read by hodens_power_kernel (doubles):
//     coef[nz][nm][Spad][4] = (Nc, Ns, 2 NcNs, NsNsm1)   Spad = S rounded up to HE_TS; the sets S .. Spad-1 hold zeros
//     craw[S][nz]           = sum_m (wm nzm bh) (Nc + Ns)  in the tile order of hod_sums_row (C = craw / ngal)
// The occupations are stored raw: every 1/ngal is applied to the finished sums in the epilogue of the contraction.
#pragma once
#include "hod_occ.hpp"
#include "leg_form.hpp"

namespace hmg {

constexpr int HE_TS = 8;            // sets of a thread of the contraction: 24 accumulators
constexpr int HE_TS_SHORT = 2;      // ... where the columns do not fill one workgroup
constexpr int HE_KT = 256;          // columns of a workgroup, at most
constexpr int HE_OCC_THREADS = 256;

static inline size_t hodens_spad(int S) { return ((size_t)S + HE_TS - 1) / HE_TS * HE_TS; }

struct HodEnsArgs {
    int S, Spad, nz, nm, corr;
    const double *par, *lthr;       // [S][6], [S][nz]
    const double *zs, *ms, *nzm, *bh, *wm;
    const double* lms;              // [nz][nm] the SHMR inversion, shared by the sets
    double *ngal, *bg;              // [S][nz]
    double *occ;                    // [4][S][nz][nm] = (Nc, Ns, NsNsm1, NcNs) or NULL
    double *coef, *craw;            // the coefficient block or NULL
};

// log10 M*(z, m) of every point once: the part of hod_occ_point that does not depend on the HOD parameters.
__global__ __launch_bounds__(256) void hodens_lmstar_kernel(int nz, int nm, const double* __restrict__ zs,
                                                            const double* __restrict__ ms, double* __restrict__ lms) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)nz * nm) return;
    const int z = (int)(e / nm), m = (int)(e - (size_t)z * nm);
    const double zz = zs[z], a = 1.0 / (1.0 + zz);
    const ShmrSet S = shmr_for(zz);
    const double lmh = log10(ms[m]);
    lms[e] = shmr_inverse_direct(lmh, a, S);
}

// Occupations and sums of one (set, z) per workgroup: grid (S or Spad, nz).  The operations of a point are those of
// hod_occ_point with log10 M* read instead of inverted; the sums are those of hod_sums_row - wavefront sums over 64-mass
// tiles, then the tiles in order - from the values in registers, so nothing of size S nz nm has to exist.
__global__ __launch_bounds__(HE_OCC_THREADS) void hodens_occ_kernel(HodEnsArgs A) {
#pragma clang fp contract(off)
    __shared__ double part[3 * HOD_MAX_TILES];
    const int s = blockIdx.x, z = blockIdx.y, nm = A.nm;
    if (s >= A.S) {                 // a padding set of the coefficient block
        for (int m = threadIdx.x; m < nm; m += blockDim.x) {
            double* c = A.coef + (((size_t)z * nm + m) * A.Spad + s) * 4;
            c[0] = c[1] = c[2] = c[3] = 0.0;
        }
        return;
    }
    const double* p = A.par + 6 * (size_t)s;
    const HodDev P{p[0], p[1], p[2], p[3], p[4], p[5], A.corr};
    const double zz = A.zs[z], a = 1.0 / (1.0 + zz);
    const ShmrSet S = shmr_for(zz);
    const double thr = A.lthr[(size_t)s * A.nz + z];
    const double mthr_halo = shmr_log10mh(thr, a, S);
    const double Msat = 1.0e12 * P.Bsat * pow10_fast((mthr_halo - 12.0) * P.betasat);
    const double Mcut = 1.0e12 * P.Bcut * pow10_fast((mthr_halo - 12.0) * P.betacut);
    const double denom = sqrt(2.0) * P.sig;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int ntile = (nm + 63) / 64;
    const size_t plane = (size_t)A.S * A.nz * nm;
    for (int tile = w; tile < ntile; tile += nw) {
        const int m = tile * 64 + lane;
        double t = 0.0, tb = 0.0, tc = 0.0;
        if (m < nm) {
            const size_t idx = (size_t)z * nm + m;
            const double lmh = log10(A.ms[m]);
            const double lmstar = A.lms[idx];
            const double nc = 0.5 * (1.0 - erf((thr - lmstar) / denom));
            const double mass = pow10_fast(lmh);
            const double ns = nc * powr_fast(mass / Msat, P.alphasat) * exp(-Mcut / mass);
            double nn, cn;
            if (P.corr == 0) {
                nn = (fabs(nc) <= 1.0e-8) ? 0.0 : (ns * ns) / nc;   // np.isclose(Nc, 0)
                cn = ns;
            } else {
                nn = ns * ns;
                cn = ns * nc;
            }
            if (A.occ) {
                const size_t o = ((size_t)s * A.nz + z) * nm + m;
                A.occ[o] = nc; A.occ[plane + o] = ns; A.occ[2 * plane + o] = nn; A.occ[3 * plane + o] = cn;
            }
            if (A.coef) {
                double* c = A.coef + (idx * A.Spad + s) * 4;
                c[0] = nc; c[1] = ns; c[2] = 2.0 * cn; c[3] = nn;
            }
            t = A.wm[m] * (A.nzm[idx] * (nc + ns));
            tb = t * A.bh[idx];
            tc = ((A.wm[m] * A.nzm[idx]) * A.bh[idx]) * (nc + ns);
        }
        const double tn = wave_sum(t), tbs = wave_sum(tb), tcs = wave_sum(tc);
        if (lane == 0) { part[3 * tile] = tn; part[3 * tile + 1] = tbs; part[3 * tile + 2] = tcs; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sn = 0.0, sb = 0.0, sc = 0.0;
        for (int tile = 0; tile < ntile; ++tile) { sn += part[3 * tile]; sb += part[3 * tile + 1]; sc += part[3 * tile + 2]; }
        const size_t o = (size_t)s * A.nz + z;
        A.ngal[o] = sn;
        A.bg[o] = sb / sn;
        if (A.craw) A.craw[o] = sc;
    }
}

// side[nz][nm][4] = (w, w bh, w m/rho, w bh m/rho) with w = wm nzm: what the contraction needs of a mass bin besides the
// sets' coefficients.  One thread per (z, m).
__global__ __launch_bounds__(256) void hodens_side_kernel(HaloGrid g, double* __restrict__ side) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)g.nz * g.nm) return;
    const int m = (int)(e % g.nm);
    const double w = g.wm[m] * g.nzm[e], wb = w * g.bh[e], r = g.ms[m] / g.rho_m0;
    side[4 * e] = w; side[4 * e + 1] = wb; side[4 * e + 2] = w * r; side[4 * e + 3] = wb * r;
}

// raises *bad (a plain store) if a column's node is off the k grid
__global__ __launch_bounds__(256) void hodens_check_kernel(int n, int nk, const int* __restrict__ kidx, int* __restrict__ bad) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && (kidx[e] < 0 || kidx[e] >= nk)) *bad = 1;
}

struct HodEnsPowerArgs {
    int S, Spad, nz, nm, nk, n;
    int ngroups, ntiles;            // (z, column tile) groups; set tiles
    const double *us, *um;          // [nz][nm][nk]
    const double *coef, *craw;      // the coefficient block
    const double *side, *Cm;        // [nz][nm][4], [nz]
    const double *ngal, *bg;        // [S][nz]
    const double *Pzk, *damp;       // [nz][nk], [n]
    const int* kidx;                // [n] or NULL: column = node
    double *out, *parts;            // [4][S][nz][n], [3][S][nz][n] or NULL
};

// The contraction.  A thread owns one column (a node of the k grid) at one redshift and TS sets: G, X, I of each set and
// the matter sum I_m walk the mass axis in order, one FMA chain per accumulator, so an element depends on its own (set,
// z, node) only.  Per mass bin the thread loads u_s (and u_m unless it is the same tensor); the sets' coefficients and
// the side data have wave-uniform addresses and come through the scalar cache.  5 FMA per set and element:
//     G += (2 NcNs) (w u_s) + NsNsm1 (w u_s^2);  t = Ns u_s + Nc;  X += t (w m/rho u_m);  I += t (w bh)
// Epilogue, in this order: G / ngal^2, X / ngal, I / ngal, C = craw / ngal, J_g = (I + bg) - C, J_m = (I_m + 1) - C_m,
// P1h_gg = D G, P2h_gg = (Pzk J_g) J_g, P1h_gm = D X, P2h_gm = (Pzk J_g) J_m.
// 1-D grid: block L runs on XCD L % 8, so the set tiles of one (z, column tile) get ids of one residue and are
// consecutive there: they find the tensor tile in that XCD's L2.
template <int TS, bool ALIAS>
__global__ __launch_bounds__(HE_KT) void hodens_power_kernel(HodEnsPowerArgs A) {
#pragma clang fp contract(off)
    const int L = blockIdx.x, j = L >> 3;
    const int grp = (j / A.ntiles) * 8 + (L & 7), tile = j % A.ntiles;
    if (grp >= A.ngroups) return;
    const int nkt = (A.n + (int)blockDim.x - 1) / (int)blockDim.x;
    const int z = grp / nkt, kt = grp - z * nkt;
    const int col = kt * (int)blockDim.x + (int)threadIdx.x;
    const bool live = col < A.n;
    const int k = live ? (A.kidx ? A.kidx[col] : col) : 0;          // (a column past the end reads node 0)
    const int s0 = tile * TS, nm = A.nm;
    const size_t cstride = (size_t)A.Spad * 4;
    const double* __restrict__ cf = A.coef + (size_t)z * nm * cstride + (size_t)s0 * 4;
    const double* __restrict__ sd = A.side + (size_t)z * nm * 4;
    const double* __restrict__ pu = A.us + (size_t)z * nm * A.nk + k;
    const double* __restrict__ pm = A.um + (size_t)z * nm * A.nk + k;
    double G[TS], X[TS], I[TS], Im = 0.0;
#pragma unroll
    for (int i = 0; i < TS; ++i) G[i] = X[i] = I[i] = 0.0;
#pragma unroll 2
    for (int m = 0; m < nm; ++m) {
        const double us = pu[(size_t)m * A.nk];
        const double um = ALIAS ? us : pm[(size_t)m * A.nk];
        const double* __restrict__ q = sd + 4 * (size_t)m;
        const double wb = q[1];
        const double a = q[0] * us, b = a * us, xm = q[2] * um;
        Im = fma(q[3], um, Im);
        const double* __restrict__ c = cf + (size_t)m * cstride;
#pragma unroll
        for (int i = 0; i < TS; ++i) {
            G[i] = fma(c[4 * i + 2], a, G[i]);
            G[i] = fma(c[4 * i + 3], b, G[i]);
            const double t = fma(c[4 * i + 1], us, c[4 * i]);
            X[i] = fma(t, xm, X[i]);
            I[i] = fma(t, wb, I[i]);
        }
    }
    if (!live) return;
    const double Jm = (Im + 1.0) - A.Cm[z];
    const double P = A.Pzk[(size_t)z * A.nk + k], D = A.damp[col];
    const size_t plane = (size_t)A.S * A.nz * A.n;
#pragma unroll
    for (int i = 0; i < TS; ++i) {
        const int s = s0 + i;
        if (s >= A.S) continue;
        const size_t sz = (size_t)s * A.nz + z, o = sz * A.n + col;
        const double ng = A.ngal[sz];
        const double Gn = G[i] / (ng * ng), Xn = X[i] / ng, In = I[i] / ng;
        const double C = A.craw[sz] / ng;
        const double Jg = (In + A.bg[sz]) - C;
        const double PJ = P * Jg;
        A.out[o] = D * Gn;
        A.out[plane + o] = PJ * Jg;
        A.out[2 * plane + o] = D * Xn;
        A.out[3 * plane + o] = PJ * Jm;
        if (A.parts) { A.parts[o] = Gn; A.parts[plane + o] = Xn; A.parts[2 * plane + o] = In; }
    }
}

}  // namespace hmg
