// K3 - analytic NFW u(k|m,z) through Si/Ci and its small-argument series (hmvec/hmvec.py:346-353).
// Part of the ONE translation unit hmgrid.hip (included there in this order; not a stand-alone header).
#pragma once

namespace hmg {

// ---------------------------------------------------------------- K3: analytic NFW (A6)
// fp64-VALU bound (two Si/Ci rational evaluations + two sincos per 8 bytes written), so the
// kernel is organised to minimise instructions, not bytes: one block per (z,m) row so the
// row constants (c, r_s, 1/m_c: a log and two divisions) are computed once per thread
// instead of once per point; sin(c x) comes from the angle-difference identity on the two
// sincos the Si/Ci asymptotics need anyway; k is the fast axis -> coalesced 8 B stores.
// Small-argument series of the NFW transform, one coefficient row per (z,m):
//   u(k) = (1/m_c) int_0^c [sin(x t)/(x t)] t/(1+t)^2 dt = sum_n a_n x^(2n),
//   a_n = (-1)^n J_(2n+1)(c) / ((2n+1)! m_c),   J_p(c) = int_0^c t^p/(1+t)^2 dt,
//   J_0 = c/(1+c), J_1 = m_c,  J_p = c^(p-1)/(p-1) - 2 J_(p-1) - J_(p-2).
// With NFW_NS = 16 terms the series is exact to 2 ulp for (1+c) x <= 4 and c >= 0.5 (checked
// against 50-digit arithmetic for c in [0.5, 60]); it replaces two Si/Ci rational evaluations
// and two sincos by 16 FMAs on about 2/3 of a typical grid, and it does not suffer the
// cancellation of the closed form at small x.  a[row][0] = 0 flags "do not use" (c < 0.5).
constexpr int NFW_NS = 16;     // terms used for (1+c) x <= 4
constexpr int NFW_NS2 = 32;    // terms used for 4 < (1+c) x <= NFW_X2 (same coefficient row, first 16 shared)
constexpr double NFW_X2 = 10.0;
constexpr int NFW_ROW = HMG_NFW_SERIES_STRIDE;   // doubles per (z,m) row: 32 series coefficients + row constants
constexpr int NFW_NT1 = 5;          // terms for (1+c) x <= NFW_XS1
constexpr double NFW_XS1 = 0.1;
constexpr int NFW_NT2 = 8;          // terms for (1+c) x <= NFW_XS2
constexpr double NFW_XS2 = 0.8;
constexpr int NFW_NQ = 10;          // a_1 .. a_NFW_NQ of a row with c < NFW_CQ come from quadrature (nfw_series_row)
constexpr double NFW_CQ = 1.5;
// With 32 terms the series stays within 3e-15 (absolute, against 50-digit arithmetic, c in [0.5, 100])
// up to (1+c) x = 10: the band 4 < (1+c) x <= 10 - where x itself is still on the small-argument
// branch of Si/Ci, the most expensive case of the closed form - costs 32 FMAs instead.
__device__ __forceinline__ void nfw_series_row(double c, double* __restrict__ a) {
    constexpr double INVFACT[NFW_NS2] = {1.0, 0.16666666666666666, 0.008333333333333333, 0.0001984126984126984, 2.7557319223985893e-06, 2.505210838544172e-08, 1.6059043836821613e-10, 7.647163731819816e-13, 2.8114572543455206e-15, 8.22063524662433e-18, 1.9572941063391263e-20, 3.8681701706306835e-23, 6.446950284384474e-26, 9.183689863795546e-29, 1.1309962886447718e-31, 1.2161250415535181e-34, 1.151633562077195e-37, 9.67759295863189e-41, 7.265460179153071e-44, 4.902469756513544e-47, 2.9893108271424046e-50, 1.6552108677421951e-53, 8.359650847182804e-57, 3.866628513960594e-60, 1.643974708316579e-63, 6.446959640457174e-67, 2.3392451525606576e-70, 7.876246304918039e-74, 2.4674957095607893e-77, 7.210682961895936e-81, 1.9701319568021682e-84, 5.043860616493007e-88};
    const double opc = 1.0 + c;
    const double mc = log(opc) - c / opc;
    const double inv_mc = 1.0 / mc;
    double jm2 = c / opc, jm1 = mc, cp = c;   // J_0, J_1, c^(p-1) for p = 2
    a[NFW_NS2 + 0] = log(opc);              // row constants of the closed forms, computed once per row
    a[NFW_NS2 + 1] = inv_mc;                //   here instead of once per thread of the row's workgroup
    a[NFW_NS2 + 2] = 1.0 / (opc * opc);
    a[NFW_NS2 + 3] = 0.0;
    a[0] = (c >= 0.5) ? 1.0 : 0.0;
    // unrolled: 1/(p-1) becomes a compile-time factor (a division here is ~15 dependent instructions in a
    // 62-step chain).  The recurrence carries the rounding errors of J_0 and J_1 = m_c (up to 1.5e-16) into every J_p
    // undamped, as (-1)^p (alpha + beta p): harmless where J_p grows with p, but below c = 1.25 the low moments, the
    // ones that matter at (1+c) x = 10, lose up to 1.3e-13 of the row's largest term to it.  Rows with c < NFW_CQ
    // therefore take J_3 .. J_(2 NFW_NQ + 1) from a 16-point Gauss-Legendre rule instead (a positive integrand, the
    // pole at t = -1 far off: full double precision, checked for c in [0.5, 1.5)).  With that the coefficients stay
    // within 5e-15 of 60-digit arithmetic for c in [0.5, 100], measured as |da_n| x^(2n) over the row's largest term
    // at (1+c) x = 10 (worst 1.5e-15: tests/test_nfw_cpu.py).
#pragma unroll
    for (int p = 2; p < 2 * NFW_NS2; ++p) {
        const double jp = cp * (1.0 / (double)(p - 1)) - 2.0 * jm1 - jm2;
        cp *= c;
        if (p & 1) {
            const int n = (p - 1) >> 1;
            a[n] = ((n & 1) ? -jp : jp) * INVFACT[n] * inv_mc;
        }
        jm2 = jm1;
        jm1 = jp;
    }
    if (c >= 0.5 && c < NFW_CQ) {
        constexpr double GX[8] = {0.09501250983763744, 0.2816035507792589, 0.45801677765722737, 0.6178762444026438, 0.755404408355003, 0.8656312023878318, 0.9445750230732326, 0.9894009349916499};
        constexpr double GW[8] = {0.1894506104550685, 0.18260341504492358, 0.16915651939500254, 0.14959598881657674, 0.12462897125553388, 0.09515851168249279, 0.062253523938647894, 0.027152459411754096};
        const double h = 0.5 * c;
        double acc[NFW_NQ];
#pragma unroll
        for (int n = 0; n < NFW_NQ; ++n) acc[n] = 0.0;
#pragma unroll      // (the 16 nodes are independent chains: one thread per row, so latency is the cost)
        for (int i = 0; i < 16; ++i) {
            const double t = h * ((i & 1) ? -GX[i >> 1] : GX[i >> 1]) + h, d = 1.0 + t, t2 = t * t;
            double pw = (h * GW[i >> 1]) / (d * d) * t;      // w t / (1+t)^2
#pragma unroll
            for (int n = 0; n < NFW_NQ; ++n) {
                pw *= t2;
                acc[n] += pw;                                 // J_(2n+3)
            }
        }
#pragma unroll
        for (int n = 1; n <= NFW_NQ; ++n) a[n] = ((n & 1) ? -acc[n - 1] : acc[n - 1]) * INVFACT[n] * inv_mc;
    }
}
__global__ void nfw_series_kernel(int rows, const double* __restrict__ cs, double* __restrict__ acoef) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    nfw_series_row(cs[row], acoef + (size_t)row * NFW_ROW);
}

// The two short forms of the series, for a point with (1+c) x <= NFW_XS2 of a row whose series is on.  The series
// alternates and its n-th term is below (xc)^(2n) / (2n (2n+1)! m_c): 5 terms are exact to 1e-18 for (1+c) x <= 0.1,
// 8 terms to 2e-17 for <= 0.8 - about 60 % of a typical grid (k starts four decades below the halo scale) takes one
// of the two.  a: the row's coefficients a[0..7], wave-uniform.  EVERY evaluation of these points goes through this
// function - the row kernel, the batched mass integrals that evaluate instead of loading (series deferral, DESIGN.md
// section 3) and the fill kernel -, so all of them produce the same bits.
__device__ __forceinline__ double nfw_series_short(const double* __restrict__ a, double x, double xc) {
    const double z = x * x;
    double u;
    if (xc <= NFW_XS1) {
        u = fma_svs(a[NFW_NT1 - 1], z, a[NFW_NT1 - 2]);
#pragma unroll
        for (int n = NFW_NT1 - 3; n >= 0; --n) u = fma_vvs(u, z, a[n]);
    } else {
        u = fma_svs(a[NFW_NT2 - 1], z, a[NFW_NT2 - 2]);
#pragma unroll
        for (int n = NFW_NT2 - 3; n >= 0; --n) u = fma_vvs(u, z, a[n]);
    }
    return u;
}
// Number of leading wavenumbers of a row that take a short form: the k with opc * (ks[k] * rs * z1) <= NFW_XS2, the
// value and the operation order nfw_rows tests.  ks ascending, so the test is monotone in k: a 64-way search, one
// wavefront, one load and one ballot per level (two levels up to nk = 4096).  Every lane returns the count.
__device__ __forceinline__ int nfw_series_count(const double* __restrict__ ks, int nk, double rs, double z1, double opc,
                                                int lane) {
    int lo = 0, n = nk;          // every k < lo passes; the first that fails, if any, is in [lo, lo + n)
    while (n > 0) {
        const int s = (n + 63) >> 6, nchunk = (n + s - 1) / s;      // lane l: the chunk [lo + l s, lo + (l+1) s) of it
        const int last = min(lo + (lane + 1) * s, lo + n) - 1;
        const bool pass = lane < nchunk && opc * (ks[lane < nchunk ? last : 0] * rs * z1) <= NFW_XS2;
        const int np = __builtin_amdgcn_readfirstlane(__popcll(__ballot(pass)));      // chunks that pass whole
        if (np >= nchunk) { lo += n; n = 0; break; }
        const int end = min(lo + (np + 1) * s, lo + n);
        lo += np * s;
        n = end - lo - 1;        // (the last k of chunk np fails)
    }
    return lo;
}

// Order in which the row workgroups of a launch take the masses of a redshift: heaviest first.  Workgroups are
// dispatched in index order and the rows of the heavy end of the mass grid are the expensive ones in both tensor
// producers (NFW: most of their wavenumbers are on the Si/Ci branch; Battaglia: many FFT modes are reachable), so
// ascending order leaves the most expensive rows for the tail of the launch.  Measured on MI355X (rows group +
// profile group): 58.9 -> 55.3 us on a 4-redshift slab, 97.9 -> 96.1 at nz = 8, +-0 at nz = 32; folding the mass
// axis (light half ascending, heavy half descending) and mass-major order over all redshifts were no better.
__device__ __forceinline__ int row_order(int r, int nm) {
    const int z = r / nm, i = r - z * nm;
    return z * nm + (nm - 1 - i);
}

// ktile = k values per workgroup (a multiple of the block size)
// 46 VGPRs, no scratch (with machine LICM off: see the Makefile); the bound only keeps it under 64.
#ifndef HMG_NFW_OCC
#define HMG_NFW_OCC 8
#endif
struct NfwArgs {
    const SiciTable* T;
    const double* acoef;
    int ktile, nm, nk;
    const double *cs, *rss, *zs, *ks;
    double* uk;
    int* nser;       // series deferral: the per-row counts the launch writes (nullptr: the tensor is written whole)
};
// blk: index of the (row, k tile) this workgroup owns; nthr: threads that share it (the workgroup size).
// The pointers must reach this function as __restrict__ KERNEL PARAMETERS (not as fields of a by-value
// struct): only then can hipcc prove that the stores to uk do not clobber the row constants, series
// coefficients and Si/Ci tables and fetch those with scalar loads - as struct fields they became 249 vector
// loads per thread and the kernel ran 2.6x slower (0.15 -> 0.40 ms at Config 3).
__device__ __forceinline__ void nfw_rows(const SiciTable* __restrict__ T, const double* __restrict__ acoef, int ktile,
                                         int nm, int nk, const double* __restrict__ cs,
                                         const double* __restrict__ rss, const double* __restrict__ zs,
                                         const double* __restrict__ ks, double* __restrict__ uk, int blk, int nthr,
                                         int tid, int* __restrict__ nser = nullptr) {
    // one (z,m) row per nthr threads, the whole k axis in one tile.  Measured on whole rows of 4096 wavenumbers, 256
    // threads: two rows per workgroup +4 %, half tiles +40 %, 128 threads per row +-0 - a workgroup's fixed cost is
    // the latency of its scalar loads (row constants, series coefficients), not instructions.  Under series deferral a
    // row is about 1600 wavenumbers and often none: there every wavefront's prologue counts, and the tensor group
    // gives a row 256 of its 512 threads on full grids (nfw_row_group; profiles/r12/nfw_rows_per_wg_ab.txt)
    const int ktiles = (nk + ktile - 1) / ktile;
    const int brow = blk / ktiles;
    const int row = row_order(brow, nm);  // z*nm + m
    const int k_lo = (blk - brow * ktiles) * ktile;
    const int k_hi = min(nk, k_lo + ktile);
    const int z = row / nm;
    const double c = cs[row];
    const double rs = rss[row];
    const double z1 = 1.0 + zs[z];
    const double opc = 1.0 + c;
    // small-argument series coefficients and closed-form constants of this row: wave-uniform -> SGPRs
    const double* __restrict__ a = acoef + (size_t)row * NFW_ROW;
    const double ln_opc = a[NFW_NS2 + 0], inv_mc = a[NFW_NS2 + 1], inv_opc2 = a[NFW_NS2 + 2];
    const bool use_series = (a[0] != 0.0);
    double* __restrict__ dst = uk + (size_t)row * nk;
    // series deferral (nser != nullptr): the count of this row's short-series wavenumbers goes to nser[row] and the whole
    // HMG_PREFIX_TILE-wide tiles below it stay unwritten - whoever reads them evaluates nfw_series_short instead
    int k_first = k_lo;
    if (nser) {
        const int cnt = use_series ? nfw_series_count(ks, nk, rs, z1, opc, tid & 63) : 0;
        if (tid == 0 && k_lo == 0) nser[row] = cnt;
        k_first = max(k_lo, cnt & ~(HMG_PREFIX_TILE - 1));
    }
    for (int k = k_first + tid; k < k_hi; k += nthr) {
        const double x = ks[k] * rs * z1;
        const double xc = opc * x;
        if (use_series && xc <= 4.0) {
            double u;
            if (xc <= NFW_XS2) {
                u = nfw_series_short(a, x, xc);
            } else {
                const double z = x * x;
                u = fma_svs(a[NFW_NS - 1], z, a[NFW_NS - 2]);
#pragma unroll
                for (int n = NFW_NS - 3; n >= 0; --n) u = fma_vvs(u, z, a[n]);
            }
            __builtin_nontemporal_store(u, &dst[k]);
            continue;
        }
        if (use_series && xc <= NFW_X2) {
            const double z = x * x;
            double u = fma_svs(a[NFW_NS2 - 1], z, a[NFW_NS2 - 2]);
#pragma unroll
            for (int n = NFW_NS2 - 3; n >= 0; --n) u = fma_vvs(u, z, a[n]);
            __builtin_nontemporal_store(u, &dst[k]);
            continue;
        }
        if (x > 4.0 && xc < 1.0e9) {
            // Both arguments on the auxiliary-function branch, Si = pi/2 - f cos - g sin,
            // Ci = f sin - g cos.  Substituting into the NFW formula the terms in f(x) cancel and
            // the rest collapses, exactly, to
            //     u m_c = g(x) + f(xc) sin(c x) - g(xc) cos(c x) - sin(c x)/xc :
            // one sincos (of c x, the argument the reference itself uses for sin(c x)) instead of
            // two, three rationals instead of four, and none of the pi/2-sized cancellations.
            const double zx = rcp_fast(x * x), zc = zx * inv_opc2;
            double f1, g1, f2, g2, sd, cd;
            sici_aux<false>(T, x, zx, f1, g1);
            sici_aux<true>(T, xc, zc, f2, g2);
            sincos_fast(c * x, sd, cd);
            __builtin_nontemporal_store((g1 + (f2 - xc * zc) * sd - g2 * cd) * inv_mc, &dst[k]);
            continue;
        }
        if (x <= 4.0 && xc > 8.0) {
            // Mixed band (3.5 % of a typical grid, beyond the reach of the series): x on the rational
            // branch of Si/Ci, (1+c)x on the auxiliary-function branch.  Substituting
            // Si(xc) = pi/2 - f cos xc - g sin xc, Ci(xc) = f sin xc - g cos xc and xc - x = c x,
            //     u m_c = (pi/2) sin x + f(xc) sin(cx) - g(xc) cos(cx) - sin(cx)/xc - sin x Si(x) - cos x Ci(x):
            // sincos of x and c x (the reference's own arguments) instead of x and xc, two rational
            // pairs instead of four, one short logarithm.
            double s1, c1, sd, cd, f2, g2;
            sincos_fast(x, s1, c1);
            sincos_fast(c * x, sd, cd);
            const double x2 = x * x;
            const double zc = rcp_fast(x2) * inv_opc2;                   // 1/xc^2
            const double sden = horner_s<6>(x2, T->SD), cden = horner_s<6>(x2, T->CD);
            const double r = rcp_fast(sden * cden);
            const double si = x * horner_s<6>(x2, T->SN) * (cden * r);
            const double ci = (EULER_GAMMA + log_fast(x)) + x2 * horner_s<6>(x2, T->CN) * (sden * r);
            sici_aux<true>(T, xc, zc, f2, g2);
            __builtin_nontemporal_store((HALF_PI * s1 + (f2 - xc * zc) * sd - g2 * cd - s1 * si - c1 * ci) * inv_mc,
                                        &dst[k]);
            continue;
        }
        // everything else (rows with c < 0.5, arguments beyond 1e9): the closed form as the reference writes it
        double s1, c1, s2, c2;
        if (xc < 1.0e9) {
            sincos_fast(x, s1, c1);
            sincos_fast(xc, s2, c2);
        } else {  // outside the Cody-Waite range: library reduction
            sincos(x, &s1, &c1);
            sincos(xc, &s2, &c2);
        }
        const double zx = rcp_fast(x * x);   // 1/x^2
        const double zc = zx * inv_opc2;     // 1/xc^2
        double si1, ci1, si2, ci2;
        bool sm1, sm2;
        sici_fast(T, x, s1, c1, zx, si1, ci1, sm1);
        sici_fast(T, xc, s2, c2, zc, si2, ci2, sm2);
        // Ci((1+c)x) - Ci(x): x <= xc, so the cases are (small,small), (small,large), (large,large)
        double dci = ci2 - ci1;
        if (sm1) dci += sm2 ? ln_opc : -(EULER_GAMMA + log(x));
        const double scx = s2 * c1 - c2 * s1;  // sin(c x) = sin((1+c)x - x)
        // sin(cx)/((1+c)x) = scx * xc / xc^2
        __builtin_nontemporal_store((s1 * (si2 - si1) - scx * (xc * zc) + c1 * dci) * inv_mc, &dst[k]);
    }
}
// Rows of the NFW role per workgroup of the tensor group (1, 2 or 4: NT / NR stays a multiple of the wavefront), and
// the number of rows per compute unit from which the launch takes that form (below it: one row per workgroup).
// Measured on MI355X at nm = 512, nk = 4096 against one row per workgroup (ms_per_step, medians of four alternating
// runs; profiles/r12/nfw_rows_per_wg_ab.txt): two rows -14 us at nz = 32 (0.432 -> 0.418, every run faster than every
// run before), -10 at nz = 24, -5 at 16, -3 at 12, +-0 at 8, +1.3 at nz = 4 (8 rows per unit: the launch is two rounds
// of workgroups there and the longer NFW workgroups lengthen its tail); four rows 2 us better than two at nz = 32 and
// worse than one from nz = 12 down.  Hence two rows from 24 rows per unit (nz = 12 on that grid) and one below.
#ifndef HMG_NFW_ROWS_PER_WG
#define HMG_NFW_ROWS_PER_WG 2
#endif
#ifndef HMG_NFW_GROUP_MIN_PER_CU
#define HMG_NFW_GROUP_MIN_PER_CU 24
#endif
// The NFW role of a grouped launch whose workgroups have NT threads: workgroup q of the role serves NR consecutive
// blocks of nfw_rows (positions of the heavy-first order), NT / NR threads each.  The sub-group index is
// wave-uniform and goes through readfirstlane, so the row and everything derived from it stay in SGPRs and the
// row's constants still arrive by scalar loads.  No barrier, no LDS: a sub-group past the last block returns.
// nblk: blocks of the role.  NR == 1 is nfw_rows on the workgroup, instruction for instruction.
template <int NT, int NR>
__device__ __forceinline__ void nfw_row_group(const SiciTable* __restrict__ T, const double* __restrict__ acoef,
                                              int ktile, int nm, int nk, const double* __restrict__ cs,
                                              const double* __restrict__ rss, const double* __restrict__ zs,
                                              const double* __restrict__ ks, double* __restrict__ uk, int q, int nblk,
                                              int* __restrict__ nser) {
    static_assert(NR >= 1 && NT % (64 * NR) == 0, "a sub-group is whole wavefronts");
    if constexpr (NR == 1) {
        nfw_rows(T, acoef, ktile, nm, nk, cs, rss, zs, ks, uk, q, NT, threadIdx.x, nser);
    } else {
        constexpr int nthr = NT / NR;
        const int sub = __builtin_amdgcn_readfirstlane((int)threadIdx.x / nthr);
        const int blk = q * NR + sub;
        if (blk >= nblk) return;
        nfw_rows(T, acoef, ktile, nm, nk, cs, rss, zs, ks, uk, blk, nthr, (int)threadIdx.x % nthr, nser);
    }
}
__global__ __launch_bounds__(256, HMG_NFW_OCC) void nfw_kernel(const SiciTable* __restrict__ T,
                                                  const double* __restrict__ acoef, int ktile, int nm, int nk,
                                                  const double* __restrict__ cs, const double* __restrict__ rss,
                                                  const double* __restrict__ zs, const double* __restrict__ ks,
                                                  double* __restrict__ uk) {
    nfw_rows(T, acoef, ktile, nm, nk, cs, rss, zs, ks, uk, blockIdx.x, blockDim.x, threadIdx.x);
}

// The tiles a deferring launch left unwritten (nfw_rows with nser), for every reader other than the batched mass
// integrals: one workgroup per row writes nfw_series_short into [0, nser[row] & ~(HMG_PREFIX_TILE-1)).
__global__ __launch_bounds__(256) void nfw_series_fill_kernel(int nm, int nk, const int* __restrict__ nser,
                                                              const double* __restrict__ acoef,
                                                              const double* __restrict__ cs,
                                                              const double* __restrict__ rss,
                                                              const double* __restrict__ zs,
                                                              const double* __restrict__ ks, double* __restrict__ uk) {
    const int row = blockIdx.x;
    const int n = min(nk, nser[row] & ~(HMG_PREFIX_TILE - 1));
    const double rs = rss[row], z1 = 1.0 + zs[row / nm], opc = 1.0 + cs[row];
    const double* __restrict__ a = acoef + (size_t)row * NFW_ROW;
    double* __restrict__ dst = uk + (size_t)row * nk;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const double x = ks[k] * rs * z1;
        dst[k] = nfw_series_short(a, x, opc * x);
    }
}

}  // namespace hmg
