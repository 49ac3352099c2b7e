// kSZ forecasts (hmvec/ksz.py): the Ma-Fry P_q_perp(k, z) table, the kSZ-tomography reconstruction noise N_vv and
// the Limber projection of a P(z, k) table into C_ell^kSZ.  Definitions and accuracy: DESIGN.md section 11.  Compiled
// in ksz.hip, a translation unit of its own (kept out of the power-path units).
//
// Every sum follows numpy's order for the reference's expression (np.trapz = (d * (y[1:] + y[:-1]) / 2.0).sum()):
// a trapezoid along axis 0 of a 2-D mesh adds the rows one after the other, a 1-D trapezoid is numpy's pairwise
// sum (np_sum below).  Floating-point contraction is off in this unit, so each integrand value is the reference's
// expression rounded operation by operation; no atomics, so a repeated call is bit-identical.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace hmg {

// numpy's pairwise_sum for n <= 128 (eight strided partial sums, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
// then the tail); the reference's grids (102 mu, 101 k_S, 100 chi nodes) are all below that.  Longer sums are taken
// in sequence: the same value to rounding, not numpy's bits.
template <class F>
__device__ __forceinline__ double np_sum(int n, F term) {
    if (n < 8 || n > 128) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += term(i);
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = term(j);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += term(i + j);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += term(i);
    return res;
}

// np.nan_to_num: NaN -> 0, +-inf -> +-DBL_MAX
__device__ __forceinline__ double nan_to_num(double v) {
    if (v != v) return 0.0;
    if (isinf(v)) return v > 0 ? 1.7976931348623157e308 : -1.7976931348623157e308;
    return v;
}

// the reference's _sanitize: anything non-finite -> 0
__device__ __forceinline__ double sanitize(double v) { return isfinite(v) ? v : 0.0; }

// index j of the bracket x[j] <= v < x[j+1] of an ascending table of n >= 2 entries, clipped to [0, n-2]
// (binary search: the tables need not be log-uniform)
__device__ __forceinline__ int bracket(const double* __restrict__ x, int n, double v) {
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// scipy interp1d(x, y, bounds_error=False, fill_value=0) at v: np.interp inside [x0, x_{n-1}] (exact at a node, the
// retry from the right end when the left one gives NaN), 0 outside, NaN for NaN
__device__ __forceinline__ double interp_fill0(const double* __restrict__ x, const double* __restrict__ y, int n,
                                               double v) {
    if (v != v) return v;
    if (v < x[0] || v > x[n - 1]) return 0.0;
    if (n == 1 || v == x[n - 1]) return y[n - 1];
    const int j = bracket(x, n, v);
    if (x[j] == v) return y[j];
    const double slope = (y[j + 1] - y[j]) / (x[j + 1] - x[j]);
    double r = slope * (v - x[j]) + y[j];
    if (r != r) {
        r = slope * (v - x[j + 1]) + y[j + 1];
        if (r != r && y[j] == y[j + 1]) r = y[j];
    }
    return r;
}

// ---------------------------------------------------------------- Ma-Fry P_q_perp(k, z)  (hmvec/ksz.py:542-580)
// out[k, z] = adotf_z^2 (2 pi)^-2 trapz_mu[ trapz_k'[ nan_to_num(I(k, k', mu)) ] ],
// I = k'^2 k (k - 2 k' mu)(1 - mu^2) / (k'^2 (k'^2 + k^2 - 2 k k' mu)) Pmm(k') Pee(|k - k'|),
// Pee linear in k on ks with 0 outside.  One block per (k, z); thread j takes mu_j (strided) and runs the k' trapezoid
// in order; thread 0 then takes the mu trapezoid from LDS.  STAGE: the z-row of ks / Pee / Pmm is copied to LDS first.
constexpr int KSZ_PQ_THREADS = 128;
constexpr double KSZ_INV_2PI_SQ = 0x1.9f02f6222c720p-6;      // (2 pi)**-2 as Python evaluates it

__device__ __forceinline__ double pqperp_integrand(double k, double kp, double mu, double pmm, const double* ks,
                                                   const double* pee, int nk) {
    const double kp2 = kp * kp;
    const double d2 = (kp2 + k * k) - ((2.0 * k) * kp) * mu;
    const double frac = ((k * (k - (2.0 * kp) * mu)) * (1.0 - mu * mu)) / (kp2 * d2);
    const double kmkp = sqrt(d2);
    return nan_to_num((kp2 * frac) * (pmm * interp_fill0(ks, pee, nk, kmkp)));
}

template <bool STAGE>
__global__ __launch_bounds__(KSZ_PQ_THREADS) void ksz_pqperp_kernel(int nz, int nk, int nmu,
                                                                    const double* __restrict__ ks,
                                                                    const double* __restrict__ mus,
                                                                    const double* __restrict__ Pee,
                                                                    const double* __restrict__ Pmm,
                                                                    const double* __restrict__ adotf,
                                                                    double* __restrict__ out) {
    extern __shared__ double ksz_lds[];
    const int ik = blockIdx.x, iz = blockIdx.y;
    double* Imu = ksz_lds;                               // nmu
    const double* sk = ks;
    const double* spee = Pee + (size_t)iz * nk;
    const double* spmm = Pmm + (size_t)iz * nk;
    if (STAGE) {
        double* t = ksz_lds + nmu;
        for (int i = threadIdx.x; i < nk; i += KSZ_PQ_THREADS) {
            t[i] = ks[i];
            t[nk + i] = spee[i];
            t[2 * nk + i] = spmm[i];
        }
        __syncthreads();
        sk = t;
        spee = t + nk;
        spmm = t + 2 * nk;
    }
    const double k = sk[ik];
    for (int j = threadIdx.x; j < nmu; j += KSZ_PQ_THREADS) {
        const double mu = mus[j];
        double yprev = pqperp_integrand(k, sk[0], mu, spmm[0], sk, spee, nk);
        double acc = 0.0;
        for (int i = 1; i < nk; ++i) {
            const double y = pqperp_integrand(k, sk[i], mu, spmm[i], sk, spee, nk);
            const double term = ((sk[i] - sk[i - 1]) * (y + yprev)) / 2.0;
            acc = i == 1 ? term : acc + term;
            yprev = y;
        }
        Imu[j] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double integral =
            np_sum(nmu - 1, [&](int j) { return ((mus[j + 1] - mus[j]) * (Imu[j + 1] + Imu[j])) / 2.0; });
        const double a = adotf[iz];
        out[(size_t)ik * nz + iz] = ((a * a) * KSZ_INV_2PI_SQ) * integral;
    }
}

// ---------------------------------------------------------------- N_vv  (hmvec/ksz.py:297-336, 283-292)
// Nvv[z, mu, kL] = mu^-2 2 pi chi_z^2 / F_z^2 / trapz_kS[ _sanitize(kS (W Pge)^2 / ((W^2 Pgg + ngg) C(chi_z kS))) ],
// C(l) = Cls[int(l)] for l <= lmax (0 for l < 2), inf above (get_interpolated_cls).  With photo-z (sig != 0)
// W = exp(-sig_z^2 (mu kL)^2 / 2 / H_z^2); without it W = 1.  Pge/Pgg/Pph rows: one per z (rows == 0) or one per
// (z, mu, kL) (rows == 1, the general arrays of Nvv_core_integral).  Pph != nullptr: the robust term, the integrand
// times Pph / (W^2 Pgg + ngg), sanitized again.  A non-finite output sets *bad (host raises).
constexpr int KSZ_NVV_THREADS = 256;

struct KszNvvArgs {
    int nz, nmu, nkL, nkS, ncl, rows, photo;
    const double *mus, *kLs, *kSs, *cls, *chi, *F, *sig, *H, *ngg, *Pge, *Pgg, *Pph;
    double* out;
    int* bad;
};

__device__ __forceinline__ double ksz_cl_at(const double* __restrict__ cls, int ncl, double ell) {
    if (!(ell <= (double)(ncl - 1))) return __longlong_as_double(0x7ff0000000000000LL);    // inf above lmax
    const long long i = (long long)ell;
    return i < 2 ? 0.0 : cls[i];
}

__device__ __forceinline__ double ksz_nvv_integral(const KszNvvArgs& a, int iz, size_t row, double W) {
    const size_t off = a.rows ? (((size_t)iz * a.nmu * a.nkL) + row) * a.nkS : (size_t)iz * a.nkS;
    const double* pge = a.Pge + off;
    const double* pgg = a.Pgg + off;
    const double* pph = a.Pph ? a.Pph + off : nullptr;
    const double chi = a.chi[iz], ngg = a.ngg[iz];
    const double WW = W * W;
    auto y = [&](int s) {
        const double ge = a.photo ? pge[s] * W : pge[s];
        const double gg = (a.photo ? pgg[s] * WW : pgg[s]) + ngg;
        const double kS = a.kSs[s];
        double v = sanitize(kS * ((ge * ge) / (gg * ksz_cl_at(a.cls, a.ncl, chi * kS))));
        if (pph) v = sanitize(v * (pph[s] / gg));
        return v;
    };
    return np_sum(a.nkS - 1, [&](int s) { return ((a.kSs[s + 1] - a.kSs[s]) * (y(s + 1) + y(s))) / 2.0; });
}

__device__ __forceinline__ void ksz_nvv_store(const KszNvvArgs& a, int iz, size_t row, double integral) {
    const double mu = a.mus[row / a.nkL];
    const double chi = a.chi[iz], F = a.F[iz];
    const double pref = ((((1.0 / (mu * mu)) * 2.0) * M_PI) * (chi * chi)) / (F * F);
    const double v = pref / integral;
    a.out[(size_t)iz * a.nmu * a.nkL + row] = v;
    if (!isfinite(v)) *a.bad = 1;                  // every writer stores the same value: no atomic needed
}

// photo-z or per-row inputs: one thread per (mu, kL), grid (rows / 256, nz)
__global__ __launch_bounds__(KSZ_NVV_THREADS) void ksz_nvv_rows_kernel(KszNvvArgs a) {
    const size_t row = (size_t)blockIdx.x * KSZ_NVV_THREADS + threadIdx.x;
    const int iz = blockIdx.y;
    if (row >= (size_t)a.nmu * a.nkL) return;
    double W = 1.0;
    if (a.photo) {
        const double kr = a.mus[row / a.nkL] * a.kLs[row % a.nkL];
        const double s = a.sig[iz], H = a.H[iz];
        W = exp((((-(s * s)) * (kr * kr)) / 2.0) / (H * H));
    }
    ksz_nvv_store(a, iz, row, ksz_nvv_integral(a, iz, row, W));
}

// no photo-z, one row per z: the k_S integral once per z (thread 0), broadcast over (mu, kL) by the block
__global__ __launch_bounds__(KSZ_NVV_THREADS) void ksz_nvv_shared_kernel(KszNvvArgs a) {
    __shared__ double integral;
    const int iz = blockIdx.x;
    if (threadIdx.x == 0) integral = ksz_nvv_integral(a, iz, 0, 1.0);
    __syncthreads();
    const double I = integral;
    for (size_t row = threadIdx.x; row < (size_t)a.nmu * a.nkL; row += KSZ_NVV_THREADS) ksz_nvv_store(a, iz, row, I);
}

// ---------------------------------------------------------------- Limber C_ell  (hmvec/ksz.py:596-631, 835-862)
// cl[l] = trapz_chi[ v ] over the nchi nodes chi[l, :] (z[l, :] = z(chi) from the host), k = ell / chi,
// P = bilinear, edge-clamped interp2d(zs, ks, P[k, z]) at (z, k), and in the reference's order
//   Ma-Fry (squeezed == 0):  v = P / (chi^2 / (1+z)^4) * 0.5 * c2 * T2
//   squeezed (squeezed == 1): v = P / chi^2 * (1+z)^4 * c2 * T2
// with c2 = (sigma_T n_e0 / m->Mpc)^2 and T2 = T_CMB^2 from the host.  One thread per ell.
constexpr int KSZ_CL_THREADS = 128;

// FITPACK's degree-1 B-spline evaluation (fpbisp/fpbspl) of the interpolating spline of P[k, z] on (zs, ks): the
// arguments are clamped into the table, then the two basis values per axis are (t1 - x)/(t1 - t0), (x - t0)/(t1 - t0)
__device__ __forceinline__ double bilinear_clamped(const double* __restrict__ zs, int nz,
                                                   const double* __restrict__ ks, int nk,
                                                   const double* __restrict__ P, double z, double k) {
    z = fmin(fmax(z, zs[0]), zs[nz - 1]);
    k = fmin(fmax(k, ks[0]), ks[nk - 1]);
    const int i = bracket(zs, nz, z), j = bracket(ks, nk, k);
    const double fz = 1.0 / (zs[i + 1] - zs[i]), fk = 1.0 / (ks[j + 1] - ks[j]);
    const double hz0 = fz * (zs[i + 1] - z), hz1 = fz * (z - zs[i]);
    const double hk0 = fk * (ks[j + 1] - k), hk1 = fk * (k - ks[j]);
    double sp = 0.0;
    sp = sp + (P[(size_t)j * nz + i] * hz0) * hk0;
    sp = sp + (P[(size_t)(j + 1) * nz + i] * hz0) * hk1;
    sp = sp + (P[(size_t)j * nz + i + 1] * hz1) * hk0;
    sp = sp + (P[(size_t)(j + 1) * nz + i + 1] * hz1) * hk1;
    return sp;
}

__global__ __launch_bounds__(KSZ_CL_THREADS) void ksz_limber_cl_kernel(int nell, int nchi, int nz, int nk,
                                                                       const double* __restrict__ ells,
                                                                       const double* __restrict__ chi,
                                                                       const double* __restrict__ zn,
                                                                       const double* __restrict__ zs,
                                                                       const double* __restrict__ ks,
                                                                       const double* __restrict__ P, int squeezed,
                                                                       double c2, double T2,
                                                                       double* __restrict__ out) {
    const int l = blockIdx.x * KSZ_CL_THREADS + threadIdx.x;
    if (l >= nell) return;
    const double ell = ells[l];
    const double* c = chi + (size_t)l * nchi;
    const double* z = zn + (size_t)l * nchi;
    auto v = [&](int n) {
        const double x = c[n], zp1 = 1.0 + z[n];
        const double p = bilinear_clamped(zs, nz, ks, nk, P, z[n], ell / x);
        const double zp4 = (zp1 * zp1) * (zp1 * zp1);
        double r;
        if (squeezed) {
            r = (p / (x * x)) * zp4;
        } else {
            r = (p / ((x * x) / zp4)) * 0.5;
        }
        return (r * c2) * T2;
    };
    out[l] = np_sum(nchi - 1, [&](int n) { return ((c[n + 1] - c[n]) * (v(n + 1) + v(n))) / 2.0; });
}

}  // namespace hmg
