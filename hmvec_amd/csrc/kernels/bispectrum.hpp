// Halo-model bispectrum of three tracers, 1-halo + 2-halo + 3-halo:
//     B1h[z,t] = sigma D1 D2 D3 sum_m wm nzm w_a(s1) w_b(s2) w_c(s3)
//     B2h[z,t] = sigma [D1 D2 I_ab(s1,s2) J_c(s3) P_3 + D2 D3 I_bc(s2,s3) J_a(s1) P_1 + D1 D3 I_ac(s1,s3) J_b(s2) P_2]
//     B3h[z,t] = sigma J_a(s1) J_b(s2) J_c(s3) B_tree(k1, k2, k3)
// w_x the single-tracer weight of get_power_1halo's cross-spectrum case at a sample, I_xy = sum_m wm nzm bh w_x w_y.
// Included by bispectrum.hip alone (its own translation unit: the headline path's units do not see these kernels).  The
// form of one leg's weight is in kernels/leg_form.hpp; the leg prepass that leaves J, P, D, k and the z sum are
// sampled.hip's.
#pragma once
#include "leg_form.hpp"

namespace hmg {

constexpr int BIS_TPT = 4;                          // triangles per thread
constexpr int BIS_BLOCK = BIS_THREADS * BIS_TPT;    // triangles per workgroup
constexpr int BIS_MAXN = 256;                       // samples per redshift
constexpr int BIS_MAXCHUNK = 32;                    // mass bins staged through LDS at a time, at most
constexpr int BIS_ROW = 2048;                       // chunk * n <= BIS_ROW: 3 legs * 2048 * 8 B = 48 KB of staged weights

// chunk length of the triangle kernel for n samples: 32 up to n = 64, 8 at n = 256 (the kernel's static LDS is
// 55,040 B whatever n is: two workgroups fit a CU's 160 KB)
static inline int bis_chunk(int n) { return BIS_ROW / n < BIS_MAXCHUNK ? BIS_ROW / n : BIS_MAXCHUNK; }

struct BisArgs {
    BisLeg uq[3];                   // the distinct legs; slot[l] is leg l's entry (legs of one tracer are staged once)
    int nu, slot[3];
    HaloGrid g;
    SampleTable s;
    const int* tri;                 // [nt][3]
    double *J;                      // [3][nz][n] by leg
    double *Ps, *Ds, *Ks;           // [nz][n] sampled P_lin, damping factor, wavenumber
    double* B;                      // [3][nz][nt]
    int nt, chunk;
};

// F2(p, q; r) = 5/7 + mu/2 (p/q + q/p) + 2/7 mu^2, mu the cosine between the sides p and q of the closed triangle
// (p, q, r).  The numerator of mu is factored, (r - p)(r + p) - q^2: with r^2 - p^2 - q^2 the rounding error of a
// squeezed triangle grows as (k_max / k_min)^2.  F2 is symmetric in (p, q) and is evaluated with the longer of the two
// as p: then r - p is exact when q is the short side, nothing cancels when r is, and mu stays within a few ulp for
// every order of the sides (with the short side as p, (r - p)(r + p) and q^2 would cancel to k_min / k_max of their size).
__device__ __forceinline__ double bis_F2(double p, double q, double r) {
    const double a = fmax(p, q), b = fmin(p, q);
    double mu = fma(-b, b, (r - a) * (r + a)) / (2.0 * a * b);
    mu = fmin(1.0, fmax(-1.0, mu));
    const double s = a / b + b / a;
    return fma(2.0 / 7.0 * mu, mu, fma(0.5 * mu, s, 5.0 / 7.0));
}

// leg u of the distinct legs, field by field through compile-time indices and selects (a run-time index into the
// argument block, or a copy of a whole entry, would go through scratch)
#define BIS_PICK(field) (u == 0 ? A.uq[0].field : u == 1 ? A.uq[1].field : A.uq[2].field)
__device__ __forceinline__ BisLeg bis_pick(const BisArgs& A, int u) {
    BisLeg L;
    L.kind = BIS_PICK(kind);
    L.prof = BIS_PICK(prof);
    L.cprof = BIS_PICK(cprof);
    L.Nc = BIS_PICK(Nc);
    L.Ns = BIS_PICK(Ns);
    L.ngal = BIS_PICK(ngal);
    return L;
}
#undef BIS_PICK

// stage leg U's weights of the chunk: sV[(U chunk + ml) n + s], a wave per mass bin, its lanes over the samples
template <int U>
__device__ __forceinline__ void bis_stage(const BisArgs& A, const double* cf, double* sV, const int* sId,
                                          const double* sFr, int z, int m0, int mc) {
    const BisLeg& L = A.uq[U];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int ml = w; ml < mc; ml += BIS_THREADS / 64) {
        const size_t row = ((size_t)z * A.g.nm + (m0 + ml)) * (size_t)A.g.nk;
        const double* c = cf + (U * BIS_MAXCHUNK + ml) * 3;
        for (int s = lane; s < A.s.n; s += 64)
            sV[(U * A.chunk + ml) * A.s.n + s] = bis_leg_at(L, c, row + sId[s], sFr[s]);
    }
}

// Triangle kernel.  grid (blocks of BIS_BLOCK triangles, nz), BIS_THREADS threads, BIS_TPT triangles per thread
// (triangle t0 + r 256 + tid).  A workgroup walks the whole mass axis itself, in order, in chunks staged through LDS:
// no split over workgroups, no atomics - a result depends on its own (z, t), the tables and the tensors alone, not on
// the block it falls in or the chunk length.  Per triangle four sums: the 1-halo sum and I_ab, I_bc, I_ac; scales and
// damping multiply the finished sums.  The three terms are assembled here from the prepass's J, P, D, k.
__global__ __launch_bounds__(BIS_THREADS) void bispectrum_kernel(BisArgs A) {
    __shared__ __align__(16) double sV[3 * BIS_ROW];
    __shared__ double cf[3 * BIS_MAXCHUNK * 3], sW[BIS_MAXCHUNK], sWb[BIS_MAXCHUNK], sFr[BIS_MAXN];
    __shared__ int sId[BIS_MAXN];
    const int tid = threadIdx.x, z = blockIdx.y;
    const int t0 = blockIdx.x * BIS_BLOCK;
    const int n = A.s.n, chunk = A.chunk;
    if (tid < n) { sId[tid] = A.s.idx[(size_t)z * n + tid]; sFr[tid] = A.s.frac[(size_t)z * n + tid]; }
    int s1[BIS_TPT], s2[BIS_TPT], s3[BIS_TPT];
    double a1[BIS_TPT], aab[BIS_TPT], abc[BIS_TPT], aac[BIS_TPT];
#pragma unroll
    for (int r = 0; r < BIS_TPT; ++r) {
        const int t = t0 + r * BIS_THREADS + tid;
        s1[r] = s2[r] = s3[r] = 0;              // (a dead slot gathers sample 0 and stores nothing)
        if (t < A.nt) { s1[r] = A.tri[3 * (size_t)t]; s2[r] = A.tri[3 * (size_t)t + 1]; s3[r] = A.tri[3 * (size_t)t + 2]; }
        a1[r] = aab[r] = abc[r] = aac[r] = 0.0;
    }
    const int oa = A.slot[0] * chunk * n, ob = A.slot[1] * chunk * n, oc = A.slot[2] * chunk * n;

    for (int m0 = 0; m0 < A.g.nm; m0 += chunk) {
        const int mc = min(chunk, A.g.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed (and, first, the tables are there)
        if (tid < 3 * BIS_MAXCHUNK) {          // the coefficient rows of the chunk: one thread per (distinct leg, m)
            const int ml = tid & (BIS_MAXCHUNK - 1), u = tid / BIS_MAXCHUNK;
            if (ml < mc && u < A.nu) {
                const size_t zm = (size_t)z * A.g.nm + m0 + ml;
                double lowk, ngals;
                const BisLeg L = bis_pick(A, u);
                bis_leg_form(L, zm, z, A.g.ms[m0 + ml], A.g.rho_m0, cf + tid * 3, lowk, ngals);
                if (u == 0) {
                    const double wn = A.g.wm[m0 + ml] * A.g.nzm[zm];
                    sW[ml] = wn;
                    sWb[ml] = wn * A.g.bh[zm];
                }
            }
        }
        __syncthreads();
        bis_stage<0>(A, cf, sV, sId, sFr, z, m0, mc);
        if (A.nu > 1) bis_stage<1>(A, cf, sV, sId, sFr, z, m0, mc);
        if (A.nu > 2) bis_stage<2>(A, cf, sV, sId, sFr, z, m0, mc);
        __syncthreads();
        for (int ml = 0; ml < mc; ++ml) {
            const double w = sW[ml], wb = sWb[ml];
            const double* row = sV + ml * n;
#pragma unroll
            for (int r = 0; r < BIS_TPT; ++r) {
                const double a = row[oa + s1[r]], b = row[ob + s2[r]], c = row[oc + s3[r]];
                const double ab = a * b;
                a1[r] = fma(ab * c, w, a1[r]);
                aab[r] = fma(ab, wb, aab[r]);
                abc[r] = fma(b * c, wb, abc[r]);
                aac[r] = fma(a * c, wb, aac[r]);
            }
        }
    }

    const size_t zn = (size_t)z * n, nzn = (size_t)A.g.nz * n, plane = (size_t)A.g.nz * A.nt;
#pragma unroll
    for (int r = 0; r < BIS_TPT; ++r) {
        const int t = t0 + r * BIS_THREADS + tid;
        if (t >= A.nt) continue;
        const size_t e1 = zn + s1[r], e2 = zn + s2[r], e3 = zn + s3[r];
        const double sigma = A.s.scale[e1] * A.s.scale[e2] * A.s.scale[e3];
        const double D1 = A.Ds[e1], D2 = A.Ds[e2], D3 = A.Ds[e3];
        const double P1 = A.Ps[e1], P2 = A.Ps[e2], P3 = A.Ps[e3];
        const double k1 = A.Ks[e1], k2 = A.Ks[e2], k3 = A.Ks[e3];
        const double Ja = A.J[e1], Jb = A.J[nzn + e2], Jc = A.J[2 * nzn + e3];
        // (the pieces without damping first: with D = 1 the sum below has the bits of the undamped one)
        const double x3 = aab[r] * Jc * P3, x1 = abc[r] * Ja * P1, x2 = aac[r] * Jb * P2;
        const double two = fma(D1 * D3, x2, fma(D2 * D3, x1, (D1 * D2) * x3));
        const double tree = 2.0 * fma(bis_F2(k3, k1, k2), P3 * P1,
                                      fma(bis_F2(k2, k3, k1), P2 * P3, bis_F2(k1, k2, k3) * (P1 * P2)));
        const size_t o = (size_t)z * A.nt + t;
        A.B[o] = sigma * (D1 * D2 * D3) * a1[r];
        A.B[plane + o] = sigma * two;
        A.B[2 * plane + o] = sigma * (Ja * Jb * Jc) * tree;
    }
}

// Raises bad[0] for a bad sample table entry, bad[1] for a triangle index outside 0 .. n-1, bad[2] for a triangle that
// does not close at some z: k_max <= (k_mid + k_min)(1 + 2^-40).  One thread per (z, sample) and per (z, triangle); a
// triangle's wavenumbers are read only through entries this thread has checked itself.
__global__ __launch_bounds__(256) void bispectrum_check_kernel(int nz, int nk, int n, int nt, const int* __restrict__ idx,
                                                               const double* __restrict__ frac,
                                                               const int* __restrict__ tri, const double* __restrict__ ks,
                                                               int* __restrict__ bad) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (size_t)nz * n && !bis_sample_ok(idx[e], frac[e], nk)) bad[0] = 1;
    if (e >= (size_t)nz * nt) return;
    const size_t z = e / nt, t = e - z * nt;
    double k[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int s = tri[3 * t + j];
        if (s < 0 || s >= n) { bad[1] = 1; return; }
        const int id = idx[z * n + s];
        const double f = frac[z * n + s];
        if (!bis_sample_ok(id, f, nk)) { bad[0] = 1; return; }
        k[j] = bis_sample_k(ks, id, f);
    }
    const double hi = fmax(k[0], fmax(k[1], k[2])), lo = fmin(k[0], fmin(k[1], k[2]));
    const double mid = fmax(fmin(k[0], k[1]), fmin(fmax(k[0], k[1]), k[2]));
    if (!(hi <= (mid + lo) * (1.0 + 0x1p-40))) bad[2] = 1;
}

}  // namespace hmg
