// Halo-model bispectrum of three tracers, 1-halo + 2-halo + 3-halo:
//     B1h[z,t] = sigma D1 D2 D3 sum_m wm nzm w_a(s1) w_b(s2) w_c(s3)
//     B2h[z,t] = sigma [D1 D2 I_ab(s1,s2) J_c(s3) P_3 + D2 D3 I_bc(s2,s3) J_a(s1) P_1 + D1 D3 I_ac(s1,s3) J_b(s2) P_2]
//     B3h[z,t] = sigma J_a(s1) J_b(s2) J_c(s3) B_tree(k1, k2, k3)
// w_x the single-tracer weight of get_power_1halo's cross-spectrum case at a sample, I_xy = sum_m wm nzm bh w_x w_y.
// Included by bispectrum.hip alone (its own translation unit: the headline path's units do not see these kernels).  The
// form of one leg's weight is in kernels/leg_form.hpp, shared with response.hip.
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
    const double *nzm, *bh, *ms, *wm, *ks, *Pzk;
    double rho_m0, kstar;           // kstar <= 0: no damping
    const int* idx;                 // [nz][n] left node
    const double *frac, *scale;     // [nz][n]
    const int* tri;                 // [nt][3]
    double *J;                      // [3][nz][n] by leg
    double *Ps, *Ds, *Ks;           // [nz][n] sampled P_lin, damping factor, wavenumber
    double* B;                      // [3][nz][nt]
    int nz, nm, nk, n, nt, chunk;
};

// The wavenumber of a sample: ks[id] where f == 0, else RN(RN((1 - f) ks[id]) + RN(f ks[id + 1])) - three separately
// rounded operations, no contraction: a host that follows the contract gets the same bits, which the 3-halo kernel
// F2 needs (one ulp of a long side moves mu of a squeezed triangle by k_max / k_min ulp).
__device__ __forceinline__ double bis_sample_k(const double* __restrict__ ks, int id, double f) {
#pragma clang fp contract(off)
    const double k0 = ks[id];
    if (f == 0.0) return k0;
    const double a = (1.0 - f) * k0, b = f * ks[id + 1];
    return a + b;
}

// D = 1 - exp(-(k / kstar)^2) by a fixed sequence of separately rounded IEEE operations (hmvec_amd.bispectrum.damping
// is the same sequence in numpy: the two agree to the bit).  x = (k/kstar)^2 > 40 gives exactly 1 (exp(-x) < 2^-57).
// Else n = rint(x log2 e), t = -((x - n ln2_hi) - n ln2_lo) in [-0.35, 0.35] (n ln2_hi is exact: ln2_hi has 32
// significant bits, n < 2^6), exp(t) by its Taylor polynomial of degree 13 in Horner form (truncation < 2^-57), scaled
// by 2^-n.  exp(-x) is within 3 ulp, so D within 3 ulp(exp(-x)) + half an ulp of its own.
__device__ __forceinline__ double bis_damping(double k, double kstar) {
#pragma clang fp contract(off)
    const double q = k / kstar;
    const double x = q * q;
    if (!(x <= 40.0)) return 1.0;
    const double n = rint(x * 1.4426950408889634);
    const double r = (x - n * 6.93147180369123816490e-01) - n * 1.90821492927058770002e-10;
    const double t = -r;
    double p = 1.0 / 6227020800.0;
    p = p * t + 1.0 / 479001600.0;
    p = p * t + 1.0 / 39916800.0;
    p = p * t + 1.0 / 3628800.0;
    p = p * t + 1.0 / 362880.0;
    p = p * t + 1.0 / 40320.0;
    p = p * t + 1.0 / 5040.0;
    p = p * t + 1.0 / 720.0;
    p = p * t + 1.0 / 120.0;
    p = p * t + 1.0 / 24.0;
    p = p * t + 1.0 / 6.0;
    p = p * t + 0.5;
    p = p * t + 1.0;
    p = p * t + 1.0;
    return 1.0 - ldexp(p, -(int)n);
}

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

__device__ __forceinline__ double bis_leg_node(const BisLeg& L, const double* c, size_t at) {
    double v = fma(c[1], L.prof[at], c[0]);
    if (L.cprof) v = fma(c[2], L.cprof[at], v);
    return v;
}

// the weight interpolated to a sample; `at` is the offset of (z, m, left node).  Node id + 1 is read only where f != 0.
__device__ __forceinline__ double bis_leg_at(const BisLeg& L, const double* c, size_t at, double f) {
    double v = bis_leg_node(L, c, at);
    if (f != 0.0) v = fma(f, bis_leg_node(L, c, at + 1), (1.0 - f) * v);
    return v;
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

// Leg prepass, one launch per distinct leg (the leg is an argument of its own: picked from the argument block by a
// run-time index it would go through scratch); `legs` has bit l set for every leg l of the triple that is this tracer,
// and J is written once per such leg: legs of one tracer have the same bits.  grid nz, BIS_THREADS threads: thread s owns sample s at redshift blockIdx.x and
// walks the mass axis in order, I = sum_m wm nzm bh w(z,m,s); the k -> 0 sum C and the HOD bias sum are block sums over
// per-thread strided partial sums, as power_prep_kernel forms them.  J = (I + b) - C is the bracket of P_2h.  The
// launch that serves leg 0 also samples P_lin, the wavenumber and the damping factor.
__global__ __launch_bounds__(BIS_THREADS) void bispectrum_legs_kernel(BisArgs A, BisLeg L, int legs) {
    __shared__ double cf[BIS_PREP_CHUNK * 3], sWb[BIS_PREP_CHUNK], red[BIS_THREADS];
    const int tid = threadIdx.x, z = blockIdx.x;
    const bool live = tid < A.n;
    int id = 0;
    double f = 0.0;
    if (live) { id = A.idx[(size_t)z * A.n + tid]; f = A.frac[(size_t)z * A.n + tid]; }
    double accI = 0.0, accC = 0.0, accB = 0.0;
    for (int m0 = 0; m0 < A.nm; m0 += BIS_PREP_CHUNK) {
        const int mc = min(BIS_PREP_CHUNK, A.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed
        if (tid < mc) {
            const size_t zm = (size_t)z * A.nm + m0 + tid;
            const double wnb = A.wm[m0 + tid] * A.nzm[zm] * A.bh[zm];
            double lowk, ngals;
            bis_leg_form(L, zm, z, A.ms[m0 + tid], A.rho_m0, cf + 3 * tid, lowk, ngals);
            sWb[tid] = wnb;
            accC = fma(wnb, lowk, accC);
            accB = fma(wnb, ngals, accB);
        }
        __syncthreads();
        if (live) {
            const size_t at = ((size_t)z * A.nm + m0) * (size_t)A.nk + id;
            for (int ml = 0; ml < mc; ++ml)
                accI = fma(sWb[ml], bis_leg_at(L, cf + 3 * ml, at + (size_t)ml * A.nk, f), accI);
        }
    }
    const double C = bis_block_sum(accC, red);
    const double Bs = bis_block_sum(accB, red);
    if (!live) return;
    const double b = L.kind == HMG_TRACER_MATTER ? 1.0 : L.kind == HMG_TRACER_PRESSURE ? 0.0 : Bs / L.ngal[z];
    const size_t o = (size_t)z * A.n + tid;
    const double J = (accI + b) - C;
#pragma unroll
    for (int l = 0; l < 3; ++l)
        if (legs >> l & 1) A.J[(size_t)l * A.nz * A.n + o] = J;
    if (legs & 1) {
        const double* P = A.Pzk + (size_t)z * A.nk;
        double ps = P[id];
        if (f != 0.0) ps = fma(f, P[id + 1], (1.0 - f) * ps);
        const double k = bis_sample_k(A.ks, id, f);
        A.Ps[o] = ps;
        A.Ks[o] = k;
        A.Ds[o] = A.kstar > 0.0 ? bis_damping(k, A.kstar) : 1.0;
    }
}

// stage leg U's weights of the chunk: sV[(U chunk + ml) n + s], a wave per mass bin, its lanes over the samples
template <int U>
__device__ __forceinline__ void bis_stage(const BisArgs& A, const double* cf, double* sV, const int* sId,
                                          const double* sFr, int z, int m0, int mc) {
    const BisLeg& L = A.uq[U];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int ml = w; ml < mc; ml += BIS_THREADS / 64) {
        const size_t row = ((size_t)z * A.nm + (m0 + ml)) * (size_t)A.nk;
        const double* c = cf + (U * BIS_MAXCHUNK + ml) * 3;
        for (int s = lane; s < A.n; s += 64)
            sV[(U * A.chunk + ml) * A.n + s] = bis_leg_at(L, c, row + sId[s], sFr[s]);
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
    const int n = A.n, chunk = A.chunk;
    if (tid < n) { sId[tid] = A.idx[(size_t)z * n + tid]; sFr[tid] = A.frac[(size_t)z * n + tid]; }
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

    for (int m0 = 0; m0 < A.nm; m0 += chunk) {
        const int mc = min(chunk, A.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed (and, first, the tables are there)
        if (tid < 3 * BIS_MAXCHUNK) {          // the coefficient rows of the chunk: one thread per (distinct leg, m)
            const int ml = tid & (BIS_MAXCHUNK - 1), u = tid / BIS_MAXCHUNK;
            if (ml < mc && u < A.nu) {
                const size_t zm = (size_t)z * A.nm + m0 + ml;
                double lowk, ngals;
                const BisLeg L = bis_pick(A, u);
                bis_leg_form(L, zm, z, A.ms[m0 + ml], A.rho_m0, cf + tid * 3, lowk, ngals);
                if (u == 0) {
                    const double wn = A.wm[m0 + ml] * A.nzm[zm];
                    sW[ml] = wn;
                    sWb[ml] = wn * A.bh[zm];
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

    const size_t zn = (size_t)z * n, nzn = (size_t)A.nz * n, plane = (size_t)A.nz * A.nt;
#pragma unroll
    for (int r = 0; r < BIS_TPT; ++r) {
        const int t = t0 + r * BIS_THREADS + tid;
        if (t >= A.nt) continue;
        const size_t e1 = zn + s1[r], e2 = zn + s2[r], e3 = zn + s3[r];
        const double sigma = A.scale[e1] * A.scale[e2] * A.scale[e3];
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

// Bz[term][t] = sum_z g[z] B[term][z][t], z in order; one thread per (term, t)
__global__ __launch_bounds__(256) void bispectrum_zsum_kernel(int nz, int nt, const double* __restrict__ g,
                                                              const double* __restrict__ B, double* __restrict__ Bz) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)3 * nt) return;
    const size_t term = e / nt, t = e - term * nt;
    const double* src = B + term * (size_t)nz * nt + t;
    double s = 0.0;
    for (int z = 0; z < nz; ++z) s = fma(g[z], src[(size_t)z * nt], s);
    Bz[e] = s;
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
