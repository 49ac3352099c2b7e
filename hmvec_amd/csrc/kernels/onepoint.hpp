// One-point statistics of a field that is a sum of halo profiles on the sky.  Compiled in
// onepoint.hip, a translation unit of its own.
//
// A sample is a ring t of a halo (z, m): its signal s = signal[z][m][t] (times amp[z][m] where the call gives one) and
// its weight W = ((zw[z] wm[m]) nzm[z][m]) area[z][m][t], the products rounded in this order.  Of the samples of the mass
// window [m_lo, m_hi), numbered n = (m - m_lo) nt + t,
//   exponent:  A[z][lambda_j] = sum_n W_n (exp(i lambda_j s_n) - 1),  lambda_j = j dlambda,
//   moments:   K[z][p - 1]    = sum_n W_n s_n^p,  p = 1 .. 4.
// With h = (lambda_j s) / 2 - lambda_j = (double)j * dlambda and the product each rounded once - the term is
//   Re = -2 sin^2 h,  Im = 2 sin h cos h:
// one sine/cosine pair, and no cos(phi) - 1, which in fp64 has no digits left at phi ~ 1e-8.
//
// Summation order.  It depends on (count, nt) = ((m_hi - m_lo) nt, nt) alone - never on nz, on z or on nlambda - so a row
// of a batch has the bits of the call with that redshift alone.  A thread adds its terms in the order of n into a ladder
// of accumulators: every OP_RADIX terms the lowest is added to the next and cleared, every OP_RADIX of those the next to
// the one above, the fourth takes the rest; at the end the four are added from the lowest up.  No chain of additions is
// then longer than 3 OP_RADIX + n / OP_RADIX^3 + 3 (onepoint.chain_length in Python is this count).
#pragma once
#include "../sici.hpp"

namespace hmg {

constexpr int OP_THREADS = 256;
constexpr int OP_WAVES = OP_THREADS / 64;
constexpr int OP_TILE = 64;                  // values of lambda per workgroup: one per lane
constexpr int OP_RADIX = 8;                  // terms per rung of the ladder
constexpr int OP_SLICE = 4096;               // samples per slice of the exponent: count <= OP_SLICE is one slice ...
constexpr int OP_MAXSPLIT = 8;               // ... and no call has more slices than this

struct OnepointArgs {
    int nz, nm, nt, m_lo, m_hi;
    const double *signal, *area;             // [nz][nm][nt]
    const double* amp;                       // [nz][nm] or NULL
    const double *nzm, *wm, *zw;             // [nz][nm], [nm], [nz]
    int nl, split;
    double dl;
    double* out;                             // exponent: [split][nz][2][nl]; moments: [nz][4]
};

// slices of the exponent's sample axis
static inline int onepoint_split(long long count) {
    const long long s = (count + OP_SLICE - 1) / OP_SLICE;
    return s < 1 ? 1 : s > OP_MAXSPLIT ? OP_MAXSPLIT : (int)s;
}

// sin and cos of h, any sign: sici.hpp's route below 2^30, the library's full-range reduction beyond
__device__ __forceinline__ void onepoint_sincos(double h, double& s, double& c) {
    const double a = fabs(h);
    double sa;
    if (a < 0x1p30) sincos_fast(a, sa, c);
    else sincos(a, &sa, &c);
    s = h < 0.0 ? -sa : sa;
}

template <int N>
struct OnepointLadder {                      // N sums side by side through the ladder described above
    double a0[N], a1[N], a2[N], a3[N];
    __device__ __forceinline__ OnepointLadder() {
#pragma unroll
        for (int k = 0; k < N; ++k) a0[k] = a1[k] = a2[k] = a3[k] = 0.0;
    }
    // after the terms of local index i were added to a0
    __device__ __forceinline__ void carry(int i) {
        if ((i & (OP_RADIX - 1)) != OP_RADIX - 1) return;
#pragma unroll
        for (int k = 0; k < N; ++k) { a1[k] += a0[k]; a0[k] = 0.0; }
        if ((i & (OP_RADIX * OP_RADIX - 1)) != OP_RADIX * OP_RADIX - 1) return;
#pragma unroll
        for (int k = 0; k < N; ++k) { a2[k] += a1[k]; a1[k] = 0.0; }
        if ((i & (OP_RADIX * OP_RADIX * OP_RADIX - 1)) != OP_RADIX * OP_RADIX * OP_RADIX - 1) return;
#pragma unroll
        for (int k = 0; k < N; ++k) { a3[k] += a2[k]; a2[k] = 0.0; }
    }
    __device__ __forceinline__ double total(int k) const { return ((a0[k] + a1[k]) + a2[k]) + a3[k]; }
};

// The walk of the samples [n0, n1) of redshift z in order: f(i, s, W) for the i-th of them.
template <class F>
__device__ __forceinline__ void onepoint_walk(const OnepointArgs& A, int z, int n0, int n1, F f) {
    if (n0 >= n1) return;
    const int nt = A.nt;
    int m = A.m_lo + n0 / nt, t = n0 % nt;
    const size_t zrow = (size_t)z * A.nm;
    const double gz = A.zw[z];
    double wz = (gz * A.wm[m]) * A.nzm[zrow + m];
    double am = A.amp ? A.amp[zrow + m] : 1.0;
    for (int n = n0, i = 0; n < n1; ++n, ++i) {
        const size_t at = (zrow + m) * nt + t;
        const double raw = A.signal[at];
        f(i, A.amp ? am * raw : raw, wz * A.area[at]);
        if (++t == nt && n + 1 < n1) {
            t = 0;
            ++m;
            wz = (gz * A.wm[m]) * A.nzm[zrow + m];
            if (A.amp) am = A.amp[zrow + m];
        }
    }
}

// out[slice][z][0 / 1][j]: real and imaginary part of the slice's share of A[z][lambda_j].  One workgroup per (tile of
// OP_TILE values of lambda, z, slice); a lane owns one lambda, the four wavefronts take a quarter of the slice's samples
// each - consecutive n, so a wavefront's sample is the same in every lane and comes through the scalar cache - and wave
// 0 .. 3 are added in this order through LDS.  The tiles start at j = 1: every term of lambda_0 = 0 is exactly 0, so
// A[z][0] is written, not summed, and the nbins / 2 other values of a PDF of nbins bins fill whole tiles.
__global__ __launch_bounds__(OP_THREADS) void onepoint_exponent_kernel(OnepointArgs A) {
    __shared__ double part[OP_WAVES][2][OP_TILE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int z = blockIdx.y, slice = blockIdx.z;
    const int j = blockIdx.x * OP_TILE + lane + 1;
    const double lam = (double)j * A.dl;             // (lanes past nl work on a lambda nobody stores)
    const int count = (A.m_hi - A.m_lo) * A.nt;
    const int shares = OP_WAVES * A.split;
    const int chunk = (count + shares - 1) / shares;
    const int q = slice * OP_WAVES + wave;
    const long long lo = (long long)q * chunk, hi = lo + chunk;
    const int n0 = lo < count ? (int)lo : count, n1 = hi < count ? (int)hi : count;
    OnepointLadder<2> acc;
    onepoint_walk(A, z, n0, n1, [&](int i, double s, double W) {
        const double h = 0.5 * (lam * s);
        double sh, ch;
        onepoint_sincos(h, sh, ch);
        acc.a0[0] += (-2.0 * W) * (sh * sh);
        acc.a0[1] += (2.0 * W) * (sh * ch);
        acc.carry(i);
    });
    part[wave][0][lane] = acc.total(0);
    part[wave][1][lane] = acc.total(1);
    __syncthreads();
    if (threadIdx.x < 2 * OP_TILE) {
        const int c = threadIdx.x >> 6;
        const double v = ((part[0][c][lane] + part[1][c][lane]) + part[2][c][lane]) + part[3][c][lane];
        double* row = A.out + (((size_t)slice * A.nz + z) * 2 + c) * A.nl;
        if (j < A.nl) row[j] = v;
        if (blockIdx.x == 0 && lane == 0) row[0] = 0.0;
    }
}

// out[z][p - 1] = K[z][p - 1].  One workgroup per z; a thread takes count / OP_THREADS consecutive samples through the
// ladder, then a fixed LDS tree (stride 128, 64, .. 1) adds the threads.
__global__ __launch_bounds__(OP_THREADS) void onepoint_moments_kernel(OnepointArgs A) {
    __shared__ double part[4][OP_THREADS];
    const int tid = threadIdx.x, z = blockIdx.x;
    const int count = (A.m_hi - A.m_lo) * A.nt;
    const int chunk = (count + OP_THREADS - 1) / OP_THREADS;
    const long long lo = (long long)tid * chunk, hi = lo + chunk;
    const int n0 = lo < count ? (int)lo : count, n1 = hi < count ? (int)hi : count;
    OnepointLadder<4> acc;
    onepoint_walk(A, z, n0, n1, [&](int i, double s, double W) {
        const double s2 = s * s;
        acc.a0[0] += W * s;
        acc.a0[1] += W * s2;
        acc.a0[2] += W * (s2 * s);
        acc.a0[3] += W * (s2 * s2);
        acc.carry(i);
    });
#pragma unroll
    for (int k = 0; k < 4; ++k) part[k][tid] = acc.total(k);
    __syncthreads();
    for (int stride = OP_THREADS / 2; stride > 0; stride >>= 1) {
        if (tid < stride) {
#pragma unroll
            for (int k = 0; k < 4; ++k) part[k][tid] += part[k][tid + stride];
        }
        __syncthreads();
    }
    if (tid < 4) A.out[(size_t)z * 4 + tid] = part[tid][0];
}

// rows[z][e] = parts[0][z][e] + parts[1][z][e] + .. (slices in order; parts == rows with one slice: nothing to add), and
// total[e] = rows[0][e] + rows[1][e] + .. (z in order) where total is not NULL.  e < n.
__global__ void onepoint_finish_kernel(int nz, int n, int split, const double* __restrict__ parts, double* rows,
                                       double* __restrict__ total) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    double sum = 0.0;
    for (int z = 0; z < nz; ++z) {
        double v = parts[(size_t)z * n + e];
        for (int s = 1; s < split; ++s) v += parts[((size_t)s * nz + z) * n + e];
        if (split > 1) rows[(size_t)z * n + e] = v;
        sum = z ? sum + v : v;
    }
    if (total) total[e] = sum;
}

}  // namespace hmg
