// 1-halo trispectrum of two spectra:
//     T[z,i,j] = sum_m wm[m] nzm[z,m] s_ab[z,m,i] s_cd[z,m,j],
// s the sampled square term of get_power_1halo (kernels/square_term.hpp, shared with response.hip).  Included by
// trispectrum.hip alone (its own translation unit: the headline path's units do not see these kernels).
#pragma once
#include "square_term.hpp"

namespace hmg {

constexpr int TRI_TILE = 64;        // samples per tile side
constexpr int TRI_CHUNK = 32;       // mass bins staged through LDS at a time
constexpr int TRI_THREADS = 256;    // 16 x 16 threads, a 4 x 4 register block each

struct TriArgs {
    TriSide ab, cd;
    HaloGrid g;                     // (bh, ks, Pzk are not read)
    SampleTable s;
    double* T;                      // [nz][n][n]
};

// stage the interpolated square term of one spectrum at (z, m0 + ml, sample first + il) for ml < mc into dst[ml][il];
// the thread's sample il = tid % 64 is the same for all of its elements, so its table entry (id, f) is read once by
// the caller.  The scale does not depend on m: it multiplies the finished sum (the kernel's last step).
__device__ __forceinline__ void tri_stage(const TriSide& S, const double* cf /*[TRI_CHUNK][2][TRI_NC]*/, double* dst,
                                          int z, int m0, int mc, int nm, int nk, bool live, int id, double f) {
    const int il = threadIdx.x & (TRI_TILE - 1), w = threadIdx.x >> 6;
#pragma unroll 2
    for (int ml = w; ml < mc; ml += TRI_THREADS / TRI_TILE) {
        double s = 0.0;
        if (live) {
            const double* x1 = cf + ml * (2 * TRI_NC);
            const double* x2 = x1 + TRI_NC;
            const size_t at = ((size_t)z * nm + (m0 + ml)) * (size_t)nk + id;
            s = tri_square_at(S, x1, x2, at);
            if (f != 0.0) s = fma(f, tri_square_at(S, x1, x2, at + 1), (1.0 - f) * s);   // node id + 1 is read only here
        }
        dst[ml * TRI_TILE + il] = s;
    }
}

// grid (tiles of j, tiles of i, nz), TRI_THREADS threads.  Each workgroup walks the whole mass axis itself, in order:
// no split over workgroups, no atomics - an element depends on its own (z, i, j), the tables and the tensors alone.
// The weight wm * nzm multiplies the product of the two sides (it is not folded into one of them), and the finished
// sum is multiplied by scale_i * scale_j as one factor: every step is symmetric in the two sides, so exchanging the
// two spectra and transposing gives the same bits, and a scale is applied once, not once per mass bin.
__global__ __launch_bounds__(TRI_THREADS) void trispectrum_1h_kernel(TriArgs A) {
    __shared__ __align__(16) double sA[TRI_CHUNK * TRI_TILE], sB[TRI_CHUNK * TRI_TILE];
    __shared__ double cfA[TRI_CHUNK * 2 * TRI_NC], cfB[TRI_CHUNK * 2 * TRI_NC];
    __shared__ double sW[TRI_CHUNK];
    const int tid = threadIdx.x;
    const int z = blockIdx.z, i0 = blockIdx.y * TRI_TILE, j0 = blockIdx.x * TRI_TILE;
    const int tx = tid & 15, ty = tid >> 4;
    // this thread's sample of each side in the loader
    const int il = tid & (TRI_TILE - 1);
    const bool liveA = i0 + il < A.s.n, liveB = j0 + il < A.s.n;
    int idA = 0, idB = 0;
    double fA = 0.0, fB = 0.0;
    if (liveA) { const size_t o = (size_t)z * A.s.n + i0 + il; idA = A.s.idx[o]; fA = A.s.frac[o]; }
    if (liveB) { const size_t o = (size_t)z * A.s.n + j0 + il; idB = A.s.idx[o]; fB = A.s.frac[o]; }

    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;

    for (int m0 = 0; m0 < A.g.nm; m0 += TRI_CHUNK) {
        const int mc = min(TRI_CHUNK, A.g.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed
        if (tid < 2 * TRI_CHUNK) {             // the coefficient rows of the chunk: one thread per (side, m)
            const int ml = tid & (TRI_CHUNK - 1);
            if (ml < mc) {
                const size_t zm = (size_t)z * A.g.nm + m0 + ml;
                const double mass = A.g.ms[m0 + ml];
                if (tid < TRI_CHUNK) {
                    tri_square_forms(A.ab, zm, z, mass, A.g.rho_m0, cfA + ml * (2 * TRI_NC), cfA + ml * (2 * TRI_NC) + TRI_NC);
                    sW[ml] = A.g.wm[m0 + ml] * A.g.nzm[zm];
                } else {
                    tri_square_forms(A.cd, zm, z, mass, A.g.rho_m0, cfB + ml * (2 * TRI_NC), cfB + ml * (2 * TRI_NC) + TRI_NC);
                }
            }
        }
        __syncthreads();
        tri_stage(A.ab, cfA, sA, z, m0, mc, A.g.nm, A.g.nk, liveA, idA, fA);
        tri_stage(A.cd, cfB, sB, z, m0, mc, A.g.nm, A.g.nk, liveB, idB, fB);
        __syncthreads();
#pragma unroll 4
        for (int ml = 0; ml < mc; ++ml) {
            const double w = sW[ml];
            const double2 a01 = *reinterpret_cast<const double2*>(&sA[ml * TRI_TILE + ty * 4]);
            const double2 a23 = *reinterpret_cast<const double2*>(&sA[ml * TRI_TILE + ty * 4 + 2]);
            const double2 b01 = *reinterpret_cast<const double2*>(&sB[ml * TRI_TILE + tx * 4]);
            const double2 b23 = *reinterpret_cast<const double2*>(&sB[ml * TRI_TILE + tx * 4 + 2]);
            const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r] * b[c], w, acc[r][c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty * 4 + r;
        if (i >= A.s.n) continue;
        double* out = A.T + ((size_t)z * A.s.n + i) * (size_t)A.s.n;
        const double sci = A.s.scale[(size_t)z * A.s.n + i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + tx * 4 + c;
            if (j < A.s.n) out[j] = acc[r][c] * (sci * A.s.scale[(size_t)z * A.s.n + j]);
        }
    }
}

}  // namespace hmg
