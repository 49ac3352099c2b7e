// Non-Limber angular power spectra of separable sources: the transfer functions
//   T_l^f(k_i) = sum_g src[f, g, i] j_l(k_i chi_g),   l = 0 .. lmax,
// and the k sum C_l = (2/pi) sum_i wk_i k_i^2 T_l^a T_l^b.  Compiled in
// nonlimber.hip, a translation unit of its own; the spherical Bessel walk is sphbessel.hpp's.
//
// nonlimber_transfer_kernel.  One workgroup of NL_THREADS lanes per k node; it walks the chi nodes in chunks of
// NL_THREADS.  In a chunk lane t owns the node g0 + t, x = k chi: it holds the walk's state in registers and leaves a tile
// of NL_TILE orders in LDS (sj[order][lane]); the chunk's source columns stand in LDS too (ss[lane][field]).  After the
// barrier thread (order, field) = (t / F, t % F) of the first NL_TILE F threads contracts its row of the tile with its
// column of the sources - four partial sums over the lanes 4m, 4m + 1, 4m + 2, 4m + 3 in ascending m, then (p0 + p1) + (p2 + p3) -
// and adds the result to its element of the output, which belongs to this workgroup alone: no atomics, and the chunks
// arrive in order.  The walk at one (k, chi) runs once for all F <= NL_FMAX fields.
//   Lanes with x >= lmax walk upwards and emit in ascending tiles (phase A); lanes with x < lmax walk downwards twice -
// once to l = 0 for the scale, once more emitting in descending tiles (phase B).  A lane that has nothing to say in a phase
// leaves exact zeros, and a phase that no lane of the chunk needs is skipped (a block-uniform vote).  An element is
//   sum over chunks in order of [phase A's sum, then phase B's sum], a zero term changing no bits:
// it depends on its field's source column, its k node, the chi nodes and lmax (through the branch and the start order)
// alone - not on F, not on the other fields or k nodes.
//   LDS: sj NL_TILE x (NL_THREADS + 2) doubles (rows two doubles apart in bank: the two orders a half-wave reads are in
// different banks) + ss NL_THREADS x (NL_FMAX + 1) (an odd pitch: the lanes' stores of one field spread over the banks; a
// half-wave reads 16 consecutive doubles, once per order it holds, broadcast) = 33,024 + 34,816 B: two workgroups per CU.
#pragma once
#include <hip/hip_runtime.h>

#include "../sphbessel.hpp"

namespace hmg {

#pragma clang fp contract(off)

constexpr int NL_THREADS = 256;               // lanes of a workgroup = chi nodes of a chunk
constexpr int NL_TILE = 16;                   // orders per tile
constexpr int NL_FMAX = 16;                   // fields per launch (HMG_NONLIMBER_FMAX)
constexpr int NL_JPITCH = NL_THREADS + 2, NL_SPITCH = NL_FMAX + 1;
static_assert(NL_TILE * NL_FMAX <= NL_THREADS && NL_THREADS % 4 == 0, "one thread per (order of the tile, field)");

// out[l][n] = j_l(xs[n]), l = 0 .. lmax; one thread per argument
__global__ __launch_bounds__(256) void sph_bessel_kernel(int lmax, int nstart, int nx, const double* __restrict__ xs,
                                                         double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < nx) sb_all(xs[n], lmax, nstart, out + n, (size_t)nx);
}

__global__ __launch_bounds__(NL_THREADS) void nonlimber_transfer_kernel(int F, int ngz, int nkq, int lmax, int nstart,
                                                                        const double* __restrict__ kq,
                                                                        const double* __restrict__ chis,
                                                                        const double* __restrict__ src,
                                                                        double* __restrict__ out) {
    __shared__ double sj[NL_TILE][NL_JPITCH];
    __shared__ double ss[NL_THREADS][NL_SPITCH];
    const int tid = threadIdx.x, i = blockIdx.x;
    const double k = kq[i];
    const int ntiles = lmax / NL_TILE + 1;
    const int lt = tid / F, fo = tid - lt * F;                   // this thread's (order of the tile, field)
    const bool contracts = tid < NL_TILE * F;
    bool wrote = false;                                          // does the output hold a sum already (block-uniform)
    // the tile in sj against the source columns in ss; l0 its first order
    auto contract = [&](int l0, int nlive) {
        const int l = l0 + lt;
        if (contracts && l <= lmax) {
            double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
            const double* row = sj[lt];
            for (int g = 0; g < nlive; g += 4) {                 // (past nlive: zeros on both sides)
                p0 = fma(ss[g][fo], row[g], p0);
                p1 = fma(ss[g + 1][fo], row[g + 1], p1);
                p2 = fma(ss[g + 2][fo], row[g + 2], p2);
                p3 = fma(ss[g + 3][fo], row[g + 3], p3);
            }
            const double sum = (p0 + p1) + (p2 + p3);
            double* o = out + ((size_t)fo * (lmax + 1) + l) * nkq + i;
            *o = wrote ? *o + sum : sum;
        }
    };
#pragma unroll 1
    for (int g0 = 0; g0 < ngz; g0 += NL_THREADS) {
        const int g = g0 + tid, nlive = min(NL_THREADS, ngz - g0);
        const bool live = g < ngz;
        const double x = live ? k * chis[g] : 1.0;
        const bool tiny = !(x >= SB_XMIN), up = x >= (double)lmax;
        __syncthreads();                                         // the previous chunk's tiles and sources have been read
        for (int f = 0; f < F; ++f) ss[tid][f] = live ? src[((size_t)f * ngz + g) * nkq + i] : 0.0;
        const sb_recip rx = sb_recip_of(tiny ? 1.0 : x);
        double j0, j1;
        sb_j01(tiny ? 1.0 : x, rx.h, j0, j1);
        if (tiny) j0 = 1.0, j1 = x * (1.0 / 3.0);
        const bool walks_up = live && (up || tiny), walks_down = live && !up && !tiny;
        // the downward walk's scale and final count
        double s = 0.0;
        int c0 = 0;
        if (walks_down) {
            sb_down d = sb_down_start();
#pragma unroll 1
            for (int l = nstart; l > 0; --l) sb_down_step(d, l, rx);
            s = sb_down_scale(d, j0, j1);
            c0 = d.c;
        }
        const int any_up = __syncthreads_or(walks_up), any_down = __syncthreads_or(walks_down);
        if (any_up) {                                            // phase A: ascending tiles
            sb_up u{j0, j1};
#pragma unroll 1
            for (int t = 0; t < ntiles; ++t) {
#pragma unroll 1
                for (int q = 0; q < NL_TILE; ++q) {
                    const int l = t * NL_TILE + q;
                    sj[q][tid] = walks_up && l <= lmax ? (tiny && l >= 2 ? 0.0 : u.a) : 0.0;
                    if (walks_up && !tiny) sb_up_step(u, l, rx);
                    else if (l == 0) u.a = u.b;                  // (a tiny argument: j_1, then zeros)
                }
                __syncthreads();
                contract(t * NL_TILE, nlive);
                __syncthreads();
            }
            wrote = true;
        }
        if (any_down) {                                          // phase B: descending tiles
            sb_down d = sb_down_start();
            if (walks_down) {
#pragma unroll 1
                for (int l = nstart; l > ntiles * NL_TILE - 1; --l) sb_down_step(d, l, rx);
            }
#pragma unroll 1
            for (int t = ntiles - 1; t >= 0; --t) {
#pragma unroll 1
                for (int q = NL_TILE - 1; q >= 0; --q) {
                    const int l = t * NL_TILE + q;
                    sj[q][tid] = walks_down && l <= lmax ? sb_down_value(d.a, d.c, s, c0) : 0.0;
                    if (walks_down && l > 0) sb_down_step(d, l, rx);
                }
                __syncthreads();
                contract(t * NL_TILE, nlive);
                __syncthreads();
            }
            wrote = true;
        }
    }
}

// C[p][l] = (2/pi) sum_i wk_i kq_i^2 T[a][l][i] T[b][l][i] for the pair p = (a, b): one wavefront per (p, l); lane j sums
// the nodes j, j + 64, ... in ascending order, then the lanes' sums fold 32, 16, 8, 4, 2, 1 apart through LDS.  The
// product T_a T_b is formed first: (a, b) and (b, a) give the same bits.
__global__ __launch_bounds__(64) void nonlimber_cl_kernel(int nkq, int lmax, const int* __restrict__ pairs,
                                                          const double* __restrict__ kq, const double* __restrict__ wk,
                                                          const double* __restrict__ T, double* __restrict__ out) {
    __shared__ double red[64];
    const int l = blockIdx.x, p = blockIdx.y, j = threadIdx.x;
    const double* Ta = T + ((size_t)pairs[2 * p] * (lmax + 1) + l) * nkq;
    const double* Tb = T + ((size_t)pairs[2 * p + 1] * (lmax + 1) + l) * nkq;
    double acc = 0.0;
    for (int i = j; i < nkq; i += 64) acc = fma(wk[i] * (kq[i] * kq[i]), Ta[i] * Tb[i], acc);
    red[j] = acc;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (j < h) red[j] = red[j] + red[j + h];
        __syncthreads();
    }
    if (j == 0) out[(size_t)p * (lmax + 1) + l] = (2.0 / M_PI) * red[0];
}

}  // namespace hmg
