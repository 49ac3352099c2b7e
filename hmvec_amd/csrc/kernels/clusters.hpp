// Cluster number counts: the survey selection of every (z, m) halo in bins of detection significance and its sum over
// the mass function.  Kernels of the unit clusters.hip only.  Needs rowdev.hpp (wave_sum) before it.
//
// A launch holds at most CL_BINS consecutive bins (the entry point walks the chunks).  Order of every sum:
//   1. a pair p = tau G + g of a halo (gaussian), or a tile tau (none), belongs to lane p % 64 of the halo's wavefront;
//      a lane adds its terms in ascending p, one chain per bin;
//   2. the 64 lanes are summed by wave_sum (a balanced tree of depth 6): S_a[z, m];
//   3. the halos of a 64-mass tile (grid index m / 64) are summed by wave_sum, halos outside the window as 0;
//   4. cluster_finish_kernel adds the tiles in ascending order.
// Nothing depends on which other bins or redshifts the call holds, nor on the chunk a bin falls in.
#pragma once

namespace hmg {

constexpr int CL_BINS = 8;          // bins of one launch
constexpr int CL_THREADS = 1024;    // 16 wavefronts: a wavefront owns 4 halos of the tile, one after the other
constexpr int CL_WAVES = CL_THREADS / 64;
constexpr int CL_GAUSSIAN = 0, CL_NONE = 1;

struct ClusterArgs {
    int nz, nm, T, G, kind, m_lo, m_hi;
    int nq_all, a0, nq;             // bins of the call; first bin and bins of this launch
    const double *lnobs, *sigln;    // [nz][nm]
    const double *lnnoise, *area;   // [T]
    const double *t, *w;            // [G]
    const double *edges;            // [nq_all + 1]
    const double *nzm, *bh, *wm;
    double *S;                      // [nz][nm][nq_all] or NULL
    double *part;                   // [nz][ntile][2][nq_all]
};

// One workgroup per (64-mass tile, z).
__global__ __launch_bounds__(CL_THREADS) void cluster_selection_kernel(ClusterArgs A) {
#pragma clang fp contract(off)
    __shared__ double acc[CL_BINS][CL_THREADS];     // a thread's chains, one per bin
    __shared__ double sm[64][CL_BINS];              // S_a of the tile's halos
    __shared__ double ed[CL_BINS + 1];              // the launch's edges (none: their logarithms)
    const int tile = blockIdx.x, z = blockIdx.y, nm = A.nm, nq = A.nq;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ntile = gridDim.x;
    if (tid <= nq) {
        const double e = A.edges[A.a0 + tid];
        ed[tid] = A.kind == CL_GAUSSIAN ? e : log(e);
    }
    __syncthreads();
    const int count = A.kind == CL_GAUSSIAN ? A.T * A.G : A.T;
    for (int i = wv; i < 64; i += CL_WAVES) {
        const int m = tile * 64 + i;
        if (m < A.m_lo || m >= A.m_hi) {            // (wave-uniform)
            if (lane < nq) sm[i][lane] = 0.0;
            continue;
        }
        const size_t idx = (size_t)z * nm + m;
        const double mu = A.lnobs[idx], sg = A.sigln[idx];
        const double scale = A.kind == CL_GAUSSIAN ? 0.70710678118654752440 : 1.0 / (1.41421356237309504880 * sg);
        for (int a = 0; a < nq; ++a) acc[a][tid] = 0.0;
        for (int p = lane; p < count; p += 64) {
            double c, wt;
            if (A.kind == CL_GAUSSIAN) {
                const int tau = p / A.G, g = p - tau * A.G;
                const double x = (mu + sg * A.t[g]) - A.lnnoise[tau];
                c = exp(x);
                wt = A.area[tau] * A.w[g];
            } else {
                c = mu - A.lnnoise[p];
                wt = A.area[p];
            }
            double dp = 0.0, Ep = 0.0;
            bool negp = false;
#pragma unroll 1
            for (int j = 0; j <= nq; ++j) {
                const double d = ed[j] - c;
                const double u = d * scale;
                const double E = erfc(fabs(u));     // <= 1: the tail on the edge's own side
                const bool neg = u < 0.0;
                if (j > 0) {
                    // erfc(a) - erfc(b), or erfc(-b) - erfc(-a) where the halo lies above the bin's middle
                    const bool flip = dp + d < 0.0;
                    const double hi = flip ? (neg ? E : 2.0 - E) : (negp ? 2.0 - Ep : Ep);
                    const double lo = flip ? (negp ? Ep : 2.0 - Ep) : (neg ? 2.0 - E : E);
                    const double P = 0.5 * (hi - lo);
                    acc[j - 1][tid] = acc[j - 1][tid] + wt * P;
                }
                dp = d; Ep = E; negp = neg;
            }
        }
        for (int a = 0; a < nq; ++a) {
            const double s = wave_sum(acc[a][tid]);
            if (lane == 0) sm[i][a] = s;
        }
    }
    __syncthreads();
    for (int a = wv; a < nq; a += CL_WAVES) {       // lane = halo of the tile
        const int m = tile * 64 + lane;
        double tn = 0.0, tb = 0.0;
        if (m < nm) {
            const size_t idx = (size_t)z * nm + m;
            const double s = sm[lane][a];
            if (A.S) A.S[idx * A.nq_all + A.a0 + a] = s;
            if (m >= A.m_lo && m < A.m_hi) {
                tn = A.wm[m] * (A.nzm[idx] * s);
                tb = tn * A.bh[idx];
            }
        }
        const double sn = wave_sum(tn), sb = wave_sum(tb);
        if (lane == 0) {
            double* o = A.part + ((size_t)z * ntile + tile) * 2 * A.nq_all + A.a0 + a;
            o[0] = sn;
            o[A.nq_all] = sb;
        }
    }
}

// n[z][a], bn[z][a]: the tiles in ascending order.  One thread per (z, a).
__global__ __launch_bounds__(256) void cluster_finish_kernel(int nz, int ntile, int nq, const double* __restrict__ part,
                                                             double* __restrict__ n, double* __restrict__ bn) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nz * nq) return;
    const int z = e / nq, a = e - z * nq;
    double sn = 0.0, sb = 0.0;
    for (int tile = 0; tile < ntile; ++tile) {
        const double* p = part + ((size_t)z * ntile + tile) * 2 * nq + a;
        sn += p[0];
        sb += p[nq];
    }
    n[e] = sn;
    bn[e] = sb;
}

}  // namespace hmg
