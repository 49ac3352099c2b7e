// Response of halo-model spectra to a long-wavelength density mode and the super-sample covariance built from it
// (DESIGN.md section 17):
//     R_ab[z,s]      = scale [ (47/21 - n_s/3) P2h + D I1 - (beta_a + beta_b) (P2h + D A1) ]
//     A1 = sum_m wm nzm S_ab,   I1 = sum_m wm nzm bh S_ab,   P2h = P_s J_a J_b
//     Cov[p,i,q,j]   = sum_z g[z] r[p,z,i] r[q,z,j],   r[p,z,s] = zscale[p][z] R_p[z,s]
// S_ab the sampled square term of get_power_1halo (kernels/square_term.hpp, the code the trispectrum integrates), J, P,
// D from the leg prepass and beta from the leg sums (both sampled.hip's), the form of a leg from kernels/leg_form.hpp.
// Included by response.hip alone (its own translation unit: the other units do not see these kernels).
#pragma once
#include "leg_form.hpp"
#include "square_term.hpp"

namespace hmg {

constexpr int RESP_THREADS = 256;   // samples per workgroup: one (pair, z) each, n <= RESP_THREADS
constexpr int RESP_CHUNK = 128;     // mass bins staged through LDS at a time: 128 * (2 * 5 + 2) * 8 B = 12 KB
constexpr int RESP_MAXP = 16;       // pairs per call
constexpr int SSC_TILE = 64;        // rows per tile side
constexpr int SSC_THREADS = 256;    // 16 x 16 threads, a 4 x 4 register block each
constexpr int SSC_ZCHUNK = 32;      // redshifts staged through LDS at a time: 2 * 32 * 64 * 8 B = 32 KB

struct RespPair {                   // one spectrum of the request, read from device memory by its workgroups
    TriSide S;                      // its square term
    int la, lb;                     // its legs among the distinct legs of the call: rows of J and beta
};
struct RespArgs {
    const RespPair* pairs;          // [np]
    HaloGrid g;                     // (ks, Pzk are read by the leg prepass alone)
    SampleTable s;
    const double* dlnP;             // [nz][nk]
    const double *J;                // [nu][nz][n] by distinct leg
    const double *beta;             // [nu][nz]
    const double *Ps, *Ds;          // [nz][n]
    double* R;                      // [np][nz][n]
    double* parts;                  // [3][np][nz][n] = (A1, I1, P2h), or NULL
    int np;
};

// grid (np, nz), RESP_THREADS threads: thread s owns sample s of pair blockIdx.x at redshift blockIdx.y and walks the
// whole mass axis in order with two accumulators - no split over workgroups, no atomics: a result depends on its own
// (pair, z, s), the tables and the tensors alone.  A wave's lanes are consecutive samples of one mass bin: their loads
// fall in one tensor row.  The two linear forms of the square term and the weights wm nzm, wm nzm bh of a chunk of
// mass bins are formed once, one thread per bin, and staged through LDS.  The pair's description is read through the
// uniform block index (scalar loads: nothing is indexed at run time in the argument block).
__global__ __launch_bounds__(RESP_THREADS) void response_pairs_kernel(RespArgs A) {
    __shared__ double cf[RESP_CHUNK * 2 * TRI_NC], sW[RESP_CHUNK], sWb[RESP_CHUNK];
    const int tid = threadIdx.x, p = blockIdx.x, z = blockIdx.y;
    const TriSide S = A.pairs[p].S;
    const bool live = tid < A.s.n;
    const size_t o = (size_t)z * A.s.n + tid;
    int id = 0;
    double f = 0.0;
    if (live) { id = A.s.idx[o]; f = A.s.frac[o]; }
    double a1 = 0.0, i1 = 0.0;
    for (int m0 = 0; m0 < A.g.nm; m0 += RESP_CHUNK) {
        const int mc = min(RESP_CHUNK, A.g.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed
        if (tid < mc) {
            const size_t zm = (size_t)z * A.g.nm + m0 + tid;
            tri_square_forms(S, zm, z, A.g.ms[m0 + tid], A.g.rho_m0, cf + tid * (2 * TRI_NC), cf + tid * (2 * TRI_NC) + TRI_NC);
            const double wn = A.g.wm[m0 + tid] * A.g.nzm[zm];
            sW[tid] = wn;
            sWb[tid] = wn * A.g.bh[zm];
        }
        __syncthreads();
        if (live) {
            const size_t at0 = ((size_t)z * A.g.nm + m0) * (size_t)A.g.nk + id;
            for (int ml = 0; ml < mc; ++ml) {
                const double* x1 = cf + ml * (2 * TRI_NC);
                const double* x2 = x1 + TRI_NC;
                const size_t at = at0 + (size_t)ml * A.g.nk;
                double s = tri_square_at(S, x1, x2, at);
                if (f != 0.0) s = fma(f, tri_square_at(S, x1, x2, at + 1), (1.0 - f) * s);   // node id + 1 is read only here
                a1 = fma(s, sW[ml], a1);
                i1 = fma(s, sWb[ml], i1);
            }
        }
    }
    if (!live) return;
    {   // the epilogue, every operation rounded by itself in the order of the definition
#pragma clang fp contract(off)
    const int la = A.pairs[p].la, lb = A.pairs[p].lb;
    const size_t zn = (size_t)A.g.nz * A.s.n;
    const double* dl = A.dlnP + (size_t)z * A.g.nk;
    double ns = dl[id];
    if (f != 0.0) ns = fma(f, dl[id + 1], (1.0 - f) * ns);
    const double p2h = A.Ps[o] * A.J[la * zn + o] * A.J[lb * zn + o];
    const double D = A.Ds[o];
    const double bsum = A.beta[(size_t)la * A.g.nz + z] + A.beta[(size_t)lb * A.g.nz + z];
    const double growth = (47.0 / 21.0 - ns / 3.0) * p2h;
    const double halo = D * i1;
    const double mean = bsum * (p2h + D * a1);
    const size_t e = (size_t)p * zn + o;
    A.R[e] = A.s.scale[o] * ((growth + halo) - mean);
    if (A.parts) {
        const size_t plane = (size_t)A.np * zn;
        A.parts[e] = a1;
        A.parts[plane + e] = i1;
        A.parts[2 * plane + e] = p2h;
    }
    }
}

// Cov[a,b] = sum_z g[z] r[a,z] r[b,z] over the N = np n rows a = p n + i, r[a,z] = zscale[p][z] R[p][z][i] (zscale NULL:
// R itself).  grid (tiles of b, tiles of a), SSC_THREADS threads: a workgroup owns a 64 x 64 tile, a thread a 4 x 4
// block of it; the rows of both sides for SSC_ZCHUNK redshifts at a time are staged through LDS and the z loop runs in
// order.  The weight multiplies the product of the two sides (it is on neither): exchanging the sides gives the same
// bits, so Cov[a,b] has the bits of Cov[b,a] without a mirror pass.
__global__ __launch_bounds__(SSC_THREADS) void ssc_kernel(int nz, int n, int N, const double* __restrict__ R,
                                                          const double* __restrict__ zscale,
                                                          const double* __restrict__ g, double* __restrict__ cov) {
    __shared__ __align__(16) double sA[SSC_ZCHUNK * SSC_TILE], sB[SSC_ZCHUNK * SSC_TILE];
    __shared__ double sG[SSC_ZCHUNK];
    const int tid = threadIdx.x;
    const int a0 = blockIdx.y * SSC_TILE, b0 = blockIdx.x * SSC_TILE;
    const int tx = tid & 15, ty = tid >> 4;
    const int il = tid & (SSC_TILE - 1), w = tid >> 6;
    const int ra = a0 + il, rb = b0 + il;
    const bool liveA = ra < N, liveB = rb < N;
    const int pa = liveA ? ra / n : 0, ia = liveA ? ra - pa * n : 0;
    const int pb = liveB ? rb / n : 0, ib = liveB ? rb - pb * n : 0;

    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;

    for (int z0 = 0; z0 < nz; z0 += SSC_ZCHUNK) {
        const int zc = min(SSC_ZCHUNK, nz - z0);
        __syncthreads();                       // the previous chunk has been consumed
        if (tid < zc) sG[tid] = g[z0 + tid];
        for (int zl = w; zl < zc; zl += SSC_THREADS / SSC_TILE) {
            const int z = z0 + zl;
            double va = 0.0, vb = 0.0;
            if (liveA) {
                va = R[((size_t)pa * nz + z) * n + ia];
                if (zscale) va = zscale[(size_t)pa * nz + z] * va;
            }
            if (liveB) {
                vb = R[((size_t)pb * nz + z) * n + ib];
                if (zscale) vb = zscale[(size_t)pb * nz + z] * vb;
            }
            sA[zl * SSC_TILE + il] = va;
            sB[zl * SSC_TILE + il] = vb;
        }
        __syncthreads();
        for (int zl = 0; zl < zc; ++zl) {
            const double gz = sG[zl];
            const double2 a01 = *reinterpret_cast<const double2*>(&sA[zl * SSC_TILE + ty * 4]);
            const double2 a23 = *reinterpret_cast<const double2*>(&sA[zl * SSC_TILE + ty * 4 + 2]);
            const double2 b01 = *reinterpret_cast<const double2*>(&sB[zl * SSC_TILE + tx * 4]);
            const double2 b23 = *reinterpret_cast<const double2*>(&sB[zl * SSC_TILE + tx * 4 + 2]);
            const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r] * b[c], gz, acc[r][c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int a = a0 + ty * 4 + r;
        if (a >= N) continue;
        double* out = cov + (size_t)a * N;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int b = b0 + tx * 4 + c;
            if (b < N) out[b] = acc[r][c];
        }
    }
}

}  // namespace hmg
