// The small kernels that the units which contract the profile tensors at sampled wavenumbers share - the table check,
// the weighted z sum, the leg prepass and the leg sums - and their launchers (declared in kernels/sampled.hpp).  A
// translation unit of its own: trispectrum.hip, bispectrum.hip, response.hip and rsd.hip launch these through the
// launchers and do not depend on one another.  Definitions and resources: DESIGN.md sections 15, 16, 17 and 19.
#include "hmctx.hpp"
#include "kernels/leg_form.hpp"

using namespace hmg;

namespace hmg {

// raises *bad (a plain store) if a sample's table entry is not usable; one thread per (z, sample)
__global__ __launch_bounds__(256) void sample_check_kernel(size_t count, int nk, const int* __restrict__ idx,
                                                           const double* __restrict__ frac, int* __restrict__ bad) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    if (!bis_sample_ok(idx[e], frac[e], nk)) *bad = 1;
}

// out[p stride + t] = sum_z g[z] src[(p nz + z) stride + t], z in order; one thread per element
__global__ __launch_bounds__(256) void zsum_kernel(int nz, size_t count, size_t stride, const double* __restrict__ g,
                                                   const double* __restrict__ src, double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const size_t p = e / stride, t = e - p * stride;
    src += p * (size_t)nz * stride + t;
    double s = 0.0;
    for (int z = 0; z < nz; ++z) s = fma(g[z], src[(size_t)z * stride], s);
    out[e] = s;
}

// Leg prepass, one launch per distinct leg; J is written once per leg of the request that is this tracer: legs of one
// tracer have the same bits.  grid nz, BIS_THREADS threads: thread s owns sample s at redshift blockIdx.x and walks the
// mass axis in order, I = sum_m wm nzm bh w(z,m,s); the k -> 0 sum C and the HOD bias sum are block sums over per-thread
// strided partial sums, as power_prep_kernel forms them.  J = (I + b) - C is the bracket of P_2h.  A launch with out.Ps
// also samples P_lin, the wavenumber and the damping factor.
__global__ __launch_bounds__(BIS_THREADS) void leg_prepass_kernel(HaloGrid g, BisLeg L, const int* __restrict__ idx,
                                                                  const double* __restrict__ frac, int n, double kstar,
                                                                  LegOut out) {
    __shared__ double cf[BIS_PREP_CHUNK * 3], sWb[BIS_PREP_CHUNK], red[BIS_THREADS];
    const int tid = threadIdx.x, z = blockIdx.x;
    const bool live = tid < n;
    int id = 0;
    double f = 0.0;
    if (live) { id = idx[(size_t)z * n + tid]; f = frac[(size_t)z * n + tid]; }
    double accI = 0.0, accC = 0.0, accB = 0.0;
    for (int m0 = 0; m0 < g.nm; m0 += BIS_PREP_CHUNK) {
        const int mc = min(BIS_PREP_CHUNK, g.nm - m0);
        __syncthreads();                       // the previous chunk has been consumed
        if (tid < mc) {
            const size_t zm = (size_t)z * g.nm + m0 + tid;
            const double wnb = g.wm[m0 + tid] * g.nzm[zm] * g.bh[zm];
            double lowk, ngals;
            bis_leg_form(L, zm, z, g.ms[m0 + tid], g.rho_m0, cf + 3 * tid, lowk, ngals);
            sWb[tid] = wnb;
            accC = fma(wnb, lowk, accC);
            accB = fma(wnb, ngals, accB);
        }
        __syncthreads();
        if (live) {
            const size_t at = ((size_t)z * g.nm + m0) * (size_t)g.nk + id;
            for (int ml = 0; ml < mc; ++ml)
                accI = fma(sWb[ml], bis_leg_at(L, cf + 3 * ml, at + (size_t)ml * g.nk, f), accI);
        }
    }
    const double C = bis_block_sum(accC, red);
    const double Bs = bis_block_sum(accB, red);
    if (!live) return;
    const double b = L.kind == HMG_TRACER_MATTER ? 1.0 : L.kind == HMG_TRACER_PRESSURE ? 0.0 : Bs / L.ngal[z];
    const size_t o = (size_t)z * n + tid;
    const double J = (accI + b) - C;
#pragma unroll
    for (int l = 0; l < 3; ++l)
        if (out.J[l]) out.J[l][o] = J;
    if (out.Ps) {
        const double* P = g.Pzk + (size_t)z * g.nk;
        double ps = P[id];
        if (f != 0.0) ps = fma(f, P[id + 1], (1.0 - f) * ps);
        const double k = bis_sample_k(g.ks, id, f);
        out.Ps[o] = ps;
        out.Ks[o] = k;
        out.Ds[o] = kstar > 0.0 ? bis_damping(k, kstar) : 1.0;
    }
}

// C = sum_m wm nzm bh lowk, C0 = sum_m wm nzm lowk and b (sum_m wm nzm bh (Nc + Ns) / ngal of an HOD, b_other of any other
// name) of one leg: they depend neither on k nor on mu.  Per-thread strided partial sums over steps of BIS_PREP_CHUNK,
// then the block sum - the order in which the leg prepass forms C and b: the same bits.  A kernel of its own: the prepass
// keeps J = (I + b) - C and not its terms.  grid nz, BIS_THREADS threads.
__global__ __launch_bounds__(BIS_THREADS) void leg_sums_kernel(HaloGrid g, BisLeg L, double b_other, size_t plane,
                                                               double* __restrict__ out) {
    __shared__ double red[BIS_THREADS];
    const int tid = threadIdx.x, z = blockIdx.x;
    double accC = 0.0, accC0 = 0.0, accB = 0.0;
    for (int m0 = 0; m0 < g.nm; m0 += BIS_PREP_CHUNK) {
        if (tid < min(BIS_PREP_CHUNK, g.nm - m0)) {
            const size_t zm = (size_t)z * g.nm + m0 + tid;
            const double wn = g.wm[m0 + tid] * g.nzm[zm];
            const double wnb = wn * g.bh[zm];
            double c[3], lowk, ngals;
            bis_leg_form(L, zm, z, g.ms[m0 + tid], g.rho_m0, c, lowk, ngals);
            accC = fma(wnb, lowk, accC);
            accC0 = fma(wn, lowk, accC0);
            accB = fma(wnb, ngals, accB);
        }
    }
    const double C = bis_block_sum(accC, red);
    const double C0 = bis_block_sum(accC0, red);
    const double Bs = bis_block_sum(accB, red);
    if (tid == 0) {
        out[z] = C;
        out[plane + z] = C0;
        out[2 * plane + z] = L.kind == HMG_TRACER_HOD ? Bs / L.ngal[z] : b_other;
    }
}

}  // namespace hmg

int hmg::samples_checked(hmg_ctx* c, const SampleTable& table, int nz, int nk, int* d_bad) {
    const size_t count = (size_t)nz * table.n;
    int bad = 0;
    if (check_words(c, d_bad, &bad, 1, [&] {
            hipLaunchKernelGGL(sample_check_kernel, grid1d(count, 256), dim3(256), 0, c->stream, count, nk, table.idx,
                               table.frac, d_bad);
        }))
        return 1;
    REQUIRE(!bad, BAD_SAMPLE_TABLE);
    return 0;
}

int hmg::zsum_launch(hmg_ctx* c, int nz, size_t count, size_t stride, const double* g, const double* src, double* out) {
    hipLaunchKernelGGL(zsum_kernel, grid1d(count, 256), dim3(256), 0, c->stream, nz, count, stride, g, src, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg::leg_prepass_launch(hmg_ctx* c, const HaloGrid& g, const BisLeg& L, const int* idx, const double* frac, int n,
                            double kstar, const LegOut& out) {
    hipLaunchKernelGGL(leg_prepass_kernel, dim3(g.nz), dim3(BIS_THREADS), 0, c->stream, g, L, idx, frac, n, kstar, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg::leg_sums_launch(hmg_ctx* c, const HaloGrid& g, const BisLeg& L, double b_other, size_t plane, double* out) {
    hipLaunchKernelGGL(leg_sums_kernel, dim3(g.nz), dim3(BIS_THREADS), 0, c->stream, g, L, b_other, plane, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
