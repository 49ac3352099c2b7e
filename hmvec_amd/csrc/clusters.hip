// Cluster number counts: the C-ABI entry point hmg_cluster_selection (include/hmgrid.h) and its kernels
// (kernels/clusters.hpp).  A translation unit of its own: the other units do not see these instantiations, and theirs do
// not change.  Definition, order of the sums, gates and resources: DESIGN.md section 25.
#include "hmctx.hpp"
#include "rowdev.hpp"
#include "kernels/clusters.hpp"

using namespace hmg;

int hmg_cluster_selection(hmg_ctx* c, int nz, int nm, int T, int G, int nq, int kind, const double* lnobs,
                          const double* sigln, const double* lnnoise, const double* area, const double* t, const double* w,
                          const double* edges, int m_lo, int m_hi, const double* nzm, const double* bh, const double* wm,
                          double* n, double* bn, double* S) {
    REQUIRE(c && lnobs && sigln && lnnoise && area && t && w && edges && nzm && bh && wm, "NULL argument");
    REQUIRE(n && bn, "d_n or d_bn is NULL: no output");
    REQUIRE(kind == CL_GAUSSIAN || kind == CL_NONE, "kind must be 0 (gaussian) or 1 (none)");
    REQUIRE(nz >= 1 && nm >= 1 && T >= 1 && G >= 1 && nq >= 1, "empty grid, no tile, no node or no bin");
    REQUIRE(m_lo >= 0 && m_lo < m_hi, "empty mass window: 0 <= m_lo < m_hi is required");
    REQUIRE(m_hi <= nm, "mass window past the grid: m_hi <= nm is required");
    REQUIRE(nz <= 65535, "nz too large");
    REQUIRE((long long)T * G <= 2147483647LL - 64, "too many (tile, node) pairs");
    REQUIRE((long long)nz * nm <= 2147483647LL / nq, "output too large");
    const int ntile = (nm + 63) / 64;
    return with_block(c, sizeof(double) * 2 * (size_t)nz * ntile * nq, [&](void* blk) {
        ClusterArgs A = {nz, nm, T, G, kind, m_lo, m_hi, nq, 0, 0, lnobs, sigln, lnnoise, area, t, w, edges, nzm, bh, wm, S,
                         (double*)blk};
        for (A.a0 = 0; A.a0 < nq; A.a0 += CL_BINS) {
            A.nq = nq - A.a0 < CL_BINS ? nq - A.a0 : CL_BINS;
            hipLaunchKernelGGL(cluster_selection_kernel, dim3(ntile, nz), dim3(CL_THREADS), 0, c->stream, A);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(cluster_finish_kernel, grid1d((size_t)nz * nq, 256), dim3(256), 0, c->stream, nz, ntile, nq,
                           (const double*)blk, n, bn);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
