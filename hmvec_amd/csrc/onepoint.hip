// One-point statistics of a sum of halo profiles: the C-ABI entry points hmg_onepoint_exponent and hmg_onepoint_moments
// (include/hmgrid.h) and their kernels (kernels/onepoint.hpp).  A translation unit of its own: the other units do not see
// these instantiations, and theirs do not change.  Definition, gates and resources: DESIGN.md section 20.
#include <cmath>

#include "hmctx.hpp"
#include "kernels/onepoint.hpp"

using namespace hmg;

namespace {

// the checks both entry points share
int onepoint_checked(hmg_ctx* c, const OnepointArgs& A) {
    REQUIRE(c && A.signal && A.area && A.nzm && A.wm && A.zw, "NULL argument");
    REQUIRE(A.nz >= 1 && A.nm >= 1 && A.nt >= 1, "empty grid");
    REQUIRE(A.m_lo >= 0 && A.m_lo < A.m_hi, "empty mass window: 0 <= m_lo < m_hi is required");
    REQUIRE(A.m_hi <= A.nm, "mass window past the grid: m_hi <= nm is required");
    REQUIRE(A.nz <= 65535, "nz too large");
    REQUIRE((long long)(A.m_hi - A.m_lo) * A.nt <= 2147483647LL - 8 * OP_SLICE, "too many samples per redshift");
    return 0;
}

}  // namespace

int hmg_onepoint_exponent(hmg_ctx* c, int nz, int nm, int nt, const double* signal, const double* area, const double* amp,
                          const double* nzm, const double* wm, const double* zw, int m_lo, int m_hi, int nlambda,
                          double dlambda, double* rows, double* total) {
    OnepointArgs A = {nz, nm, nt, m_lo, m_hi, signal, area, amp, nzm, wm, zw, nlambda, 1, dlambda, rows};
    if (onepoint_checked(c, A)) return 1;
    REQUIRE(rows, "d_rows is NULL: no output");
    REQUIRE(nlambda >= 1, "empty grid: nlambda >= 1 is required");
    REQUIRE(std::isfinite(dlambda) && dlambda > 0.0, "dlambda must be finite and positive");
    REQUIRE((long long)nz * 2 * nlambda <= 2147483647LL, "output too large");
    A.split = onepoint_split((long long)(m_hi - m_lo) * nt);
    const int n = 2 * nlambda;
    const dim3 grid(nlambda > 1 ? (nlambda - 2) / OP_TILE + 1 : 1, nz, A.split);       // (tiles of j = 1 .. nlambda - 1)
    const auto finish = [&](const double* parts) {
        if (A.split == 1 && !total) return 0;
        hipLaunchKernelGGL(onepoint_finish_kernel, grid1d(n, 256), dim3(256), 0, c->stream, nz, n, A.split, parts, rows, total);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if (A.split == 1) {
        hipLaunchKernelGGL(onepoint_exponent_kernel, grid, dim3(OP_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        return finish(rows);
    }
    // the slices' shares are a temporary of the call
    return with_block(c, sizeof(double) * A.split * nz * n, [&](void* blk) {
        A.out = (double*)blk;
        hipLaunchKernelGGL(onepoint_exponent_kernel, grid, dim3(OP_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        return finish(A.out);
    });
}

int hmg_onepoint_moments(hmg_ctx* c, int nz, int nm, int nt, const double* signal, const double* area, const double* amp,
                         const double* nzm, const double* wm, const double* zw, int m_lo, int m_hi, double* rows,
                         double* total) {
    const OnepointArgs A = {nz, nm, nt, m_lo, m_hi, signal, area, amp, nzm, wm, zw, 0, 1, 0.0, rows};
    if (onepoint_checked(c, A)) return 1;
    REQUIRE(rows, "d_rows is NULL: no output");
    hipLaunchKernelGGL(onepoint_moments_kernel, dim3(nz), dim3(OP_THREADS), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    if (total) {
        hipLaunchKernelGGL(onepoint_finish_kernel, grid1d(4, 64), dim3(64), 0, c->stream, nz, 4, 1, rows, rows, total);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
