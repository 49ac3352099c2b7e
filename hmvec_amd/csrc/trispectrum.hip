// 1-halo trispectrum of two halo-model spectra: the C-ABI entry point hmg_trispectrum_1h (include/hmgrid.h) and its
// kernels (kernels/trispectrum.hpp).  A translation unit of its own: the headline path's units do not see these
// instantiations.  Definition, gate and resources: DESIGN.md section 15.
#include "hmctx.hpp"
#include "kernels/trispectrum.hpp"

using namespace hmg;

// the launches of one call; d_bad is a device word of the caller's
static int tri_run(hmg_ctx* c, TriArgs& A, int nz, int nm, int nk, int n, int tiles, const double* nzm, const double* ms,
                   const double* wm, double rho_m0, const int* idx, const double* frac, const double* scale,
                   const double* zweights, double* T, double* Tz, int* d_bad) {
    const size_t nn = (size_t)n * n;
    // the tables are checked on the device before anything reads a tensor through them
    const size_t count = (size_t)nz * n;
    int bad = 0;
    HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(trispectrum_check_kernel, grid1d(count, 256), dim3(256), 0, c->stream, count, nk, idx, frac, d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    REQUIRE(!bad, "a sample's left node is outside 0 .. nk-1, its fraction outside [0, 1], or it is node nk-1 with a "
                  "non-zero fraction");
    A.nzm = nzm; A.ms = ms; A.wm = wm; A.rho_m0 = rho_m0;
    A.idx = idx; A.frac = frac; A.scale = scale; A.T = T;
    A.nm = nm; A.nk = nk; A.n = n;
    hipLaunchKernelGGL(trispectrum_1h_kernel, dim3(tiles, tiles, nz), dim3(TRI_THREADS), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    if (Tz) {
        hipLaunchKernelGGL(trispectrum_zsum_kernel, grid1d(nn, 256), dim3(256), 0, c->stream, nz, nn, zweights, T, Tz);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int hmg_trispectrum_1h(hmg_ctx* c, int nz, int nm, int nk, int n, const hmg_tracer* ta, const hmg_tracer* tb,
                       const hmg_tracer* tc, const hmg_tracer* td, const double* nzm, const double* ms,
                       const double* wm, double rho_m0, const int* idx, const double* frac, const double* scale,
                       const double* zweights, double* T, double* Tz) {
    REQUIRE(c && ta && tb && tc && td && nzm && ms && wm && idx && frac && scale, "NULL argument");
    REQUIRE(T || Tz, "no output requested");
    REQUIRE(!Tz || zweights, "d_Tz needs d_zweights");
    REQUIRE(nz > 0 && nm > 0 && nk > 0, "empty grid");
    REQUIRE(n >= 1, "no sample points");
    REQUIRE(nz <= 65535, "nz too large");
    const int tiles = (n - 1) / TRI_TILE + 1;
    REQUIRE(tiles <= 65535, "n too large");
    REQUIRE(!c->capturing, "hmg_trispectrum_1h waits on the host for its table check and cannot be part of a captured step");
    for (const hmg_tracer* t : {ta, tb, tc, td})       // (an NFW tensor with deferred series tiles is filled first)
        if (series_ensure_whole(c, t->d_prof) || series_ensure_whole(c, t->d_cprof)) return 1;
    TriArgs A;
    if (tri_side(ta, tb, &A.ab)) return 1;
    if (tri_side(tc, td, &A.cd)) return 1;
    // The word of the table check and, when only the z sum is asked for, the per-z matrices are ordinary blocks of the
    // context's allocator (no scratch arena grows here: a captured step may have an arena's address baked in).  They go
    // back to the free list before this returns; whatever reuses them is enqueued behind the kernels below.
    const size_t nn = (size_t)n * n;
    void* blk = nullptr;
    if (hmg_malloc(c, 64 + (T ? 0 : (size_t)nz * nn * 8), &blk)) return 1;
    int* d_bad = (int*)blk;
    if (!T) T = (double*)((char*)blk + 64);
    const int rc = tri_run(c, A, nz, nm, nk, n, tiles, nzm, ms, wm, rho_m0, idx, frac, scale, zweights, T, Tz, d_bad);
    return hmg_free(c, blk) || rc;
}
