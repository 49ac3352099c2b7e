// 1-halo trispectrum of two halo-model spectra: the C-ABI entry point hmg_trispectrum_1h (include/hmgrid.h) and its
// kernels (kernels/trispectrum.hpp).  A translation unit of its own: the headline path's units do not see these
// instantiations.  Definition, gate and resources: DESIGN.md section 15.
#include "hmctx.hpp"
#include "kernels/trispectrum.hpp"

using namespace hmg;

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
    const hmg_tracer* tr[4] = {ta, tb, tc, td};
    if (tracers_ensure_whole(c, tr, 4)) return 1;
    TriArgs A;
    if (tri_side(ta, tb, &A.ab)) return 1;
    if (tri_side(tc, td, &A.cd)) return 1;
    A.g = {nz, nm, nk, nzm, nullptr, ms, wm, nullptr, nullptr, rho_m0};
    A.s = {idx, frac, scale, n};
    // the block: the word of the table check and, when only the z sum is asked for, the per-z matrices
    const size_t nn = (size_t)n * n;
    return with_block(c, 64 + (T ? 0 : (size_t)nz * nn * 8), [&](void* blk) {
        if (samples_checked(c, A.s, nz, nk, (int*)blk)) return 1;
        A.T = T ? T : (double*)((char*)blk + 64);
        hipLaunchKernelGGL(trispectrum_1h_kernel, dim3(tiles, tiles, nz), dim3(TRI_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        return Tz ? zsum_launch(c, nz, nn, nn, zweights, A.T, Tz) : 0;
    });
}
