// Angular correlation functions of tabulated spectra: the C-ABI entry points hmg_angular_transform and hmg_angular_zsum
// (include/hmgrid.h) and their kernels (kernels/angular.hpp).  A translation unit of its own: realspace.hip does not
// see these instantiations.  Definition and accuracy: DESIGN.md section 22.
#include "hmctx.hpp"
#include "kernels/angular.hpp"

using namespace hmg;

template <bool W0, bool W2, bool W4>
static void angular_launch(hmg_ctx* c, int rows, int tiles, int nz, int nk, int nt, const double* ks, const double* P,
                           const double* chis, const double* thetas, double* w0, double* w2, double* w4) {
    hipLaunchKernelGGL((angular_transform_kernel<AG_THREADS, AG_TILE, W0, W2, W4>), dim3(rows, tiles), dim3(AG_THREADS),
                       0, c->stream, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4);
}

int hmg_angular_transform(hmg_ctx* c, int n, int nz, int nk, int nt, const double* ks, const double* P,
                          const double* chis, const double* thetas, double* w0, double* w2, double* w4) {
    REQUIRE(c && ks && P && chis && thetas, "NULL argument");
    REQUIRE(w0 || w2 || w4, "no output asked for");
    REQUIRE(n > 0 && nz > 0 && nt > 0, "empty grid");
    REQUIRE((long long)n * nz <= 2147483647LL, "too many rows");
    REQUIRE(nk >= 2, "the transform needs at least two wavenumbers");
    const int rows = n * nz, tiles = (nt - 1) / AG_TILE + 1;
    REQUIRE(tiles <= 65535, "nt too large");
    switch ((w0 ? 1 : 0) | (w2 ? 2 : 0) | (w4 ? 4 : 0)) {
        case 1: angular_launch<true, false, false>(c, rows, tiles, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4); break;
        case 2: angular_launch<false, true, false>(c, rows, tiles, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4); break;
        case 3: angular_launch<true, true, false>(c, rows, tiles, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4); break;
        case 4: angular_launch<false, false, true>(c, rows, tiles, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4); break;
        case 5: angular_launch<true, false, true>(c, rows, tiles, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4); break;
        case 6: angular_launch<false, true, true>(c, rows, tiles, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4); break;
        default: angular_launch<true, true, true>(c, rows, tiles, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_angular_zsum(hmg_ctx* c, int n, int nz, int nt, int nw, const double* zw, const double* w, double* out) {
    REQUIRE(c && zw && w && out, "NULL argument");
    REQUIRE(n > 0 && nz > 0 && nt > 0 && nw > 0, "empty grid");
    const long long total = (long long)n * nw * nt, blocks = (total - 1) / 256 + 1;
    REQUIRE(blocks <= 2147483647LL, "too many outputs");
    hipLaunchKernelGGL(angular_zsum_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, nz, nt, nw, (size_t)total,
                       zw, w, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
