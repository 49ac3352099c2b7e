// Configuration-space statistics of tabulated spectra: the C-ABI entry points hmg_xi_transform and hmg_hankel_transform
// (include/hmgrid.h) and their kernels (kernels/realspace.hpp).  A translation unit of its own: the headline path's
// units do not see these instantiations.  Definition and accuracy: DESIGN.md sections 13 and 14.
#include "hmctx.hpp"
#include "kernels/realspace.hpp"

using namespace hmg;

int hmg_xi_transform(hmg_ctx* c, int rows, int nk, int nr, const double* ks, const double* P, const double* rs,
                     double* out) {
    REQUIRE(c && ks && P && rs && out, "NULL argument");
    REQUIRE(rows > 0 && nr > 0, "empty grid");
    REQUIRE(nk >= 2, "the transform needs at least two wavenumbers");
    const int tiles = (nr - 1) / XI_TILE + 1;
    REQUIRE(tiles <= 65535, "nr too large");
    hipLaunchKernelGGL((xi_transform_kernel<XI_THREADS, XI_TILE>), dim3(rows, tiles), dim3(XI_THREADS), 0, c->stream,
                       nk, nr, ks, P, rs, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <bool W0, bool W2>
static void hankel_launch(hmg_ctx* c, int rows, int tiles, int nk, int nr, const double* ks, const double* P,
                          const double* rs, double* w0, double* w2) {
    hipLaunchKernelGGL((hankel_transform_kernel<HK_THREADS, HK_TILE, W0, W2>), dim3(rows, tiles), dim3(HK_THREADS), 0,
                       c->stream, nk, nr, ks, P, rs, w0, w2);
}

int hmg_hankel_transform(hmg_ctx* c, int rows, int nk, int nr, const double* ks, const double* P, const double* rs,
                         double* w0, double* w2) {
    REQUIRE(c && ks && P && rs, "NULL argument");
    REQUIRE(w0 || w2, "no output asked for");
    REQUIRE(rows > 0 && nr > 0, "empty grid");
    REQUIRE(nk >= 2, "the transform needs at least two wavenumbers");
    const int tiles = (nr - 1) / HK_TILE + 1;
    REQUIRE(tiles <= 65535, "nr too large");
    if (w0 && w2) hankel_launch<true, true>(c, rows, tiles, nk, nr, ks, P, rs, w0, w2);
    else if (w0) hankel_launch<true, false>(c, rows, tiles, nk, nr, ks, P, rs, w0, w2);
    else hankel_launch<false, true>(c, rows, tiles, nk, nr, ks, P, rs, w0, w2);
    HIP_TRY(hipGetLastError());
    return 0;
}
