// Configuration-space statistics of tabulated spectra: the C-ABI entry point hmg_xi_transform (include/hmgrid.h) and
// its kernel (kernels/realspace.hpp).  A translation unit of its own: the headline path's units do not see this
// instantiation.  Definition and accuracy: DESIGN.md section 13.
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
