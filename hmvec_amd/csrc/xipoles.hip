// Redshift-space correlation multipoles of tabulated multipole spectra: the C-ABI entry point hmg_xi_multipoles
// (include/hmgrid.h) and its kernel (kernels/xipoles.hpp).  A translation unit of its own: realspace.hip does not see
// these instantiations.  Definition and accuracy: DESIGN.md section 24.
#include "hmctx.hpp"
#include "kernels/xipoles.hpp"

using namespace hmg;

template <bool X0, bool X2, bool X4>
static void xipoles_launch(hmg_ctx* c, int rows, int tiles, int nk, int ns, const double* ks, const double* P0,
                           const double* P2, const double* P4, long long row_stride, long long node_stride,
                           const double* ss, double* x0, double* x2, double* x4) {
    hipLaunchKernelGGL((xi_multipole_kernel<XP_THREADS, XP_TILE, X0, X2, X4>), dim3(rows, tiles), dim3(XP_THREADS), 0,
                       c->stream, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, c->d_sici, x0, x2, x4);
}

int hmg_xi_multipoles(hmg_ctx* c, int rows, int nk, int ns, const double* ks, const double* P0, const double* P2,
                      const double* P4, long long row_stride, long long node_stride, const double* ss, double* x0,
                      double* x2, double* x4) {
    REQUIRE(c && ks && ss, "NULL argument");
    REQUIRE(x0 || x2 || x4, "no output asked for");
    REQUIRE((!x0 || P0) && (!x2 || P2) && (!x4 || P4), "an order that is asked for needs its input rows");
    REQUIRE(rows > 0 && ns > 0, "empty grid");
    REQUIRE(nk >= 2, "the transform needs at least two wavenumbers");
    REQUIRE(node_stride >= 1, "node_stride must be at least 1");
    REQUIRE(node_stride <= (9223372036854775807LL - 1) / (nk - 1) && row_stride >= (nk - 1) * node_stride + 1,
            "row_stride is shorter than a row");
    REQUIRE(row_stride <= 9223372036854775807LL / 8 / rows, "rows times row_stride overflows");
    const int tiles = (ns - 1) / XP_TILE + 1;
    REQUIRE(tiles <= 65535, "ns too large");
    switch ((x0 ? 1 : 0) | (x2 ? 2 : 0) | (x4 ? 4 : 0)) {
        case 1: xipoles_launch<true, false, false>(c, rows, tiles, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, x0, x2, x4); break;
        case 2: xipoles_launch<false, true, false>(c, rows, tiles, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, x0, x2, x4); break;
        case 3: xipoles_launch<true, true, false>(c, rows, tiles, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, x0, x2, x4); break;
        case 4: xipoles_launch<false, false, true>(c, rows, tiles, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, x0, x2, x4); break;
        case 5: xipoles_launch<true, false, true>(c, rows, tiles, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, x0, x2, x4); break;
        case 6: xipoles_launch<false, true, true>(c, rows, tiles, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, x0, x2, x4); break;
        default: xipoles_launch<true, true, true>(c, rows, tiles, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, x0, x2, x4); break;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
