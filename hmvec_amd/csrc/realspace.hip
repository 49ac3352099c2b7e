// The sine family of the transforms of tabulated spectra: the C-ABI entry points hmg_xi_transform and hmg_xi_multipoles
// (include/hmgrid.h) and their kernel (kernels/realspace.hpp).  A translation unit of its own: no other unit sees these
// instantiations.  Definition and accuracy: DESIGN.md sections 13 and 24.
#include "hmctx.hpp"
#include "kernels/realspace.hpp"

using namespace hmg;

template <bool X0, bool X2, bool X4, bool UNIT = false>
static void xi_launch(hmg_ctx* c, int rows, int tiles, int nk, int ns, const double* ks, const double* P0,
                      const double* P2, const double* P4, long long row_stride, long long node_stride,
                      const double* ss, double* x0, double* x2, double* x4) {
    hipLaunchKernelGGL((xi_multipole_kernel<XI_THREADS, XI_TILE, X0, X2, X4, UNIT>), dim3(rows, tiles), dim3(XI_THREADS), 0,
                       c->stream, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, c->d_sici, x0, x2, x4);
}

int hmg_xi_transform(hmg_ctx* c, int rows, int nk, int nr, const double* ks, const double* P, const double* rs,
                     double* out) {
    REQUIRE(c && ks && P && rs && out, "NULL argument");
    REQUIRE(rows > 0 && nr > 0, "empty grid");
    REQUIRE(nk >= 2, "the transform needs at least two wavenumbers");
    const int tiles = (nr - 1) / XI_TILE + 1;
    REQUIRE(tiles <= 65535, "nr too large");
    xi_launch<true, false, false, true>(c, rows, tiles, nk, nr, ks, P, nullptr, nullptr, nk, 1, rs, out, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
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
    const int tiles = (ns - 1) / XI_TILE + 1;
    REQUIRE(tiles <= 65535, "ns too large");
    with_flags([&](auto X0, auto X2, auto X4) {
        if constexpr (X0() || X2() || X4())
            xi_launch<X0(), X2(), X4()>(c, rows, tiles, nk, ns, ks, P0, P2, P4, row_stride, node_stride, ss, x0, x2, x4);
    }, x0, x2, x4);
    HIP_TRY(hipGetLastError());
    return 0;
}
