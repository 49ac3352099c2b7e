// The Bessel family of the transforms of tabulated spectra: the C-ABI entry points hmg_hankel_transform,
// hmg_angular_transform and hmg_angular_zsum (include/hmgrid.h) and their kernels (kernels/hankel.hpp).  A translation
// unit of its own: no other unit sees these instantiations.  Definition and accuracy: DESIGN.md sections 14 and 22.
#include "hmctx.hpp"
#include "kernels/hankel.hpp"

using namespace hmg;

template <bool W0, bool W2, bool W4, class Radius>
static void hankel_launch(hmg_ctx* c, int rows, int tiles, int nz, int nk, int nr, const double* ks, const double* P,
                          const double* ra, const double* rb, double* w0, double* w2, double* w4) {
    hipLaunchKernelGGL((angular_transform_kernel<HK_THREADS, HK_TILE, W0, W2, W4, Radius>), dim3(rows, tiles),
                       dim3(HK_THREADS), 0, c->stream, nz, nk, nr, ks, P, ra, rb, w0, w2, w4);
}

int hmg_hankel_transform(hmg_ctx* c, int rows, int nk, int nr, const double* ks, const double* P, const double* rs,
                         double* w0, double* w2) {
    REQUIRE(c && ks && P && rs, "NULL argument");
    REQUIRE(w0 || w2, "no output asked for");
    REQUIRE(rows > 0 && nr > 0, "empty grid");
    REQUIRE(nk >= 2, "the transform needs at least two wavenumbers");
    const int tiles = (nr - 1) / HK_TILE + 1;
    REQUIRE(tiles <= 65535, "nr too large");
    with_flags([&](auto W0, auto W2) {
        if constexpr (W0() || W2())
            hankel_launch<W0(), W2(), false, PlainRadius>(c, rows, tiles, 0, nk, nr, ks, P, rs, nullptr, w0, w2, nullptr);
    }, w0, w2);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_angular_transform(hmg_ctx* c, int n, int nz, int nk, int nt, const double* ks, const double* P,
                          const double* chis, const double* thetas, double* w0, double* w2, double* w4) {
    REQUIRE(c && ks && P && chis && thetas, "NULL argument");
    REQUIRE(w0 || w2 || w4, "no output asked for");
    REQUIRE(n > 0 && nz > 0 && nt > 0, "empty grid");
    REQUIRE((long long)n * nz <= 2147483647LL, "too many rows");
    REQUIRE(nk >= 2, "the transform needs at least two wavenumbers");
    const int rows = n * nz, tiles = (nt - 1) / HK_TILE + 1;
    REQUIRE(tiles <= 65535, "nt too large");
    with_flags([&](auto W0, auto W2, auto W4) {
        if constexpr (W0() || W2() || W4())
            hankel_launch<W0(), W2(), W4(), ChiThetaRadius>(c, rows, tiles, nz, nk, nt, ks, P, chis, thetas, w0, w2, w4);
    }, w0, w2, w4);
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
