// Curved-sky angular correlation functions: the C-ABI entry points hmg_curvedsky_weights and hmg_curvedsky_scale_spectra
// (include/hmgrid.h) and their kernels (kernels/curvedsky.hpp).  A translation unit of its own; the contraction and the
// node weights (hmg_curvedsky_gaussian, hmg_curvedsky_node_weights) are in angcov.hip with the kernels they share with
// the flat sky.  Definition and accuracy: DESIGN.md section 27.
#include "hmctx.hpp"
#include "kernels/curvedsky.hpp"

using namespace hmg;

int hmg_curvedsky_weights(hmg_ctx* c, int l0, int nl, int nt, const double* edges, const double* cosdiff, double* kw,
                          double* kg, double* kp, double* km) {
    REQUIRE(c && edges && cosdiff, "NULL argument");
    REQUIRE(kw || kg || kp || km, "no kind asked for");
    REQUIRE(l0 >= 1 && nl > 0 && (long long)l0 + nl - 1 <= HMG_CURVEDSKY_LMAX,
            "the multipoles must be 1 <= l0 .. l0 + nl - 1 <= HMG_CURVEDSKY_LMAX");
    REQUIRE(nt > 0, "empty grid");
    const long long tiles = (nt - 1) / (CS_THREADS - 1) + 1, segments = (nl - 1) / CS_SEGMENT + 1;
    REQUIRE(tiles <= 2147483647LL && segments <= 65535, "too many bins or multipoles");
    hipLaunchKernelGGL(curvedsky_weights_kernel, dim3((unsigned)tiles, (unsigned)segments), dim3(CS_THREADS), 0, c->stream,
                       l0, nl, nt, edges, cosdiff, kw, kg, kp, km);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_curvedsky_scale_spectra(hmg_ctx* c, int nf, int nn, const double* nodes, const int* spins, const int* d_spins,
                                double* C) {
    REQUIRE(c && nodes && spins && d_spins && C, "NULL argument");
    REQUIRE(nf > 0 && nn > 0, "empty table");
    for (int f = 0; f < nf; ++f) REQUIRE(spins[f] == 0 || spins[f] == 2, "a field's spin must be 0 or 2");
    const long long total = (long long)nf * nf * nn;
    REQUIRE((total - 1) / 256 + 1 <= 2147483647LL, "too many entries");
    hipLaunchKernelGGL(curvedsky_scale_kernel, dim3((unsigned)((total - 1) / 256 + 1)), dim3(256), 0, c->stream, nf, nn, nodes,
                       d_spins, C);
    HIP_TRY(hipGetLastError());
    return 0;
}
