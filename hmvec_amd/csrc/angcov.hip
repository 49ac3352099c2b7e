// Covariance of angular correlation functions: the C-ABI entry points hmg_angcov_weights, hmg_angcov_gaussian and
// hmg_angcov_node_weights (include/hmgrid.h) and their kernels (kernels/angcov.hpp), and the curved-sky forms of the
// last two, hmg_curvedsky_gaussian and hmg_curvedsky_node_weights: the same kernels with the measure l + 1/2.  A
// translation unit of its own.  Definition and accuracy: DESIGN.md sections 23 and 27.
#include "hmctx.hpp"
#include "kernels/angcov.hpp"

using namespace hmg;

namespace {

// the contraction and its ordered combine of either sky; ks: the weights by a probe's third entry (nk of them), geom:
// the edges (flat) or the bins' cos a - cos b (curved)
template <bool CURVED>
int gaussian(hmg_ctx* c, int nf, int nn, const double* nodes, const double* C, const double* noise, int l0, int nl, int nt,
             const double* geom, int np, const int* probes, const int* d_probes, double area, const double* const* ks,
             int nk, size_t work_words, double* work, double* cov) {
    REQUIRE(c && nodes && C && noise && geom && probes && d_probes && work && cov, "NULL argument");
    REQUIRE(nf > 0 && nn >= 2, "the spectra need a field and two nodes");
    REQUIRE(l0 >= 1 && nl > 0 && (long long)l0 + nl <= 2147483647LL, "the multipoles must be 1 <= l0 .. l0 + nl - 1 < 2^31");
    REQUIRE(nt > 0 && np > 0, "empty data vector");
    REQUIRE(area > 0.0, "the survey area must be positive");
    for (int p = 0; p < np; ++p) {
        const int f = probes[3 * p], g = probes[3 * p + 1], o = probes[3 * p + 2];
        REQUIRE(f >= 0 && f < nf && g >= 0 && g < nf, "a probe names a field out of range");
        REQUIRE(o >= 0 && o < nk, CURVED ? "a probe's kind must be 0 .. 3 (w, gammat, xip, xim)"
                                         : "a probe's order index must be 0, 1 or 2 (mu / 2)");
        REQUIRE(ks[o], CURVED ? "a probe's kind has no weights" : "a probe's order has no weights");
    }
    const long long pairs = (long long)np * (np + 1) / 2, chunks = (nl - 1) / AC_CHUNK + 1;
    const long long tiles = (nt - 1) / AC_TILE + 1;
    REQUIRE(pairs <= 2147483647LL && chunks <= 65535 && tiles * tiles <= 65535, "too many probes, multipoles or bins");
    const long long total = (long long)np * nt * np * nt;
    REQUIRE((total - 1) / 256 + 1 <= 2147483647LL, "too many outputs");
    REQUIRE((long long)work_words >= pairs * chunks * nt * nt, "the work buffer is too small");
    double* partial = work;
    hipLaunchKernelGGL(angcov_gaussian_kernel<CURVED>, dim3((unsigned)pairs, (unsigned)chunks, (unsigned)(tiles * tiles)),
                       dim3(AC_THREADS), 0, c->stream, nf, nn, nodes, C, noise, l0, nl, nt, np, d_probes, ks[0], ks[1], ks[2],
                       nk > 3 ? ks[3] : nullptr, partial);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(angcov_combine_kernel<CURVED>, dim3((unsigned)((total - 1) / 256 + 1)), dim3(256), 0, c->stream,
                       (int)chunks, nt, np, (size_t)total, d_probes, noise, geom, 1.0 / (2.0 * M_PI * area), area * M_PI,
                       partial, cov);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <bool CURVED>
int node_weights(hmg_ctx* c, int nn, const double* nodes, int l0, int nl, int nt, const double* k, double scale,
                 int by_node, double* r) {
    REQUIRE(c && nodes && k && r, "NULL argument");
    REQUIRE(nn >= 2 && nt > 0, "the weights need two nodes and a bin");
    REQUIRE(l0 >= 1 && nl > 0 && (long long)l0 + nl <= 2147483647LL, "the multipoles must be 1 <= l0 .. l0 + nl - 1 < 2^31");
    const long long total = (long long)nn * nt;
    REQUIRE((total - 1) / 256 + 1 <= 2147483647LL, "too many outputs");
    hipLaunchKernelGGL(angcov_node_weights_kernel<CURVED>, dim3((unsigned)((total - 1) / 256 + 1)), dim3(256), 0, c->stream,
                       nn, nodes, l0, nl, nt, k, scale, by_node, r);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int hmg_angcov_weights(hmg_ctx* c, int nl, int nt, const double* ells, const double* edges, double* k0, double* k2,
                       double* k4) {
    REQUIRE(c && ells && edges, "NULL argument");
    REQUIRE(k0 || k2 || k4, "no output asked for");
    REQUIRE(nl > 0 && nt > 0, "empty grid");
    hipLaunchKernelGGL(angcov_weights_kernel, dim3((nl - 1) / 256 + 1), dim3(256), 0, c->stream, nl, nt, ells, edges, k0,
                       k2, k4);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_angcov_gaussian(hmg_ctx* c, int nf, int nn, const double* nodes, const double* C, const double* noise, int l0,
                        int nl, int nt, const double* edges, int np, const int* probes, const int* d_probes, double area,
                        const double* k0, const double* k2, const double* k4, size_t work_words, double* work,
                        double* cov) {
    const double* ks[3] = {k0, k2, k4};
    return gaussian<false>(c, nf, nn, nodes, C, noise, l0, nl, nt, edges, np, probes, d_probes, area, ks, 3, work_words,
                           work, cov);
}

int hmg_angcov_node_weights(hmg_ctx* c, int nn, const double* nodes, int l0, int nl, int nt, const double* k,
                            double scale, int by_node, double* r) {
    return node_weights<false>(c, nn, nodes, l0, nl, nt, k, scale, by_node, r);
}

int hmg_curvedsky_gaussian(hmg_ctx* c, int nf, int nn, const double* nodes, const double* C, const double* noise, int l0,
                           int nl, int nt, const double* cosdiff, int np, const int* probes, const int* d_probes,
                           double area, const double* kw, const double* kg, const double* kp, const double* km,
                           size_t work_words, double* work, double* cov) {
    const double* ks[4] = {kw, kg, kp, km};
    return gaussian<true>(c, nf, nn, nodes, C, noise, l0, nl, nt, cosdiff, np, probes, d_probes, area, ks, 4, work_words,
                          work, cov);
}

int hmg_curvedsky_node_weights(hmg_ctx* c, int nn, const double* nodes, int l0, int nl, int nt, const double* k,
                               double scale, int by_node, double* r) {
    return node_weights<true>(c, nn, nodes, l0, nl, nt, k, scale, by_node, r);
}
