// Non-Limber angular power spectra of separable sources: the C-ABI entry points hmg_sph_bessel, hmg_nonlimber_transfer
// and hmg_nonlimber_cl (include/hmgrid.h) and their kernels (kernels/nonlimber.hpp, sphbessel.hpp).  A translation unit of its own.  Definition, accuracy and resources:
// DESIGN.md section 29.
#include "hmctx.hpp"
#include "kernels/nonlimber.hpp"

using namespace hmg;

static_assert(NL_FMAX == HMG_NONLIMBER_FMAX && NL_THREADS == HMG_NONLIMBER_THREADS && NL_TILE == HMG_NONLIMBER_TILE,
              "the header states the kernel's layout");

int hmg_sph_bessel(hmg_ctx* c, int lmax, int nx, const double* xs, double* out) {
    REQUIRE(c && xs && out, "NULL argument");
    REQUIRE(lmax >= 0 && lmax <= HMG_NONLIMBER_LMAX, "lmax must be 0 .. HMG_NONLIMBER_LMAX");
    REQUIRE(nx > 0, "no arguments");
    hipLaunchKernelGGL(sph_bessel_kernel, grid1d((size_t)nx, 256), dim3(256), 0, c->stream, lmax, sb_start_order(lmax), nx, xs,
                       out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_nonlimber_transfer(hmg_ctx* c, int F, int ngz, int nkq, int lmax, const double* kq, const double* chis,
                           const double* src, double* out) {
    REQUIRE(c && kq && chis && src && out, "NULL argument");
    REQUIRE(F >= 1 && F <= HMG_NONLIMBER_FMAX, "1 <= F <= HMG_NONLIMBER_FMAX fields per launch");
    REQUIRE(ngz > 0 && nkq > 0, "empty rule");
    REQUIRE(lmax >= 0 && lmax <= HMG_NONLIMBER_LMAX, "lmax must be 0 .. HMG_NONLIMBER_LMAX");
    hipLaunchKernelGGL(nonlimber_transfer_kernel, dim3((unsigned)nkq), dim3(NL_THREADS), 0, c->stream, F, ngz, nkq, lmax,
                       sb_start_order(lmax), kq, chis, src, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_nonlimber_cl(hmg_ctx* c, int F, int nkq, int lmax, int np, const int* pairs, const int* d_pairs, const double* kq,
                     const double* wk, const double* T, double* out) {
    REQUIRE(c && pairs && d_pairs && kq && wk && T && out, "NULL argument");
    REQUIRE(F > 0 && nkq > 0 && lmax >= 0 && lmax <= HMG_NONLIMBER_LMAX, "empty request");
    REQUIRE(np > 0 && np <= 65535, "1 .. 65535 pairs per call");
    for (int p = 0; p < 2 * np; ++p) REQUIRE(pairs[p] >= 0 && pairs[p] < F, "a pair names a field outside 0 .. F - 1");
    hipLaunchKernelGGL(nonlimber_cl_kernel, dim3((unsigned)(lmax + 1), (unsigned)np), dim3(64), 0, c->stream, nkq, lmax,
                       d_pairs, kq, wk, T, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
