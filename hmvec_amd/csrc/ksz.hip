// kSZ forecasts: the C-ABI entry points hmg_ksz_* (include/hmgrid.h) and their kernels (kernels/ksz.hpp).  A
// translation unit of its own: the headline path's units do not see these instantiations.  Definitions and accuracy:
// DESIGN.md section 11.
#include "hmctx.hpp"
#include "kernels/ksz.hpp"

using namespace hmg;

namespace {
// dynamic LDS of the P_q_perp kernel: the mu partial integrals always, the z-row of ks / Pee / Pmm when it fits
constexpr size_t KSZ_LDS_MAX = 48 * 1024;
constexpr int KSZ_MAX_MU = 4096;
}  // namespace

int hmg_ksz_pqperp(hmg_ctx* c, int nz, int nk, int nmu, const double* ks, const double* mus, const double* Pee,
                   const double* Pmm, const double* adotf, double* out) {
    REQUIRE(c && ks && mus && Pee && Pmm && adotf && out, "NULL argument");
    REQUIRE(nz > 0 && nk > 0 && nmu > 0, "empty grid");
    REQUIRE(nz <= 65535, "nz too large");
    REQUIRE(nmu <= KSZ_MAX_MU, "more than 4096 mu nodes");
    const size_t lds_mu = (size_t)nmu * sizeof(double);
    const size_t lds_all = lds_mu + 3 * (size_t)nk * sizeof(double);
    if (lds_all <= KSZ_LDS_MAX) {
        hipLaunchKernelGGL(ksz_pqperp_kernel<true>, dim3(nk, nz), dim3(KSZ_PQ_THREADS), lds_all, c->stream, nz, nk,
                           nmu, ks, mus, Pee, Pmm, adotf, out);
    } else {
        hipLaunchKernelGGL(ksz_pqperp_kernel<false>, dim3(nk, nz), dim3(KSZ_PQ_THREADS), lds_mu, c->stream, nz, nk,
                           nmu, ks, mus, Pee, Pmm, adotf, out);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_ksz_nvv(hmg_ctx* c, int nz, int nmu, int nkL, int nkS, int ncl, int rows, const double* mus,
                const double* kLs, const double* kSs, const double* cls, const double* chi, const double* F,
                const double* sig, const double* H, const double* ngg, const double* Pge, const double* Pgg,
                const double* Pph, double* out, int* bad) {
    REQUIRE(c && mus && kLs && kSs && cls && chi && F && ngg && Pge && Pgg && out && bad, "NULL argument");
    REQUIRE(nz > 0 && nmu > 0 && nkL > 0 && nkS > 0 && ncl > 0, "empty grid");
    REQUIRE(nz <= 65535, "nz too large");
    REQUIRE(rows == 0 || rows == 1, "rows must be 0 (one row per z) or 1 (one row per (z, mu, kL))");
    const int photo = sig != nullptr;
    REQUIRE(!photo || H, "photo-z needs H");
    REQUIRE(!(photo && rows), "photo-z takes one row per z");
    const size_t nrow = (size_t)nmu * nkL;
    REQUIRE((nrow + KSZ_NVV_THREADS - 1) / KSZ_NVV_THREADS <= 2147483647u, "grid too large");
    const KszNvvArgs a{nz, nmu, nkL, nkS, ncl, rows, photo, mus, kLs, kSs, cls, chi, F, sig, H, ngg, Pge, Pgg, Pph,
                       out, bad};
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), c->stream));
    if (photo || rows) {
        hipLaunchKernelGGL(ksz_nvv_rows_kernel, dim3((unsigned)((nrow + KSZ_NVV_THREADS - 1) / KSZ_NVV_THREADS), nz),
                           dim3(KSZ_NVV_THREADS), 0, c->stream, a);
    } else {
        hipLaunchKernelGGL(ksz_nvv_shared_kernel, dim3(nz), dim3(KSZ_NVV_THREADS), 0, c->stream, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_ksz_limber_cl(hmg_ctx* c, int nell, int nchi, int nz, int nk, const double* ells, const double* chi,
                      const double* zn, const double* zs, const double* ks, const double* P, int squeezed, double c2,
                      double T2, double* out) {
    REQUIRE(c && ells && chi && zn && zs && ks && P && out, "NULL argument");
    REQUIRE(nell > 0 && nchi > 0, "empty grid");
    REQUIRE(nz >= 2 && nk >= 2, "the bilinear table needs at least two redshifts and two wavenumbers");
    hipLaunchKernelGGL(ksz_limber_cl_kernel, grid1d((size_t)nell, KSZ_CL_THREADS), dim3(KSZ_CL_THREADS), 0,
                       c->stream, nell, nchi, nz, nk, ells, chi, zn, zs, ks, P, squeezed ? 1 : 0, c2, T2, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
