// The CIB halo model: the C-ABI entry points hmg_cib_luminosity and hmg_emission_power (include/hmgrid.h) and their
// kernels (kernels/cib.hpp).  A translation unit of its own: the other units do not see these instantiations, and theirs
// do not change.  Definitions, order of the operations, gates and resources: DESIGN.md section 26.
#include <cmath>

#include "hmctx.hpp"
#include "kernels/cib.hpp"

using namespace hmg;

int hmg_cib_luminosity(hmg_ctx* c, int F, int nz, int nm, int nsub, const double* nus, const double* zs, const double* ms,
                       const double* chis, const double* scut, const double* t, const double* w,
                       const double par[HMG_CIB_NPAR], double* Lc, double* Ls) {
    REQUIRE(c && nus && zs && ms && chis && t && w && par, "NULL argument");
    REQUIRE(Lc && Ls, "d_Lc or d_Ls is NULL: no output");
    REQUIRE(F >= 1 && F <= CIB_FMAX, "F must lie in 1 .. HMG_CIB_FMAX (16)");
    REQUIRE(nz >= 1 && nm >= 1 && nsub >= 1, "empty grid or no node");
    REQUIRE((long long)nz * nm <= 2147483647LL / CIB_FMAX, "grid too large");
    const double alpha = par[0], T0 = par[1], beta = par[2], gamma = par[3], delta = par[4], zp = par[5], lMeff = par[6],
                 sigma2 = par[7], Mmin = par[8], L0 = par[9], x0 = par[10];
    for (int i = 0; i < HMG_CIB_NPAR; ++i) REQUIRE(std::isfinite(par[i]), "a parameter is not finite");
    REQUIRE(T0 > 0.0 && sigma2 > 0.0 && Mmin > 0.0 && x0 > 0.0 && zp > -1.0, "T0, sigma2, M_min and x0 must be positive, z_p above -1");
    CibLumArgs A = {F, nz, nm, nsub, nus, zs, ms, chis, scut, t, w, alpha, T0, beta, gamma, delta, zp, lMeff, Mmin, L0, x0,
                    1.0 / std::sqrt((2.0 * M_PI) * sigma2), 1.0 / (2.0 * sigma2), std::expm1(x0), Lc, Ls};
    const size_t total = (size_t)nz * nm;
    hipLaunchKernelGGL(cib_luminosity_kernel, grid1d(total, CIB_LW), dim3(64 * CIB_LW), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

namespace {

template <int NP>
void emission_launch(hmg_ctx* c, const EmissionArgs& A, unsigned blocks, int threads) {
    hipLaunchKernelGGL((emission_power_kernel<NP>), dim3(blocks), dim3(threads), 0, c->stream, A);
}

}  // namespace

// The block of the call: the word of the check, the frequency-padded coefficients and the side data of the mass bins.
int hmg_emission_power(hmg_ctx* c, int F, int nz, int nm, int nk, int n, const double* us, const double* Lc,
                       const double* Ls, int NP, const hmg_tracer* partners, const double* nzm, const double* bh,
                       const double* ms, const double* wm, double rho_m0, const int* kidx, const double* damp, double* P1h,
                       double* I, double* X1h) {
    REQUIRE(c && us && Lc && Ls && nzm && bh && ms && wm && damp, "NULL argument");
    REQUIRE(P1h && I, "d_P1h or d_I is NULL: no output");
    REQUIRE(F >= 1 && F <= CIB_FMAX, "F must lie in 1 .. HMG_CIB_FMAX (16)");
    REQUIRE(nz > 0 && nm > 0 && nk > 0, "empty grid");
    REQUIRE(n >= 1, "no columns");
    REQUIRE(kidx || n == nk, "without d_kindex the columns are the whole k grid: n must be nk");
    REQUIRE(rho_m0 > 0.0, "rho_m0 must be positive");
    REQUIRE(NP >= 0 && NP <= 2, "NP must be 0, 1 or 2");
    REQUIRE(NP == 0 || (partners && X1h), "partners without h_partners or d_X1h");
    EmissionPrepArgs Q = {F, 0, nz, nm, NP, {0, 0}, Lc, Ls, nzm, bh, ms, wm, rho_m0, nullptr, nullptr};
    EmissionArgs A = {};
    for (int p = 0; p < NP; ++p) {
        REQUIRE(partners[p].kind == HMG_TRACER_MATTER || partners[p].kind == HMG_TRACER_PRESSURE,
                "a partner of an emission must be a matter or a pressure tracer");
        REQUIRE(partners[p].d_prof, "a partner has no profile tensor");
        Q.kind[p] = partners[p].kind;
        A.prof[p] = partners[p].d_prof;
    }
    const int nb = (F + CIB_T - 1) / CIB_T, Fpad = nb * CIB_T, ntiles = nb * (nb + 1) / 2;
    const int threads = n < CIB_KT ? (n + 63) / 64 * 64 : CIB_KT;
    const size_t ngroups = (size_t)nz * ((n + threads - 1) / threads);
    REQUIRE((ngroups + 8) * ntiles < ((size_t)1 << 31), "too many workgroups");
    REQUIRE(!kidx || !c->capturing,
            "the call waits on the host for its check of d_kindex and cannot be part of a captured step");
    if (series_ensure_whole(c, us)) return 1;
    for (int p = 0; p < NP; ++p)
        if (series_ensure_whole(c, A.prof[p])) return 1;
    const size_t plane = (size_t)nz * nm;
    return with_block(c, 64 + 8 * plane * ((size_t)Fpad * 2 + 4), [&](void* blk) {
        int* d_bad = (int*)blk;
        double* coef = (double*)((char*)blk + 64);
        double* side = coef + plane * Fpad * 2;
        if (kidx) {                 // checked on the device before anything reads a tensor through it
            int bad = 0;
            if (check_words(c, d_bad, &bad, 1, [&] {
                    hipLaunchKernelGGL(emission_check_kernel, grid1d(n, 256), dim3(256), 0, c->stream, n, nk, kidx, d_bad);
                }))
                return 1;
            REQUIRE(!bad, "a column's node is outside 0 .. nk-1");
        }
        Q.Fpad = Fpad; Q.coef = coef; Q.side = side;
        hipLaunchKernelGGL(emission_prep_kernel, grid1d(plane, 256), dim3(256), 0, c->stream, Q);
        HIP_TRY(hipGetLastError());
        A.F = F; A.Fpad = Fpad; A.nb = nb; A.nz = nz; A.nm = nm; A.nk = nk; A.n = n;
        A.ngroups = (int)ngroups; A.ntiles = ntiles;
        A.us = us; A.coef = coef; A.side = side; A.damp = damp; A.kidx = kidx;
        A.P1h = P1h; A.I = I; A.X1h = X1h;
        const unsigned blocks = (unsigned)((ngroups + 7) / 8 * 8) * (unsigned)ntiles;
        if (NP == 0) emission_launch<0>(c, A, blocks, threads);
        else if (NP == 1) emission_launch<1>(c, A, blocks, threads);
        else emission_launch<2>(c, A, blocks, threads);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
