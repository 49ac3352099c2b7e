// HOD parameter ensembles: the C-ABI entry points hmg_hod_ensemble and hmg_hod_ensemble_power (include/hmgrid.h) and
// their kernels (kernels/hodens.hpp; the HOD's device functions are kernels/hod_occ.hpp, shared with hmgrid.hip).  A
// translation unit of its own: the other units do not see these instantiations, and theirs do not change.  The matter
// leg's k -> 0 sum C_m is the leg sums of sampled.hip.  Definition, layout, gates and resources: DESIGN.md section 21.
#include "hmctx.hpp"
#include "rowdev.hpp"
#include "kernels/hodens.hpp"

using namespace hmg;

int hmg_hod_ensemble(hmg_ctx* c, int S, int nz, int nm, int corr, const double* par, const double* lthr, const double* zs,
                     const double* ms, const double* nzm, const double* bh, const double* wm, double* ngal, double* bg,
                     double* occ, double* coef) {
    REQUIRE(c && par && lthr && zs && ms && nzm && bh && wm && ngal && bg, "NULL argument");
    REQUIRE(S > 0 && nz > 0 && nm > 0, "empty grid or no parameter set");
    REQUIRE(corr == 0 || corr == 1, "corr must be 0 (max) or 1 (min)");
    REQUIRE((nm + 63) / 64 <= HOD_MAX_TILES, "nm too large for the HOD reduction (65536)");
    REQUIRE(nz <= 65535, "nz too large");
    const size_t Spad = hodens_spad(S);
    REQUIRE(Spad < ((size_t)1 << 30), "too many parameter sets");
    return with_block(c, 8 * (size_t)nz * nm, [&](void* blk) {
        double* lms = (double*)blk;
        hipLaunchKernelGGL(hodens_lmstar_kernel, grid1d((size_t)nz * nm, 256), dim3(256), 0, c->stream, nz, nm, zs, ms, lms);
        HIP_TRY(hipGetLastError());
        const HodEnsArgs A{S, (int)Spad, nz, nm, corr, par, lthr, zs, ms, nzm, bh, wm, lms, ngal, bg, occ, coef,
                           coef ? coef + 4 * (size_t)nz * nm * Spad : nullptr};
        // the padding sets of the coefficient block are workgroups of the same launch
        hipLaunchKernelGGL(hodens_occ_kernel, dim3(coef ? (unsigned)Spad : (unsigned)S, nz), dim3(HE_OCC_THREADS), 0,
                           c->stream, A);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

namespace {

template <int TS>
void power_launch(hmg_ctx* c, HodEnsPowerArgs& A, int threads) {
    A.ngroups = A.nz * ((A.n + threads - 1) / threads);
    A.ntiles = (A.S + TS - 1) / TS;
    const unsigned blocks = (unsigned)((A.ngroups + 7) / 8 * 8) * (unsigned)A.ntiles;
    if (A.um == A.us)
        hipLaunchKernelGGL((hodens_power_kernel<TS, true>), dim3(blocks), dim3(threads), 0, c->stream, A);
    else
        hipLaunchKernelGGL((hodens_power_kernel<TS, false>), dim3(blocks), dim3(threads), 0, c->stream, A);
}

}  // namespace

// The block of the call: the word of the check, C_m (C, C0, b of the matter leg) and the side data of the mass bins.
int hmg_hod_ensemble_power(hmg_ctx* c, int S, int nz, int nm, int nk, int n, const double* us, const double* um,
                           const double* coef, const double* ngal, const double* bg, const double* nzm, const double* bh,
                           const double* ms, const double* wm, const double* ks, const double* Pzk, double rho_m0,
                           const int* kidx, const double* damp, double* out, double* parts) {
    REQUIRE(c && us && um && coef && ngal && bg && nzm && bh && ms && wm && ks && Pzk && damp, "NULL argument");
    REQUIRE(out, "d_out is NULL: no output");
    REQUIRE(S > 0 && nz > 0 && nm > 0 && nk > 0, "empty grid or no parameter set");
    REQUIRE(n >= 1, "no columns");
    REQUIRE(kidx || n == nk, "without d_kindex the columns are the whole k grid: n must be nk");
    REQUIRE(rho_m0 > 0.0, "rho_m0 must be positive");
    const HaloGrid g = {nz, nm, nk, nzm, bh, ms, wm, ks, Pzk, rho_m0};
    const size_t Spad = hodens_spad(S);
    REQUIRE(((size_t)nz * ((n + 63) / 64) + 8) * ((S + HE_TS_SHORT - 1) / HE_TS_SHORT) < ((size_t)1 << 31),
            "too many workgroups");
    REQUIRE(!kidx || !c->capturing,
            "the call waits on the host for its check of d_kindex and cannot be part of a captured step");
    if (series_ensure_whole(c, us) || series_ensure_whole(c, um)) return 1;
    return with_block(c, 64 + 8 * (3 * (size_t)nz + 4 * (size_t)nz * nm), [&](void* blk) {
        int* d_bad = (int*)blk;
        double* legs = (double*)((char*)blk + 64);
        double* side = legs + 3 * (size_t)nz;
        if (kidx) {                 // checked on the device before anything reads a tensor through it
            int bad = 0;
            if (check_words(c, d_bad, &bad, 1, [&] {
                    hipLaunchKernelGGL(hodens_check_kernel, grid1d(n, 256), dim3(256), 0, c->stream, n, nk, kidx, d_bad);
                }))
                return 1;
            REQUIRE(!bad, "a column's node is outside 0 .. nk-1");
        }
        const BisLeg matter = {HMG_TRACER_MATTER, um, nullptr, nullptr, nullptr, nullptr};
        if (leg_sums_launch(c, g, matter, 1.0, nz, legs)) return 1;
        hipLaunchKernelGGL(hodens_side_kernel, grid1d((size_t)nz * nm, 256), dim3(256), 0, c->stream, g, side);
        HIP_TRY(hipGetLastError());
        HodEnsPowerArgs A = {S, (int)Spad, nz, nm, nk, n, 0, 0, us, um, coef, coef + 4 * (size_t)nz * nm * Spad,
                             side, legs, ngal, bg, Pzk, damp, kidx, out, parts};
        // fewer columns than one workgroup takes cannot fill the machine: split the sets, not the masses, across more
        // workgroups (an element's bits do not depend on the tile: each accumulator is its own chain)
        if (n < HE_KT) power_launch<HE_TS_SHORT>(c, A, (n + 63) / 64 * 64);
        else power_launch<HE_TS>(c, A, HE_KT);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
