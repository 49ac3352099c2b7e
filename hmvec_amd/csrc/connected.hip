// The 2-, 3- and 4-halo terms of the trispectrum of two halo-model spectra: the C-ABI entry points hmg_pt_averages and
// hmg_trispectrum_connected (include/hmgrid.h) and their kernels (kernels/connected.hpp).  A translation unit of its own:
// the headline path's units do not see these instantiations.  The 1-halo plane is hmg_trispectrum_1h's, the brackets J
// and the z sum are sampled.hip's.  Definition, gates and resources: DESIGN.md section 31.
#include "hmctx.hpp"
#include "kernels/connected.hpp"

using namespace hmg;

static int pt_launch(hmg_ctx* c, PtArgs A) {
    const size_t lds = (2 * (size_t)A.nk + 4 * (size_t)A.nr) * sizeof(double);
    const int pairs = A.n * (A.n + 1) / 2;
    if (lds > 48 * 1024)                   // beyond the default limit of a launch: ask for it (up to 139,264 B of 160 KB)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(pt_average_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pt_average_kernel, dim3((pairs - 1) / PT_THREADS + 1, A.nz), dim3(PT_THREADS), lds, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int pt_shapes(int nz, int nk, int n, int nr) {
    REQUIRE(nz > 0 && nk > 1, "empty grid (the interpolant of P_lin needs two wavenumbers)");
    REQUIRE(nk <= PT_MAXNK, "more than 8192 wavenumbers: the row's ln k and ln P do not fit the workgroup's LDS");
    REQUIRE(n >= 1, "no sample points");
    REQUIRE(n <= CON_MAXN, "more than 256 samples per redshift");
    REQUIRE(nr >= 1, "no rule nodes");
    REQUIRE(nr <= CON_MAXR, "more than 256 rule nodes");
    REQUIRE(nz <= 65535, "nz too large");
    return 0;
}

int hmg_pt_averages(hmg_ctx* c, int nz, int nk, int n, int nr, const double* ks, const double* Pzk, const int* idx,
                    const double* frac, const double* mu, const double* omm, const double* opm, const double* w,
                    double* Pbar, double* Bbar, double* Tbar) {
    REQUIRE(c && ks && Pzk && idx && frac && mu && omm && opm && w && Pbar && Bbar && Tbar, "NULL argument");
    if (pt_shapes(nz, nk, n, nr)) return 1;
    REQUIRE(!c->capturing, "hmg_pt_averages waits on the host for its table check and cannot be part of a captured step");
    const SampleTable s = {idx, frac, nullptr, n};
    return with_block(c, 64, [&](void* blk) {
        if (samples_checked(c, s, nz, nk, (int*)blk)) return 1;
        return pt_launch(c, {nz, nk, n, nr, ks, Pzk, idx, frac, mu, omm, opm, w, Pbar, Bbar, Tbar});
    });
}

int hmg_trispectrum_connected(hmg_ctx* c, int nz, int nm, int nk, int n, int nr, const hmg_tracer* ta,
                              const hmg_tracer* tb, const hmg_tracer* tc, const hmg_tracer* td, const double* nzm,
                              const double* bh, const double* ms, const double* wm, const double* ks, const double* Pzk,
                              double rho_m0, double kstar, const int* idx, const double* frac, const double* scale,
                              const double* scale1h, const double* mu, const double* omm, const double* opm,
                              const double* w, const double* zweights, double* T, double* Tz) {
    REQUIRE(c && ta && tb && tc && td && nzm && bh && ms && wm && ks && Pzk && idx && frac && scale && scale1h && mu &&
                omm && opm && w,
            "NULL argument");
    REQUIRE(T || Tz, "no output requested");
    REQUIRE(!Tz || zweights, "d_Tz needs d_zweights");
    REQUIRE(nm > 0, "empty grid");
    if (pt_shapes(nz, nk, n, nr)) return 1;
    REQUIRE(!c->capturing,
            "hmg_trispectrum_connected waits on the host for its table check and cannot be part of a captured step");
    const hmg_tracer* tr[4] = {ta, tb, tc, td};
    ConArgs A;
    BisLeg* legs[4] = {&A.la, &A.lb, &A.lc, &A.ld};
    const hmg_tracer* hod = nullptr;
    for (int l = 0; l < 4; ++l) {
        if (bis_leg(tr[l], legs[l])) return 1;
        if (tr[l]->kind != HMG_TRACER_HOD) continue;
        REQUIRE(tr[l]->d_NcNs && tr[l]->d_NsNsm1, "HOD tracer needs NcNs,NsNsm1");
        if (!hod) { hod = tr[l]; A.h = *legs[l]; }
        REQUIRE(bis_same(A.h, *legs[l]) && hod->d_NcNs == tr[l]->d_NcNs && hod->d_NsNsm1 == tr[l]->d_NsNsm1,
                "two different HOD tracers in one request: their pair term needs cross moments of the two HODs, which the "
                "model does not carry");
    }
    if (!hod) A.h = A.la;
    A.NcNs = hod ? hod->d_NcNs : nullptr;
    A.NsNsm1 = hod ? hod->d_NsNsm1 : nullptr;
    const auto is_hod = [&](int l) { return tr[l]->kind == HMG_TRACER_HOD; };
    A.hod_ac = is_hod(0) && is_hod(2); A.hod_ad = is_hod(0) && is_hod(3);
    A.hod_bc = is_hod(1) && is_hod(2); A.hod_bd = is_hod(1) && is_hod(3);
    if (tracers_ensure_whole(c, tr, 4)) return 1;
    if (tri_side(ta, tb, &A.ab)) return 1;
    if (tri_side(tc, td, &A.cd)) return 1;
    A.g = {nz, nm, nk, nzm, bh, ms, wm, ks, Pzk, rho_m0};
    A.s = {idx, frac, scale, n};
    // the distinct legs: one prepass each; legs of one tracer share its J
    int nu = 0, slot[4];
    for (int l = 0; l < 4; ++l) {
        int u = 0;
        while (u < nu && !bis_same(*legs[slot[u]], *legs[l])) ++u;       // (slot[u] here: the first leg of distinct leg u)
        if (u == nu) slot[nu++] = l;
    }
    // the block: the word of the check, J of the distinct legs, P, D, k at the samples, the three PT matrices, and the
    // per-z terms when only the z sum is asked for
    const size_t zn = (size_t)nz * n, nn = (size_t)n * n, plane = (size_t)nz * nn;
    const int tiles = (n - 1) / CON_TILE + 1;
    return with_block(c, 64 + 8 * (7 * zn + 3 * plane + (T ? 0 : 5 * plane)), [&](void* blk) {
        if (samples_checked(c, A.s, nz, nk, (int*)blk)) return 1;
        double* wsp = (double*)((char*)blk + 64);
        double* J = wsp;
        double *Ps = wsp + 4 * zn, *Ds = wsp + 5 * zn, *Ks = wsp + 6 * zn;
        double* pt = wsp + 7 * zn;
        A.T = T ? T : pt + 3 * plane;
        const double* Jl[4];
        for (int u = 0; u < nu; ++u) {
            LegOut out = {};
            out.J[0] = J + u * zn;
            if (u == 0) { out.Ps = Ps; out.Ds = Ds; out.Ks = Ks; }
            if (leg_prepass_launch(c, A.g, *legs[slot[u]], idx, frac, n, kstar, out)) return 1;
            for (int l = 0; l < 4; ++l)
                if (bis_same(*legs[slot[u]], *legs[l])) Jl[l] = J + u * zn;
        }
        A.Ja = Jl[0]; A.Jb = Jl[1]; A.Jc = Jl[2]; A.Jd = Jl[3];
        A.Ps = Ps; A.Ds = Ds;
        A.Pbar = pt; A.Bbar = pt + plane; A.Tbar = pt + 2 * plane;
        if (pt_launch(c, {nz, nk, n, nr, ks, Pzk, idx, frac, mu, omm, opm, w, pt, pt + plane, pt + 2 * plane})) return 1;
        // plane 0: the 1-halo term by its own entry point and kernel, with the scale its caller folds the damping into
        if (hmg_trispectrum_1h(c, nz, nm, nk, n, ta, tb, tc, td, nzm, ms, wm, rho_m0, idx, frac, scale1h, nullptr, A.T,
                               nullptr))
            return 1;
        hipLaunchKernelGGL(connected_kernel, dim3(tiles, tiles, nz), dim3(CON_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        return Tz ? zsum_launch(c, nz, 5 * nn, nn, zweights, A.T, Tz) : 0;
    });
}
