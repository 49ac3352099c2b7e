// Halo-model bispectrum of three tracers: the C-ABI entry point hmg_bispectrum (include/hmgrid.h) and its kernels
// (kernels/bispectrum.hpp).  A translation unit of its own: the headline path's units do not see these instantiations.
// Definition, gates and resources: DESIGN.md section 16.
#include "hmctx.hpp"
#include "kernels/bispectrum.hpp"

using namespace hmg;

int hmg_bispectrum(hmg_ctx* c, int nz, int nm, int nk, int n, int nt, const hmg_tracer* ta, const hmg_tracer* tb,
                   const hmg_tracer* tc, const double* nzm, const double* bh, const double* ms, const double* wm,
                   const double* ks, const double* Pzk, double rho_m0, double kstar, const int* idx, const double* frac,
                   const double* scale, const int* tri, const double* zweights, double* B, double* Bz, double* J) {
    REQUIRE(c && ta && tb && tc && nzm && bh && ms && wm && ks && Pzk && idx && frac && scale && tri, "NULL argument");
    REQUIRE(B || Bz || J, "no output requested");
    REQUIRE(!Bz || zweights, "d_Bz needs d_zweights");
    REQUIRE(nz > 0 && nm > 0 && nk > 0, "empty grid");
    REQUIRE(n >= 1, "no sample points");
    REQUIRE(nt >= 1, "no triangles");
    REQUIRE(n <= BIS_MAXN, "more than 256 samples per redshift");
    REQUIRE(nz <= 65535, "nz too large");
    REQUIRE(nt <= (1 << 20), "more than 2^20 triangles");
    REQUIRE(!c->capturing, "hmg_bispectrum waits on the host for its table check and cannot be part of a captured step");
    const hmg_tracer* tr[3] = {ta, tb, tc};
    int hods = 0;
    for (auto t : tr) hods += t->kind == HMG_TRACER_HOD;
    REQUIRE(hods < 2, "two or more HOD tracers in one triple: the 1-halo term needs third factorial moments of the HOD, "
                      "which the model does not carry");
    if (tracers_ensure_whole(c, tr, 3)) return 1;
    BisArgs A;
    A.nu = 0;
    for (int l = 0; l < 3; ++l) {
        BisLeg L;
        if (bis_leg(tr[l], &L)) return 1;
        int u = 0;
        while (u < A.nu && !bis_same(A.uq[u], L)) ++u;
        if (u == A.nu) A.uq[A.nu++] = L;
        A.slot[l] = u;
    }
    for (int u = A.nu; u < 3; ++u) A.uq[u] = A.uq[0];
    A.g = {nz, nm, nk, nzm, bh, ms, wm, ks, Pzk, rho_m0};
    A.s = {idx, frac, scale, n};
    A.tri = tri; A.nt = nt; A.chunk = bis_chunk(n);
    // the block: the words of the check, the sampled P, D and k, and whichever of J and the per-z terms the caller did
    // not ask for
    const size_t zn = (size_t)nz * n, znt = (size_t)nz * nt;
    const bool need_b = B || Bz;
    return with_block(c, 64 + 8 * (3 * zn + (J ? 0 : 3 * zn) + (need_b && !B ? 3 * znt : 0)), [&](void* blk) {
        double* w = (double*)((char*)blk + 64);
        A.Ps = w; A.Ds = w + zn; A.Ks = w + 2 * zn;
        w += 3 * zn;
        if (J) A.J = J; else { A.J = w; w += 3 * zn; }
        A.B = B ? B : need_b ? w : nullptr;
        // the tables and the triangles are checked on the device before anything reads a tensor through them
        const size_t count = (size_t)nz * (size_t)(n > nt ? n : nt);
        int* d_bad = (int*)blk;
        int bad[3] = {0, 0, 0};
        if (check_words(c, d_bad, bad, 3, [&] {
                hipLaunchKernelGGL(bispectrum_check_kernel, grid1d(count, 256), dim3(256), 0, c->stream, nz, nk, n, nt, idx,
                                   frac, tri, ks, d_bad);
            }))
            return 1;
        REQUIRE(!bad[0], BAD_SAMPLE_TABLE);
        REQUIRE(!bad[1], "a triangle names a sample outside 0 .. n-1");
        REQUIRE(!bad[2], "a triangle does not close at some redshift: k_max > (k_mid + k_min)(1 + 2^-40)");
        for (int u = 0; u < A.nu; ++u) {            // one prepass per distinct leg; it writes J for every leg it serves
            LegOut out = {};
            for (int l = 0; l < 3; ++l)
                if (A.slot[l] == u) out.J[l] = A.J + l * zn;
            if (A.slot[0] == u) { out.Ps = A.Ps; out.Ds = A.Ds; out.Ks = A.Ks; }
            if (leg_prepass_launch(c, A.g, A.uq[u], idx, frac, n, kstar, out)) return 1;
        }
        if (A.B) {
            hipLaunchKernelGGL(bispectrum_kernel, dim3((nt - 1) / BIS_BLOCK + 1, nz), dim3(BIS_THREADS), 0, c->stream, A);
            HIP_TRY(hipGetLastError());
        }
        return Bz ? zsum_launch(c, nz, (size_t)3 * nt, nt, zweights, A.B, Bz) : 0;
    });
}
