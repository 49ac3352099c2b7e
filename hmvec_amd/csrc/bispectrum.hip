// Halo-model bispectrum of three tracers: the C-ABI entry point hmg_bispectrum (include/hmgrid.h) and its kernels
// (kernels/bispectrum.hpp).  A translation unit of its own: the headline path's units do not see these instantiations.
// Definition, gates and resources: DESIGN.md section 16.
#include "hmctx.hpp"
#include "kernels/bispectrum.hpp"

using namespace hmg;

// the launches of one call; d_bad holds the three words of the check
static int bis_run(hmg_ctx* c, const BisArgs& A, const double* zweights, double* Bz, int* d_bad) {
    // the tables and the triangles are checked on the device before anything reads a tensor through them
    const size_t count = (size_t)A.nz * (size_t)(A.n > A.nt ? A.n : A.nt);
    int bad[3] = {0, 0, 0};
    HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(bad), c->stream));
    hipLaunchKernelGGL(bispectrum_check_kernel, grid1d(count, 256), dim3(256), 0, c->stream, A.nz, A.nk, A.n, A.nt, A.idx,
                       A.frac, A.tri, A.ks, d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    REQUIRE(!bad[0], "a sample's left node is outside 0 .. nk-1, its fraction outside [0, 1], or it is node nk-1 with a "
                     "non-zero fraction");
    REQUIRE(!bad[1], "a triangle names a sample outside 0 .. n-1");
    REQUIRE(!bad[2], "a triangle does not close at some redshift: k_max > (k_mid + k_min)(1 + 2^-40)");
    for (int u = 0; u < A.nu; ++u) {            // one prepass per distinct leg; it writes J for every leg it serves
        int legs = 0;
        for (int l = 0; l < 3; ++l) legs |= (A.slot[l] == u) << l;
        hipLaunchKernelGGL(bispectrum_legs_kernel, dim3(A.nz), dim3(BIS_THREADS), 0, c->stream, A, A.uq[u], legs);
        HIP_TRY(hipGetLastError());
    }
    if (A.B) {
        hipLaunchKernelGGL(bispectrum_kernel, dim3((A.nt - 1) / BIS_BLOCK + 1, A.nz), dim3(BIS_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
    }
    if (Bz) {
        hipLaunchKernelGGL(bispectrum_zsum_kernel, grid1d((size_t)3 * A.nt, 256), dim3(256), 0, c->stream, A.nz, A.nt,
                           zweights, A.B, Bz);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// the prepass alone, for hmg_response (response.hip): see kernels/leg_form.hpp
int hmg::bis_legs_launch(hmg_ctx* c, const BisLeg& L, int nz, int nm, int nk, int n, const double* nzm, const double* bh,
                         const double* ms, const double* wm, const double* ks, const double* Pzk, double rho_m0,
                         double kstar, const int* idx, const double* frac, double* J, double* Ps, double* Ds, double* Ks) {
    BisArgs A = {};
    A.nu = 1;
    A.uq[0] = A.uq[1] = A.uq[2] = L;
    A.nzm = nzm; A.bh = bh; A.ms = ms; A.wm = wm; A.ks = ks; A.Pzk = Pzk;
    A.rho_m0 = rho_m0; A.kstar = kstar;
    A.idx = idx; A.frac = frac;
    A.nz = nz; A.nm = nm; A.nk = nk; A.n = n; A.nt = 0; A.chunk = bis_chunk(n);
    // leg bit 0 also samples P, D and k; bit 1 writes the plane behind A.J and nothing else
    A.J = Ps ? J : J - (size_t)nz * n;
    A.Ps = Ps; A.Ds = Ds; A.Ks = Ks;
    hipLaunchKernelGGL(bispectrum_legs_kernel, dim3(nz), dim3(BIS_THREADS), 0, c->stream, A, L, Ps ? 1 : 2);
    HIP_TRY(hipGetLastError());
    return 0;
}

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
    for (auto t : tr)       // (an NFW tensor with deferred series tiles is filled first)
        if (series_ensure_whole(c, t->d_prof) || series_ensure_whole(c, t->d_cprof)) return 1;
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
    // The words of the check, the sampled P, D and k, and whichever of J and the per-z terms the caller did not ask for
    // are one ordinary block of the context's allocator (no scratch arena grows here: a captured step may have an
    // arena's address baked in).  It goes back to the free list before this returns; whatever reuses it is enqueued
    // behind the kernels below.
    const size_t zn = (size_t)nz * n, znt = (size_t)nz * nt;
    const bool need_b = B || Bz;
    void* blk = nullptr;
    if (hmg_malloc(c, 64 + 8 * (3 * zn + (J ? 0 : 3 * zn) + (need_b && !B ? 3 * znt : 0)), &blk)) return 1;
    double* w = (double*)((char*)blk + 64);
    A.Ps = w; A.Ds = w + zn; A.Ks = w + 2 * zn;
    w += 3 * zn;
    if (J) A.J = J; else { A.J = w; w += 3 * zn; }
    A.B = B ? B : need_b ? w : nullptr;
    A.nzm = nzm; A.bh = bh; A.ms = ms; A.wm = wm; A.ks = ks; A.Pzk = Pzk;
    A.rho_m0 = rho_m0; A.kstar = kstar;
    A.idx = idx; A.frac = frac; A.scale = scale; A.tri = tri;
    A.nz = nz; A.nm = nm; A.nk = nk; A.n = n; A.nt = nt; A.chunk = bis_chunk(n);
    const int rc = bis_run(c, A, zweights, Bz, (int*)blk);
    return hmg_free(c, blk) || rc;
}
