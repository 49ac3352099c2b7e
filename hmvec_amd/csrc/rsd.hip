// Redshift-space spectra of the dispersion halo model: the C-ABI entry points hmg_rsd_wedges and hmg_rsd_multipoles
// (include/hmgrid.h) and their kernels (kernels/rsd.hpp, gauss_moments.hpp).  A translation unit of its own: the other
// units do not see these instantiations, and theirs do not change.  It launches nothing of another unit: the k- and
// mu-independent sums C, C0, b of a leg come from a small kernel here.  Definition, gates and resources: DESIGN.md
// section 19.
#include "hmctx.hpp"
#include "kernels/rsd.hpp"

using namespace hmg;

namespace {

struct RsdCall {                    // what the two entry points share
    int nz, nm, nk, n, nmu;
    const hmg_tracer *ta, *tb;
    const double *nzm, *bh, *ms, *wm, *ks, *Pzk;
    double rho_m0;
    const int* kidx;
    const double *damp, *mus, *sigma, *f;
    double am, ac, as;
};

int rsd_checked(hmg_ctx* c, const RsdCall& q) {
    REQUIRE(c && q.ta && q.tb && q.nzm && q.bh && q.ms && q.wm && q.ks && q.Pzk && q.kidx && q.damp && q.mus && q.sigma &&
                q.f, "NULL argument");
    REQUIRE(q.nz > 0 && q.nm > 0 && q.nk > 0, "empty grid");
    REQUIRE(q.n >= 1, "no sample points");
    REQUIRE(q.n <= q.nk, "more samples than nodes of the k grid");
    REQUIRE(q.nmu >= 1, "no mu nodes");
    REQUIRE(q.nmu <= RSD_MAXMU, "more than 32 mu nodes");
    REQUIRE(q.nz <= 65535, "nz too large");
    REQUIRE(q.ta->kind != HMG_TRACER_PRESSURE && q.tb->kind != HMG_TRACER_PRESSURE,
            "a pressure tracer has no redshift-space spectrum");
    REQUIRE(!c->capturing, "the call waits on the host for its table check and cannot be part of a captured step");
    return 0;
}

// the argument block of the kernels from the call; blk holds the word of the check and the legs' sums
int rsd_prepare(hmg_ctx* c, const RsdCall& q, RsdArgs& A, void* blk) {
    // (an NFW tensor with deferred series tiles is filled first)
    for (const hmg_tracer* t : {q.ta, q.tb})
        if (series_ensure_whole(c, t->d_prof) || series_ensure_whole(c, t->d_cprof)) return 1;
    if (bis_leg(q.ta, &A.a) || bis_leg(q.tb, &A.b)) return 1;
    A.same = bis_same(A.a, A.b);
    A.hh = q.ta->kind == HMG_TRACER_HOD && q.tb->kind == HMG_TRACER_HOD;
    if (A.hh) {
        REQUIRE(q.ta->d_NcNs && q.ta->d_NsNsm1, "HOD tracer needs NcNs,NsNsm1");
        A.NcNs = q.ta->d_NcNs; A.NsNsm1 = q.ta->d_NsNsm1;
    }
    const double hm = 0.5 * (q.am * q.am), hc = 0.5 * (q.ac * q.ac), hs = 0.5 * (q.as * q.as);
    A.ha0 = hc; A.ha1 = q.ta->kind == HMG_TRACER_HOD ? hs : hm;
    A.hb0 = hc; A.hb1 = q.tb->kind == HMG_TRACER_HOD ? hs : hm;
    A.nzm = q.nzm; A.bh = q.bh; A.ms = q.ms; A.wm = q.wm; A.ks = q.ks; A.Pzk = q.Pzk; A.sigma = q.sigma; A.f = q.f;
    A.rho_m0 = q.rho_m0; A.kidx = q.kidx; A.damp = q.damp; A.mus = q.mus;
    A.nz = q.nz; A.nm = q.nm; A.nk = q.nk; A.n = q.n; A.nmu = q.nmu;
    int* d_bad = (int*)blk;
    double* legs = (double*)((char*)blk + 64);
    // the table is checked on the device before anything reads a tensor through it
    int bad = 0;
    HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(rsd_check_kernel, grid1d(q.n, 256), dim3(256), 0, c->stream, q.n, q.nk, q.kidx, d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    REQUIRE(!bad, "a sample's node is outside 0 .. nk-1");
    A.legs_a = legs;
    A.legs_b = A.same ? legs : legs + 3 * (size_t)q.nz;
    for (int u = 0; u < (A.same ? 1 : 2); ++u) {
        hipLaunchKernelGGL(rsd_legs_kernel, dim3(q.nz), dim3(BIS_THREADS), 0, c->stream, u ? A.b : A.a, q.nz, q.nm, q.nzm,
                           q.bh, q.ms, q.wm, q.rho_m0, legs + 3 * (size_t)q.nz * u);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

dim3 rsd_grid(const RsdArgs& A, int chunks) { return dim3((A.n - 1) / RSD_THREADS + 1, A.nz, chunks); }

int rsd_wedges_run(hmg_ctx* c, const RsdCall& q, double* out, double* parts, void* blk) {
    RsdArgs A = {};
    if (rsd_prepare(c, q, A, blk)) return 1;
    A.out = out; A.parts = parts;
    hipLaunchKernelGGL(rsd_wedge_kernel<true>, rsd_grid(A, (q.nmu - 1) / RSD_MU + 1), dim3(RSD_THREADS), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int rsd_multipoles_run(hmg_ctx* c, const RsdCall& q, const double* wl, double* out, double* Q, void* blk) {
    RsdArgs A = {};
    if (rsd_prepare(c, q, A, blk)) return 1;
    A.out = out; A.parts = Q; A.wl = wl;
    A.w2h = (double*)((char*)blk + 64) + 6 * (size_t)q.nz;
    hipLaunchKernelGGL(rsd_multipole_kernel, rsd_grid(A, 1), dim3(RSD_THREADS), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rsd_wedge_kernel<false>, rsd_grid(A, (q.nmu - 1) / RSD_MU + 1), dim3(RSD_THREADS), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rsd_contract_kernel, grid1d((size_t)q.nz * q.n, 256), dim3(256), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

// The temporaries of either call - the word of the check, C, C0, b of the two legs and, of the multipoles, the 2-halo
// wedge - are one ordinary block of the context's allocator.  It goes back to the free list before the call returns;
// whatever reuses it is enqueued behind the kernels above.
int hmg_rsd_wedges(hmg_ctx* c, int nz, int nm, int nk, int n, int nmu, const hmg_tracer* h_a, const hmg_tracer* h_b,
                   const double* nzm, const double* bh, const double* ms, const double* wm, const double* ks,
                   const double* Pzk, double rho_m0, const int* kidx, const double* damp, const double* mus,
                   const double* sigma, const double* f, double alpha_m, double alpha_c, double alpha_s, double* out,
                   double* parts) {
    const RsdCall q = {nz, nm, nk, n, nmu, h_a, h_b, nzm, bh, ms, wm, ks, Pzk, rho_m0, kidx, damp, mus, sigma, f,
                       alpha_m, alpha_c, alpha_s};
    if (rsd_checked(c, q)) return 1;
    REQUIRE(out, "d_out is NULL: no output");
    void* blk = nullptr;
    if (hmg_malloc(c, 64 + 8 * 6 * (size_t)nz, &blk)) return 1;
    const int rc = rsd_wedges_run(c, q, out, parts, blk);
    return hmg_free(c, blk) || rc;
}

int hmg_rsd_multipoles(hmg_ctx* c, int nz, int nm, int nk, int n, int nmu, const hmg_tracer* h_a, const hmg_tracer* h_b,
                       const double* nzm, const double* bh, const double* ms, const double* wm, const double* ks,
                       const double* Pzk, double rho_m0, const int* kidx, const double* damp, const double* mus,
                       const double* wl, const double* sigma, const double* f, double alpha_m, double alpha_c,
                       double alpha_s, double* out, double* Q) {
    const RsdCall q = {nz, nm, nk, n, nmu, h_a, h_b, nzm, bh, ms, wm, ks, Pzk, rho_m0, kidx, damp, mus, sigma, f,
                       alpha_m, alpha_c, alpha_s};
    if (rsd_checked(c, q)) return 1;
    REQUIRE(wl, "NULL argument");
    REQUIRE(out, "d_out is NULL: no output");
    void* blk = nullptr;
    if (hmg_malloc(c, 64 + 8 * (6 * (size_t)nz + (size_t)nz * n * nmu), &blk)) return 1;
    const int rc = rsd_multipoles_run(c, q, wl, out, Q, blk);
    return hmg_free(c, blk) || rc;
}
