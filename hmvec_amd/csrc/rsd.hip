// Redshift-space spectra of the dispersion halo model: the C-ABI entry points hmg_rsd_wedges and hmg_rsd_multipoles
// (include/hmgrid.h) and their kernels (kernels/rsd.hpp, gauss_moments.hpp).  A translation unit of its own: the other
// units do not see these instantiations, and theirs do not change.  The k- and mu-independent sums C, C0, b of a leg are
// the leg sums of sampled.hip.  Definition, gates and resources: DESIGN.md section 19.
#include "hmctx.hpp"
#include "kernels/rsd.hpp"

using namespace hmg;

namespace {

struct RsdCall {                    // what the two entry points share
    HaloGrid g;
    int n, nmu;
    const hmg_tracer *ta, *tb;
    const int* kidx;
    const double *damp, *mus, *sigma, *f;
    double am, ac, as;
};

int rsd_checked(hmg_ctx* c, const RsdCall& q) {
    REQUIRE(c && q.ta && q.tb && q.g.nzm && q.g.bh && q.g.ms && q.g.wm && q.g.ks && q.g.Pzk && q.kidx && q.damp && q.mus &&
                q.sigma && q.f, "NULL argument");
    REQUIRE(q.g.nz > 0 && q.g.nm > 0 && q.g.nk > 0, "empty grid");
    REQUIRE(q.n >= 1, "no sample points");
    REQUIRE(q.n <= q.g.nk, "more samples than nodes of the k grid");
    REQUIRE(q.nmu >= 1, "no mu nodes");
    REQUIRE(q.nmu <= RSD_MAXMU, "more than 32 mu nodes");
    REQUIRE(q.g.nz <= 65535, "nz too large");
    REQUIRE(q.ta->kind != HMG_TRACER_PRESSURE && q.tb->kind != HMG_TRACER_PRESSURE,
            "a pressure tracer has no redshift-space spectrum");
    REQUIRE(!c->capturing, "the call waits on the host for its table check and cannot be part of a captured step");
    return 0;
}

// the argument block of the kernels from the call; blk holds the word of the check and the legs' sums
int rsd_prepare(hmg_ctx* c, const RsdCall& q, RsdArgs& A, void* blk) {
    const hmg_tracer* tr[2] = {q.ta, q.tb};
    if (tracers_ensure_whole(c, tr, 2)) return 1;
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
    A.g = q.g; A.sigma = q.sigma; A.f = q.f;
    A.kidx = q.kidx; A.damp = q.damp; A.mus = q.mus;
    A.n = q.n; A.nmu = q.nmu;
    int* d_bad = (int*)blk;
    double* legs = (double*)((char*)blk + 64);
    // the table is checked on the device before anything reads a tensor through it
    int bad = 0;
    if (check_words(c, d_bad, &bad, 1, [&] {
            hipLaunchKernelGGL(rsd_check_kernel, grid1d(q.n, 256), dim3(256), 0, c->stream, q.n, q.g.nk, q.kidx, d_bad);
        }))
        return 1;
    REQUIRE(!bad, "a sample's node is outside 0 .. nk-1");
    const size_t nz = q.g.nz;
    A.legs_a = legs;
    A.legs_b = A.same ? legs : legs + 3 * nz;
    for (int u = 0; u < (A.same ? 1 : 2); ++u)             // (b of a matter name is 1)
        if (leg_sums_launch(c, q.g, u ? A.b : A.a, 1.0, nz, legs + 3 * nz * u)) return 1;
    return 0;
}

dim3 rsd_grid(const RsdArgs& A, int chunks) { return dim3((A.n - 1) / RSD_THREADS + 1, A.g.nz, chunks); }

}  // namespace

// The block of either call: the word of the check, C, C0, b of the two legs and, of the multipoles, the 2-halo wedge.
int hmg_rsd_wedges(hmg_ctx* c, int nz, int nm, int nk, int n, int nmu, const hmg_tracer* h_a, const hmg_tracer* h_b,
                   const double* nzm, const double* bh, const double* ms, const double* wm, const double* ks,
                   const double* Pzk, double rho_m0, const int* kidx, const double* damp, const double* mus,
                   const double* sigma, const double* f, double alpha_m, double alpha_c, double alpha_s, double* out,
                   double* parts) {
    const RsdCall q = {{nz, nm, nk, nzm, bh, ms, wm, ks, Pzk, rho_m0}, n, nmu, h_a, h_b, kidx, damp, mus, sigma, f,
                       alpha_m, alpha_c, alpha_s};
    if (rsd_checked(c, q)) return 1;
    REQUIRE(out, "d_out is NULL: no output");
    return with_block(c, 64 + 8 * 6 * (size_t)nz, [&](void* blk) {
        RsdArgs A = {};
        if (rsd_prepare(c, q, A, blk)) return 1;
        A.out = out; A.parts = parts;
        hipLaunchKernelGGL(rsd_wedge_kernel<true>, rsd_grid(A, (nmu - 1) / RSD_MU + 1), dim3(RSD_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int hmg_rsd_multipoles(hmg_ctx* c, int nz, int nm, int nk, int n, int nmu, const hmg_tracer* h_a, const hmg_tracer* h_b,
                       const double* nzm, const double* bh, const double* ms, const double* wm, const double* ks,
                       const double* Pzk, double rho_m0, const int* kidx, const double* damp, const double* mus,
                       const double* wl, const double* sigma, const double* f, double alpha_m, double alpha_c,
                       double alpha_s, double* out, double* Q) {
    const RsdCall q = {{nz, nm, nk, nzm, bh, ms, wm, ks, Pzk, rho_m0}, n, nmu, h_a, h_b, kidx, damp, mus, sigma, f,
                       alpha_m, alpha_c, alpha_s};
    if (rsd_checked(c, q)) return 1;
    REQUIRE(wl, "NULL argument");
    REQUIRE(out, "d_out is NULL: no output");
    return with_block(c, 64 + 8 * (6 * (size_t)nz + (size_t)nz * n * nmu), [&](void* blk) {
        RsdArgs A = {};
        if (rsd_prepare(c, q, A, blk)) return 1;
        A.out = out; A.parts = Q; A.wl = wl;
        A.w2h = (double*)((char*)blk + 64) + 6 * (size_t)nz;
        hipLaunchKernelGGL(rsd_multipole_kernel, rsd_grid(A, 1), dim3(RSD_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(rsd_wedge_kernel<false>, rsd_grid(A, (nmu - 1) / RSD_MU + 1), dim3(RSD_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(rsd_contract_kernel, grid1d((size_t)nz * n, 256), dim3(256), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
