// Response of halo-model spectra to a long-wavelength density mode and the super-sample covariance: the C-ABI entry
// points hmg_response and hmg_ssc (include/hmgrid.h) and their kernels (kernels/response.hpp).  A translation unit of
// its own: the other units do not see these instantiations, and theirs do not change.  The leg prepass is launched
// through bispectrum.hip, which owns its kernel.  Definition, gates and resources: DESIGN.md section 17.
#include "hmctx.hpp"
#include "kernels/response.hpp"

using namespace hmg;

// the launches of one call; blk holds the word of the check, the pairs' descriptions and the doubles
static int resp_run(hmg_ctx* c, RespArgs& A, const RespPair* hp, const BisLeg* uq, int nu, const double* ks,
                    const double* Pzk, double kstar, void* blk, size_t desc_bytes) {
    int* d_bad = (int*)blk;
    RespPair* d_pairs = (RespPair*)((char*)blk + 64);
    double* w = (double*)((char*)blk + 64 + desc_bytes);
    const size_t zn = (size_t)A.nz * A.n;
    double *Ks = w, *Ps = w + zn, *Ds = w + 2 * zn, *J = w + 3 * zn, *beta = w + (3 + (size_t)nu) * zn;
    // the tables are checked on the device before anything reads a tensor through them; the same wait covers the copy of
    // the descriptions out of the caller's frame
    int bad = 0;
    HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int), c->stream));
    HIP_TRY(hipMemcpyAsync(d_pairs, hp, (size_t)A.np * sizeof(RespPair), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(response_check_kernel, grid1d(zn, 256), dim3(256), 0, c->stream, zn, A.nk, A.idx, A.frac, d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    REQUIRE(!bad, "a sample's left node is outside 0 .. nk-1, its fraction outside [0, 1], or it is node nk-1 with a "
                  "non-zero fraction");
    for (int u = 0; u < nu; ++u) {             // one prepass per distinct leg; the first also samples P, D and k
        if (bis_legs_launch(c, uq[u], A.nz, A.nm, A.nk, A.n, A.nzm, A.bh, A.ms, A.wm, ks, Pzk, A.rho_m0, kstar, A.idx,
                            A.frac, J + u * zn, u ? nullptr : Ps, u ? nullptr : Ds, u ? nullptr : Ks))
            return 1;
        hipLaunchKernelGGL(response_beta_kernel, dim3(A.nz), dim3(BIS_THREADS), 0, c->stream, uq[u], A.nm, A.nzm, A.bh,
                           A.ms, A.wm, A.rho_m0, beta + (size_t)u * A.nz);
        HIP_TRY(hipGetLastError());
    }
    A.pairs = d_pairs; A.J = J; A.beta = beta; A.Ps = Ps; A.Ds = Ds;
    hipLaunchKernelGGL(response_pairs_kernel, dim3(A.np, A.nz), dim3(RESP_THREADS), 0, c->stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int hmg_response(hmg_ctx* c, int nz, int nm, int nk, int n, int np, const hmg_tracer* h_pairs, const double* nzm,
                 const double* bh, const double* ms, const double* wm, const double* ks, const double* Pzk,
                 const double* dlnP, double rho_m0, double kstar, const int* idx, const double* frac, const double* scale,
                 double* R, double* parts) {
    REQUIRE(c && h_pairs && nzm && bh && ms && wm && ks && Pzk && dlnP && idx && frac && scale, "NULL argument");
    REQUIRE(R, "d_R is NULL: no output");
    REQUIRE(nz > 0 && nm > 0 && nk > 0, "empty grid");
    REQUIRE(n >= 1, "no sample points");
    REQUIRE(n <= RESP_THREADS, "more than 256 samples per redshift");
    REQUIRE(np >= 1, "no pairs");
    REQUIRE(np <= RESP_MAXP, "more than 16 pairs");
    REQUIRE(nz <= 65535, "nz too large");
    REQUIRE(!c->capturing, "hmg_response waits on the host for its table check and cannot be part of a captured step");
    for (int t = 0; t < 2 * np; ++t)       // (an NFW tensor with deferred series tiles is filled first)
        if (series_ensure_whole(c, h_pairs[t].d_prof) || series_ensure_whole(c, h_pairs[t].d_cprof)) return 1;
    RespPair hp[RESP_MAXP];
    BisLeg uq[2 * RESP_MAXP];
    int nu = 0;
    for (int p = 0; p < np; ++p) {
        int slot[2];
        for (int l = 0; l < 2; ++l) {
            BisLeg L;
            if (bis_leg(&h_pairs[2 * p + l], &L)) return 1;
            int u = 0;
            while (u < nu && !bis_same(uq[u], L)) ++u;
            if (u == nu) uq[nu++] = L;
            slot[l] = u;
        }
        if (tri_side(&h_pairs[2 * p], &h_pairs[2 * p + 1], &hp[p].S)) return 1;
        hp[p].la = slot[0];
        hp[p].lb = slot[1];
    }
    // The word of the check, the pairs' descriptions, the sampled k, P, D, and J and beta of every distinct leg are one
    // ordinary block of the context's allocator (no scratch arena grows here: a captured step may have an arena's
    // address baked in).  It goes back to the free list before this returns; whatever reuses it is enqueued behind the
    // kernels above.
    const size_t zn = (size_t)nz * n;
    const size_t desc_bytes = ((size_t)np * sizeof(RespPair) + 63) / 64 * 64;
    void* blk = nullptr;
    if (hmg_malloc(c, 64 + desc_bytes + 8 * ((3 + (size_t)nu) * zn + (size_t)nu * nz), &blk)) return 1;
    RespArgs A = {};
    A.nzm = nzm; A.bh = bh; A.ms = ms; A.wm = wm; A.dlnP = dlnP; A.rho_m0 = rho_m0;
    A.idx = idx; A.frac = frac; A.scale = scale;
    A.R = R; A.parts = parts;
    A.nz = nz; A.nm = nm; A.nk = nk; A.n = n; A.np = np;
    const int rc = resp_run(c, A, hp, uq, nu, ks, Pzk, kstar, blk, desc_bytes);
    return hmg_free(c, blk) || rc;
}

int hmg_ssc(hmg_ctx* c, int nz, int n, int np, const double* R, const double* zscale, const double* g, double* cov) {
    REQUIRE(c && R && g, "NULL argument");
    REQUIRE(cov, "d_cov is NULL: no output");
    REQUIRE(nz > 0, "empty grid");
    REQUIRE(n >= 1, "no sample points");
    REQUIRE(n <= RESP_THREADS, "more than 256 samples per redshift");
    REQUIRE(np >= 1, "no pairs");
    REQUIRE(np <= RESP_MAXP, "more than 16 pairs");
    REQUIRE(!c->capturing, "hmg_ssc contracts what hmg_response wrote, which cannot be part of a captured step");
    const int N = np * n, tiles = (N - 1) / SSC_TILE + 1;
    hipLaunchKernelGGL(ssc_kernel, dim3(tiles, tiles), dim3(SSC_THREADS), 0, c->stream, nz, n, N, R, zscale, g, cov);
    HIP_TRY(hipGetLastError());
    return 0;
}
