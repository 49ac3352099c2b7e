// Response of halo-model spectra to a long-wavelength density mode and the super-sample covariance: the C-ABI entry
// points hmg_response and hmg_ssc (include/hmgrid.h) and their kernels (kernels/response.hpp).  A translation unit of
// its own: the other units do not see these instantiations, and theirs do not change.  The leg prepass and the leg
// sums are sampled.hip's.  Definition, gates and resources: DESIGN.md section 17.
#include "hmctx.hpp"
#include "kernels/response.hpp"

using namespace hmg;

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
    if (tracers_ensure_whole(c, h_pairs, 2 * np)) return 1;
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
    RespArgs A = {};
    A.g = {nz, nm, nk, nzm, bh, ms, wm, ks, Pzk, rho_m0};
    A.s = {idx, frac, scale, n};
    A.dlnP = dlnP; A.R = R; A.parts = parts; A.np = np;
    // the block: the word of the check, the pairs' descriptions, the sampled k, P, D, J of every distinct leg and the
    // three planes (C, C0, beta) of the leg sums, a row per distinct leg each
    const size_t zn = (size_t)nz * n, unz = (size_t)nu * nz;
    const size_t desc_bytes = ((size_t)np * sizeof(RespPair) + 63) / 64 * 64;
    return with_block(c, 64 + desc_bytes + 8 * ((3 + (size_t)nu) * zn + 3 * unz), [&](void* blk) {
        RespPair* d_pairs = (RespPair*)((char*)blk + 64);
        double* w = (double*)((char*)blk + 64 + desc_bytes);
        double *Ks = w, *Ps = w + zn, *Ds = w + 2 * zn, *J = w + 3 * zn, *sums = w + (3 + (size_t)nu) * zn;
        // the wait of the table check also covers the copy of the descriptions out of this frame
        HIP_TRY(hipMemcpyAsync(d_pairs, hp, (size_t)np * sizeof(RespPair), hipMemcpyHostToDevice, c->stream));
        if (samples_checked(c, A.s, nz, nk, (int*)blk)) return 1;
        for (int u = 0; u < nu; ++u) {             // one prepass per distinct leg; the first also samples P, D and k
            LegOut out = {};
            out.J[0] = J + u * zn;
            if (u == 0) { out.Ps = Ps; out.Ds = Ds; out.Ks = Ks; }
            if (leg_prepass_launch(c, A.g, uq[u], idx, frac, n, kstar, out)) return 1;
            if (leg_sums_launch(c, A.g, uq[u], 0.0, unz, sums + (size_t)u * nz)) return 1;
        }
        A.pairs = d_pairs; A.J = J; A.beta = sums + 2 * unz; A.Ps = Ps; A.Ds = Ds;
        hipLaunchKernelGGL(response_pairs_kernel, dim3(np, nz), dim3(RESP_THREADS), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        return 0;
    });
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
