// One leg of a halo-model spectrum: the weight w(z,m,k) of a single tracer in get_power_1halo's cross-spectrum case as a
// linear form in its tensors, its k -> 0 limit and the HOD bias term - the pieces of the 2-halo bracket J that the units
// which form it share: sampled.hip (the leg prepass and the leg sums), bispectrum.hip,
// response.hip (section 17) and rsd.hip (section 19).  Device functions and host helpers only, no kernel.  The tracer
// weights restate tracer_form / power_prep_kernel of kernels/power.hpp, which is not a stand-alone header.
#pragma once
#include "sampled.hpp"

namespace hmg {

constexpr int BIS_THREADS = 256;
constexpr int BIS_PREP_CHUNK = 256;                 // mass bins per step of the leg prepass

struct BisLeg {                     // w(z,m,k) = c0(z,m) + c1(z,m) prof(z,m,k) + c2(z,m) cprof(z,m,k)
    int kind;
    const double *prof, *cprof;     // cprof: an HOD's central profile or NULL
    const double *Nc, *Ns, *ngal;
};

// the coefficients of one leg's weight at (z, m), its k -> 0 limit (lowk) and - of an HOD - Nc + Ns
__device__ __forceinline__ void bis_leg_form(const BisLeg& L, size_t zm, int z, double mass, double rho_m0, double* c,
                                             double& lowk, double& ngals) {
    c[0] = c[1] = c[2] = 0.0;
    ngals = 0.0;
    if (L.kind == HMG_TRACER_MATTER) {
        c[1] = mass / rho_m0;
        lowk = c[1];
    } else if (L.kind == HMG_TRACER_PRESSURE) {
        c[1] = 1.0;
        lowk = 0.0;
    } else {
        const double ng = L.ngal[z], nc = L.Nc[zm], ns = L.Ns[zm];
        if (L.cprof) c[2] = nc / ng; else c[0] = nc / ng;
        c[1] = ns / ng;
        lowk = (nc + ns) / ng;
        ngals = nc + ns;
    }
}

__device__ __forceinline__ double bis_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = BIS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double bis_leg_node(const BisLeg& L, const double* c, size_t at) {
    double v = fma(c[1], L.prof[at], c[0]);
    if (L.cprof) v = fma(c[2], L.cprof[at], v);
    return v;
}

// the weight interpolated to a sample; `at` is the offset of (z, m, left node).  Node id + 1 is read only where f != 0.
__device__ __forceinline__ double bis_leg_at(const BisLeg& L, const double* c, size_t at, double f) {
    double v = bis_leg_node(L, c, at);
    if (f != 0.0) v = fma(f, bis_leg_node(L, c, at + 1), (1.0 - f) * v);
    return v;
}

// ---- host side: a leg from its hmg_tracer
static inline int bis_leg(const hmg_tracer* t, BisLeg* L) {
    REQUIRE(t->kind == HMG_TRACER_MATTER || t->kind == HMG_TRACER_HOD || t->kind == HMG_TRACER_PRESSURE,
            "unknown tracer kind");
    REQUIRE(t->d_prof, "tracer has no profile tensor");
    L->kind = t->kind;
    L->prof = t->d_prof;
    L->cprof = nullptr;
    L->Nc = L->Ns = L->ngal = nullptr;
    if (t->kind == HMG_TRACER_HOD) {
        REQUIRE(t->d_Nc && t->d_Ns && t->d_ngal, "HOD tracer needs Nc,Ns,ngal");
        L->cprof = t->d_cprof;
        L->Nc = t->d_Nc; L->Ns = t->d_Ns; L->ngal = t->d_ngal;
    }
    return 0;
}

static inline bool bis_same(const BisLeg& x, const BisLeg& y) {
    return x.kind == y.kind && x.prof == y.prof && x.cprof == y.cprof && x.Nc == y.Nc && x.Ns == y.Ns && x.ngal == y.ngal;
}

}  // namespace hmg
