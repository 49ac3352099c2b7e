// One leg of a halo-model spectrum: the weight w(z,m,k) of a single tracer in get_power_1halo's cross-spectrum case as a
// linear form in its tensors, its k -> 0 limit and the HOD bias term - the pieces of the 2-halo bracket J that the units
// which form it share: bispectrum.hip and response.hip (section 17).  Device functions and host
// helpers only, no kernel.  The tracer weights restate tracer_form / power_prep_kernel of kernels/power.hpp, which is
// not a stand-alone header.
#pragma once

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

// a sample's table entry is usable: left node on the grid, fraction in [0, 1], node nk - 1 only with fraction 0
__device__ __forceinline__ bool bis_sample_ok(int id, double f, int nk) {
    return id >= 0 && id < nk && f >= 0.0 && f <= 1.0 && !(id == nk - 1 && f != 0.0);
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

// The leg prepass of section 16 (bispectrum_legs_kernel) for one leg, enqueued on the context's stream by the unit that
// owns the kernel (bispectrum.hip): J (nz, n) = (I + b) - C at the samples and, if Ps, P_lin, the damping factor and
// the wavenumber at the samples (kstar <= 0: D = 1).  When Ps is NULL the zn doubles before J must belong to the
// caller's block (the kernel addresses J as the second plane of an array).
int bis_legs_launch(hmg_ctx* c, const BisLeg& L, int nz, int nm, int nk, int n, const double* nzm, const double* bh,
                    const double* ms, const double* wm, const double* ks, const double* Pzk, double rho_m0, double kstar,
                    const int* idx, const double* frac, double* J, double* Ps, double* Ds, double* Ks);

}  // namespace hmg
