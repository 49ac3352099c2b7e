// The sampled square term of get_power_1halo, S_ab(z, m, k) = x1(k) x2(k) with x1, x2 linear forms in the pair's
// tensors: the device functions and the host-side description of one spectrum (a, b) that the units which integrate it
// share - trispectrum.hip and response.hip (section 17).  Device functions and host helpers
// only, no kernel: each unit instantiates its own.  The tracer logic restates tracer_form / power_prep_kernel of
// kernels/power.hpp, which is not a stand-alone header.
#pragma once
#include "sampled.hpp"

namespace hmg {

constexpr int TRI_MAXT = 4;         // distinct tensors of one pair
constexpr int TRI_NC = 1 + TRI_MAXT;

struct TriTracer {
    int kind;
    int t_prof, t_cprof;            // slots in the pair's tensor list, -1 = none
    const double *Nc, *Ns, *NcNs, *NsNsm1, *ngal;
};
struct TriSide {                    // one spectrum (a, b): its square term is form1 * form2
    TriTracer a, b;
    int nt;
    const double* tens[TRI_MAXT];
};

// c[0..TRI_NC) += the linear form of one tracer's 1-halo weight (c lives in LDS: the slots are run-time indices)
__device__ __forceinline__ void tri_tracer_form(const TriTracer& T, size_t zm, int z, double mass, double rho_m0,
                                                double* c) {
    if (T.kind == HMG_TRACER_MATTER) {
        c[1 + T.t_prof] += mass / rho_m0;
    } else if (T.kind == HMG_TRACER_PRESSURE) {
        c[1 + T.t_prof] += 1.0;
    } else {
        const double ng = T.ngal[z], nc = T.Nc[zm], ns = T.Ns[zm];
        if (T.t_cprof >= 0) c[1 + T.t_cprof] += nc / ng; else c[0] += nc / ng;
        c[1 + T.t_prof] += ns / ng;
    }
}

// the two linear forms x1, x2 of the square term S = x1 * x2 of one spectrum at (z, m) (hmvec/hmvec.py:510-523)
__device__ __forceinline__ void tri_square_forms(const TriSide& S, size_t zm, int z, double mass, double rho_m0,
                                                 double* x1, double* x2) {
    for (int i = 0; i < TRI_NC; ++i) x1[i] = x2[i] = 0.0;
    if (S.a.kind == HMG_TRACER_HOD && S.b.kind == HMG_TRACER_HOD) {
        // (2 u_c u_s <NcNs> + <Ns(Ns-1)> u_s^2)/ngal^2 of the FIRST name
        const double ng = S.a.ngal[z], ng2 = ng * ng;
        x1[1 + S.a.t_prof] = 1.0;
        const double cc = 2.0 * S.a.NcNs[zm] / ng2;
        if (S.a.t_cprof >= 0) x2[1 + S.a.t_cprof] += cc; else x2[0] += cc;
        x2[1 + S.a.t_prof] += S.a.NsNsm1[zm] / ng2;
    } else if (S.a.kind == HMG_TRACER_PRESSURE && S.b.kind == HMG_TRACER_PRESSURE) {
        // pk_a**2 - first name only
        tri_tracer_form(S.a, zm, z, mass, rho_m0, x1);
        tri_tracer_form(S.a, zm, z, mass, rho_m0, x2);
    } else {
        tri_tracer_form(S.a, zm, z, mass, rho_m0, x1);
        tri_tracer_form(S.b, zm, z, mass, rho_m0, x2);
    }
}

// S(z, m, node) = x1(node) * x2(node) of one spectrum; `at` is the offset of (z, m, node) in its tensors
__device__ __forceinline__ double tri_square_at(const TriSide& S, const double* x1, const double* x2, size_t at) {
    double f1 = x1[0], f2 = x2[0];
#pragma unroll
    for (int t = 0; t < TRI_MAXT; ++t) {
        if (t < S.nt) {
            const double v = S.tens[t][at];
            f1 = fma(x1[1 + t], v, f1);
            f2 = fma(x2[1 + t], v, f2);
        }
    }
    return f1 * f2;
}

// ---- host side: one spectrum (a, b) from its two hmg_tracer
static inline int tri_slot(TriSide* S, const double* p) {
    if (!p) return -1;
    for (int i = 0; i < S->nt; ++i)
        if (S->tens[i] == p) return i;
    if (S->nt == TRI_MAXT) return -2;
    S->tens[S->nt] = p;
    return S->nt++;
}

static inline int tri_tracer(const hmg_tracer* t, bool stream, TriSide* S, TriTracer* out) {
    REQUIRE(t->kind == HMG_TRACER_MATTER || t->kind == HMG_TRACER_HOD || t->kind == HMG_TRACER_PRESSURE,
            "unknown tracer kind");
    REQUIRE(t->d_prof, "tracer has no profile tensor");
    if (t->kind == HMG_TRACER_HOD)
        REQUIRE(t->d_Nc && t->d_Ns && t->d_NcNs && t->d_NsNsm1 && t->d_ngal, "HOD tracer needs Nc,Ns,NcNs,NsNsm1,ngal");
    out->kind = t->kind;
    out->t_prof = out->t_cprof = -1;
    if (stream) {
        out->t_prof = tri_slot(S, t->d_prof);
        if (t->kind == HMG_TRACER_HOD) out->t_cprof = tri_slot(S, t->d_cprof);
        REQUIRE(out->t_prof != -2 && out->t_cprof != -2, "bad tensor count");
    }
    out->Nc = t->d_Nc; out->Ns = t->d_Ns; out->NcNs = t->d_NcNs; out->NsNsm1 = t->d_NsNsm1; out->ngal = t->d_ngal;
    return 0;
}

// one spectrum (a, b): its tracers and the distinct tensors its square term reads - of two HOD or two pressure names
// the first name's alone (the reference's first-name-only rules)
static inline int tri_side(const hmg_tracer* a, const hmg_tracer* b, TriSide* S) {
    S->nt = 0;
    for (auto& p : S->tens) p = nullptr;
    const bool first_only = a->kind == b->kind && (a->kind == HMG_TRACER_HOD || a->kind == HMG_TRACER_PRESSURE);
    if (tri_tracer(a, true, S, &S->a)) return 1;
    if (tri_tracer(b, !first_only, S, &S->b)) return 1;
    return 0;
}

}  // namespace hmg
