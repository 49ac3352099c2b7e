// The frame of the units that contract the resident profile tensors over the mass axis at a table of sampled
// wavenumbers - trispectrum.hip, bispectrum.hip (16), response.hip (17), rsd.hip (19): the model
// block and the sample table as they travel to every kernel, the device functions of a sample, and the launchers of the
// small kernels the units share, which sampled.hip owns.  No kernel here: kernels live in exactly one unit.
#pragma once

namespace hmg {

struct HaloGrid {                   // the model block: what an entry point gets of the halo model, filled once per call
    int nz, nm, nk;
    const double *nzm, *bh;         // [nz][nm] mass function, halo bias (the trispectrum leaves bh, ks, Pzk NULL)
    const double *ms, *wm;          // [nm] masses, quadrature weights
    const double *ks, *Pzk;         // [nk], [nz][nk]
    double rho_m0;
};
struct SampleTable {
    const int* idx;                 // [nz][n] left node
    const double *frac, *scale;     // [nz][n]
    int n;
};

// a sample's table entry is usable: left node on the grid, fraction in [0, 1], node nk - 1 only with fraction 0
__device__ __forceinline__ bool bis_sample_ok(int id, double f, int nk) {
    return id >= 0 && id < nk && f >= 0.0 && f <= 1.0 && !(id == nk - 1 && f != 0.0);
}

// The wavenumber of a sample: ks[id] where f == 0, else RN(RN((1 - f) ks[id]) + RN(f ks[id + 1])) - three separately
// rounded operations, no contraction: a host that follows the contract gets the same bits, which the 3-halo kernel
// F2 needs (one ulp of a long side moves mu of a squeezed triangle by k_max / k_min ulp).
__device__ __forceinline__ double bis_sample_k(const double* __restrict__ ks, int id, double f) {
#pragma clang fp contract(off)
    const double k0 = ks[id];
    if (f == 0.0) return k0;
    const double a = (1.0 - f) * k0, b = f * ks[id + 1];
    return a + b;
}

// D = 1 - exp(-(k / kstar)^2) by a fixed sequence of separately rounded IEEE operations (hmvec_amd.bispectrum.damping
// is the same sequence in numpy: the two agree to the bit).  x = (k/kstar)^2 > 40 gives exactly 1 (exp(-x) < 2^-57).
// Else n = rint(x log2 e), t = -((x - n ln2_hi) - n ln2_lo) in [-0.35, 0.35] (n ln2_hi is exact: ln2_hi has 32
// significant bits, n < 2^6), exp(t) by its Taylor polynomial of degree 13 in Horner form (truncation < 2^-57), scaled
// by 2^-n.  exp(-x) is within 3 ulp, so D within 3 ulp(exp(-x)) + half an ulp of its own.
__device__ __forceinline__ double bis_damping(double k, double kstar) {
#pragma clang fp contract(off)
    const double q = k / kstar;
    const double x = q * q;
    if (!(x <= 40.0)) return 1.0;
    const double n = rint(x * 1.4426950408889634);
    const double r = (x - n * 6.93147180369123816490e-01) - n * 1.90821492927058770002e-10;
    const double t = -r;
    double p = 1.0 / 6227020800.0;
    p = p * t + 1.0 / 479001600.0;
    p = p * t + 1.0 / 39916800.0;
    p = p * t + 1.0 / 3628800.0;
    p = p * t + 1.0 / 362880.0;
    p = p * t + 1.0 / 40320.0;
    p = p * t + 1.0 / 5040.0;
    p = p * t + 1.0 / 720.0;
    p = p * t + 1.0 / 120.0;
    p = p * t + 1.0 / 24.0;
    p = p * t + 1.0 / 6.0;
    p = p * t + 0.5;
    p = p * t + 1.0;
    p = p * t + 1.0;
    return 1.0 - ldexp(p, -(int)n);
}

// ---- host side
// the refusal of a table with an entry that is not usable
constexpr const char* BAD_SAMPLE_TABLE =
    "a sample's left node is outside 0 .. nk-1, its fraction outside [0, 1], or it is node nk-1 with a non-zero fraction";

// the launchers of sampled.hip, each enqueued on the context's stream
struct BisLeg;                      // kernels/leg_form.hpp
struct LegOut {                     // what one launch of the leg prepass writes, each [nz][n]; a NULL is not written
    double* J[3];                   // the bracket, once per leg of the request that this tracer is
    double *Ps, *Ds, *Ks;           // sampled P_lin, damping factor, wavenumber: all three or none
};

// The table is checked on the device before anything reads a tensor through it: refuses unless every entry of
// idx, frac (nz, table.n) is usable (bis_sample_ok).  d_bad is a device word of the caller's; waits for the stream.
int samples_checked(hmg_ctx* c, const SampleTable& table, int nz, int nk, int* d_bad);
// out[e] = sum_z g[z] src[p nz stride + z stride + t] for e = p stride + t < count, z in order: the z sum of `count /
// stride` planes of (nz, stride) each.
int zsum_launch(hmg_ctx* c, int nz, size_t count, size_t stride, const double* g, const double* src, double* out);
// The leg prepass of section 16 for one leg: J = (I + b) - C at the samples and, if out.Ps, P_lin, the damping factor and
// the wavenumber at the samples (kstar <= 0: D = 1).
int leg_prepass_launch(hmg_ctx* c, const HaloGrid& g, const BisLeg& L, const int* idx, const double* frac, int n,
                       double kstar, const LegOut& out);
// The k- and mu-independent sums of one leg: out[z] = C, out[plane + z] = C0, out[2 plane + z] = b, with b = b_other of a
// leg that is not an HOD.
int leg_sums_launch(hmg_ctx* c, const HaloGrid& g, const BisLeg& L, double b_other, size_t plane, double* out);

}  // namespace hmg
