// Cluster-lensing profiles: the C-ABI entry points hmg_lensing_* (include/hmgrid.h) and their kernels
// (kernels/lensing.hpp).  A translation unit of its own: the headline path's units (hmgrid.hip, longgrid.hip) do not
// see these instantiations.  Definitions and accuracy: DESIGN.md sections 10 (Sigma, kappa) and 12 (Delta Sigma,
// gamma_t).
#include <cmath>

#include "hmctx.hpp"
#include "kernels/lensing.hpp"

using namespace hmg;

namespace {

// Gauss-Legendre nodes and weights on [0, 1] (Newton on P_n from the Chebyshev-like first guess)
void gauss_legendre01(int n, double* x, double* w) {
    for (int i = 0; i < n; ++i) {
        double t = std::cos(M_PI * (i + 0.75) / (n + 0.5)), p1 = 0.0, dp = 0.0;
        const auto legendre = [&] {                          // P_n(t) into p1, P_n'(t) into dp
            double p0 = 1.0;
            p1 = t;
            for (int k = 2; k <= n; ++k) {
                const double p2 = ((2.0 * k - 1.0) * t * p1 - (k - 1.0) * p0) / k;
                p0 = p1;
                p1 = p2;
            }
            dp = n * (t * p1 - p0) / (t * t - 1.0);
        };
        for (int it = 0; it < 100; ++it) {
            legendre();
            const double dt = p1 / dp;
            t -= dt;
            if (std::fabs(dt) < 1e-16) break;
        }
        legendre();                                          // P_n' at the converged node for the weight
        x[n - 1 - i] = 0.5 * (t + 1.0);                      // ascending
        w[n - 1 - i] = 1.0 / ((1.0 - t * t) * dp * dp);      // 2 / ((1-t^2) P'^2), halved for [0, 1]
    }
}

LensQuad build_lens_quad() {
    LensQuad q;
    gauss_legendre01(LENS_QUAD_N / 2, q.w_outer, q.wt_outer);
    double x[LENS_QUAD_N], w[LENS_QUAD_N];
    gauss_legendre01(LENS_QUAD_N, x, w);
    for (int j = 0; j < LENS_QUAD_N; ++j) {      // phi = pi u^3: (1/pi) dphi = 3 u^2 du
        const double phi = M_PI * x[j] * x[j] * x[j];
        const double s = std::sin(0.5 * phi);
        q.s2_phi[j] = s * s;
        q.wt_phi[j] = 3.0 * x[j] * x[j] * w[j];
    }
    return q;
}

LensDiscQuad build_lens_disc_quad() {
    LensDiscQuad q;
    double x[LENS_QUAD_N], w[LENS_QUAD_N];
    gauss_legendre01(LENS_QUAD_N, x, w);
    for (int j = 0; j < LENS_QUAD_N; ++j) {      // psi = pi u^2: dpsi = 2 pi u du
        const double psi = M_PI * x[j] * x[j];
        const double s = std::sin(0.5 * psi), c = std::cos(0.5 * psi);
        q.sp[j] = s * s;
        q.cp[j] = c * c;
        q.wt[j] = 2.0 * M_PI * x[j] * w[j] * std::sin(psi);
    }
    return q;
}

constexpr int MAX_DEVICES = 64;
bool quad_ready[MAX_DEVICES] = {};
bool disc_quad_ready[MAX_DEVICES] = {};

// builds a quadrature table once and copies it to its __constant__ symbol before the first launch on a device
template <class Table>
int upload_once(hmg_ctx* c, Table (*build)(), const void* symbol, bool* ready) {
    REQUIRE(c->device >= 0 && c->device < MAX_DEVICES, "device index out of range");
    if (ready[c->device]) return 0;
    REQUIRE(!c->capturing, "the lensing quadrature table cannot be uploaded inside a captured step: run the call once "
                           "eagerly first");
    static const Table q = build();
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyToSymbol(symbol, &q, sizeof(q), 0, hipMemcpyHostToDevice));
    ready[c->device] = true;
    return 0;
}

constexpr int OFF_WAVES = 4;
constexpr int K2H_THREADS = 256;

// One launcher per family; its template argument is the kernel's: false / 0 for Sigma and kappa, true / 2 for
// Delta Sigma and gamma_t.
template <bool DELTA>
int launch_centred(hmg_ctx* c, int n, int nr, int rbins_per_halo, const double* rs, const double* delta_c,
                   const double* rho_crit, const double* rbins, double* out) {
    REQUIRE(c && rs && delta_c && rho_crit && rbins && out, "NULL argument");
    REQUIRE(n > 0 && nr > 0, "empty grid");
    const size_t total = (size_t)n * nr;
    REQUIRE((total + 255) / 256 <= 2147483647u, "grid too large");
    hipLaunchKernelGGL(lensing_centred_kernel<DELTA>, grid1d(total, 256), dim3(256), 0, c->stream, total, nr,
                       rbins_per_halo ? nr : 0, rs, delta_c, rho_crit, rbins, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the miscentred Delta Sigma kernel (DISC) reads both tables
template <bool DISC>
int launch_off(hmg_ctx* c, int n, int nr, int rbins_per_halo, const double* rs, const double* delta_c,
               const double* rho_crit, const double* rbins, const double* offsets, double* out) {
    REQUIRE(c && rs && delta_c && rho_crit && rbins && offsets && out, "NULL argument");
    REQUIRE(n > 0 && nr > 0, "empty grid");
    const size_t total = (size_t)n * nr;
    REQUIRE((total + OFF_WAVES - 1) / OFF_WAVES <= 2147483647u, "grid too large");
    if (upload_once(c, build_lens_quad, &lens_quad, quad_ready)) return 1;
    if (DISC && upload_once(c, build_lens_disc_quad, &lens_disc_quad, disc_quad_ready)) return 1;
    hipLaunchKernelGGL((lensing_off_kernel<OFF_WAVES, DISC>), grid1d(total, OFF_WAVES), dim3(64 * OFF_WAVES), 0,
                       c->stream, total, nr, rbins_per_halo ? nr : 0, rs, delta_c, rho_crit, rbins, offsets, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int ORDER>
int launch_two_halo(hmg_ctx* c, int nz, int nk, int ntheta, int nm, int nM, const double* ks, const double* chi,
                    const double* pre, const double* Pzk, const double* thetas, double lmin, double lmax,
                    const double* ms, const double* bh, const double* Ms, double* out) {
    REQUIRE(c && ks && chi && pre && Pzk && thetas && ms && bh && Ms && out, "NULL argument");
    REQUIRE(nz > 0 && nk > 0 && ntheta > 0 && nM > 0, "empty grid");
    REQUIRE(nm >= 2, "the bias interpolation needs at least two masses");
    REQUIRE(nz <= 65535, "nz too large");
    hipLaunchKernelGGL((lensing_2h_kernel<K2H_THREADS, ORDER>), dim3(ntheta, nz), dim3(K2H_THREADS), 0, c->stream, nk,
                       ntheta, nm, nM, ks, chi, pre, Pzk, thetas, lmin, lmax, ms, bh, Ms, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int hmg_lensing_sigma_nfw(hmg_ctx* c, int n, int nr, int rbins_per_halo, const double* rs, const double* delta_c,
                          const double* rho_crit, const double* rbins, double* out) {
    return launch_centred<false>(c, n, nr, rbins_per_halo, rs, delta_c, rho_crit, rbins, out);
}

int hmg_lensing_delta_sigma_nfw(hmg_ctx* c, int n, int nr, int rbins_per_halo, const double* rs, const double* delta_c,
                                const double* rho_crit, const double* rbins, double* out) {
    return launch_centred<true>(c, n, nr, rbins_per_halo, rs, delta_c, rho_crit, rbins, out);
}

int hmg_lensing_sigma_nfw_off(hmg_ctx* c, int n, int nr, int rbins_per_halo, const double* rs, const double* delta_c,
                              const double* rho_crit, const double* rbins, const double* offsets, double* out) {
    return launch_off<false>(c, n, nr, rbins_per_halo, rs, delta_c, rho_crit, rbins, offsets, out);
}

int hmg_lensing_delta_sigma_nfw_off(hmg_ctx* c, int n, int nr, int rbins_per_halo, const double* rs,
                                    const double* delta_c, const double* rho_crit, const double* rbins,
                                    const double* offsets, double* out) {
    return launch_off<true>(c, n, nr, rbins_per_halo, rs, delta_c, rho_crit, rbins, offsets, out);
}

int hmg_lensing_kappa_2h(hmg_ctx* c, int nz, int nk, int ntheta, int nm, int nM, const double* ks, const double* chi,
                         const double* pre, const double* Pzk, const double* thetas, double lmin, double lmax,
                         const double* ms, const double* bh, const double* Ms, double* out) {
    return launch_two_halo<0>(c, nz, nk, ntheta, nm, nM, ks, chi, pre, Pzk, thetas, lmin, lmax, ms, bh, Ms, out);
}

int hmg_lensing_gamma_t_2h(hmg_ctx* c, int nz, int nk, int ntheta, int nm, int nM, const double* ks, const double* chi,
                           const double* pre, const double* Pzk, const double* thetas, double lmin, double lmax,
                           const double* ms, const double* bh, const double* Ms, double* out) {
    return launch_two_halo<2>(c, nz, nk, ntheta, nm, nM, ks, chi, pre, Pzk, thetas, lmin, lmax, ms, bh, Ms, out);
}
