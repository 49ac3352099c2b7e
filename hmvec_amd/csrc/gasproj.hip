// Projected generalised-NFW profiles: the C-ABI entry points hmg_gnfw_projected, hmg_gnfw_projected_smooth and
// hmg_gnfw_quad_table (include/hmgrid.h) and their kernels (kernels/gasproj.hpp).  A translation unit of its own: the
// headline path's units (hmgrid.hip, longgrid.hip) do not see these instantiations.  Definitions and accuracy: DESIGN.md
// section 18.
#include <cmath>
#include <cstring>

#include "hmctx.hpp"
#include "kernels/gasproj.hpp"

using namespace hmg;

static_assert(sizeof(GnfwQuad) == HMG_GNFW_TABLE_DOUBLES * sizeof(double), "hmgrid.h describes the node table");

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

GnfwQuad build_gnfw_quad() {
    GnfwQuad q;
    gauss_legendre01(GNFW_N, q.u, q.w);
    for (int i = 0; i < GNFW_N; ++i) {           // r = b v^2: dr = 2 b v dv
        q.v2[i] = q.u[i] * q.u[i];
        q.lv2[i] = 2.0 * std::log(q.u[i]);
        q.wv[i] = 2.0 * q.u[i] * q.w[i];
    }
    double u[GNFW_NS], w[GNFW_NS];
    gauss_legendre01(GNFW_NS, u, w);
    for (int k = 0; k < GNFW_NS; ++k) {          // g = sin^2(pi u / 2): dg = (pi/2) sin(pi u) du
        const double sn = std::sin(0.5 * M_PI * u[k]), cs = std::cos(0.5 * M_PI * u[k]);
        q.sg[k] = sn * sn;
        q.cg[k] = cs * cs;
        q.wj[k] = w[k] * 0.5 * M_PI * std::sin(M_PI * u[k]);
    }
    return q;
}

const GnfwQuad& gnfw_quad_host() {
    static const GnfwQuad q = build_gnfw_quad();
    return q;
}

constexpr int MAX_DEVICES = 64;
bool quad_ready[MAX_DEVICES] = {};

// copies the node table to its __constant__ symbol before the first launch on a device
int upload_quad(hmg_ctx* c) {
    REQUIRE(c->device >= 0 && c->device < MAX_DEVICES, "device index out of range");
    if (quad_ready[c->device]) return 0;
    REQUIRE(!c->capturing, "the projection's node table cannot be uploaded inside a captured step: run the call once "
                           "eagerly first");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gnfw_quad), &gnfw_quad_host(), sizeof(GnfwQuad), 0, hipMemcpyHostToDevice));
    quad_ready[c->device] = true;
    return 0;
}

constexpr int SMOOTH_WAVES = 4;

// the checks both entry points share; sigma == nullptr: the unsmoothed kernel
int launch(hmg_ctx* c, int n, int nr, int per_row_x, int kind, const double* alpha, const double* eta,
           const double* xcut, double gamma, const double* x, const double* sigma, bool smooth, double* out) {
    REQUIRE(c && alpha && eta && xcut && x && out && (sigma || !smooth), "NULL argument");
    REQUIRE(n > 0 && nr > 0, "empty grid");
    const int what = kind & ~HMG_GNFW_GENERAL;
    REQUIRE(what == HMG_GNFW_SIGMA || (!smooth && (what == HMG_GNFW_MEAN || what == HMG_GNFW_EXCESS)),
            smooth ? "only the projection itself (kind sigma) can be smoothed" : "unknown kind");
    REQUIRE(std::isfinite(gamma) && gamma > -1.0, "gamma must be finite and above -1");
    const size_t total = (size_t)n * nr;
    const int per_block = smooth ? SMOOTH_WAVES : 256;
    REQUIRE((total + per_block - 1) / per_block <= 2147483647u, "grid too large");
    if (upload_quad(c)) return 1;
    const int general = (kind & HMG_GNFW_GENERAL) != 0;
    if (smooth)
        hipLaunchKernelGGL(gnfw_smooth_kernel<SMOOTH_WAVES>, grid1d(total, SMOOTH_WAVES), dim3(64 * SMOOTH_WAVES), 0,
                           c->stream, total, nr, per_row_x ? nr : 0, general, alpha, eta, xcut, gamma, x, sigma, out);
    else
        hipLaunchKernelGGL(gnfw_projected_kernel, grid1d(total, 256), dim3(256), 0, c->stream, total, nr,
                           per_row_x ? nr : 0, what, general, alpha, eta, xcut, gamma, x, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int hmg_gnfw_projected(hmg_ctx* c, int n, int nr, int per_row_x, int kind, const double* alpha, const double* eta,
                       const double* xcut, double gamma, const double* x, double* out) {
    return launch(c, n, nr, per_row_x, kind, alpha, eta, xcut, gamma, x, nullptr, false, out);
}

int hmg_gnfw_projected_smooth(hmg_ctx* c, int n, int nr, int per_row_x, int kind, const double* alpha, const double* eta,
                              const double* xcut, double gamma, const double* x, const double* sigma, double* out) {
    return launch(c, n, nr, per_row_x, kind, alpha, eta, xcut, gamma, x, sigma, true, out);
}

int hmg_gnfw_quad_table(double* h_table) {
    if (!h_table) return fail("invalid argument", "NULL argument", __FILE__, __LINE__);
    std::memcpy(h_table, &gnfw_quad_host(), sizeof(GnfwQuad));
    return 0;
}
