// Host build of the weight functions of hmvec_amd/csrc/kernels/curvedsky.hpp (tests/test_curvedsky_cpu.py compiles and
// runs it): reads "l a b" per line as printf's %a writes them from standard input and prints K_w, K_gammat, K_xip, K_xim
// of the annulus [a, b] at the integer multipole l the same way, walking the header's recurrence from l = 0 at both
// edges.  Checks by itself what needs no reference: G(l; 0) = 0, spin-2 kinds vanish at l = 1, the series and the closed
// forms meet at their switches, and the values are finite.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../hmvec_amd/csrc/kernels/curvedsky.hpp"

static int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            ++fails;                                                    \
        }                                                               \
    } while (0)

// G of the four kinds at the multipole l >= 1 and the angle theta
static void g_all(int l, double theta, double* g) {
    const double sh = std::sin(0.5 * theta), s = sh * sh, t = 2.0 * s, x = 1.0 - t;
    hmg::cs_state q = hmg::cs_start(t);
    for (int k = 0; k < l; ++k) hmg::cs_step(q, (double)k, t, hmg::cs_consts_of((double)k).r);
    hmg::cs_g_all(q, hmg::cs_consts_of((double)l), (double)l, s, x, 15, g);
}

int main() {
    double g[4], h[4];
    for (int l = 1; l < 6; ++l) {
        g_all(l, 0.0, g);
        for (int k = 0; k < 4; ++k) CHECK(g[k] == 0.0);
    }
    g_all(1, 0.7, g);
    CHECK(g[0] != 0.0 && g[1] == 0.0 && g[2] == 0.0 && g[3] == 0.0);
    const int ls[3] = {3, 40, 1000};
    const double sw[2] = {hmg::CS_SWITCH_2, hmg::CS_SWITCH_4};
    for (int l : ls)
        for (double z : sw) {
            double th = 2.0 * std::asin(std::sqrt(z / (l * (l + 1.0))));
            // the neighbouring doubles on the two sides of M s = z
            double lo = th, hi = th;
            const double M = l * (l + 1.0);
            auto ms = [&](double v) { const double sh = std::sin(0.5 * v); return M * (sh * sh); };
            while (ms(lo) >= z) lo = std::nextafter(lo, 0.0);
            while (ms(hi) < z) hi = std::nextafter(hi, 4.0);
            g_all(l, lo, g), g_all(l, hi, h);
            for (int k = 0; k < 4; ++k) CHECK(std::fabs(g[k] - h[k]) < 1e-13 * std::fabs(h[k]));
        }
    char line[256];
    int count = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        char* p = line;
        char* end = nullptr;
        double v[3];
        int n = 0;
        for (; n < 3; ++n) {
            v[n] = std::strtod(p, &end);
            if (end == p) break;
            p = end;
        }
        if (n < 3) continue;
        const int l = (int)v[0];
        const double pre = 1.0 / hmg::cs_cosdiff(v[1], v[2]);
        g_all(l, v[1], g), g_all(l, v[2], h);
        double k[4];
        for (int o = 0; o < 4; ++o) {
            k[o] = hmg::cs_weight(g[o], h[o], pre);
            CHECK(std::isfinite(k[o]));
        }
        std::printf("%a %a %a %a\n", k[0], k[1], k[2], k[3]);
        ++count;
    }
    std::fprintf(stderr, "curved-sky weights: %d values, %d failed checks\n", count, fails);
    return fails ? 1 : 0;
}
