// Host build of the weight functions of hmvec_amd/csrc/kernels/angcov.hpp (tests/test_angcov_cpu.py compiles and runs
// it): reads "l a b" per line as printf's %a writes them from standard input and prints K_0, K_2, K_4 of the annulus
// [a, b] at the multipole l the same way, with the C library's j0 and j1 in the place of the device's j01.hpp.  Checks by
// itself what needs no reference: G_mu(0) = 0, the two branches of G_2 and G_4 meet at their switches, and the values
// are finite.
#include <math.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../hmvec_amd/csrc/kernels/angcov.hpp"

static int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static double g(int o, double x) { return hmg::angcov_g(o, x, ::j0(x), ::j1(x)); }

int main() {
    for (int o = 0; o < 3; ++o) CHECK(g(o, 0.0) == 0.0);
    const double sw[2] = {hmg::AC_SERIES_X2, hmg::AC_SERIES_X4};
    for (int o = 1; o < 3; ++o) {
        const double below = g(o, std::nextafter(sw[o - 1], 0.0)), at = g(o, sw[o - 1]);
        CHECK(std::fabs(below - at) < 1e-14 * std::fabs(at));
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
        const double l = v[0], a = v[1], b = v[2], pre = 2.0 / ((b - a) * (b + a));
        double k[3];
        for (int o = 0; o < 3; ++o) {
            k[o] = hmg::angcov_weight(g(o, l * a), g(o, l * b), pre, l);
            CHECK(std::isfinite(k[o]));
        }
        std::printf("%a %a %a\n", k[0], k[1], k[2]);
        ++count;
    }
    std::fprintf(stderr, "angcov weights: %d values, %d failed checks\n", count, fails);
    return fails ? 1 : 0;
}
