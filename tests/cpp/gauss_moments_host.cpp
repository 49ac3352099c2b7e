// Host build of hmvec_amd/csrc/gauss_moments.hpp (tests/test_rsd_cpu.py compiles and runs it): reads values of t, one
// per line as printf's %a writes them, from standard input and prints M_0(t), M_1(t), M_2(t) the same way, which the
// test compares with 40-digit arithmetic.  Checks by itself what needs no reference: t = 0 gives exactly 1 / (2n + 1),
// the moments are finite, positive and ordered M_0 >= M_1 >= M_2, and the two branches meet at the switch.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../hmvec_amd/csrc/gauss_moments.hpp"

static int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            ++fails;                                                    \
        }                                                               \
    } while (0)

int main() {
    double m0, m1, m2;
    hmg::gauss_moments(0.0, m0, m1, m2);
    CHECK(m0 == 1.0 && m1 == 1.0 / 3.0 && m2 == 1.0 / 5.0);
    double a0, a1, a2;
    hmg::gauss_moments(std::nextafter(hmg::GM_SWITCH, 0.0), a0, a1, a2);
    hmg::gauss_moments(hmg::GM_SWITCH, m0, m1, m2);
    CHECK(std::fabs(a0 - m0) < 1e-15 && std::fabs(a1 - m1) < 1e-15 && std::fabs(a2 - m2) < 1e-15);
    char line[128];
    int count = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        char* end = nullptr;
        const double t = std::strtod(line, &end);
        if (end == line) continue;
        hmg::gauss_moments(t, m0, m1, m2);
        CHECK(std::isfinite(m0) && std::isfinite(m1) && std::isfinite(m2));
        CHECK(m0 > 0.0 && m0 <= 1.0 && m1 >= 0.0 && m1 <= m0 && m2 >= 0.0 && m2 <= m1);
        std::printf("%a %a %a\n", m0, m1, m2);
        ++count;
    }
    std::fprintf(stderr, "gauss_moments: %d values, %d failed checks\n", count, fails);
    return fails ? 1 : 0;
}
