// Host build of hmvec_amd/csrc/sphbessel.hpp (tests/test_nonlimber_cpu.py compiles and runs it, plain and under
// AddressSanitizer + UBSan): reads "lmax x" per line as printf's %a writes them from standard input and prints
// j_0(x) .. j_lmax(x) of sb_all the same way, one line per argument.  Checks by itself what needs no reference: every
// value is finite, and the walk taken a tile of 16 orders at a time - upwards in ascending tiles, downwards in
// descending tiles after a first walk for the scale, as the transfer kernel steps it - gives the bits of sb_all.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hmvec_amd/csrc/sphbessel.hpp"

static int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);     \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static void tiled(double x, int L, int N, std::vector<double>& out) {
    const int tile = 16, ntiles = L / tile + 1;
    const hmg::sb_recip rx = hmg::sb_recip_of(x);
    double j0, j1;
    hmg::sb_j01(x, rx.h, j0, j1);
    if (x >= (double)L) {
        hmg::sb_up u{j0, j1};
        for (int t = 0; t < ntiles; ++t)
            for (int q = 0; q < tile; ++q) {
                const int l = t * tile + q;
                if (l <= L) out[l] = u.a;
                hmg::sb_up_step(u, l, rx);
            }
        return;
    }
    hmg::sb_down d = hmg::sb_down_start();
    for (int l = N; l > 0; --l) hmg::sb_down_step(d, l, rx);
    const double s = hmg::sb_down_scale(d, j0, j1);
    const int c0 = d.c;
    d = hmg::sb_down_start();
    for (int l = N; l > ntiles * tile - 1; --l) hmg::sb_down_step(d, l, rx);
    for (int t = ntiles - 1; t >= 0; --t)
        for (int q = tile - 1; q >= 0; --q) {
            const int l = t * tile + q;
            if (l <= L) out[l] = hmg::sb_down_value(d.a, d.c, s, c0);
            if (l > 0) hmg::sb_down_step(d, l, rx);
        }
}

int main() {
    char line[256];
    int count = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        char* end = nullptr;
        const double lv = std::strtod(line, &end);
        if (end == line) continue;
        char* p = end;
        const double x = std::strtod(p, &end);
        if (end == p) continue;
        const int L = (int)lv, N = hmg::sb_start_order(L);
        CHECK(N >= (L / 16 + 1) * 16);
        std::vector<double> a(L + 1), b(L + 1);
        hmg::sb_all(x, L, N, a.data(), 1);
        tiled(x, L, N, b);
        for (int l = 0; l <= L; ++l) {
            CHECK(std::isfinite(a[l]));
            CHECK(a[l] == b[l]);
            std::printf(l == L ? "%a\n" : "%a ", a[l]);
        }
        ++count;
    }
    std::fprintf(stderr, "spherical Bessel walk: %d arguments, %d failed checks\n", count, fails);
    return fails ? 1 : 0;
}
