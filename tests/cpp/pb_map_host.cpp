// Host check of hmvec_amd/csrc/kernels/pb_map.hpp - the block map of the batched mass integrals - as a stand-alone
// program: exit status 0 when every property holds, else 1 with the first failures on stderr.  The same header is
// compiled into power_batch_kernel; tests/test_pb_map_cpu.py builds this file plainly and under ASan + UBSan.
#include <cstdio>
#include <utility>
#include <vector>

#include "../../hmvec_amd/csrc/kernels/pb_map.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            if (failures < 20) { std::fprintf(stderr, "FAIL %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

// every (tile, z) exactly once, each inside its range; buffers sized exactly, so a stray index trips ASan
template <int ORDER>
static void bijection(int ntile, int nz) {
    const long n = (long)ntile * nz;
    std::vector<unsigned char> seen((size_t)n, 0);
    for (long id = 0; id < n; ++id) {
        int tile = -1, z = -1;
        hmg::pb_map<ORDER>((int)id, ntile, nz, tile, z);
        const bool in = tile >= 0 && tile < ntile && z >= 0 && z < nz;
        CHECK(in, "order %d (%d,%d): id %ld -> (%d,%d)", ORDER, ntile, nz, id, tile, z);
        if (!in) return;
        unsigned char& s = seen[(size_t)tile * nz + z];
        CHECK(!s, "order %d (%d,%d): (%d,%d) hit twice, second time by id %ld", ORDER, ntile, nz, tile, z, id);
        s = 1;
    }
    // n distinct in-range hits of n cells: onto
}

static void order0_is_the_2d_grid(int ntile, int nz) {
    for (int id = 0; id < ntile * nz; ++id) {
        int tile, z;
        hmg::pb_map<hmg::PB_ORDER_TILE_FASTEST>(id, ntile, nz, tile, z);
        CHECK(tile == id % ntile && z == id / ntile, "O0 (%d,%d): id %d -> (%d,%d)", ntile, nz, id, tile, z);
    }
}

static void order1(int ntile, int nz) {
    int prev = ntile;
    std::vector<int> count((size_t)8 * ntile, 0);
    for (int id = 0; id < ntile * nz; ++id) {
        int tile, z;
        hmg::pb_map<hmg::PB_ORDER_HEAVY_FIRST>(id, ntile, nz, tile, z);
        CHECK(tile <= prev, "O1 (%d,%d): tile rises from %d to %d at id %d", ntile, nz, prev, tile, id);
        CHECK(tile == ntile - 1 - id / nz && z == id % nz, "O1 (%d,%d): id %d -> (%d,%d)", ntile, nz, id, tile, z);
        prev = tile;
        if (tile >= 0 && tile < ntile) ++count[(size_t)(id % 8) * ntile + tile];
    }
    if (nz % 8 == 0)
        for (int c = 0; c < 8; ++c)
            for (int t = 0; t < ntile; ++t)
                CHECK(count[(size_t)c * ntile + t] == nz / 8, "O1 (%d,%d): class %d holds tile %d %d times, not %d", ntile, nz,
                      c, t, count[(size_t)c * ntile + t], nz / 8);
}

static void order2(int ntile, int nz) {
    // the first 2 nz ids (all of them when there is one tile) hold the highest and the lowest tile, nothing else
    const int n = ntile * nz, head = ntile > 1 ? 2 * nz : nz;
    int hi = 0, lo = 0;
    for (int id = 0; id < head && id < n; ++id) {
        int tile, z;
        hmg::pb_map<hmg::PB_ORDER_ENDS_INTERLEAVED>(id, ntile, nz, tile, z);
        CHECK(tile == ntile - 1 || tile == 0, "O2 (%d,%d): id %d holds tile %d", ntile, nz, id, tile);
        hi += tile == ntile - 1;
        lo += tile == 0;
    }
    if (ntile > 1) CHECK(hi == nz && lo == nz, "O2 (%d,%d): %d highest and %d lowest tiles in the first %d ids", ntile, nz, hi, lo, head);
}

int main() {
    std::vector<std::pair<int, int>> shapes;
    for (int ntile = 1; ntile <= 40; ++ntile)
        for (int nz = 1; nz <= 40; ++nz) shapes.push_back({ntile, nz});
    for (auto s : {std::pair<int, int>{32, 32}, {64, 4}, {32, 8}, {1, 1}, {1, 65535}, {33, 7}}) shapes.push_back(s);
    for (auto s : shapes) {
        bijection<hmg::PB_ORDER_TILE_FASTEST>(s.first, s.second);
        bijection<hmg::PB_ORDER_HEAVY_FIRST>(s.first, s.second);
        bijection<hmg::PB_ORDER_ENDS_INTERLEAVED>(s.first, s.second);
        order0_is_the_2d_grid(s.first, s.second);
        order1(s.first, s.second);
        order2(s.first, s.second);
    }
    static_assert(hmg::PB_ORDER >= 0 && hmg::PB_ORDER <= 2, "the committed order is one of the three");
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    else std::printf("pb_map ok: %zu shapes, order built in: %d\n", shapes.size(), hmg::PB_ORDER);
    return failures ? 1 : 0;
}
