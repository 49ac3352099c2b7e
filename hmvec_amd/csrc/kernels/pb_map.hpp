// Block map of the batched mass integrals (power_batch_kernel): linear block id -> (k tile, redshift).
// Plain C++: __host__ __device__ under hipcc, inline under a host compiler; no HIP include (tests/cpp/pb_map_host.cpp
// builds it with g++).
//
// Why the order matters: with the constant-prefix and short-series tiles left unloaded, low tiles
// load nothing and high tiles load every bin of every tensor.  A workgroup takes about the same time either way (one
// dependent scalar round trip per mass bin), but workgroups that load slow each other down: the fewer of them are on
// the chip at a time, the shorter each one is.  Blocks are dispatched in id order and (observed, not a contract) dealt
// round-robin over the 8 XCDs, so the order decides what runs side by side and which redshifts share an L2.  It is
// used for speed only: every workgroup computes what it computed under any other order, into the same place.
#pragma once

#if defined(__HIPCC__)
#define HMG_PB_MAP_FN __host__ __device__ __forceinline__
#else
#define HMG_PB_MAP_FN inline
#endif

namespace hmg {

enum : int {
    PB_ORDER_TILE_FASTEST = 0,    // O0: tile = id % ntile, z = id / ntile (the order of the former 2-D grid (ntile, nz))
    PB_ORDER_HEAVY_FIRST = 1,     // O1: tile = ntile-1 - id / nz, z = id % nz: heaviest tiles start first, z fastest
    PB_ORDER_ENDS_INTERLEAVED = 2 // O2: tiles ntile-1, 0, ntile-2, 1, ..., z fastest: loading and no-load tiles side by side
};

// The order the library is built with (variant builds for A/B timing: make EXTRA=-DHMG_PB_ORDER=n).  Measured on one
// MI355X, Config 3 (32 x 512 x 4096), four alternating runs each (profiles/r11/pb_order_ab.txt): bracket of the launch
// 138.4-139.8 us with the 2-D grid, 138.2-139.5 O0, 134.0-135.8 O1, 128.5-129.2 O2; no slab size is slower than before.
#ifndef HMG_PB_ORDER
#define HMG_PB_ORDER 2
#endif
constexpr int PB_ORDER = HMG_PB_ORDER;

// id in [0, ntile nz) -> tile in [0, ntile), z in [0, nz); a bijection for every ORDER
template <int ORDER>
HMG_PB_MAP_FN void pb_map(int id, int ntile, int nz, int& tile, int& z) {
    static_assert(ORDER >= 0 && ORDER <= 2, "unknown block order");
    if (ORDER == PB_ORDER_TILE_FASTEST) {
        z = id / ntile;
        tile = id - z * ntile;
    } else {
        const int s = id / nz;              // position of the tile in the order's tile sequence
        z = id - s * nz;
        if (ORDER == PB_ORDER_HEAVY_FIRST) tile = ntile - 1 - s;
        else tile = (s & 1) ? (s >> 1) : ntile - 1 - (s >> 1);
    }
}

}  // namespace hmg
