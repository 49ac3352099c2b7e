// The scaffold the transforms of tabulated spectra share (DESIGN.md sections 13, 14, 22, 24): one workgroup of NT threads
// per (row, tile of TR radii), the nk - 1 panels of the row dealt to the threads, one LDS word per (thread, output, radius)
// and a fixed tree over them.  The sine family (kernels/realspace.hpp) and the Bessel family (kernels/hankel.hpp) keep
// their own panel loops; what is here is the part that does not know which of the two it serves.
#pragma once

namespace hmg {

// radii of the tile that starts at j0, of n in all (>= 1 by the launch geometry)
template <int TR>
__device__ __forceinline__ int tile_count(int n, int j0) { return n - j0 < TR ? n - j0 : TR; }

// Contiguous-run ownership: thread tid owns the panels lo ... hi - 1 of np, c = ceil(np / NT) of them (the last owners'
// runs are short or empty: lo == hi).
struct PanelRun { int lo, hi; };
template <int NT>
__device__ __forceinline__ PanelRun panel_run(int tid, int np) {
    const int c = (np - 1) / NT + 1;
    const int lo = tid * c < np ? tid * c : np, hi = lo + c < np ? lo + c : np;
    return {lo, hi};
}

// Sum of the NT words of each row into red[row][0], by a tree whose shape depends on NT alone: the same bits whatever
// the launch.  Waits for the words first; every thread of the workgroup calls it.
template <int ROWS, int NT>
__device__ __forceinline__ void panel_tree_sum(double (&red)[ROWS][NT], int tid) {
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s >= 1; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int t = 0; t < ROWS; ++t) red[t][tid] += red[t][tid + s];
        }
        __syncthreads();
    }
}

}  // namespace hmg
