// K7 - the HOD kernel of the headline path; its device functions (SHMR, occupation numbers, n_gal and b_g) are
// kernels/hod_occ.hpp, shared with the ensemble unit hodens.hip.
// Part of the ONE translation unit hmgrid.hip (included there in this order; not a stand-alone header).
#pragma once
#include "hod_occ.hpp"

namespace hmg {

// One block per z: both halves.
__global__ __launch_bounds__(1024) void hod_kernel(HodRowArgs A) {
    __shared__ double part[2 * HOD_MAX_TILES];
    for (int m = threadIdx.x; m < A.nm; m += blockDim.x) hod_occ_point(A, blockIdx.x, m);
    __syncthreads();
    hod_sums_row(A, blockIdx.x, blockDim.x, part);
}

}  // namespace hmg
