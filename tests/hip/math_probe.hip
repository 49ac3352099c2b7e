// Pointwise probe of the device math headers (tests/helpers/math_probe.py builds it into tests/hip/libmathprobe.so with
// the library's own compiler flags; tests/test_gpu_math_probe.py drives it).  Not part of the product: it includes the
// headers of hmvec_amd/csrc as they are and restates nothing, so what it measures is the code the kernels run.
//
// One kernel: thread i reads x[i] (and y[i], z[i] where the function takes more arguments) and writes up to two results
// behind an i < n guard; a wave-uniform switch on the function id selects the function.  One entry point: host pointers
// in, host pointers out, every HIP call checked, the first error code returned.
#include <hip/hip_runtime.h>

#include "i0e.hpp"
#include "j01.hpp"
#include "sici.hpp"
#include "rowdev.hpp"
#include "gauss_moments.hpp"
#include "kernels/hankel.hpp"
#include "kernels/realspace.hpp"

namespace {

using namespace hmg;

// (the ids are restated in tests/helpers/math_probe.py: FN)
enum Fn : int {
    FN_J0 = 0, FN_J1, FN_J2, FN_J01, FN_I0E,
    FN_SINCOS_FAST, FN_XI_SINCOS, FN_SIN_MINUS_YCOS, FN_RCP_FAST, FN_SICI, FN_SICI_AUX_FG, FN_SICI_AUX_G,
    FN_LOG, FN_EXP_CLAMP, FN_EXP_NOCLAMP, FN_LOG1P, FN_LOG1P_ABS, FN_FM_RCP, FN_GNFW, FN_GNFW_ALPHA1,
    FN_NODE_G_H2, FN_NODE_H1_G4, FN_NODE_F2, FN_XI_PANEL, FN_GAUSS_M0_M1, FN_GAUSS_M2,
    FN_COUNT
};

constexpr double GNFW_GAMMA = -0.2;           // the gNFW checks: amp = 1, gamma = -0.2, x = t, y = alpha, z = expo

__global__ __launch_bounds__(256) void math_probe_kernel(int fn, int n, const double* __restrict__ x,
                                                         const double* __restrict__ y, const double* __restrict__ z,
                                                         const SiciTable* __restrict__ T, double* __restrict__ o0,
                                                         double* __restrict__ o1) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = x[i];
    double r0 = 0.0, r1 = 0.0;
    switch (fn) {
    case FN_J0: r0 = bessel_j0(a); break;
    case FN_J1: r0 = bessel_j1(a); break;
    case FN_J2: r0 = bessel_j2(a); break;
    case FN_J01: bessel_j01(a, r0, r1); break;
    case FN_I0E: r0 = bessel_i0e(a); break;
    case FN_SINCOS_FAST: sincos_fast(a, r0, r1); break;
    case FN_XI_SINCOS: xi_sincos(a, r0, r1); break;
    case FN_SIN_MINUS_YCOS: r0 = sin_minus_ycos_nosign(a, y[i]); break;
    case FN_RCP_FAST: r0 = rcp_fast(a); break;
    case FN_SICI: {                                           // fed as xp_trig (kernels/realspace.hpp) feeds it
        double s, c;
        bool small;
        xi_sincos(a, s, c);
        const double r = rcp_fast(a);
        sici_fast(T, a, s, c, r * r, r0, r1, small);
        if (small) r1 += EULER_GAMMA + log(a);
        break;
    }
    case FN_SICI_AUX_FG: {
        const double r = rcp_fast(a);
        sici_aux<true>(T, a, r * r, r0, r1);
        break;
    }
    case FN_SICI_AUX_G: {
        const double r = rcp_fast(a);
        sici_aux<false>(T, a, r * r, r0, r1);
        break;
    }
    case FN_LOG: r0 = log_fast(a); break;
    case FN_EXP_CLAMP: r0 = exp_fast<true>(a); break;
    case FN_EXP_NOCLAMP: r0 = exp_fast<false>(a); break;
    case FN_LOG1P: r0 = log1p_fast(a); break;
    case FN_LOG1P_ABS: r0 = log1p_abs(a); break;
    case FN_FM_RCP: r0 = fm_rcp(a); break;
    case FN_GNFW: r0 = gnfw_rho_fast(log_fast(a), 1.0, y[i], z[i], GNFW_GAMMA); break;
    case FN_GNFW_ALPHA1: r0 = gnfw_rho_alpha1(log_fast(a), a, 1.0, z[i], GNFW_GAMMA); break;
    case FN_NODE_G_H2: {
        double j0, j1;
        bessel_j01(a, j0, j1);
        hankel_node_j<true, true>(a, j0, j1, r0, r1);
        break;
    }
    case FN_NODE_H1_G4: {
        double j0, j1;
        bessel_j01(a, j0, j1);
        r0 = hankel_h1(a, j0, j1);
        r1 = bessel_g4(a, j0, j1);
        break;
    }
    case FN_NODE_F2: {
        double j0, j1;
        bessel_j01(a, j0, j1);
        r0 = angular_f2(a, j0, j1);
        break;
    }
    case FN_XI_PANEL: xi_panel_factors(a, r0, r1); break;
    case FN_GAUSS_M0_M1: {
        double m2;
        gauss_moments(a, r0, r1, m2);
        break;
    }
    case FN_GAUSS_M2: {
        double m0, m1;
        gauss_moments(a, m0, m1, r0);
        break;
    }
    default: break;
    }
    o0[i] = r0;
    o1[i] = r1;
}

}  // namespace

// out0[i], out1[i] = function fn at (x[i], y[i], z[i]), i < n.  x, out0 and out1 hold n doubles; y and z may be null for
// the functions that do not read them.  Returns 0, the first HIP error code, or -1 for a bad argument.
extern "C" int math_probe_run(int fn, int n, const double* x, const double* y, const double* z, double* out0,
                              double* out1) {
    if (fn < 0 || fn >= FN_COUNT || n <= 0 || !x || !out0 || !out1) return -1;
    const bool need_y = fn == FN_SIN_MINUS_YCOS || fn == FN_GNFW;
    const bool need_z = fn == FN_GNFW || fn == FN_GNFW_ALPHA1;
    if ((need_y && !y) || (need_z && !z)) return -1;
    const size_t bytes = (size_t)n * sizeof(double);
    double *dx = nullptr, *dy = nullptr, *dz = nullptr, *d0 = nullptr, *d1 = nullptr;
    hmg::SiciTable* dT = nullptr;
    const hmg::SiciTable hT = hmg::sici_table_host();
    hipError_t rc = hipSuccess;
    auto ok = [&rc](hipError_t e) {
        if (rc == hipSuccess && e != hipSuccess) rc = e;
        return rc == hipSuccess;
    };
    // every input array exists on the device (a copy of x where the caller gave none): the kernel reads only what the
    // function takes, and never past n
    if (ok(hipMalloc(&dx, bytes)) && ok(hipMalloc(&dy, bytes)) && ok(hipMalloc(&dz, bytes)) && ok(hipMalloc(&d0, bytes)) &&
        ok(hipMalloc(&d1, bytes)) && ok(hipMalloc(&dT, sizeof(hmg::SiciTable))) &&
        ok(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice)) && ok(hipMemcpy(dy, y ? y : x, bytes, hipMemcpyHostToDevice)) &&
        ok(hipMemcpy(dz, z ? z : x, bytes, hipMemcpyHostToDevice)) &&
        ok(hipMemcpy(dT, &hT, sizeof(hmg::SiciTable), hipMemcpyHostToDevice))) {
        const int nt = 256, nb = (n + nt - 1) / nt;
        hipLaunchKernelGGL(math_probe_kernel, dim3(nb), dim3(nt), 0, 0, fn, n, dx, dy, dz, dT, d0, d1);
        if (ok(hipGetLastError()) && ok(hipDeviceSynchronize()) && ok(hipMemcpy(out0, d0, bytes, hipMemcpyDeviceToHost)))
            ok(hipMemcpy(out1, d1, bytes, hipMemcpyDeviceToHost));
    }
    for (void* p : {(void*)dx, (void*)dy, (void*)dz, (void*)d0, (void*)d1, (void*)dT})
        if (p) ok(hipFree(p));
    return (int)rc;
}
