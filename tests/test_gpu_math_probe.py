"""The device math headers, function by function and point by point, on the GPU against mpmath at 50 digits.

tests/hip/math_probe.hip includes j0.hpp, j1.hpp, j01.hpp, i0e.hpp, sici.hpp, fastmath.hpp, rowdev.hpp, gauss_moments.hpp,
kernels/hankel.hpp, kernels/bessel_g4.hpp and kernels/realspace.hpp as they are and is built with the library's own
flags, so what runs here is what the kernels run: the hardware reciprocal and its Newton steps, the inline-assembly
FMAs with a scalar operand, hipcc's contraction.  Every test is one probe call; the point sets, references and gates are
those of helpers/math_probe.py, which tests/test_math_probe_cpu.py checks against independent implementations without a
device.  No point is left out of a comparison.

Worst |device - mpmath| / gate on an MI355X, as the tests print them (28 tests, 3.2 s in all):
    j0              |x|<=5 0.344   5<|x|<2^30 0.932   |x|>=2^30 0.937          (1483 points)
    j1              |x|<=5 0.207   5<|x|<2^30 0.882   |x|>=2^30 0.956
    j2              |x|<2 0.412    2<=|x|<=5 0.123    above: 0.932, 0.937
    j01             J0 0.344, 0.932, 0.937    J1 0.207, 0.936, 0.974           (1301 points)
    i0e             0.292                                                      (968 points)
    sincos_fast     sin 0.846   cos 0.842                                      (1791 points)
    xi_sincos       sin 0.760   cos 0.816                                      (702 points)
    sin_minus_ycos  0.335                                                      (1701 points)
    rcp_fast        0.5         fm_rcp 0.5                                     (2509 points)
    sici            Si 0.584    Ci 0.903                                       (1411 points)
    sici_aux        f 0.785 (x = 4.8e5)   g 0.459 (x = 64); g alone the same   (1002 points)
    log 0.352   exp 0.407 (both forms)   log1p 0.503   log1p_abs 0.925         (3130, 2516, 2504 points)
    gnfw 0.307  gnfw_alpha1 0.136                                              (2500 points)
    g               x<2 0.450   2<=x<5 0.126   x>=5 0.935                      (1014 points)
    H2              0.585, 0.166, 0.918       H1  0.189, 0.111, 0.930
    F1 = G4         0.277, 0.255, 0.930       F2  0.476, 0.477, 0.878
    S 0.414   G 0.646                                                          (908 points)
    M0 0.322  M1 0.117  M2 0.169                                               (673 points)
The ratios near 0.93 are the phase term alone, at x of 1e5 and beyond: x - pi/4 rounded by half a spacing of x.

That the gates bite: with one line of a scratch copy of the headers changed and the probe rebuilt from it, on the same
MI355X (nothing of it is committed):
    the 13th digit of j0c::PP[5]                   j0, j01 fail at 20.9 (x = 7.02), j2 14.8, g 14.5, H2 9.2, F1 6.2
    x <= 5.5 for x <= 5.0 in bessel_j01             j01 fails: J1 8.1 at 5.5, J0 2.8 at 5.45; the nodes 1.1 to 1.7
    one Newton step of fm_rcp removed               fm_rcp fails at 8.7 ulp
    the third Cody-Waite term of sincos_fast out    sincos_fast fails at 8.8e5 (cos), 7.8e4 (sin); xi_sincos 1.9e4
    G4_SERIES_N = 8                                 F1 fails at 5.6e7, F2 at 1.9e7, just below 5
The last PRINTED digit of a coefficient (PP[0] ...624E-4 to ...625E-4) is the same double: nothing changes, all pass.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import math_probe as mpb  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(mpb.COMPARISONS))
def test_device_function_against_mpmath(name):
    points, ratios = mpb.COMPARISONS[name](mpb.call)
    w = mpb.report(name, points, ratios)
    assert all(r.shape == points.shape for r in ratios.values())      # every point is in the comparison
    assert all(v <= 1.0 for v, _ in w.values()), w


def test_exp_without_the_clamp_is_the_same_bits():
    y = mpb.fastmath_points()["exp"]
    assert np.all(np.abs(y) < 700.0)
    assert np.array_equal(mpb.call("exp_noclamp", y)[0], mpb.call("exp_clamp", y)[0])


def test_special_values():
    """What tests/test_fastmath_cpu.py and tests/test_rsd_cpu.py ask of the host builds: saturation of exp outside
    +-700, ln(1 + 0) = 0, M_n(0) = 1 / (2n + 1) exactly; and the exact zeros of the odd and even functions at 0."""
    sat = mpb.call("exp_clamp", np.array([800.0, -800.0]))[0]
    assert sat[0] == np.inf and sat[1] == 0.0
    far = mpb.call("exp_noclamp", np.array([5000.0, -5000.0, 1e8, -1e8]))[0]
    assert np.all(far[[0, 2]] == np.inf) and np.all(far[[1, 3]] == 0.0)
    assert mpb.call("log1p", np.zeros(1))[0][0] == 0.0
    m01, m2 = mpb.call("gauss_m0_m1", np.zeros(1)), mpb.call("gauss_m2", np.zeros(1))
    assert [m01[0][0], m01[1][0], m2[0][0]] == [1.0, 1.0 / 3.0, 1.0 / 5.0]
    zero = np.zeros(1)
    assert mpb.call("j1", zero)[0][0] == 0.0 and mpb.call("j2", zero)[0][0] == 0.0
    for name in ("node_g_h2", "node_h1_g4", "node_f2"):
        assert all(o[0] == 0.0 for o in mpb.call(name, zero))
    assert all(o[0] == 1.0 for o in mpb.call("xi_panel", zero))
