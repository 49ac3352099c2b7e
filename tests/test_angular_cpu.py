"""Host checks of the angular correlation functions (hmvec_amd.angular.angular_from_power): the
order-4 by-parts sum the kernel evaluates against 40-digit mpmath of an independent form, its node functions either
side of the series switch, the identity that ties W_4 to moments of W_0 inside R, its small-argument bound, the
argument checks of angular_from_power and of the facade methods, Cosmology.angular_weights and the ABI declarations.
The device is checked in tests/test_gpu_angular.py."""
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import REPO
import hmvec_amd
from hmvec_amd import _native as nat
from hmvec_amd import angular, angular_from_power

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import angular_model as am  # noqa: E402
import projected_model as pm  # noqa: E402

RADII = np.array([1e-3, 0.03, 1.0, 30.0, 300.0])
SWITCH_NODE = 20            # the interior node whose x = k R the two extra radii put either side of the switch


def grid_and_radii(grid):
    if grid == "two":
        ks = np.array([0.5, 1.5])
        return ks, np.concatenate([RADII, am.switch_radii4(ks[1])])
    ks = np.geomspace(1e-4, 100, 33) if grid == "log" else am.uneven_grid(33)
    return ks, np.concatenate([RADII, am.switch_radii4(ks[SWITCH_NODE])])


# ---------------------------------------------------------------- 1. the by-parts sum of order 4 against mpmath
@pytest.mark.parametrize("row", ["positive", "sign_changing"])
@pytest.mark.parametrize("grid", ["two", "log", "uneven"])
def test_order_4_by_parts_sum_meets_the_gate_against_mpmath(grid, row):
    ks, rs = grid_and_radii(grid)
    x = rs[-2:] * (ks[1] if grid == "two" else ks[SWITCH_NODE])
    assert x[0] < am.SERIES_X4 < x[1] and abs(x[1] - x[0]) < 2e-5
    if grid == "two":
        P = np.array([2.0, 0.7]) if row == "positive" else np.array([3.0, -1.0])
    else:
        P = am.power_like(ks) if row == "positive" else am.sign_changing(ks)
        if row == "sign_changing":
            assert np.sum(np.diff(np.sign(P)) != 0) >= 3
    got, ref = am.w4_numpy(ks, P, rs), am.w4_mpmath(ks, P, rs)
    err, tol = np.abs(got - ref), am.gate(ks, P, rs, 4)
    print("err / gate:", err / tol, " |W_4| / A:", np.abs(ref) / am.panel_scale(ks, P, rs))
    assert np.all(err <= tol), (err / tol).max()


def test_order_4_series_and_closed_forms_at_the_switch():
    """At the switch and above, F1 and F2 are within 8 roundings of the size of the terms their closed forms add
    (12 + 2x for F1, 4 x^2 + 24 for F2) of their 50-digit values, and so are the series just below it (their terms sum to
    less than that in absolute value); well below the switch the series are relative: 8 ulp of the value."""
    import mpmath as mp
    xs = am.SERIES_X4 * np.array([1e-3, 0.2, 1 - 1e-9, 1 + 1e-9, 2.0, 20.0])
    f1, f2 = am.f1_fn(xs), am.f2_fn(xs)
    with mp.workdps(50):
        for i, x in enumerate(xs):
            x = mp.mpf(float(x))
            j0, j1, j2 = mp.besselj(0, x), mp.besselj(1, x), mp.besselj(2, x)
            ref = (4 + 8 * j0 + x * j1 - 24 * j1 / x, 2 * x * x + 8 * x * j1 + x * x * j2 + 24 * (j0 - 1))
            for got, r, size in zip((f1[i], f2[i]), ref, (12 + 2 * x, 4 * x * x + 24)):
                bound = 8 * 2.0 ** -53 * abs(r) if x < 1.5 else 8 * 2.0 ** -53 * size
                assert abs(got - r) <= bound, (float(x), float(got), float(r))


# ---------------------------------------------------------------- 2. identities on section 14's Gaussian row
GK = np.linspace(0.01, 12, 1200)
GP = np.exp(-0.5 * GK ** 2)


def test_w4_is_w0_plus_moments_of_w0_inside_R():
    """J4(x) = J0 - 8 J1/x + 24 J2/x^2, and with int_0^R r J0(k r) dr = R J1(x)/k,
    int_0^R r^3 J0(k r) dr = (x^3 J1 - 2 x^2 J2)/k^4 this is
    J4(k R) = J0(k R) + (4/R^2) int_0^R r J0(k r) dr - (12/R^4) int_0^R r^3 J0(k r) dr, so for any row
    W_4(R) = W_0(R) + (4/R^2) int_0^R r W_0 dr - (12/R^4) int_0^R r^3 W_0 dr, exactly.  The integrals by n-point
    Gauss-Legendre: the remainder of int_0^R f is R^(2n+1) (n!)^4 / ((2n+1) ((2n)!)^3) max|f^(2n)|, and with
    |d^m/dr^m J0(k r)| <= k^m, k <= K = 12, Leibniz gives |(r^p W_0)^(m)| <= A K^m (R + m/K)^p (A the panel scale):
    with n = 64 far below 1e-25 A.  What is left is the rounding of the transforms, each inside its gate."""
    n, K = 64, GK[-1]
    t, w = np.polynomial.legendre.leggauss(n)
    A = am.panel_scale(GK, GP, [1.0])[0]
    for R in (0.5, 1.0, 2.0, 4.0):
        Rq, wq = 0.5 * R * (t + 1), 0.5 * R * w
        w0q, g0q = pm.hankel_numpy(GK, GP, Rq, 0), am.gate(GK, GP, Rq, 0)
        m1 = 4.0 / R ** 2 * np.sum(wq * Rq * w0q)
        m3 = 12.0 / R ** 4 * np.sum(wq * Rq ** 3 * w0q)
        w0, w4 = pm.hankel_numpy(GK, GP, [R], 0)[0], am.w4_numpy(GK, GP, [R])[0]
        log_q = ((2 * n + 1) * math.log(R) + 4 * math.lgamma(n + 1) - math.log(2 * n + 1) - 3 * math.lgamma(2 * n + 1)
                 + 2 * n * math.log(K))
        rem = A * math.exp(log_q) * (4.0 / R ** 2 * (R + 2 * n / K) + 12.0 / R ** 4 * (R + 2 * n / K) ** 3)
        assert rem < 1e-25 * A
        tol = (rem + am.gate(GK, GP, [R], 4)[0] + am.gate(GK, GP, [R], 0)[0] + 4.0 / R ** 2 * np.sum(wq * Rq * g0q)
               + 12.0 / R ** 4 * np.sum(wq * Rq ** 3 * g0q))
        err = abs(w0 + m1 - m3 - w4)
        print(f"R = {R}: |W_0 + m1 - m3 - W_4| = {err:.3g}, tol {tol:.3g}, W_4 = {w4:.6g}, W_0 = {w0:.6g}")
        assert err <= tol
        assert abs(w4) > 1e3 * tol or R < 1.0          # (the identity is not vacuous where W_4 has grown)


def test_w4_is_far_below_w0_at_small_radii():
    """With x = k_last R << 1: 0 < J4(k R) <= x^4/384 and J0(k R) >= 1 - x^2/4 on the whole grid, so for a positive row
    0 < W_4 <= (x^4/384)/(1 - x^2/4) W_0.  W_4 is 1e-11 A and less here - far below the gate's floor - and keeps its
    sign and size because F1 and F2 vanish at 0 (no constant is left to cancel)."""
    ks = np.geomspace(1e-4, 100, 33)
    P = am.power_like(ks)
    R = np.array([1e-6, 1e-5, 1e-4])
    x = ks[-1] * R
    assert np.all(P > 0) and np.all(x <= 0.0100001)
    w0, w4 = pm.hankel_numpy(ks, P, R, 0), am.w4_numpy(ks, P, R)
    print("W_4 / W_0 at k_last R = 1e-4, 1e-3, 1e-2:", w4 / w0)
    assert np.all(w4 > 0)
    assert np.all(w4 <= (x ** 4 / 384) / (1 - x ** 2 / 4) * w0)


# ---------------------------------------------------------------- 3. argument checks of angular_from_power
class NoLaunch:
    """A context that fails the test on any use: the argument checks come before every upload and launch."""

    def __getattr__(self, name):
        raise AssertionError(f"context used ({name}) before the arguments were checked")


KS = np.geomspace(1e-3, 10, 16)
NZ = 3
GOOD_P = np.stack([am.power_like(KS) * a for a in (1.0, 0.8, 0.5)])
CHIS = np.array([800.0, 1500.0, 2300.0])
ZW = np.array([0.2, 0.5, 0.3])


@pytest.mark.parametrize("order", [0, 2, 4, (0, 2, 4)])
@pytest.mark.parametrize("ks,P,thetas,chis,zw", [
    (KS[::-1], GOOD_P, [1e-3], CHIS, ZW),                                  # decreasing
    (np.r_[0.0, KS[1:]], GOOD_P, [1e-3], CHIS, ZW),                        # k = 0
    (KS[:1], GOOD_P[:, :1], [1e-3], CHIS, ZW),                             # nk < 2
    (KS, np.where(np.arange(KS.size) == 3, np.nan, GOOD_P), [1e-3], CHIS, ZW),   # non-finite P
    (KS, GOOD_P[:, :-1], [1e-3], CHIS, ZW),                                # wrong length
    (KS, GOOD_P[0], [1e-3], CHIS, ZW),                                     # no z axis
    (KS, np.ones((2, 2, NZ, KS.size)), [1e-3], CHIS, ZW),                  # too many axes
    (KS, np.ones((0, KS.size)), [1e-3], np.ones(0), np.ones(0)),           # no redshift at all
    (KS, GOOD_P, [1e-3, 0.0], CHIS, ZW),                                   # theta = 0
    (KS, GOOD_P, [-1e-3], CHIS, ZW),                                       # negative theta
    (KS, GOOD_P, [np.nan], CHIS, ZW),                                      # non-finite theta
    (KS, GOOD_P, [[1e-3, 2e-3]], CHIS, ZW),                                # angles not a vector
    (KS, GOOD_P, [1e-3], CHIS[:2], ZW),                                    # chis of the wrong length
    (KS, GOOD_P, [1e-3], CHIS[None, :], ZW),                               # chis not a vector
    (KS, GOOD_P, [1e-3], 1500.0, ZW),                                      # a scalar chi for three rows
    (KS, GOOD_P, [1e-3], np.r_[0.0, CHIS[1:]], ZW),                        # chi = 0
    (KS, GOOD_P, [1e-3], np.r_[-800.0, CHIS[1:]], ZW),                     # negative chi
    (KS, GOOD_P, [1e-3], np.r_[CHIS[:2], np.inf], ZW),                     # non-finite chi
    (KS, GOOD_P, [1e-3], CHIS, ZW[:2]),                                    # weights of the wrong length
    (KS, GOOD_P, [1e-3], CHIS, np.ones((2, 2, NZ))),                       # weights with too many axes
    (KS, GOOD_P, [1e-3], CHIS, np.ones((NZ, 2))),                          # nz not last
    (KS, GOOD_P, [1e-3], CHIS, np.ones((0, NZ))),                          # no row of weights
    (KS, GOOD_P, [1e-3], CHIS, 1.0),                                       # scalar weights
    (KS, GOOD_P, [1e-3], CHIS, np.r_[ZW[:2], np.nan]),                     # non-finite weights
])
def test_bad_arguments_raise_before_any_launch(ks, P, thetas, chis, zw, order):
    with pytest.raises(ValueError):
        angular_from_power(ks, P, thetas, chis, zw, order, ctx=NoLaunch())


@pytest.mark.parametrize("order", [1, 3, 6, -2, (2, 0), (4, 0), (0, 0), (0, 2, 2), (0, 2, 4, 4), (), "0", 0.0, 4.0, True, None,
                                   (0, 4.0), (0, 1)])
def test_a_bad_order_raises_before_any_launch(order):
    with pytest.raises(ValueError):
        angular_from_power(KS, GOOD_P, [1e-3], CHIS, ZW, order, ctx=NoLaunch())


def test_every_subset_of_orders_is_accepted():
    for order in (0, 2, 4, (0,), (2,), (4,), (0, 2), (0, 4), (2, 4), (0, 2, 4), [0, 4], np.int64(4)):
        assert angular.check_order(order) == (tuple(order) if isinstance(order, (tuple, list)) else (int(order),))


def test_a_resident_spectrum_of_the_wrong_shape_raises_before_any_launch():
    for shape in ((NZ, KS.size + 1), (KS.size,), (NZ + 1, KS.size)):
        P = nat.DeviceArray(None, 0, shape, owner=False)
        with pytest.raises(ValueError):
            angular_from_power(KS, P, [1e-3], CHIS, ZW, (0, 4), ctx=NoLaunch())


@pytest.mark.parametrize("shape", [(NZ, KS.size), (2, NZ, KS.size), (0, NZ, KS.size)])
def test_empty_angles_return_empty_arrays_without_a_launch(shape):
    for order in (0, 2, 4, [0, 4], (0, 2, 4)):
        for zw, mid in ((ZW, ()), (np.ones((5, NZ)), (5,))):
            out = angular_from_power(KS, np.ones(shape), [], CHIS, zw, order, ctx=NoLaunch())
            many = isinstance(order, (list, tuple))
            assert isinstance(out, tuple) == many
            outs = out if many else (out,)
            assert len(outs) == (len(order) if many else 1)
            for o in outs:
                assert o.shape == shape[:-2] + mid + (0,) and o.dtype == np.float64
    out = angular_from_power(KS, np.ones((0, NZ, KS.size)), [1e-3, 2e-3], CHIS, ZW, 4, ctx=NoLaunch())
    assert out.shape == (0, 2)


# ---------------------------------------------------------------- 4. argument checks of the facade
def test_the_facade_refuses_bad_requests_before_any_launch():
    from hmvec_amd.halomodel import HaloModel
    h = HaloModel.__new__(HaloModel)          # no constructor: nothing may be touched but the request
    h.ks, h.zs = KS, np.array([0.3, 0.6, 0.9])
    h.angular_weights = lambda zs, W1, W2: ZW
    h.comoving_radial_distance = lambda zs: CHIS
    h.lensing_window = lambda ezs, zs, dndz=None: np.ones(NZ)
    for term in ("one-halo", None, "3h"):
        with pytest.raises(ValueError):
            h.get_angular([1e-3], "nfw", term=term)
        with pytest.raises(ValueError):
            h.get_w_theta([1e-3], "nfw", term=term)
        with pytest.raises(ValueError):
            h.get_gamma_t([1e-3], "nfw", zsource=1.0, term=term)
        with pytest.raises(ValueError):
            h.get_xi_pm([1e-3], zsource=1.0, term=term)
        with pytest.raises(ValueError):
            h.get_angular_all([("nfw", "nfw")], [1e-3], ZW, term=term)
    for thetas in ([0.0], [np.nan], [[1e-3, 2e-3]]):
        with pytest.raises(ValueError):
            h.get_angular(thetas, "nfw")
        with pytest.raises(ValueError):
            h.get_angular_all([("nfw", "nfw")], thetas, ZW)
    for order in (1, (4, 0), True, ()):
        with pytest.raises(ValueError):
            h.get_angular([1e-3], "nfw", order=order)
        with pytest.raises(ValueError):
            h.get_angular_all([("nfw", "nfw")], [1e-3], ZW, order=order)
    for zw in (ZW[:2], np.ones((NZ, 2)), np.r_[ZW[:2], np.inf]):
        with pytest.raises(ValueError):
            h.get_angular([1e-3], "nfw", zweights=zw)
        with pytest.raises(ValueError):
            h.get_angular_all([("nfw", "nfw")], [1e-3], zw)
    with pytest.raises(ValueError):
        h.get_angular_all([("nfw", "nfw"), ("g", "g")], [1e-3], {("nfw", "nfw"): ZW})       # a pair without weights
    with pytest.raises(ValueError):
        h.get_gamma_t([1e-3], "nfw")                                                        # no source
    with pytest.raises(ValueError):
        h.get_xi_pm([1e-3])
    with pytest.raises(ValueError):
        h.get_gamma_t([1e-3], "nfw", zsource=[0.8, 1.0, 1.2])                               # a grid without its dndz
    with pytest.raises(ValueError):
        h.get_w_theta([1e-3], "nfw", dndz=[1.0, 2.0])                                       # dndz not on zs
    with pytest.raises(ValueError):
        h.get_w_theta([1e-3], "nfw", dndz=[0.0, 0.0, 0.0])                                  # nothing to normalise
    h.comoving_radial_distance = lambda zs: np.r_[0.0, CHIS[1:]]                            # z = 0 has no angle
    with pytest.raises(ValueError):
        h.get_angular([1e-3], "nfw", zweights=ZW)


# ---------------------------------------------------------------- 5. angular_weights
def test_angular_weights_against_a_hand_computation():
    from hmvec_amd.cosmology import Cosmology
    c = Cosmology(engine="analytic", accuracy="low")
    zs = np.array([0.2, 0.5, 0.6, 1.0])
    H = np.asarray(c.h_of_z(zs), dtype=np.float64)
    dz = np.array([0.15, 0.2, 0.25, 0.2])               # trapezoid: (0.3)/2, (0.3 + 0.1)/2, (0.1 + 0.4)/2, (0.4)/2
    W1 = np.array([1.0, 2.0, 3.0, 4.0])
    W2 = np.array([[0.5, 0.5, 0.5, 0.5], [1.0, 0.0, -1.0, 2.0]])
    got = c.angular_weights(zs, W1, W2)
    assert got.shape == (2, 4)
    assert np.allclose(got, dz * H * W1 * W2, rtol=1e-15, atol=0)
    assert np.allclose(c.angular_weights(zs, 1.0, 1.0), dz * H, rtol=1e-15, atol=0)
    assert np.allclose(c.angular_weights(zs, W1, 2.0), 2.0 * dz * H * W1, rtol=1e-15, atol=0)
    assert c.angular_weights(zs, W2, W2).shape == (2, 4)
    for bad in (np.ones(3), np.ones((2, 3)), np.ones((2, 2, 4))):
        with pytest.raises(ValueError):
            c.angular_weights(zs, bad, 1.0)
        with pytest.raises(ValueError):
            c.angular_weights(zs, 1.0, bad)


# ---------------------------------------------------------------- 6. the ABI and the exports
def test_abi_declares_the_entry_points():
    assert nat.SIGNATURES["hmg_angular_transform"] == [nat._P, nat._I, nat._I, nat._I, nat._I] + [nat._P] * 7
    assert nat.SIGNATURES["hmg_angular_zsum"] == [nat._P, nat._I, nat._I, nat._I, nat._I, nat._P, nat._P, nat._P]
    with open(os.path.join(REPO, "include", "hmgrid.h")) as f:
        header = f.read()
    for name in ("hmg_angular_transform", "hmg_angular_zsum"):
        m = re.search(r"int " + name + r"\(([^)]*)\);", header)
        assert m, f"{name} is not declared in include/hmgrid.h"
        assert m.group(1).count(",") + 1 == len(nat.SIGNATURES[name])
    assert "#define HMG_ABI_VERSION 10" in header and nat.ABI_VERSION == 10


def test_library_exports_the_entry_points():
    lib = nat.load()
    assert hasattr(lib, "hmg_angular_transform") and hasattr(lib, "hmg_angular_zsum")


def test_exports():
    assert hmvec_amd.angular_from_power is angular.angular_from_power
    assert "angular_from_power" in hmvec_amd.__all__ and "angular_from_power" in angular.__all__
    assert hmvec_amd.angular is angular and "angular" in hmvec_amd.__all__
    from hmvec_amd.halomodel import HaloModel
    for name in ("get_angular", "get_w_theta", "get_gamma_t", "get_xi_pm", "get_angular_all", "angular_weights"):
        assert callable(getattr(HaloModel, name))
