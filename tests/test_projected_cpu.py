"""Host checks of the Hankel transforms of orders 0 and 2 (hmvec_amd.realspace.projected_from_power, DESIGN.md section
14): the by-parts sum the kernel evaluates against 40-digit mpmath of an independent form, a Gaussian with known W_0 and
W_2, the identity that ties W_2 to the mean of W_0 inside R, the argument checks of projected_from_power and of the
facade methods, and the ABI declaration.  The device is checked in tests/test_gpu_projected.py."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO
from hmvec_amd import _native as nat
from hmvec_amd import projected_from_power, realspace

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import projected_model as pm  # noqa: E402

RADII = np.array([1e-3, 0.03, 1.0, 30.0, 300.0])
SWITCH_NODE = 20            # the interior node whose x = k R the two extra radii put either side of the switch


def grid_and_radii(grid):
    if grid == "two":
        ks = np.array([0.5, 1.5])
        return ks, np.concatenate([RADII, pm.switch_radii(ks[1])])
    ks = np.geomspace(1e-4, 100, 33) if grid == "log" else pm.uneven_grid(33)
    return ks, np.concatenate([RADII, pm.switch_radii(ks[SWITCH_NODE])])


# ---------------------------------------------------------------- 1. the by-parts sum against mpmath
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("row", ["positive", "sign_changing"])
@pytest.mark.parametrize("grid", ["two", "log", "uneven"])
def test_by_parts_sum_meets_the_gate_against_mpmath(grid, row, order):
    ks, rs = grid_and_radii(grid)
    x = rs[-2:] * (ks[1] if grid == "two" else ks[SWITCH_NODE])
    assert x[0] < pm.SERIES_X < x[1] and abs(x[1] - x[0]) < 1e-5
    if grid == "two":
        P = np.array([2.0, 0.7]) if row == "positive" else np.array([3.0, -1.0])
    else:
        P = pm.power_like(ks) if row == "positive" else pm.sign_changing(ks)
        if row == "sign_changing":
            assert np.sum(np.diff(np.sign(P)) != 0) >= 3
    got, ref = pm.hankel_numpy(ks, P, rs, order), pm.hankel_mpmath(ks, P, rs, order)
    err, tol = np.abs(got - ref), pm.gate(ks, P, rs)
    print("err / gate:", err / tol, " |W| / A:", np.abs(ref) / pm.panel_scale(ks, P, rs))
    assert np.all(err <= tol), (err / tol).max()


def test_series_and_closed_forms_at_the_switch():
    """At the switch and above, g, H1 and H2 are within 8 roundings (8 * 2^-53) of the size of the terms their closed forms
    subtract (x^2 for H1, 2 x^2 for H2 and for the division-free g) of their 40-digit values, and so are the series just
    below it; well below the switch the series are relative: 4 ulp of the value (eleven terms summed, no cancellation)."""
    import mpmath as mp
    xs = pm.SERIES_X * np.array([1e-3, 0.5, 1 - 1e-9, 1 + 1e-9, 2.0])
    g, h1, h2 = pm.g_fn(xs), pm.h1_fn(xs), pm.h2_fn(xs)
    with mp.workdps(40):
        for i, x in enumerate(xs):
            x = mp.mpf(float(x))
            j0, j1, j2 = mp.besselj(0, x), mp.besselj(1, x), mp.besselj(2, x)
            ref = (x * x * j2, 2 * (1 - j0) - x * j1, x * x - 2 * x * j1 - x * x * j2)
            for got, r, size in zip((g[i], h1[i], h2[i]), ref, (2 * x * x, x * x, 2 * x * x)):
                bound = 4 * 2.0 ** -52 * abs(r) if x < 1.5 else 8 * 2.0 ** -53 * size
                assert abs(got - r) <= bound, (float(x), float(got), float(r))


# ---------------------------------------------------------------- 2., 3. the Gaussian
GK = np.linspace(0.01, 12, 1200)
GP = np.exp(-0.5 * GK ** 2)


def gaussian_bounds(rs):
    """Bounds on |W_n of the tabulated Gaussian - W_n of exp(-k^2/2)|, with |J_n| <= 1 where nothing better is said:
    * head, the omitted [0, k_0]: int_0^k0 k dk / (2 pi) = k_0^2/(4 pi) for W_0; |J2(x)| <= x^2/8 gives
      k_0^4 R^2/(64 pi) for W_2;
    * tail: int_K^inf k exp(-k^2/2) dk / (2 pi) = exp(-K^2/2)/(2 pi);
    * interpolation: P is exp(-u/2) in u = k^2, its linear interpolant in u is off by at most du^2/8 max|d2P/du2| =
      du^2/32 exp(-a^2/2) on a panel [a, b], du = b^2 - a^2 (the second derivative exp(-u/2)/4 is largest at the left
      end), and int_a^b k dk = du/2: (1/(2 pi)) sum_i du_i^3/64 exp(-a_i^2/2)."""
    k0, K = GK[0], GK[-1]
    du = np.diff(GK ** 2)
    interp = np.sum(du ** 3 / 64.0 * np.exp(-0.5 * GK[:-1] ** 2)) / (2 * np.pi)
    tail = math.exp(-0.5 * K * K) / (2 * np.pi)
    return k0 ** 2 / (4 * np.pi) + tail + interp, k0 ** 4 * rs ** 2 / (64 * np.pi) + tail + interp


def test_gaussian_known_answer():
    """P = exp(-k^2/2): W_0 = exp(-R^2/2)/(2 pi), W_2 = [(2/R^2)(1 - exp(-R^2/2)) - exp(-R^2/2)]/(2 pi)."""
    rs = np.array([0.5, 1.0, 2.0, 4.0])
    e = np.exp(-0.5 * rs ** 2)
    ref0, ref2 = e / (2 * np.pi), ((2 / rs ** 2) * (1 - e) - e) / (2 * np.pi)
    tol0, tol2 = gaussian_bounds(rs)
    err0 = np.abs(pm.hankel_numpy(GK, GP, rs, 0) - ref0)
    err2 = np.abs(pm.hankel_numpy(GK, GP, rs, 2) - ref2)
    print("W_0 err:", err0, "tol:", tol0, " W_2 err:", err2, "tol:", tol2)
    assert tol0 < 2e-5 and np.all(tol2 < 1e-5)                 # (the bounds are far below W_0(1) = 0.097)
    assert np.all(err0 <= tol0) and np.all(err2 <= tol2)


def test_w2_is_the_mean_of_w0_inside_R_minus_w0():
    """(2/R^2) int_0^R J0(k R') R' dR' - J0(k R) = 2 J1(k R)/(k R) - J0(k R) = J2(k R), so for any row
    W_2(R) = (2/R^2) int_0^R W_0(R') R' dR' - W_0(R), exactly.  The integral by n-point Gauss-Legendre: its remainder is
    R^(2n+1) (n!)^4 / ((2n+1) ((2n)!)^3) max|f^(2n)|, and f = W_0(R') R' has
    |f^(m)| <= A K^m (R + m/K) (|d^m/dR^m J0(k R)| <= k^m, k <= K = 12, A the panel scale): with n = 64 below 1e-30 A at
    R = 4.  What is left is the rounding of the three transforms, each inside its gate."""
    n, K = 64, GK[-1]
    t, w = np.polynomial.legendre.leggauss(n)
    A = pm.panel_scale(GK, GP, [1.0])[0]
    for R in (0.5, 1.0, 2.0, 4.0):
        Rq, wq = 0.5 * R * (t + 1), 0.5 * R * w
        mean = 2.0 / R ** 2 * np.sum(wq * Rq * pm.hankel_numpy(GK, GP, Rq, 0))
        w0, w2 = pm.hankel_numpy(GK, GP, [R], 0)[0], pm.hankel_numpy(GK, GP, [R], 2)[0]
        log_rem = ((2 * n + 1) * math.log(R) + 4 * math.lgamma(n + 1) - math.log(2 * n + 1) - 3 * math.lgamma(2 * n + 1)
                   + 2 * n * math.log(K) + math.log(R + 2 * n / K))
        rem = 2.0 / R ** 2 * A * math.exp(log_rem)
        assert rem < 1e-30 * A
        tol = rem + 2 * pm.gate(GK, GP, [R])[0] + 2.0 / R ** 2 * np.sum(wq * Rq * pm.gate(GK, GP, Rq))
        err = abs(mean - w0 - w2)
        print(f"R = {R}: |mean - W_0 - W_2| = {err:.3g}, tol {tol:.3g}, W_2 = {w2:.6g}")
        assert err <= tol


# ---------------------------------------------------------------- 4. argument checks of projected_from_power
class NoLaunch:
    """A context that fails the test on any use: the argument checks come before every upload and launch."""

    def __getattr__(self, name):
        raise AssertionError(f"context used ({name}) before the arguments were checked")


KS = np.geomspace(1e-3, 10, 16)
GOOD_P = pm.power_like(KS)


@pytest.mark.parametrize("order", [0, 2, (0, 2)])
@pytest.mark.parametrize("ks,P,rs", [
    (KS[::-1], GOOD_P, [1.0]),                                 # decreasing
    (np.r_[KS[:5], KS[4:]], np.r_[GOOD_P[:5], GOOD_P[4:]], [1.0]),   # a repeated wavenumber
    (np.r_[0.0, KS[1:]], GOOD_P, [1.0]),                       # k = 0
    (np.r_[KS[:-1], np.inf], GOOD_P, [1.0]),                   # non-finite
    (KS[:1], GOOD_P[:1], [1.0]),                               # nk < 2
    (KS.reshape(4, 4), GOOD_P, [1.0]),                         # not a vector
    (KS, np.r_[GOOD_P[:-1], np.nan], [1.0]),                   # non-finite P
    (KS, GOOD_P[:-1], [1.0]),                                  # wrong length
    (KS, np.ones((2, 3, 4, KS.size)), [1.0]),                  # too many axes
    (KS, np.ones((KS.size, 2)), [1.0]),                        # nk not last
    (KS, np.float64(1.0), [1.0]),                              # no axis at all
    (KS, GOOD_P, [1.0, 0.0]),                                  # R = 0
    (KS, GOOD_P, [-2.0]),                                      # negative R
    (KS, GOOD_P, [1.0, np.nan]),                               # non-finite R
    (KS, GOOD_P, [[1.0, 2.0]]),                                # radii not a vector
])
def test_bad_arguments_raise_before_any_launch(ks, P, rs, order):
    with pytest.raises(ValueError):
        projected_from_power(ks, P, rs, order, ctx=NoLaunch())


@pytest.mark.parametrize("order", [1, -2, (2, 0), (0, 0), (0, 2, 2), (), "0", 0.0, 2.0, True, None, (0, 2.0)])
def test_a_bad_order_raises_before_any_launch(order):
    with pytest.raises(ValueError):
        projected_from_power(KS, GOOD_P, [1.0], order, ctx=NoLaunch())


def test_a_resident_spectrum_of_the_wrong_shape_raises_before_any_launch():
    P = nat.DeviceArray(None, 0, (3, KS.size + 1), owner=False)
    with pytest.raises(ValueError):
        projected_from_power(KS, P, [1.0], (0, 2), ctx=NoLaunch())


@pytest.mark.parametrize("shape", [(KS.size,), (3, KS.size), (2, 3, KS.size)])
def test_empty_radii_return_empty_arrays_without_a_launch(shape):
    for order in (0, 2, [0, 2], np.int64(2)):
        out = projected_from_power(KS, np.ones(shape), [], order, ctx=NoLaunch())
        outs = out if isinstance(order, list) else (out,)
        assert isinstance(out, tuple) == isinstance(order, list) and len(outs) == (2 if isinstance(order, list) else 1)
        for o in outs:
            assert o.shape == shape[:-1] + (0,) and o.dtype == np.float64


# ---------------------------------------------------------------- 5. argument checks of the facade
def test_the_facade_refuses_an_unknown_term_and_bad_radii_before_any_launch():
    from hmvec_amd.halomodel import HaloModel
    h = HaloModel.__new__(HaloModel)          # no constructor: nothing may be touched but the request
    h.ks = KS
    single = (h.get_wp, h.get_surface_density, h.get_excess_surface_density)
    batch = (h.get_wp_all, h.get_surface_density_all)
    for rs, term in (([1.0], "one-halo"), ([1.0], None), ([0.0], "total"), ([np.nan], "2h"), ([[1.0, 2.0]], "1h")):
        for f in single:
            with pytest.raises(ValueError):
                f(rs, "nfw", term=term)
        for f in batch:
            with pytest.raises(ValueError):
                f([("nfw", "nfw")], rs, term=term)
    h.ks = KS[::-1]
    for f in single:
        with pytest.raises(ValueError):
            f([1.0], "nfw")
    for f in batch:
        with pytest.raises(ValueError):
            f([("nfw", "nfw")], [1.0])


# ---------------------------------------------------------------- 6. the ABI
def test_abi_declares_the_entry_point():
    assert nat.SIGNATURES["hmg_hankel_transform"] == [nat._P, nat._I, nat._I, nat._I, nat._P, nat._P, nat._P, nat._P,
                                                      nat._P]
    with open(os.path.join(REPO, "include", "hmgrid.h")) as f:
        header = f.read()
    assert "int hmg_hankel_transform(" in header
    assert "#define HMG_ABI_VERSION 10" in header and nat.ABI_VERSION == 10
    assert realspace.projected_from_power is projected_from_power


def test_library_exports_the_entry_point():
    assert hasattr(nat.load(), "hmg_hankel_transform")
