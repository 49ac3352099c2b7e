"""Host checks of the correlation-function transform (hmvec_amd.realspace): the panel formula the
kernel evaluates against 40-digit mpmath of an independent closed form, a Gaussian with a known xi(r), the argument
checks of xi_from_power and the ABI declaration.  The device is checked in tests/test_gpu_realspace.py."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO
from hmvec_amd import _native as nat
from hmvec_amd import realspace, xi_from_power

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import realspace_model as rm  # noqa: E402

RADII = np.array([1e-3, 0.03, 1.0, 30.0, 300.0])


@pytest.mark.parametrize("grid", ["log", "uneven"])
@pytest.mark.parametrize("row", ["power", "sign_changing"])
def test_panel_formula_meets_the_gate_against_mpmath(grid, row):
    ks = np.geomspace(1e-4, 100, 33) if grid == "log" else rm.uneven_grid(33)
    P = rm.power_like(ks) if row == "power" else rm.sign_changing(ks)
    if row == "sign_changing":
        assert np.sum(np.diff(np.sign(P)) != 0) >= 3
    got, ref = rm.xi_numpy(ks, P, RADII), rm.xi_mpmath(ks, P, RADII)
    err, tol = np.abs(got - ref), rm.gate(ks, P, RADII)
    print("err / gate:", err / tol, " |xi| / A:", np.abs(ref) / rm.panel_scale(ks, P, RADII))
    assert np.all(err <= tol), (err / tol).max()


def test_series_and_closed_forms_at_the_switch():
    """Either side of the switch S is within 4e-16 and G within 32 * 2^-53 of their 40-digit values: the closed form of
    G has lost 3 / theta^2 = 12 there (times the few roundings of its numerator), the series is truncated below 1e-16."""
    th = rm.SERIES_THETA * np.array([1e-3, 0.5, 1 - 1e-9, 1 + 1e-9, 2.0])
    S, G = rm.panel_factors(th)
    import mpmath as mp
    with mp.workdps(40):
        for t, s, g in zip(th, S, G):
            t = mp.mpf(float(t))
            assert abs(s - mp.sin(t) / t) < 4e-16
            assert abs(g - 3 * (mp.sin(t) - t * mp.cos(t)) / t ** 3) < 32 * 2.0 ** -53


def test_gaussian_known_answer():
    """P = exp(-k^2 s^2 / 2) has xi = exp(-r^2 / 2 s^2) / ((2 pi)^(3/2) s^3).  The tolerance is derived, with |sin| <= 1:
    linear interpolation of f = k P is off by at most h^2/8 max|f''| on a panel, so the integral by
    (1/(2 pi^2 r)) sum_i h_i^3/8 max_panel|f''|; the omitted head [0, k_0] holds at most k_0^3/(6 pi^2)
    (|sin(kr)| <= kr, P <= 1); the tail at most int_{k_max}^inf k^2 P dk / (2 pi^2) (|sin(kr)/(kr)| <= 1)."""
    s = 1.0
    ks = np.linspace(0.01, 12, 1200)
    P = np.exp(-0.5 * (ks * s) ** 2)
    rs = np.array([0.5, 1.0, 2.0])
    ref = np.exp(-0.5 * (rs / s) ** 2) / ((2 * np.pi) ** 1.5 * s ** 3)
    f2 = np.abs((ks ** 3 - 3 * ks) * np.exp(-0.5 * ks ** 2))          # |f''|, f = k exp(-k^2/2)
    h = np.diff(ks)
    # |f'''| = |k^4 - 6 k^2 + 3| exp(-k^2/2) <= 3, so |f''| on a panel is within 3 h / 2 of its value at the nearer end
    f2_panel = np.maximum(f2[1:], f2[:-1]) + 1.5 * h
    interp = np.sum(h ** 3 / 8 * f2_panel) / (2 * np.pi ** 2 * rs)
    head = ks[0] ** 3 / (6 * np.pi ** 2)
    K = ks[-1]
    tail = (K * math.exp(-0.5 * K * K) + math.sqrt(np.pi / 2) * math.erfc(K / math.sqrt(2))) / (2 * np.pi ** 2)
    tol = interp + head + tail
    got = rm.xi_numpy(ks, P, rs)
    print("err:", np.abs(got - ref), "tol:", tol)
    assert np.all(tol < 1e-3 * ref)                                   # the bound is far below the answer it brackets
    assert np.all(np.abs(got - ref) <= tol)


class NoLaunch:
    """A context that fails the test on any use: the argument checks come before every upload and launch."""

    def __getattr__(self, name):
        raise AssertionError(f"context used ({name}) before the arguments were checked")


KS = np.geomspace(1e-3, 10, 16)
GOOD_P = rm.power_like(KS)


@pytest.mark.parametrize("ks,P,rs", [
    (KS[::-1], GOOD_P, [1.0]),                                 # decreasing
    (np.r_[KS[:5], KS[4:]], np.r_[GOOD_P[:5], GOOD_P[4:]], [1.0]),   # a repeated wavenumber
    (np.r_[0.0, KS[1:]], GOOD_P, [1.0]),                       # k = 0
    (np.r_[-1.0, KS[1:]], GOOD_P, [1.0]),                      # negative
    (np.r_[KS[:-1], np.inf], GOOD_P, [1.0]),                   # non-finite
    (KS[:1], GOOD_P[:1], [1.0]),                               # nk < 2
    (KS.reshape(4, 4), GOOD_P, [1.0]),                         # not a vector
    (KS, np.r_[GOOD_P[:-1], np.nan], [1.0]),                   # non-finite P
    (KS, np.r_[np.inf, GOOD_P[1:]], [1.0]),
    (KS, GOOD_P[:-1], [1.0]),                                  # wrong length
    (KS, np.ones((2, 3, 4, KS.size)), [1.0]),                  # too many axes
    (KS, np.ones((KS.size, 2)), [1.0]),                        # nk not last
    (KS, np.float64(1.0), [1.0]),                              # no axis at all
    (KS, GOOD_P, [1.0, 0.0]),                                  # r = 0
    (KS, GOOD_P, [-2.0]),                                      # negative r
    (KS, GOOD_P, [1.0, np.nan]),                               # non-finite r
    (KS, GOOD_P, [np.inf]),
    (KS, GOOD_P, [[1.0, 2.0]]),                                # radii not a vector
])
def test_bad_arguments_raise_before_any_launch(ks, P, rs):
    with pytest.raises(ValueError):
        xi_from_power(ks, P, rs, ctx=NoLaunch())


def test_a_resident_spectrum_of_the_wrong_shape_raises_before_any_launch():
    P = nat.DeviceArray(None, 0, (3, KS.size + 1), owner=False)
    with pytest.raises(ValueError):
        xi_from_power(KS, P, [1.0], ctx=NoLaunch())


@pytest.mark.parametrize("shape", [(KS.size,), (3, KS.size), (2, 3, KS.size)])
def test_empty_radii_return_an_empty_array_without_a_launch(shape):
    out = xi_from_power(KS, np.ones(shape), [], ctx=NoLaunch())
    assert out.shape == shape[:-1] + (0,) and out.dtype == np.float64


def test_get_xi_refuses_an_unknown_term_and_bad_radii_before_any_launch():
    from hmvec_amd.halomodel import HaloModel
    h = HaloModel.__new__(HaloModel)          # no constructor: nothing may be touched but the request
    h.ks = KS
    for rs, term in (([1.0], "one-halo"), ([1.0], None), ([0.0], "total"), ([np.nan], "2h")):
        with pytest.raises(ValueError):
            h.get_xi(rs, "nfw", term=term)
        with pytest.raises(ValueError):
            h.get_xi_all([("nfw", "nfw")], rs, term=term)
    h.ks = KS[::-1]
    with pytest.raises(ValueError):
        h.get_xi([1.0], "nfw")


def test_abi_declares_the_entry_point():
    assert nat.SIGNATURES["hmg_xi_transform"] == [nat._P, nat._I, nat._I, nat._I, nat._P, nat._P, nat._P, nat._P]
    with open(os.path.join(REPO, "include", "hmgrid.h")) as f:
        header = f.read()
    assert "int hmg_xi_transform(" in header
    assert "#define HMG_ABI_VERSION 10" in header and nat.ABI_VERSION == 10
    assert realspace.xi_from_power is xi_from_power


def test_library_exports_the_entry_point():
    assert hasattr(nat.load(), "hmg_xi_transform")
