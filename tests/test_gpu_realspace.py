"""GPU checks of the correlation-function transform (hmvec_amd.realspace, HaloModel.get_xi / get_xi_all; definition and
gate in DESIGN.md section 13).  The reference has no configuration-space statistic, so there is no reference fixture:
the device is pinned by 40-digit mpmath of an independent closed form of the same integral, and at sizes where mpmath is
slow by the numpy restatement that tests/test_realspace_cpu.py pins against mpmath."""
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import xi_from_power

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import realspace_model as rm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

RADII = np.geomspace(1e-3, 300, 25)


def switch_radii(h):
    """Radii that put theta = r h / 2 of a panel of width h just below and just above the series switch."""
    return 2.0 * rm.SERIES_THETA / h * np.array([1 - 1e-6, 1 + 1e-6])


def within_gate(got, ref, ks, P, rs):
    err, tol = np.abs(got - ref), rm.gate(ks, P, rs)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"worst |xi - ref| / gate = {worst:.3g}")
    return np.all(err <= tol), worst


# ---------------------------------------------------------------- 1. device vs 40-digit mpmath
@pytest.mark.parametrize("P2", [[2.0, 0.7], [3.0, -1.0]])
def test_one_panel_against_mpmath(P2):
    ks, P = np.array([0.5, 1.5]), np.array(P2)
    rs = np.concatenate([RADII, switch_radii(1.0)])
    theta = 0.5 * rs[-2:] * (ks[1] - ks[0])
    assert theta[0] < rm.SERIES_THETA < theta[1]
    got = xi_from_power(ks, P, rs)
    assert got.shape == (rs.size,)
    ok, worst = within_gate(got, rm.xi_mpmath(ks, P, rs), ks, P, rs)
    assert ok, worst


@pytest.mark.parametrize("grid", ["log", "uneven"])
def test_33_points_against_mpmath(grid):
    ks = np.geomspace(1e-4, 100, 33) if grid == "log" else rm.uneven_grid(33)
    rs = np.concatenate([RADII, switch_radii(ks[21] - ks[20])])
    P = np.stack([rm.power_like(ks), rm.sign_changing(ks)])
    got = xi_from_power(ks, P, rs)
    assert got.shape == (2, rs.size)
    for row in range(2):
        ok, worst = within_gate(got[row], rm.xi_mpmath(ks, P[row], rs), ks, P[row], rs)
        assert ok, (row, worst)


# ---------------------------------------------------------------- 2. device vs the numpy restatement
# nk = 258: 257 panels, one past a 256-thread stride; nk = 1030: a fifth panel for six threads, on an uneven grid.  70
# radii: seventeen tiles of four and a tile of two.
RS70 = np.geomspace(1e-3, 300, 70)


def batch(ks):
    base = rm.power_like(ks)
    return np.stack([base, rm.sign_changing(ks), np.zeros_like(ks), base * (1 + 0.3 * np.sin(7 * np.log(ks))),
                     -base * ks ** 0.3])


@pytest.fixture(scope="module")
def batch258():
    ks = np.geomspace(1e-4, 100, 258)
    P = batch(ks)
    return ks, P, xi_from_power(ks, P, RS70)


@pytest.fixture(scope="module")
def batch1030():
    ks = rm.uneven_grid(1030)
    P = batch(ks)
    return ks, P, xi_from_power(ks, P, RS70)


@pytest.mark.parametrize("which", ["batch258", "batch1030"])
def test_batch_against_the_numpy_restatement(which, request):
    ks, P, got = request.getfixturevalue(which)
    assert got.shape == (5, 70)
    assert np.sum(np.diff(np.sign(P[1])) != 0) >= 3
    assert np.all(got[2] == 0.0)                       # a row of zeros: exactly zero
    ok, worst = within_gate(got, rm.xi_numpy(ks, P, RS70), ks, P, RS70)
    assert ok, worst


# ---------------------------------------------------------------- 3. determinism and independence
def test_repeat_is_bit_identical(batch258):
    ks, P, got = batch258
    assert np.array_equal(xi_from_power(ks, P, RS70), got)


def test_a_row_does_not_depend_on_the_batch(batch258):
    ks, P, got = batch258
    alone = xi_from_power(ks, P[3], RS70)
    assert alone.shape == (70,) and np.array_equal(alone, got[3])


def test_a_radius_does_not_depend_on_the_others(batch258):
    ks, P, got = batch258
    alone = xi_from_power(ks, P, RS70[41:42])
    assert alone.shape == (5, 1) and np.array_equal(alone[:, 0], got[:, 41])


def test_device_input_equals_host_input(batch258):
    ks, P, got = batch258
    ctx = nat.default_context(0)
    d_P = ctx.upload(P)
    assert np.array_equal(xi_from_power(ks, d_P, RS70), got)
    d_P3 = ctx.upload(P.reshape(1, 5, -1))
    assert np.array_equal(xi_from_power(ks, d_P3, RS70, ctx=ctx), got.reshape(1, 5, 70))


# ---------------------------------------------------------------- 4. the facade
ZS = np.array([0.3, 1.0])
RS = np.concatenate([np.geomspace(0.05, 150, 9), [10.0, 140.0, 230.0]])
PAIRS = [("g", "g"), ("g", "nfw"), ("nfw", "nfw")]


@pytest.fixture(scope="module")
def halo():
    h = model(ZS)
    h.add_hod("g", mthresh=10 ** 10.5 + ZS * 0.0)
    return h


def test_get_xi_is_the_transform_of_get_power(halo):
    got = halo.get_xi(RS, "g", "nfw")
    assert got.shape == (ZS.size, RS.size)
    assert np.array_equal(got, xi_from_power(halo.ks, halo.get_power("g", "nfw"), RS))
    assert np.array_equal(halo.get_xi(RS, "nfw"), xi_from_power(halo.ks, halo.get_power("nfw"), RS))
    assert halo.get_xi([], "g").shape == (ZS.size, 0)
    assert halo.get_xi(7.0, "g").shape == (ZS.size, 1)


def test_terms_are_the_transforms_of_the_terms(halo):
    P1, P2 = halo.get_power_1halo("g", "nfw"), halo.get_power_2halo("g", "nfw")
    x1, x2 = halo.get_xi(RS, "g", "nfw", term="1h"), halo.get_xi(RS, "g", "nfw", term="2h")
    assert np.array_equal(x1, xi_from_power(halo.ks, P1, RS))
    assert np.array_equal(x2, xi_from_power(halo.ks, P2, RS))
    # Each transform is within its gate of the exact transform of its rows, which is linear, and the device sum
    # P_1h + P_2h is rounded once (2^-53 of |P_1h + P_2h|, inside the 1e-13 A of its gate): the gates add.
    total = halo.get_xi(RS, "g", "nfw")
    tol = rm.gate(halo.ks, P1, RS) + rm.gate(halo.ks, P2, RS) + rm.gate(halo.ks, P1 + P2, RS)
    err = np.abs(x1 + x2 - total)
    print("worst |xi_1h + xi_2h - xi| / gates =", float(np.max(err / tol)))
    assert np.all(err <= tol)


def test_get_xi_all_equals_get_xi(halo):
    for term in ("total", "1h", "2h"):
        got = halo.get_xi_all(PAIRS, RS, term=term)
        assert list(got) == PAIRS
        for a, b in PAIRS:
            assert got[(a, b)].shape == (ZS.size, RS.size)
            assert np.array_equal(got[(a, b)], halo.get_xi(RS, a, b, term=term)), (term, a, b)


def test_unknown_term_raises(halo):
    with pytest.raises(ValueError):
        halo.get_xi(RS, "g", term="3h")
    with pytest.raises(ValueError):
        halo.get_xi_all(PAIRS, RS, term="both")


def test_two_halo_matter_xi_changes_sign_past_the_acoustic_peak(halo):
    """Sign and normalisation: the two-halo xi_mm is positive at r = 10 Mpc and stays positive through the acoustic
    peak of this background (the transform of its linear spectrum crosses zero between r = 170 and 180 Mpc); it is
    negative beyond, at r = 230 Mpc, by 2e-3 of the panel scale A(r) - ten orders above the gate."""
    xi = halo.get_xi(RS[-3:], "nfw", term="2h")
    print("xi_mm^2h at r = 10, 140, 230:", xi)
    assert np.all(xi[:, 0] > 0) and np.all(xi[:, 1] > 0) and np.all(xi[:, 2] < 0)
    assert np.all(xi[:, 0] > 10 * xi[:, 1])
