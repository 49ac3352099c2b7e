"""GPU checks of the angular correlation functions (hmvec_amd.angular.angular_from_power; HaloModel.get_angular,
get_w_theta, get_gamma_t, get_xi_pm and get_angular_all; definition and gates in DESIGN.md section 22).  The reference
computes none of these statistics, so there is no reference fixture: the device is pinned by 40-digit mpmath of an
independent form of the same integrals, at sizes where mpmath is slow by the numpy restatement that
tests/test_angular_cpu.py and tests/test_projected_cpu.py pin against mpmath, and by bit-identities - among them that
orders 0 and 2 are projected_from_power's bits at the radius chi theta.

Measured on an MI355X (worst |got - ref| / gate, orders 0, 2, 4): against mpmath 5.1e-3, 6.3e-4, 1.2e-3; the batches
against the numpy restatement 4.8e-3, 6.5e-5, 2.8e-5."""
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import angular_from_power, projected_from_power
from hmvec_amd.cosmology import _trapz

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import angular_model as am  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS = (0, 2, 4)
SUBSETS = [(0,), (2,), (4,), (0, 2), (0, 4), (2, 4)]


def within_gate(got, ref, tol, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what}: worst |zeta - ref| / gate = {worst:.3g}")
    return np.all(err <= tol), worst


# ---------------------------------------------------------------- 1. device vs 40-digit mpmath
# The radii chi theta run from 1e-3 to above 300 in the inverse units of ks; five angles are one more than a tile.
def check_against_mpmath(ks, P, thetas, chis):
    """All three orders of the (nz, nk) block P, z-resolved (the identity as weights) and as a genuine signed sum."""
    nz = len(chis)
    signed = np.array([[0.7, -1.3, 0.45][:nz], [-0.2, 0.9, 1.6][:nz]])
    got = {what: angular_from_power(ks, P, thetas, chis, zw, ORDERS)
           for what, zw in (("z-resolved", np.eye(nz)), ("weighted", signed))}
    for i, order in enumerate(ORDERS):
        W = am.per_z(am.wn_mpmath, ks, P, thetas, chis, order)
        for what, zw in (("z-resolved", np.eye(nz)), ("weighted", signed)):
            z = got[what][i]
            assert len(got[what]) == 3 and z.shape == (zw.shape[0], len(thetas))
            ok, worst = within_gate(z, zw @ W, am.angular_gate(ks, P, thetas, chis, zw, order, W), f"{what} order {order}")
            assert ok, (what, order, worst)


@pytest.mark.parametrize("ntheta", [1, 5])
@pytest.mark.parametrize("nz", [1, 3])
def test_one_panel_against_mpmath(nz, ntheta):
    ks = np.array([0.5, 1.5])
    P = np.array([[2.0, 0.7], [3.0, -1.0], [0.4, 1.9]])
    chis = np.array([1.0, 7.3, 41.0])
    thetas = np.array([1e-3, 0.05, 0.9, 6.0, 25.0]) if ntheta == 5 else np.array([0.9])
    if nz == 1:
        for row in (0, 1):
            check_against_mpmath(ks, P[row:row + 1], thetas, chis[1:2])
    else:
        check_against_mpmath(ks, P, thetas, chis)


@pytest.mark.parametrize("ntheta", [1, 5])
@pytest.mark.parametrize("nz", [1, 3])
def test_33_points_against_mpmath(nz, ntheta):
    ks = np.geomspace(1e-4, 100, 33)
    P = np.stack([am.power_like(ks), am.sign_changing(ks), 0.6 * am.power_like(ks) * (1 + 0.3 * np.sin(7 * np.log(ks)))])
    chis = np.array([3.0, 1.0, 0.11])[:nz]
    below, above = am.switch_radii4(ks[20]) / chis[0]           # node 20 of the first row either side of the switch
    x = np.float64(chis[0]) * np.array([below, above]) * ks[20]
    assert x[0] < am.SERIES_X4 < x[1]
    thetas = np.array([1e-3, below, above, 9.0, 100.0]) if ntheta == 5 else np.array([above])
    check_against_mpmath(ks, P[:nz], thetas, chis)


# ---------------------------------------------------------------- 2. device vs the numpy restatement
# nk = 258: 257 panels, one more than the workgroup has threads; nk = 1030 on an uneven grid: runs of five panels, the
# last owner's shorter.  n = 2 pairs x nz = 3 rows with a row of zeros and sign-changing rows; nine angles: two tiles of
# four and a tile of one; signed weights, nw = 1 and 3.
TH9 = np.geomspace(2e-3, 150, 9)
CHI3 = np.array([2.0, 0.9, 0.35])
ZW3 = np.array([[0.0, 1.0, 0.0], [0.3, -1.2, 0.7], [-0.5, 0.25, 2.0]])


def blocks(ks):
    base = am.power_like(ks)
    return np.stack([np.stack([base, np.zeros_like(ks), am.sign_changing(ks)]),
                     np.stack([base * (1 + 0.3 * np.sin(7 * np.log(ks))), -base * ks ** 0.3, 0.5 * base])])


@pytest.fixture(scope="module")
def batch258():
    ks = np.geomspace(1e-4, 100, 258)
    P = blocks(ks)
    return ks, P, angular_from_power(ks, P, TH9, CHI3, ZW3, ORDERS)


@pytest.fixture(scope="module")
def batch1030():
    ks = am.uneven_grid(1030)
    P = blocks(ks)
    return ks, P, angular_from_power(ks, P, TH9, CHI3, ZW3, ORDERS)


@pytest.mark.parametrize("which", ["batch258", "batch1030"])
def test_batch_against_the_numpy_restatement(which, request):
    ks, P, got = request.getfixturevalue(which)
    assert np.sum(np.diff(np.sign(P[0, 2])) != 0) >= 3
    one = angular_from_power(ks, P, TH9, CHI3, ZW3[1:2], ORDERS)             # nw = 1, two-dimensional
    flat = angular_from_power(ks, P, TH9, CHI3, ZW3[1], ORDERS)              # nw = 1, one-dimensional
    for order, z, z1, zf in zip(ORDERS, got, one, flat):
        assert z.shape == (2, 3, 9) and z1.shape == (2, 1, 9) and zf.shape == (2, 9)
        assert np.all(z[0, 0] == 0.0)                    # the row of zeros, picked by a unit weight: exactly zero
        assert np.array_equal(z1[:, 0], z[:, 1]) and np.array_equal(zf, z[:, 1])
        for i in range(2):
            ref, W = am.angular_sum(am.wn_numpy, ks, P[i], TH9, CHI3, ZW3, order)
            ok, worst = within_gate(z[i], ref, am.angular_gate(ks, P[i], TH9, CHI3, ZW3, order, W),
                                    f"{which} pair {i} order {order}")
            assert ok, (order, i, worst)


# ---------------------------------------------------------------- 3. determinism and independence
def test_repeat_is_bit_identical(batch258):
    ks, P, got = batch258
    again = angular_from_power(ks, P, TH9, CHI3, ZW3, ORDERS)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))


def test_every_subset_of_orders_equals_the_all_orders_launch(batch258, batch1030):
    for ks, P, got in (batch258, batch1030):
        full = dict(zip(ORDERS, got))
        for order in ORDERS:
            assert np.array_equal(angular_from_power(ks, P, TH9, CHI3, ZW3, order), full[order]), order
        for sub in SUBSETS:
            outs = angular_from_power(ks, P, TH9, CHI3, ZW3, sub)
            assert isinstance(outs, tuple) and len(outs) == len(sub)
            assert all(np.array_equal(o, full[n]) for n, o in zip(sub, outs)), sub
        assert np.array_equal(angular_from_power(ks, P, TH9, CHI3, ZW3), full[0])          # order 0 is the default


def test_a_pair_does_not_depend_on_the_batch(batch258):
    ks, P, got = batch258
    alone = angular_from_power(ks, P[1], TH9, CHI3, ZW3, ORDERS)
    assert all(a.shape == (3, 9) and np.array_equal(a, g[1]) for a, g in zip(alone, got))


def test_an_angle_does_not_depend_on_the_others(batch258):
    ks, P, got = batch258
    alone = angular_from_power(ks, P, TH9[6:7], CHI3, ZW3, ORDERS)
    assert all(a.shape == (2, 3, 1) and np.array_equal(a[..., 0], g[..., 6]) for a, g in zip(alone, got))


def test_device_input_equals_host_input(batch258):
    ks, P, got = batch258
    ctx = nat.default_context(0)
    assert all(np.array_equal(a, g) for a, g in zip(angular_from_power(ks, ctx.upload(P), TH9, CHI3, ZW3, ORDERS), got))
    d_one = ctx.upload(P[0])
    assert np.array_equal(angular_from_power(ks, d_one, TH9, CHI3, ZW3, 4, ctx=ctx), got[2][0])


@pytest.mark.parametrize("order", [0, 2])
def test_orders_0_and_2_are_the_projected_transform_at_chi_theta(batch258, batch1030, order):
    """One z with weight 1.0: the z sum returns the transform's bits, and those are hmg_hankel_transform's at the radius
    fl(chi theta)."""
    for ks, P, _ in (batch258, batch1030):
        rows = P.reshape(6, 1, -1)                      # six spectra of one redshift each
        for chi in (0.35, 2.0, 977.25):
            for theta in (TH9[0], TH9[4], TH9[8]):
                got = angular_from_power(ks, rows, [theta], [chi], [1.0], order)
                assert got.shape == (6, 1)
                assert np.array_equal(got, projected_from_power(ks, rows[:, 0], [np.float64(chi) * theta], order))
            got = angular_from_power(ks, rows, TH9, [chi], [1.0], order)
            assert np.array_equal(got, projected_from_power(ks, rows[:, 0], np.float64(chi) * TH9, order))
        both = angular_from_power(ks, rows, TH9, [2.0], [1.0], (0, 2, 4))
        assert np.array_equal(both[order // 2], projected_from_power(ks, rows[:, 0], 2.0 * TH9, order))


def test_w4_is_far_below_w0_at_small_radii():
    """0 < W_4 <= (x^4/384)/(1 - x^2/4) W_0 at x = k_last R <= 0.01 for a positive row (tests/test_angular_cpu.py), on
    the device."""
    ks = np.geomspace(1e-4, 100, 33)
    P = am.power_like(ks)[None, :]
    R = np.array([1e-6, 1e-5, 1e-4])
    x = ks[-1] * R
    w0, w4 = angular_from_power(ks, P, R / 2.0, [2.0], [1.0], (0, 4))
    print("W_4 / W_0 at k_last R = 1e-4, 1e-3, 1e-2:", w4 / w0)
    assert np.all(w4 > 0) and np.all(w4 <= (x ** 4 / 384) / (1 - x ** 2 / 4) * w0)


# ---------------------------------------------------------------- 4. the facade
ZS = np.array([0.3, 0.6, 1.0])
ARCMIN = np.pi / 180 / 60
THETAS = np.concatenate([np.geomspace(0.5, 200, 5), [1.0, 10.0]]) * ARCMIN
PAIRS = [("g", "g"), ("g", "nfw"), ("nfw", "nfw")]
FALLBACK_PAIRS = [("g", "g2"), ("g", "nfw")]            # two different HODs: not a request of the batched mass integrals
DNDZ = np.array([1.0, 2.5, 0.7])
SZ, SDNDZ = np.array([0.8, 1.1, 1.5, 2.0]), np.array([0.5, 1.0, 0.8, 0.1])


@pytest.fixture(scope="module")
def halo():
    h = model(ZS)
    h.add_hod("g", mthresh=10 ** 10.5 + ZS * 0.0)
    h.add_hod("g2", mthresh=10 ** 11.5 + ZS * 0.0)
    return h


def test_get_angular_is_the_transform_of_get_power(halo):
    chis = halo.comoving_radial_distance(ZS)
    zw = halo.angular_weights(ZS, DNDZ, [[1.0, 1.0, 1.0], [0.2, -0.4, 3.0]])
    assert zw.shape == (2, 3)
    got = halo.get_angular(THETAS, "g", "nfw", zw, (0, 2, 4))
    ref = angular_from_power(halo.ks, halo.get_power("g", "nfw"), THETAS, chis, zw, (0, 2, 4))
    assert len(got) == 3 and all(g.shape == (2, THETAS.size) and np.array_equal(g, r) for g, r in zip(got, ref))
    assert np.array_equal(halo.get_angular(THETAS, "g", "nfw", zw[1], 2), ref[1][1])
    assert np.array_equal(halo.get_angular(THETAS, "g", zweights=None),
                          angular_from_power(halo.ks, halo.get_power("g"), THETAS, chis, halo.angular_weights(ZS, 1, 1)))
    for term, P in (("1h", halo.get_power_1halo("g", "nfw")), ("2h", halo.get_power_2halo("g", "nfw"))):
        assert np.array_equal(halo.get_angular(THETAS, "g", "nfw", zw, 4, term=term),
                              angular_from_power(halo.ks, P, THETAS, chis, zw, 4))
    assert halo.get_angular([], "g", zweights=zw).shape == (2, 0) and halo.get_angular([], "g").shape == (0,)
    assert halo.get_angular(3e-3, "g").shape == (1,)


def test_each_wrapper_is_get_angular_with_its_weights(halo):
    Wg = DNDZ / _trapz(DNDZ, ZS)
    Wg2 = np.array([0.2, 1.0, 1.0]) / _trapz([0.2, 1.0, 1.0], ZS)
    Wk, Wk2 = halo.lensing_window(ZS, SZ, SDNDZ), halo.lensing_window(ZS, 1.2)
    for term in ("total", "2h"):
        assert np.array_equal(halo.get_w_theta(THETAS, "g", dndz=DNDZ, term=term),
                              halo.get_angular(THETAS, "g", None, halo.angular_weights(ZS, Wg, Wg), 0, term))
        assert np.array_equal(halo.get_w_theta(THETAS, "g", "g2", DNDZ, [0.2, 1.0, 1.0], term=term),
                              halo.get_angular(THETAS, "g", "g2", halo.angular_weights(ZS, Wg, Wg2), 0, term))
        assert np.array_equal(halo.get_gamma_t(THETAS, "g", dndz=DNDZ, zsource=SZ, sdndz=SDNDZ, term=term),
                              halo.get_angular(THETAS, "g", "nfw", halo.angular_weights(ZS, Wg, Wk), 2, term))
        assert np.array_equal(halo.get_gamma_t(THETAS, "g", dndz=DNDZ, zsource=1.2, term=term),
                              halo.get_angular(THETAS, "g", "nfw", halo.angular_weights(ZS, Wg, Wk2), 2, term))
        xip, xim = halo.get_xi_pm(THETAS, zsource=SZ, sdndz=SDNDZ, zsource2=1.2, term=term)
        ref = halo.get_angular(THETAS, "nfw", None, halo.angular_weights(ZS, Wk, Wk2), (0, 4), term)
        assert xip.shape == xim.shape == (THETAS.size,) and np.array_equal(xip, ref[0]) and np.array_equal(xim, ref[1])
        auto = halo.get_xi_pm(THETAS, zsource=1.2, term=term)
        ref = halo.get_angular(THETAS, "nfw", "nfw", halo.angular_weights(ZS, Wk2, Wk2), (0, 4), term)
        assert np.array_equal(auto[0], ref[0]) and np.array_equal(auto[1], ref[1])
    uniform = np.ones(3) / _trapz(np.ones(3), ZS)
    assert np.array_equal(halo.get_w_theta(THETAS, "g"),
                          halo.get_angular(THETAS, "g", None, halo.angular_weights(ZS, uniform, uniform), 0))


@pytest.mark.parametrize("pairs", [PAIRS, FALLBACK_PAIRS], ids=["batched", "fallback"])
def test_all_entries_equal_the_single_pair_calls(halo, pairs):
    from hmvec_amd import spectra
    rpairs = halo._resolve_pairs(pairs)
    assert spectra.batchable(spectra.pair_plan(rpairs)[0], rpairs) == (pairs is PAIRS)
    zw = halo.angular_weights(ZS, DNDZ, [[1.0, 1.0, 1.0], [0.2, -0.4, 3.0]])
    per = {p: (zw[i % 2] if i != 1 else zw * (i + 1.5)) for i, p in enumerate(pairs)}      # one- and two-dimensional
    for term in ("total", "1h", "2h"):
        shared = halo.get_angular_all(pairs, THETAS, zw, (0, 2, 4), term=term)
        own = halo.get_angular_all(pairs, THETAS, per, (0, 4), term=term)
        single = halo.get_angular_all(pairs, THETAS, zw[0], 2, term=term)
        assert list(shared) == pairs and list(own) == pairs and list(single) == pairs
        for a, b in pairs:
            ref = halo.get_angular(THETAS, a, b, zw, (0, 2, 4), term=term)
            assert all(s.shape == (2, THETAS.size) and np.array_equal(s, r) for s, r in zip(shared[(a, b)], ref))
            ref = halo.get_angular(THETAS, a, b, per[(a, b)], (0, 4), term=term)
            assert all(s.shape == r.shape and np.array_equal(s, r) for s, r in zip(own[(a, b)], ref)), (term, a, b)
            assert np.array_equal(single[(a, b)], halo.get_angular(THETAS, a, b, zw[0], 2, term=term))
    assert halo.get_angular_all([], THETAS, zw) == {}
    assert halo.get_angular_all(pairs, [], zw)[pairs[0]].shape == (2, 0)


def test_unknown_term_raises(halo):
    with pytest.raises(ValueError):
        halo.get_angular(THETAS, "g", term="3h")
    with pytest.raises(ValueError):
        halo.get_xi_pm(THETAS, zsource=1.2, term="both")
    with pytest.raises(ValueError):
        halo.get_angular_all(PAIRS, THETAS, np.ones(3), term="both")


def test_two_halo_matter_xi_plus_is_positive(halo):
    """Sign and normalisation: xi+ of the two-halo matter term is positive at 1 and 10 arcmin (J0 > 0 where the
    spectrum has its weight) and falls between them."""
    xip, xim = halo.get_xi_pm(THETAS[-2:], zsource=1.2, term="2h")
    print("xi+^2h at 1', 10':", xip, " xi-^2h:", xim)
    assert np.all(xip > 0) and xip[0] > xip[1]
