"""GPU checks of the Hankel transforms of orders 0 and 2 (hmvec_amd.realspace.projected_from_power; HaloModel.get_wp,
get_surface_density, get_excess_surface_density and their _all forms; definition and gate in DESIGN.md section 14).  The
reference computes none of these statistics, so there is no reference fixture: the device is pinned by 40-digit mpmath of
an independent form of the same integrals, and at sizes where mpmath is slow by the numpy restatement that
tests/test_projected_cpu.py pins against mpmath.

Measured on an MI355X (worst |got - ref| / gate): one panel 1.4e-2, 33 points 8.3e-3, the batches against the numpy
restatement 5.5e-3 (nk = 258) and 5.6e-3 (nk = 1030); W_2 alone stays below 7.7e-3, 2.9e-4 and 1.2e-4."""
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import projected_from_power

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import projected_model as pm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

RADII = np.geomspace(1e-3, 300, 25)


def within_gate(got, ref, ks, P, rs, what):
    err, tol = np.abs(got - ref), pm.gate(ks, P, rs)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what}: worst |W - ref| / gate = {worst:.3g}")
    return np.all(err <= tol), worst


def both_and_single(ks, P, rs):
    """(W_0, W_2) of the both-outputs launch, after checking that the single-output launches give the same bits."""
    w0, w2 = projected_from_power(ks, P, rs, (0, 2))
    assert np.array_equal(projected_from_power(ks, P, rs, 0), w0)
    assert np.array_equal(projected_from_power(ks, P, rs, 2), w2)
    return w0, w2


# ---------------------------------------------------------------- 1. device vs 40-digit mpmath
@pytest.mark.parametrize("P2", [[2.0, 0.7], [3.0, -1.0]])
def test_one_panel_against_mpmath(P2):
    ks, P = np.array([0.5, 1.5]), np.array(P2)
    rs = np.concatenate([RADII, pm.switch_radii(ks[1])])
    x = rs[-2:] * ks[1]
    assert x[0] < pm.SERIES_X < x[1]
    got = both_and_single(ks, P, rs)
    for order, w in zip((0, 2), got):
        assert w.shape == (rs.size,)
        ok, worst = within_gate(w, pm.hankel_mpmath(ks, P, rs, order), ks, P, rs, f"order {order}")
        assert ok, (order, worst)


@pytest.mark.parametrize("grid", ["log", "uneven"])
def test_33_points_against_mpmath(grid):
    ks = np.geomspace(1e-4, 100, 33) if grid == "log" else pm.uneven_grid(33)
    rs = np.concatenate([RADII, pm.switch_radii(ks[20])])
    x = rs[-2:] * ks[20]
    assert x[0] < pm.SERIES_X < x[1]
    P = np.stack([pm.power_like(ks), pm.sign_changing(ks)])
    got = both_and_single(ks, P, rs)
    for order, w in zip((0, 2), got):
        assert w.shape == (2, rs.size)
        for row in range(2):
            ok, worst = within_gate(w[row], pm.hankel_mpmath(ks, P[row], rs, order), ks, P[row], rs,
                                    f"order {order} row {row}")
            assert ok, (order, row, worst)


# ---------------------------------------------------------------- 2. device vs the numpy restatement
# nk = 258: 257 panels, one more than the workgroup has threads, so a thread owns two panels, the 129th owner one and the
# rest none; nk = 1030 on an uneven grid: runs of five panels, the last owner's shorter.  70 radii: seventeen tiles of four
# and a tile of two.
RS70 = np.geomspace(1e-3, 300, 70)


def batch(ks):
    base = pm.power_like(ks)
    return np.stack([base, pm.sign_changing(ks), np.zeros_like(ks), base * (1 + 0.3 * np.sin(7 * np.log(ks))),
                     -base * ks ** 0.3])


@pytest.fixture(scope="module")
def batch258():
    ks = np.geomspace(1e-4, 100, 258)
    P = batch(ks)
    return ks, P, projected_from_power(ks, P, RS70, (0, 2))


@pytest.fixture(scope="module")
def batch1030():
    ks = pm.uneven_grid(1030)
    P = batch(ks)
    return ks, P, projected_from_power(ks, P, RS70, (0, 2))


@pytest.mark.parametrize("which", ["batch258", "batch1030"])
def test_batch_against_the_numpy_restatement(which, request):
    ks, P, got = request.getfixturevalue(which)
    assert np.sum(np.diff(np.sign(P[1])) != 0) >= 3
    for order, w in zip((0, 2), got):
        assert w.shape == (5, 70)
        assert np.all(w[2] == 0.0)                       # a row of zeros: exactly zero
        ok, worst = within_gate(w, pm.hankel_numpy(ks, P, RS70, order), ks, P, RS70, f"{which} order {order}")
        assert ok, (order, worst)


# ---------------------------------------------------------------- 3. determinism and independence
def test_repeat_is_bit_identical(batch258):
    ks, P, (w0, w2) = batch258
    r0, r2 = projected_from_power(ks, P, RS70, (0, 2))
    assert np.array_equal(r0, w0) and np.array_equal(r2, w2)


def test_each_output_alone_equals_the_both_outputs_launch(batch258, batch1030):
    for ks, P, (w0, w2) in (batch258, batch1030):
        assert np.array_equal(projected_from_power(ks, P, RS70, 0), w0)
        assert np.array_equal(projected_from_power(ks, P, RS70, 2), w2)
        assert np.array_equal(projected_from_power(ks, P, RS70), w0)          # order 0 is the default


def test_a_row_does_not_depend_on_the_batch(batch258):
    ks, P, (w0, w2) = batch258
    a0, a2 = projected_from_power(ks, P[3], RS70, (0, 2))
    assert a0.shape == (70,) and np.array_equal(a0, w0[3]) and np.array_equal(a2, w2[3])


def test_a_radius_does_not_depend_on_the_others(batch258):
    ks, P, (w0, w2) = batch258
    a0, a2 = projected_from_power(ks, P, RS70[41:42], (0, 2))
    assert a0.shape == (5, 1) and np.array_equal(a0[:, 0], w0[:, 41]) and np.array_equal(a2[:, 0], w2[:, 41])


def test_device_input_equals_host_input(batch258):
    ks, P, (w0, w2) = batch258
    ctx = nat.default_context(0)
    d_P = ctx.upload(P)
    a0, a2 = projected_from_power(ks, d_P, RS70, (0, 2))
    assert np.array_equal(a0, w0) and np.array_equal(a2, w2)
    d_P3 = ctx.upload(P.reshape(1, 5, -1))
    assert np.array_equal(projected_from_power(ks, d_P3, RS70, 2, ctx=ctx), w2.reshape(1, 5, 70))


# ---------------------------------------------------------------- 4. the facade
ZS = np.array([0.3, 1.0])
RS = np.concatenate([np.geomspace(0.05, 150, 9), [1.0, 10.0]])
PAIRS = [("g", "g"), ("g", "nfw"), ("nfw", "nfw")]
FALLBACK_PAIRS = [("g", "g2"), ("g", "nfw")]            # two different HODs: not a request of the batched mass integrals


@pytest.fixture(scope="module")
def halo():
    h = model(ZS)
    h.add_hod("g", mthresh=10 ** 10.5 + ZS * 0.0)
    h.add_hod("g2", mthresh=10 ** 11.5 + ZS * 0.0)
    return h


def test_get_wp_is_the_transform_of_get_power(halo):
    got = halo.get_wp(RS, "g")
    assert got.shape == (ZS.size, RS.size)
    assert np.array_equal(got, projected_from_power(halo.ks, halo.get_power("g"), RS))
    assert np.array_equal(halo.get_wp(RS, "g", "nfw"), projected_from_power(halo.ks, halo.get_power("g", "nfw"), RS, 0))
    assert halo.get_wp([], "g").shape == (ZS.size, 0)
    assert halo.get_wp(7.0, "g").shape == (ZS.size, 1)


def test_surface_densities_are_rho_m0_times_the_transforms(halo):
    rho = halo._rho_m0()
    assert rho == float(halo.rho_matter_z(0)[0]) and rho > 0
    w0, w2 = projected_from_power(halo.ks, halo.get_power("g", "nfw"), RS, (0, 2))
    sig, dsig = halo.get_surface_density(RS, "g", "nfw"), halo.get_excess_surface_density(RS, "g", "nfw")
    assert sig.shape == dsig.shape == (ZS.size, RS.size)
    assert np.array_equal(sig, rho * w0) and np.array_equal(dsig, rho * w2)
    assert halo.get_surface_density([], "g", "nfw").shape == (ZS.size, 0)
    assert halo.get_excess_surface_density([], "g", "nfw").shape == (ZS.size, 0)


def test_terms_are_the_transforms_of_the_terms(halo):
    rho = halo._rho_m0()
    for term, P in (("1h", halo.get_power_1halo("g", "nfw")), ("2h", halo.get_power_2halo("g", "nfw"))):
        w0, w2 = projected_from_power(halo.ks, P, RS, (0, 2))
        assert np.array_equal(halo.get_wp(RS, "g", "nfw", term=term), w0)
        assert np.array_equal(halo.get_surface_density(RS, "g", "nfw", term=term), rho * w0)
        assert np.array_equal(halo.get_excess_surface_density(RS, "g", "nfw", term=term), rho * w2)


@pytest.mark.parametrize("pairs", [PAIRS, FALLBACK_PAIRS], ids=["batched", "fallback"])
def test_all_entries_equal_the_single_pair_calls(halo, pairs):
    from hmvec_amd import spectra
    rpairs = halo._resolve_pairs(pairs)
    assert spectra.batchable(spectra.pair_plan(rpairs)[0], rpairs) == (pairs is PAIRS)
    for term in ("total", "1h", "2h"):
        wp = halo.get_wp_all(pairs, RS, term=term)
        sd = halo.get_surface_density_all(pairs, RS, term=term)
        assert list(wp) == pairs and list(sd) == pairs
        for a, b in pairs:
            assert wp[(a, b)].shape == (ZS.size, RS.size)
            assert np.array_equal(wp[(a, b)], halo.get_wp(RS, a, b, term=term)), (term, a, b)
            sig, dsig = sd[(a, b)]
            assert np.array_equal(sig, halo.get_surface_density(RS, a, b, term=term)), (term, a, b)
            assert np.array_equal(dsig, halo.get_excess_surface_density(RS, a, b, term=term)), (term, a, b)
    assert halo.get_wp_all([], RS) == {} and halo.get_surface_density_all([], RS) == {}
    assert halo.get_wp_all(pairs, [])[pairs[0]].shape == (ZS.size, 0)
    assert [s.shape for s in halo.get_surface_density_all(pairs, [])[pairs[0]]] == [(ZS.size, 0)] * 2


def test_unknown_term_raises(halo):
    with pytest.raises(ValueError):
        halo.get_wp(RS, "g", term="3h")
    with pytest.raises(ValueError):
        halo.get_surface_density_all(PAIRS, RS, term="both")


def test_two_halo_matter_delta_sigma_is_positive(halo):
    """Sign and normalisation: the two-halo Sigma and Delta Sigma of matter are positive at R = 1 and 10 Mpc (the mean
    surface density inside R exceeds the one at R where xi_mm falls with r), and Sigma falls from 1 to 10 Mpc."""
    sig = halo.get_surface_density(RS[-2:], "nfw", term="2h")
    dsig = halo.get_excess_surface_density(RS[-2:], "nfw", term="2h")
    print("Sigma_mm^2h at R = 1, 10:", sig, " Delta Sigma_mm^2h:", dsig)
    assert np.all(sig > 0) and np.all(dsig > 0)
    assert np.all(sig[:, 0] > sig[:, 1])


def test_w2_is_far_below_w0_at_small_radii(halo):
    """With x = k_last R << 1: 0 <= J2(k R) <= x^2/8 and J0(k R) >= 1 - x^2/4 on the whole grid, so for the positive
    two-halo matter spectrum 0 < W_2 <= (x^2/8)/(1 - x^2/4) W_0, up to the gate."""
    R = np.array([1e-5, 1e-4])
    x = halo.ks[-1] * R
    P = halo.get_power_2halo("nfw")
    assert np.all(P > 0) and np.all(x <= 0.0100001)
    w0, w2 = halo.get_wp(R, "nfw", term="2h"), halo.get_excess_surface_density(R, "nfw", term="2h") / halo._rho_m0()
    print("W_2 / W_0 at k_last R = 1e-3, 1e-2:", w2 / w0)
    assert np.all(w2 > 0)
    assert np.all(w2 <= (x ** 2 / 8) / (1 - x ** 2 / 4) * w0 + pm.gate(halo.ks, P, R))
    assert np.all(w2 < 2e-5 * w0)
