"""GPU checks of the redshift-space correlation multipoles (hmvec_amd.xi_multipoles_from_power, hmg_xi_multipoles;
xi_multipoles_device and get_xi_multipoles of a HaloModel; definition and gates in DESIGN.md section 24).  The reference
computes none of these statistics, so there is no reference fixture: the device is pinned by 40-digit mpmath of an
independent per-panel form, at sizes where mpmath is slow by the numpy restatement that tests/test_xipoles_cpu.py pins
against mpmath, and by bit-identities - among them that xi_0 is hmg_xi_transform's bits.

Measured on an MI355X (worst |got - ref| / gate, orders 0, 2, 4): against mpmath 1.3e-3, 2.0e-3, 4.0e-3; the batches
against the numpy restatement 4.2e-4, 1.6e-4, 9.4e-5."""
import itertools
import os
import sys

import numpy as np
import pytest

from hmvec_amd import _native as nat
from hmvec_amd import get_xi_multipoles, xi_from_power, xi_multipoles_device, xi_multipoles_from_power

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import xipoles_model as xm  # noqa: E402
from lensing_model import model  # noqa: E402

pytestmark = pytest.mark.gpu

ELLS = (0, 2, 4)
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(ELLS, n)]


def within_gate(got, ref, tol, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"{what}: worst |xi - ref| / gate = {worst:.3g}")
    return np.all(err <= tol), worst


# ---------------------------------------------------------------- 1. device vs 40-digit mpmath
def separations(ks):
    """25 separations from 1e-3 to 300 and a node of the grid 1e-6 below and above each series switch."""
    node = ks[(2 * ks.size) // 3]
    sw = np.concatenate([xm.switch_separations(node, e) for e in (2, 4)])
    for e, (lo, hi) in zip((2, 4), sw.reshape(2, 2)):
        assert node * lo < xm.SERIES_X[e] < node * hi
    return np.concatenate([np.geomspace(1e-3, 300, 25), sw])


@pytest.mark.parametrize("grid", ["one_panel", "log33"])
def test_against_mpmath(grid):
    if grid == "one_panel":
        ks = np.array([0.5, 1.5])
        rows = np.array([[2.0, 0.7], [3.0, -1.0]])
    else:
        ks = np.geomspace(1e-4, 100, 33)
        rows = np.stack([xm.power_like(ks), xm.sign_changing(ks)])
    ss = separations(ks)
    P = np.stack([rows, -0.4 * rows[::-1], 0.1 * rows])            # a block of its own per order
    got = xi_multipoles_from_power(ks, P, ss)
    assert got.shape == (3, 2, ss.size)
    for i, ell in enumerate(ELLS):
        for r in range(2):
            ref = xm.xil_mpmath(ks, P[i, r], ss, ell)
            ok, worst = within_gate(got[i, r], ref, xm.gate(ks, P[i, r], ss, ell), f"{grid} row {r} l = {ell}")
            assert ok, (ell, r, worst)


def test_small_separations_leave_no_constant_to_cancel():
    """At k_last s = 0.1 xi_2 = -3e-8 A and xi_4 = 3e-12 A of a positive row (tests/test_xipoles_cpu.py): the device
    keeps them to 1e-12 of themselves."""
    ks = np.geomspace(1e-4, 100, 33)
    P = np.stack([xm.power_like(ks)] * 3)
    got = xi_multipoles_from_power(ks, P, [1e-3])
    for i, ell in ((1, 2), (2, 4)):
        ref = xm.xil_mpmath(ks, P[i], [1e-3], ell)
        print(f"xi_{ell}(1e-3) = {got[i, 0]!r}, relative error {abs(got[i, 0] - ref[0]) / abs(ref[0]):.3g}")
        assert xm.SIGN[ell] * got[i, 0] > 0 and abs(got[i, 0] - ref[0]) <= 1e-12 * abs(ref[0])


# ---------------------------------------------------------------- 2. device vs the numpy restatement
# nk = 258: 257 panels, one more than the workgroup has threads; nk = 1030 on an uneven grid: runs of five panels, the
# last owner's shorter.  Five rows with a row of zeros and sign-changing rows; 70 separations: 17 tiles of four and a
# tile of two.
S70 = np.geomspace(1e-3, 300, 70)


def five_rows(ks):
    base = xm.power_like(ks)
    return np.stack([base, np.zeros_like(ks), xm.sign_changing(ks), -base * ks ** 0.3,
                     base * (1 + 0.3 * np.sin(7 * np.log(ks)))])


def block(ks):
    rows = five_rows(ks)
    return np.stack([rows, -0.4 * rows[[2, 1, 0, 4, 3]], 0.1 * rows[[4, 1, 3, 2, 0]]])


@pytest.fixture(scope="module")
def batch258():
    ks = np.geomspace(1e-4, 100, 258)
    P = block(ks)
    return ks, P, xi_multipoles_from_power(ks, P, S70)


@pytest.fixture(scope="module")
def batch1030():
    ks = xm.uneven_grid(1030)
    P = block(ks)
    return ks, P, xi_multipoles_from_power(ks, P, S70)


@pytest.mark.parametrize("which", ["batch258", "batch1030"])
def test_batch_against_the_numpy_restatement(which, request):
    ks, P, got = request.getfixturevalue(which)
    assert got.shape == (3, 5, 70) and np.sum(np.diff(np.sign(P[0, 2])) != 0) >= 3
    assert np.all(got[:, 1] == 0.0)                      # the row of zeros: exactly zero in every order
    for i, ell in enumerate(ELLS):
        ok, worst = within_gate(got[i], xm.xil_numpy(ks, P[i], S70, ell), xm.gate(ks, P[i], S70, ell), f"{which} l = {ell}")
        assert ok, (ell, worst)


# ---------------------------------------------------------------- 3. determinism and independence
def test_repeat_is_bit_identical(batch258):
    ks, P, got = batch258
    assert np.array_equal(xi_multipoles_from_power(ks, P, S70), got)


def test_a_row_does_not_depend_on_the_batch(batch258, batch1030):
    for ks, P, got in (batch258, batch1030):
        alone = xi_multipoles_from_power(ks, P[:, 3], S70)
        assert alone.shape == (3, 70) and np.array_equal(alone, got[:, 3])
        nested = xi_multipoles_from_power(ks, P[:, 1:5].reshape(3, 2, 2, -1), S70)
        assert nested.shape == (3, 2, 2, 70) and np.array_equal(nested.reshape(3, 4, 70), got[:, 1:5])


def test_a_separation_does_not_depend_on_the_others(batch258, batch1030):
    for ks, P, got in (batch258, batch1030):
        for j in (0, 38, 69):
            alone = xi_multipoles_from_power(ks, P, S70[j:j + 1])
            assert alone.shape == (3, 5, 1) and np.array_equal(alone[..., 0], got[..., j]), j


def test_every_subset_of_orders_equals_the_all_orders_launch(batch258, batch1030):
    for ks, P, got in (batch258, batch1030):
        for sub in SUBSETS:
            idx = [ELLS.index(e) for e in sub]
            out = xi_multipoles_from_power(ks, P[idx], S70, sub)
            assert out.shape == (len(sub), 5, 70) and np.array_equal(out, got[idx]), sub
        swapped = xi_multipoles_from_power(ks, P[[2, 0]], S70, (4, 0))              # the order of ells is the caller's
        assert np.array_equal(swapped, got[[2, 0]])


def test_strided_rows_equal_contiguous_rows(batch258, batch1030):
    """The (rows, nk, 3) layout of multipoles_device, read in place with node_stride = 3."""
    ctx = nat.default_context(0)
    for ks, P, got in (batch258, batch1030):
        nk = ks.size
        d_ks, d_ss = ctx.upload(ks), ctx.upload(S70)
        d_P = ctx.upload(np.ascontiguousarray(np.moveaxis(P, 0, -1)))              # (5, nk, 3)
        for sub in ((0, 2, 4), (2,), (0, 4)):
            out = ctx.empty((3, 5, 70))
            ctx.call("hmg_xi_multipoles", 5, nk, 70, d_ks.ptr,
                     *(d_P.ptr + 8 * i if e in sub else None for i, e in enumerate(ELLS)), 3 * nk, 3, d_ss.ptr,
                     *(out.ptr + 8 * i * 5 * 70 if e in sub else None for i, e in enumerate(ELLS)))
            res = out.numpy()
            for i, e in enumerate(ELLS):
                if e in sub:
                    assert np.array_equal(res[i], got[i]), (sub, e)


def test_device_input_equals_host_input(batch258):
    ks, P, got = batch258
    ctx = nat.default_context(0)
    assert np.array_equal(xi_multipoles_from_power(ks, ctx.upload(P), S70), got)
    assert np.array_equal(xi_multipoles_from_power(ks, ctx.upload(P[1:2, 0]), S70, (2,), ctx=ctx), got[1:2, 0])


def test_the_monopole_is_the_correlation_function_transform(batch258, batch1030):
    for ks, P, got in (batch258, batch1030):
        assert np.array_equal(got[0], xi_from_power(ks, P[0], S70))
        assert np.array_equal(xi_multipoles_from_power(ks, P[:1, 2], S70[5:6], (0,))[0], xi_from_power(ks, P[0, 2], S70[5:6]))


def test_entry_point_errors(batch258):
    ks, P, _ = batch258
    ctx = nat.default_context(0)
    d_ks, d_ss, d_P, out = ctx.upload(ks), ctx.upload(S70), ctx.upload(P[0]), ctx.empty((5, 70))
    nk = ks.size
    good = dict(rows=5, nk=nk, ns=70, d_ks=d_ks.ptr, d_P0=d_P.ptr, d_P2=None, d_P4=None, row_stride=nk, node_stride=1,
                d_ss=d_ss.ptr, d_xi0=out.ptr, d_xi2=None, d_xi4=None)
    ctx.call("hmg_xi_multipoles", **good)
    for bad in (dict(d_xi0=None), dict(d_xi2=out.ptr), dict(d_P0=None), dict(nk=1), dict(rows=0), dict(ns=0),
                dict(node_stride=0), dict(row_stride=nk - 1), dict(node_stride=3), dict(d_ks=None)):
        with pytest.raises(nat.NativeError):
            ctx.call("hmg_xi_multipoles", **{**good, **bad})


# ---------------------------------------------------------------- 4. the facade
NM, NK = 37, 48
ZS = np.array([0.2, 0.8, 1.4])
SS = np.array([0.3, 2.0, 9.0, 30.0, 110.0])


@pytest.fixture(scope="module")
def h():
    m = model(ZS, ks=np.geomspace(1e-3, 30, NK), ms=np.geomspace(1e11, 10 ** 15.5, NM))     # tests/test_gpu_rsd.py's
    m.add_battaglia_pres_profile("y", family="pres", xmax=5, nxs=512)
    m.add_hod("g", mthresh=10 ** 10.5 + ZS * 0.0)
    return m


def test_the_monopole_is_xi_from_power_of_the_multipole_spectrum(h):
    for term in ("1h", "2h"):
        P0 = h.get_power_multipoles("g", "nfw", ells=(0,), term=term)[0]
        got = get_xi_multipoles(h, SS, "g", "nfw", ells=(0,), term=term)
        assert got.shape == (1, 3, SS.size) and np.array_equal(got[0], xi_from_power(h.ks, P0, SS)), term


def test_all_orders_are_the_transform_of_get_power_multipoles(h):
    """"1h" and "2h": within the gate evaluated on the rows (and, the rows being the same numbers strided and contiguous,
    bit for bit).  "total" is the sum of the two transforms against the transform of the summed rows: each of the three
    transforms is within its own gate of the exact value of its rows, and the sum adds one rounding."""
    dev = xi_multipoles_device(h, SS, "g").numpy()
    assert dev.shape == (2, 3, 3, SS.size)
    parts = {}
    for t, term in enumerate(("1h", "2h", "total")):
        Pl = parts[term] = h.get_power_multipoles("g", term=term)
        got = get_xi_multipoles(h, SS, "g", term=term)
        ref = xi_multipoles_from_power(h.ks, Pl, SS)
        assert got.shape == ref.shape == (3, 3, SS.size)
        if term != "total":
            assert np.array_equal(got, dev[t]) and np.array_equal(got, ref)      # the same rows, strided and contiguous
        else:
            assert np.array_equal(got, dev[0] + dev[1])
        for i, ell in enumerate(ELLS):
            tol = xm.gate(h.ks, Pl[i], SS, ell)
            if term == "total":
                tol = tol + sum(xm.gate(h.ks, parts[p][i], SS, ell) for p in ("1h", "2h")) + 2.0 ** -53 * np.abs(got[i])
            ok, worst = within_gate(got[i], ref[i], tol, f"{term} l = {ell}")
            assert ok, (term, ell, worst)
    sub = get_xi_multipoles(h, SS[1:4], "g", ells=(4, 0), term="2h")
    assert np.array_equal(sub, dev[1][[2, 0]][..., 1:4])
    assert get_xi_multipoles(h, [], "g", ells=(2,)).shape == (1, 3, 0)
    assert get_xi_multipoles(h, 5.0, "g", ells=(2,)).shape == (1, 3, 1)


def test_without_velocities_the_monopole_is_get_xi(h):
    """f = 0 and sigma_s = 0: P_0 is P.  The two sides transform rows that differ by rounding, so the bound is the
    transform's own linearity - A(s) of |P_0 - P| - plus both gates."""
    zero = np.zeros((3, NM))
    kw = dict(sigma_s=zero, f=np.zeros(3))
    for term in ("1h", "2h", "total"):
        P0 = h.get_power_multipoles("nfw", "nfw", ells=(0,), term=term, **kw)[0]
        P = {"1h": h.get_power_1halo, "2h": h.get_power_2halo, "total": h.get_power}[term]("nfw", "nfw")
        got = get_xi_multipoles(h, SS, "nfw", "nfw", ells=(0,), term=term, **kw)[0]
        ref = h.get_xi(SS, "nfw", "nfw", term=term)
        tol = xm.panel_scale(h.ks, np.abs(P0 - P), SS) + xm.gate(h.ks, P0, SS, 0) + xm.gate(h.ks, P, SS, 0)
        ok, worst = within_gate(got, ref, tol, f"{term} against get_xi")
        print("  largest |P_0 - P| / |P|:", float(np.max(np.abs(P0 - P) / np.abs(P))))
        assert ok, (term, worst)
        assert np.all(tol <= 1e-6 * xm.panel_scale(h.ks, P, SS))           # (a bound that means something)


def test_refusals_come_before_any_launch(h, monkeypatch):
    call = nat.Context.call

    def no_launch(self, name, *a, **k):
        assert name not in ("hmg_rsd_multipoles", "hmg_xi_multipoles"), f"{name} launched before the request was checked"
        return call(self, name, *a, **k)
    monkeypatch.setattr(nat.Context, "call", no_launch)
    for args, kw in (((SS, "y"), {}), ((SS, "g", "y"), {}), ((SS, "g"), dict(kindex=np.arange(5))),
                     ((SS, "g"), dict(ells=(3,))), ((SS, "g"), dict(term="3h")), (([0.0], "g"), {}),
                     ((SS, "g"), dict(nmu=0)), (([], "y"), {})):
        with pytest.raises(ValueError):
            get_xi_multipoles(h, *args, **kw)


def test_the_kaiser_quadrupole_is_negative(h):
    """The two-halo xi_2 of matter with f > 0 at s = 30 Mpc: P_2 > 0 on large scales and i^2 = -1."""
    f = h.get_growth_rate_f(h.zs)
    assert np.all(f > 0)
    xi = get_xi_multipoles(h, [30.0], "nfw", ells=(0, 2), term="2h")
    print("xi_0^2h, xi_2^2h of matter at s = 30:", xi[0, :, 0], xi[1, :, 0])
    assert np.all(xi[1] < 0)
