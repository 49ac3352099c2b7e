"""Host-side checks of the redshift-space correlation multipoles: the numpy restatement of the
by-parts sum the kernel evaluates against 40-digit mpmath of an independent per-panel form, the antiderivatives A_l and
B_l against mpmath quadrature of their defining integrals, a Gaussian against the continuous integral, the argument
checks of xi_multipoles_from_power and the ABI declaration.  The device is checked in tests/test_gpu_xipoles.py."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO
from hmvec_amd import _native as nat
from hmvec_amd import xi_multipoles_from_power, xipoles

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import xipoles_model as xm  # noqa: E402

SEPARATIONS = np.array([1e-3, 0.03, 1.0, 30.0, 300.0])
GRIDS = {"one_panel": np.array([0.5, 1.5]), "log33": np.geomspace(1e-4, 100, 33), "uneven33": xm.uneven_grid(33)}


def rows_of(ks):
    if ks.size == 2:
        return {"positive": np.array([2.0, 0.7]), "sign_changing": np.array([3.0, -1.0])}
    return {"positive": xm.power_like(ks), "sign_changing": xm.sign_changing(ks)}


def separations(ks, ell):
    """The five decades and, for orders 2 and 4, a node of the grid 1e-6 below and above each series switch."""
    if ell == 0:
        return SEPARATIONS
    node = ks[(2 * ks.size) // 3]
    sw = np.concatenate([xm.switch_separations(node, e) for e in (2, 4)])
    for e, (lo, hi) in zip((2, 4), sw.reshape(2, 2)):
        assert node * lo < xm.SERIES_X[e] < node * hi
    return np.concatenate([SEPARATIONS, sw])


# ---------------------------------------------------------------- 1. the restatement against mpmath
@pytest.mark.parametrize("ell", xm.ELLS)
@pytest.mark.parametrize("row", ["positive", "sign_changing"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_by_parts_sum_meets_the_gate_against_mpmath(grid, row, ell):
    ks = GRIDS[grid]
    P = rows_of(ks)[row]
    if row == "sign_changing" and ks.size > 2:
        assert np.sum(np.diff(np.sign(P)) != 0) >= 3
    ss = separations(ks, ell)
    got, ref = xm.xil_numpy(ks, P, ss, ell), xm.xil_mpmath(ks, P, ss, ell)
    err, tol = np.abs(got - ref), xm.gate(ks, P, ss, ell)
    print(f"l = {ell}: err / gate:", err / tol, " |xi| / A:", np.abs(ref) / xm.panel_scale(ks, P, ss))
    assert np.all(err <= tol)


def test_small_separations_leave_no_constant_to_cancel():
    """At k_last s = 0.1 xi_2 is 3e-8 A and xi_4 3e-12 A of a positive row, with the signs i^l; the restatement keeps them
    to 1e-12 of themselves, far below the gate: the antiderivatives vanish at 0."""
    ks = GRIDS["log33"]
    P = xm.power_like(ks)
    s = np.array([1e-3])
    A = xm.panel_scale(ks, P, s)
    for ell, sign in ((2, -1.0), (4, 1.0)):
        got, ref = xm.xil_numpy(ks, P, s, ell), xm.xil_mpmath(ks, P, s, ell)
        print(f"xi_{ell} / A at s = 1e-3:", ref / A, "relative error", np.abs(got - ref) / np.abs(ref))
        assert sign * ref[0] > 0 and np.abs(ref[0]) < 1e-3 * A[0]
        assert np.abs(got - ref)[0] <= 1e-12 * np.abs(ref[0])


# ---------------------------------------------------------------- 2. the antiderivatives
def term_sum(x, ell, which):
    """The sum of the sizes of the terms a closed form adds."""
    si = 1.9          # Si <= 1.852
    if which == "a":
        return 3 + 3 / x if ell == 2 else 8 / 3 + 1 + 10 / x + 35 / x ** 2 + 35 / x ** 3
    return 2 * x + 1 + 3 * si if ell == 2 else 8 * x / 3 + 1 + 7.5 * si + 17.5 / x + 17.5 / x ** 2


def node_tol(x, ell, which, value):
    """Eight roundings of the terms the closed form adds (and the 1e-15 of Si times its factor); below the switch eight
    roundings of twelve times the value (the series loses at most 12, section 24)."""
    if x < xm.SERIES_X[ell]:
        return 8 * 2.0 ** -53 * 12 * abs(value)
    si = 0.0 if which == "a" else (3.0 if ell == 2 else 7.5) * 1e-15
    return 8 * 2.0 ** -53 * term_sum(x, ell, which) + si


@pytest.mark.parametrize("ell", [2, 4])
def test_closed_forms_against_quadrature_of_their_defining_integrals(ell):
    import mpmath as mp
    with mp.workdps(40):
        jl = lambda t: mp.sqrt(mp.pi / (2 * t)) * mp.besselj(ell + mp.mpf(1) / 2, t)      # noqa: E731
        A = lambda u: mp.quad(lambda t: t * jl(t), mp.linspace(0, u, 12))                 # noqa: E731
        for x in (1.0, 3.7, 4.5, 7.0, 25.0):
            a_ref = A(mp.mpf(x))
            b_ref = mp.quad(lambda u: xm.phi_mp(u, ell, 1) if u > 0 else mp.mpf(0), mp.linspace(0, x, 12))
            assert abs(a_ref - xm.phi_mp(mp.mpf(x), ell, 1)) < mp.mpf(10) ** -25         # (the 1F2 form is the integral)
            a, b = float(xm.a_fn(x, ell)), float(xm.b_fn(x, ell))
            print(f"l = {ell}, x = {x}: A {a!r} (err {float(abs(a - a_ref)):.2g}), B {b!r} (err {float(abs(b - b_ref)):.2g})")
            assert abs(a - a_ref) <= node_tol(x, ell, "a", a)
            assert abs(b - b_ref) <= node_tol(x, ell, "b", b)


@pytest.mark.parametrize("ell", [2, 4])
def test_leading_powers(ell):
    """A_l -> x^(l+2)/LEAD_A and B_l -> x^(l+3)/LEAD_B: at x = 1e-2 the ratio is 1 - r_1 to within r_1^2."""
    x = 1e-2
    for fn, lead, p, ratio in ((xm.a_fn, xm.LEAD_A, ell + 2, xm.ratio_a), (xm.b_fn, xm.LEAD_B, ell + 3, xm.ratio_b)):
        r1 = x * x * ratio(ell, 1)
        q = float(fn(x, ell)) / (x ** p / lead[ell])
        assert 0 < 1 - q and abs(q - (1 - r1)) <= r1 * r1 + 4e-16


@pytest.mark.parametrize("ell", [2, 4])
def test_the_two_branches_agree_at_the_switch(ell):
    """A node's value enters two adjacent panels and the telescoping relies on one function of x: either side of the
    switch both branches are within their tolerance of the 40-digit value."""
    import mpmath as mp
    X = xm.SERIES_X[ell]
    with mp.workdps(40):
        for x in (np.nextafter(X, 0.0), X):
            mx = mp.mpf(float(x))
            a_ref = xm.phi_mp(mx, ell, 1)
            b_ref = mx * a_ref - xm.phi_mp(mx, ell, 2)
            a, b = float(xm.a_fn(x, ell)), float(xm.b_fn(x, ell))
            print(f"l = {ell}, x = {x!r}: relative errors", float(abs(a - a_ref) / a_ref), float(abs(b - b_ref) / b_ref))
            assert abs(a - a_ref) <= node_tol(x, ell, "a", a) and abs(b - b_ref) <= node_tol(x, ell, "b", b)


# ---------------------------------------------------------------- 3. a Gaussian
def test_gaussian_against_the_continuous_integral():
    """P_l = exp(-k^2/2): xi_l against mpmath quadrature of i^l/(2 pi^2) int_0^inf k^2 P j_l(k s) dk.  The tolerance is
    section 13's derived sum with |j_l| <= 1: linear interpolation of f = k P is off by at most h^2/8 max|f''| on a panel
    and enters times k, so the integral by (1/(2 pi^2)) sum_i h_i^3/8 k_{i+1} max_panel|f''|; the omitted head [0, k_0]
    holds at most k_0^3/(6 pi^2) (P <= 1); the tail at most int_{k_max}^inf k^2 P dk / (2 pi^2)."""
    import mpmath as mp
    ks = np.linspace(0.01, 12, 1200)
    P = np.exp(-0.5 * ks ** 2)
    ss = np.array([0.5, 1.0, 2.0])
    f2 = np.abs((ks ** 3 - 3 * ks) * np.exp(-0.5 * ks ** 2))          # |f''|, f = k exp(-k^2/2)
    h = np.diff(ks)
    f2_panel = np.maximum(f2[1:], f2[:-1]) + 1.5 * h                  # (|f'''| <= 3, as in tests/test_realspace_cpu.py)
    interp = np.sum(h ** 3 / 8 * ks[1:] * f2_panel) / (2 * np.pi ** 2)
    head = ks[0] ** 3 / (6 * np.pi ** 2)
    K = ks[-1]
    tail = (K * math.exp(-0.5 * K * K) + math.sqrt(np.pi / 2) * math.erfc(K / math.sqrt(2))) / (2 * np.pi ** 2)
    tol = interp + head + tail
    xi0 = np.exp(-0.5 * ss ** 2) / (2 * np.pi) ** 1.5
    assert np.all(tol < 1e-3 * xi0)                                   # the bound is far below the monopole's size
    with mp.workdps(30):
        for ell in xm.ELLS:
            jl = lambda t: mp.sqrt(mp.pi / (2 * t)) * mp.besselj(ell + mp.mpf(1) / 2, t)      # noqa: E731
            ref = np.array([float(xm.SIGN[ell] / (2 * mp.pi ** 2) * mp.quad(
                lambda k: k * k * mp.exp(-k * k / 2) * jl(k * mp.mpf(float(s))), mp.linspace(0, 14, 29))) for s in ss])
            got = xm.xil_numpy(ks, P, ss, ell)
            print(f"l = {ell}: xi", ref, "err", np.abs(got - ref), "tol", tol)
            if ell == 0:
                assert np.all(np.abs(ref - xi0) <= 1e-12 * xi0)
            assert np.all(np.abs(got - ref) <= tol + (1e-20 if ell else 0.0))


# ---------------------------------------------------------------- 4. the free function's refusals
class NoLaunch:
    """A context that fails the test on any use: the argument checks come before every upload and launch."""

    def __getattr__(self, name):
        raise AssertionError(f"context used ({name}) before the arguments were checked")


KS = np.geomspace(1e-3, 10, 16)
GOOD = np.stack([xm.power_like(KS), -0.4 * xm.power_like(KS), 0.1 * xm.power_like(KS)])


@pytest.mark.parametrize("ks,P,ss,ells", [
    (KS[::-1], GOOD, [1.0], (0, 2, 4)),                               # decreasing
    (np.r_[0.0, KS[1:]], GOOD, [1.0], (0, 2, 4)),                     # k = 0
    (np.r_[KS[:-1], np.inf], GOOD, [1.0], (0, 2, 4)),                 # non-finite
    (KS[:1], GOOD[:, :1], [1.0], (0, 2, 4)),                          # nk < 2
    (KS, np.where(np.arange(16) == 3, np.nan, GOOD), [1.0], (0, 2, 4)),   # non-finite P
    (KS, GOOD[:, :-1], [1.0], (0, 2, 4)),                             # wrong length
    (KS, GOOD[0], [1.0], (0,)),                                       # no leading axis of orders
    (KS, GOOD[:2], [1.0], (0, 2, 4)),                                 # two rows for three orders
    (KS, GOOD, [1.0], (0, 2)),                                        # three rows for two orders
    (KS, np.ones((3, 2, 2, 2, 16)), [1.0], (0, 2, 4)),                # too many axes
    (KS, GOOD, [1.0, 0.0], (0, 2, 4)),                                # s = 0
    (KS, GOOD, [-2.0], (0, 2, 4)),                                    # negative s
    (KS, GOOD, [np.nan], (0, 2, 4)),                                  # non-finite s
    (KS, GOOD, [[1.0, 2.0]], (0, 2, 4)),                              # separations not a vector
    (KS, GOOD, [1.0], (0, 1, 4)),                                     # an odd order
    (KS, GOOD, [1.0], (0, 2, 6)),                                     # l > 4
    (KS, GOOD[:0], [1.0], ()),                                        # no order at all
])
def test_bad_arguments_raise_before_any_launch(ks, P, ss, ells):
    with pytest.raises(ValueError):
        xi_multipoles_from_power(ks, P, ss, ells, ctx=NoLaunch())


def test_a_resident_block_of_the_wrong_shape_raises_before_any_launch():
    for shape in ((3, KS.size + 1), (2, 5, KS.size), (KS.size,)):
        with pytest.raises(ValueError):
            xi_multipoles_from_power(KS, nat.DeviceArray(None, 0, shape, owner=False), [1.0], ctx=NoLaunch())


@pytest.mark.parametrize("shape", [(3, KS.size), (3, 4, KS.size), (3, 2, 4, KS.size)])
def test_empty_separations_return_an_empty_array_without_a_launch(shape):
    out = xi_multipoles_from_power(KS, np.ones(shape), [], ctx=NoLaunch())
    assert out.shape == shape[:-1] + (0,) and out.dtype == np.float64
    assert xi_multipoles_from_power(KS, np.ones(shape)[:1], [], (4,), ctx=NoLaunch()).shape == (1,) + shape[1:-1] + (0,)


def test_the_facade_refuses_before_any_launch():
    from hmvec_amd.halomodel import HaloModel
    h = HaloModel.__new__(HaloModel)          # no constructor: nothing may be touched but the request
    h.ks = KS
    for kw in (dict(ss=[0.0]), dict(ss=[np.nan]), dict(ss=[1.0], ells=(1,)), dict(ss=[1.0], term="both"),
               dict(ss=[1.0], kindex=[0, 1])):
        with pytest.raises(ValueError):
            xipoles.get_xi_multipoles(h, name="nfw", **kw)
    with pytest.raises(ValueError):
        xipoles.xi_multipoles_device(h, [], "nfw")
    assert not hasattr(HaloModel, "get_xi_multipoles")          # (functions of the model: the class's surface is as it was)


def test_abi_declares_the_entry_point():
    assert nat.SIGNATURES["hmg_xi_multipoles"] == [nat._P, nat._I, nat._I, nat._I] + [nat._P] * 4 + [
        nat.C.c_longlong] * 2 + [nat._P] * 4
    assert nat.PARAMS["hmg_xi_multipoles"] == ("ctx", "rows", "nk", "ns", "d_ks", "d_P0", "d_P2", "d_P4", "row_stride",
                                               "node_stride", "d_ss", "d_xi0", "d_xi2", "d_xi4")
    with open(os.path.join(REPO, "include", "hmgrid.h")) as f:
        header = f.read()
    assert "int hmg_xi_multipoles(" in header
    assert "#define HMG_ABI_VERSION 10" in header and nat.ABI_VERSION == 10
    assert xipoles.xi_multipoles_from_power is xi_multipoles_from_power
    import hmvec_amd
    assert hmvec_amd.get_xi_multipoles is xipoles.get_xi_multipoles
    assert hmvec_amd.xi_multipoles_device is xipoles.xi_multipoles_device


def test_library_exports_the_entry_point():
    assert hasattr(nat.load(), "hmg_xi_multipoles")
