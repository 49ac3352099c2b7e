"""CPU checks of the gate that tests/test_gpu_nfw_bands.py holds the analytic NFW kernel to (helpers/nfw_model.py):
everything about it except the comparison with the device.  The standard is the closed form at 40 digits; the unit of
the gate, B (S in the closed band), comes from that standard alone; the gate constants K come from a plain-double
restatement of the kernel's nine forms, which this file holds to K / 4.  The float64 oracle (oracle/hmref.py) is NOT the
standard here: its own form cancels, and the last test records by how much."""
import math
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import nfw_model as nm  # noqa: E402


@pytest.fixture(scope="module")
def tab():
    return nm.table()


def test_every_point_has_exactly_one_band(tab):
    """The ladder of band() restated as nine independent conditions: each point meets exactly one, the one band() names,
    bands() agrees, and every band - the three collapsed ones too - holds at least 30 points."""
    c, x = tab.c, tab.x
    xc = (1.0 + c) * x
    ser = c >= 0.5
    col = (x > 4.0) & (xc < 1e9) & ~(ser & (xc <= 10.0))
    cond = {"s5": ser & (xc <= 0.1), "s8": ser & (xc > 0.1) & (xc <= 0.8), "s16": ser & (xc > 0.8) & (xc <= 4.0),
            "s32": ser & (xc > 4.0) & (xc <= 10.0),
            "col<8": col & (xc < 8.0), "col<64": col & (xc >= 8.0) & (xc < 64.0), "col≥64": col & (xc >= 64.0),
            "mixed": ser & (x <= 4.0) & (xc > 10.0),
            "closed": (~ser & (x <= 4.0)) | (xc >= 1e9)}
    member = np.array([cond[b] for b in nm.BANDS])
    assert np.all(member.sum(axis=0) == 1)
    assert np.array_equal(np.array(nm.BANDS)[member.argmax(axis=0)], tab.band)
    assert np.array_equal(np.array(nm.BANDS)[nm.bands(c, x)], tab.band)
    counts = {b: int(member[i].sum()) for i, b in enumerate(nm.BANDS)}
    print(counts)
    assert min(counts.values()) >= 30, counts
    # what the names promise about sici_aux's branches: x <= xc, so col<8 has both arguments below 8, col<64 neither on
    # the asymptotic series, and every x >= 64 is in col≥64
    assert np.all(x[tab.band == "col<8"] < 8.0) and np.all(xc[tab.band == "col<64"] < 64.0)
    assert np.all(tab.band[(x >= 64.0) & (xc < 1e9)] == "col≥64")


def test_point_set_holds_every_boundary_from_both_sides(tab):
    for c in nm.CS:
        x = tab.x[tab.c == c]
        xc = (1.0 + c) * x
        for b in nm.XC_EDGES:
            # the last x whose product is below b and the first whose product is above: their neighbours in x are not
            lo, hi = x[xc < b].max(), x[xc > b].min()
            assert (1.0 + c) * np.nextafter(lo, np.inf) >= b and (1.0 + c) * np.nextafter(hi, 0.0) <= b, (c, b)
        for b in nm.X_EDGES:
            assert {np.nextafter(b, 0.0), b, np.nextafter(b, np.inf)} <= set(x), (c, b)
    x = tab.x[tab.c == 5.0]
    assert np.nextafter(x[6.0 * x < 1e9].max(), np.inf) == x[6.0 * x >= 1e9].min()
    assert np.sum((1.0 + tab.c) * tab.x >= 1e9) >= 3 and np.max((1.0 + tab.c) * tab.x) <= 1e12


def test_restatement_stays_within_a_quarter_of_its_gate(tab):
    """K is 4 x what the restatement needs - so the restatement itself must fit K / 4, band by band.  A K taken from
    anywhere else (the kernel, a guess) does not survive this."""
    worst = tab.worst(tab.restated)
    for b in nm.BANDS:
        print(f"{b:7s} worst |restate - u| / unit = {worst[b]:8.4g}   K = {nm.K[b]}")
    for b in nm.BANDS:
        assert worst[b] <= nm.K[b] / 4.0, (b, worst[b])
        assert nm.K[b] == max(8, math.ceil(4.0 * nm.RESTATE_WORST[b])) and worst[b] <= nm.RESTATE_WORST[b], b


# the concentrations of the point set whose series is on; where the forward recurrence alone was worst (0.6, the double
# above 0.5) or marginal (1.2); both sides of NFW_CQ = 1.5, where the low moments change from quadrature to recurrence
@pytest.mark.parametrize("c", [v for v in nm.CS if v >= 0.5] + [float(np.nextafter(0.5, 1.0)), 0.6, 1.2,
                                                                 float(np.nextafter(1.5, 0.0)), 1.5])
def test_series_coefficients_against_mpmath(c):
    """a_n = (-1)^n J_(2n+1)(c) / ((2n+1)! m_c) with J_p = int_0^c t^p/(1+t)^2 dt = c^(p+1)/(p+1) 2F1(2, p+1; p+2; -c)
    at 60 digits, against nfw_series_row restated in doubles.  nfw.hpp claims 5e-15 for c in [0.5, 100]; a coefficient
    matters through a_n x^(2n), so the scale is the largest term of the row at the end of the series' range, xc = 10.

    The forward recurrence alone misses this below c = 1.25 - 1.1e-14 at c = 0.5, 8.7e-14 at 0.6, 1.3e-13 at the double
    above 0.5, 5.2e-15 at 1.2: it carries the rounding errors of J_0 = c/(1+c) and J_1 = m_c (up to 1.5e-16: ln(1+c)
    and c/(1+c) cancel) to every J_p undamped, as the solution (-1)^p (alpha + beta p) of its homogeneous part, while
    J_p itself falls like c^(p+1)/(p+1) for c < 1.  nfw_series_row therefore takes J_3 .. J_21 of a row with c < 1.5
    from a 16-point Gauss-Legendre rule; with that the worst over a scan of 70 concentrations in [0.5, 100] is 1.5e-15
    (n = 1: what is left is the relative rounding error of 1/m_c, which every a_n shares)."""
    a = nm.series_row(c)
    with mp.workdps(60):
        cm = mp.mpf(c)
        mc = mp.log1p(cm) - cm / (1 + cm)
        z = (mp.mpf(10) / (1 + cm)) ** 2
        ref = [(-1) ** n * cm ** (2 * n + 2) / (2 * n + 2) * mp.hyp2f1(2, 2 * n + 2, 2 * n + 3, -cm)
               / (mp.factorial(2 * n + 1) * mc) for n in range(nm.NFW_NS2)]
        scale = max(abs(r) * z ** n for n, r in enumerate(ref))
        err = [float(abs(mp.mpf(a[n]) - r) * z ** n / scale) for n, r in enumerate(ref)]
    print(f"c = {c}: worst coefficient error at xc = 10 over the row's largest term {max(err):.3g} (n = {np.argmax(err)})")
    assert max(err) <= 5e-15


def test_the_kernel_holds_the_constants_the_restatement_uses():
    """The restatement recomputes the Gauss-Legendre rule and the inverse factorials with mpmath; the kernel carries them
    as literals.  nfw.hpp's own GX, GW, NFW_NQ, NFW_CQ and INVFACT, read from the source: the nodes and weights are the
    correctly rounded ones to the last bit, the weights of the full rule sum to 2, and each 1/(2n+1)! is within one ulp
    of the correctly rounded value (the coefficient test above allows for 5e-15, an ulp is 1.1e-16)."""
    import re
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hmvec_amd", "csrc", "kernels", "nfw.hpp")
    with open(src) as f:
        text = f.read()

    def array(name, n):
        body = re.search(r"constexpr double %s\[%s\]\s*=\s*\{([^}]*)\}" % (name, n), text).group(1)
        return [float(v) for v in body.split(",")]

    gx, gw, invfact = array("GX", "8"), array("GW", "8"), array("INVFACT", "NFW_NS2")
    assert gx == nm.GAUSS_X and gw == nm.GAUSS_W
    assert abs(2.0 * math.fsum(gw) - 2.0) <= 4 * 2.0 ** -53 and all(0.0 < x < 1.0 for x in gx)
    assert int(re.search(r"constexpr int NFW_NQ = (\d+);", text).group(1)) == nm.NFW_NQ
    assert float(re.search(r"constexpr double NFW_CQ = ([0-9.]+);", text).group(1)) == nm.NFW_CQ
    assert "for (int i = 0; i < 16; ++i)" in text and len(invfact) == nm.NFW_NS2
    for lit, ref in zip(invfact, nm.INVFACT):
        assert lit in (np.nextafter(ref, 0.0), ref, np.nextafter(ref, np.inf))


def test_the_float64_oracle_is_not_the_standard(tab):
    """The closed form on scipy's sici in doubles - what the 1e-12 oracle gate of the GPU suite compares with - is
    within 1e-12 of the 40-digit value everywhere and yet wrong by more than 1e-6 of u somewhere in the collapsed band:
    an absolute gate against it cannot see a relative error where u is small."""
    from oracle.hmref import nfw_analytic
    oracle = np.array([nfw_analytic(np.array([x]), np.array([[c]]), np.ones((1, 1)), np.zeros(1))[0, 0, 0]
                       for c, x in zip(tab.c, tab.x)])
    err = tab.err(oracle)
    rel = err / np.array([float(abs(u)) for u in tab.u])
    col = np.char.startswith(tab.band, "col")
    i = int(np.argmax(np.where(col, rel, 0.0)))
    print(f"oracle vs mpmath: worst absolute {err.max():.3g}; worst relative in the collapsed band {rel[i]:.3g} "
          f"at c = {tab.c[i]}, x = {tab.x[i]:.6g}, u = {float(tab.u[i]):.3g}")
    assert err.max() < 1e-12
    assert rel[i] > 1e-6


def test_the_gate_is_not_vacuous(tab):
    """A condition on the gate, not a measurement: for the rows the library produces (c >= 0.5) and x <= 1e6 the gate
    K B must be a relative one, below 1e-9 of |u|, on at least 95 % of the points."""
    m = (tab.c >= 0.5) & (tab.x <= 1e6)
    tight = tab.K[m] * tab.B[m] <= 1e-9 * np.array([float(abs(u)) for u in tab.u])[m]
    print(f"K B <= 1e-9 |u| on {tight.mean():.4f} of {m.sum()} points")
    assert not np.any(tab.band[m] == "closed")          # (whose unit is S, not B)
    assert tight.mean() >= 0.95
