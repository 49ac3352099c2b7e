"""CPU checks of the excess-surface-density and tangential-shear definitions, no GPU needed.

The kernels' numerical rules are restated here in numpy and pinned against independent evaluations: the centred
Sigmabar / Delta Sigma branches against 50-digit mpmath of the Wright & Brainerd closed forms, the J1 / J2 branch rule
against mpmath's Bessel functions, and the offset-disc identity behind the miscentred kernel against a brute-force
integration of the centred profile over the disc.
"""
import os
import re

import mpmath as mp
import numpy as np
import pytest
from scipy import integrate

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("hmg_lensing_delta_sigma_nfw", "hmg_lensing_delta_sigma_nfw_off", "hmg_lensing_gamma_t_2h")
SERIES_T, SERIES_N = 0.1, 16            # kernels/lensing.hpp: LENS_SERIES_T, LENS_SERIES_N


# ---------------------------------------------------------------- numpy statements of the device rules
def sigma_shape(x):
    """Sigma / A: nfw_sigma_shape."""
    x = np.asarray(x, float)
    t = (1 - x) / (1 + x)
    out = np.empty_like(x)
    s = np.abs(t) < SERIES_T
    a = np.zeros(np.count_nonzero(s))
    for n in range(SERIES_N - 1, -1, -1):
        a = a * t[s] + (n + 1) / ((2 * n + 1) * (2 * n + 3))
    out[s] = (1 + t[s]) ** 2 * a
    lo, hi = ~s & (x < 1), ~s & (x >= 1)
    q = (x[lo] - 1) * (x[lo] + 1)
    ath = np.log1p(np.sqrt(t[lo])) - 0.5 * np.log(2 * x[lo] / (1 + x[lo]))
    out[lo] = (1 - 2 / np.sqrt(-q) * ath) / q
    q = (x[hi] - 1) * (x[hi] + 1)
    out[hi] = (1 - 2 / np.sqrt(q) * np.arctan(np.sqrt(-t[hi]))) / q
    return out


def mean_sigma_shape(x):
    """Sigmabar(<x) / A: nfw_mean_sigma_shape (series near x = 1, cancellation-free form below, closed form above)."""
    x = np.asarray(x, float)
    t = (1 - x) / (1 + x)
    out = np.empty_like(x)
    s = np.abs(t) < SERIES_T
    a = np.zeros(np.count_nonzero(s))
    for n in range(SERIES_N - 1, -1, -1):
        a = a * t[s] + 1.0 / (2 * n + 1)
    out[s] = 2 * ((1 + t[s]) * a + np.log(0.5 * x[s])) / (x[s] * x[s])
    lo, hi = ~s & (x < 1), ~s & (x >= 1)
    xl = x[lo]
    q = np.sqrt((1 - xl) * (1 + xl))
    u = -xl * xl / (2 * (1 + q))
    out[lo] = 2 * (np.log(2 / xl) / (q * (1 + q)) - np.log1p(u) / u / (2 * q * (1 + q)))
    xh = x[hi]
    q = (xh - 1) * (xh + 1)
    out[hi] = 2 * (2 / np.sqrt(q) * np.arctan(np.sqrt(-t[hi])) + np.log(0.5 * xh)) / (xh * xh)
    return out


def mp_shapes(x):
    """(Sigma / A, Sigmabar(<x) / A) from the Wright & Brainerd (2000) closed forms, eqs. 11 and 13-15, at 50 digits."""
    with mp.workdps(50):
        x = mp.mpf(float(x))
        if x < 1:
            h = 2 / mp.sqrt(1 - x * x) * mp.atanh(mp.sqrt((1 - x) / (1 + x)))
        elif x > 1:
            h = 2 / mp.sqrt(x * x - 1) * mp.atan(mp.sqrt((x - 1) / (1 + x)))
        else:
            return mp.mpf(1) / 3, 2 * (1 + mp.log(mp.mpf(1) / 2))
        return (1 - h) / (x * x - 1), 2 * (h + mp.log(x / 2)) / (x * x)


# Cephes j1.c coefficients, as j1.hpp states them
J1_RP = [-8.99971225705559398224E8, 4.52228297998194034323E11, -7.27494245221818276015E13, 3.68295732863852883286E15]
J1_RQ = [6.20836478118054335476E2, 2.56987256757748830383E5, 8.35146791431949253037E7, 2.21511595479792499675E10,
         4.74914122079991414898E12, 7.84369607876235854894E14, 8.95222336184627338078E16, 5.32278620332680085395E18]
J1_PP = [7.62125616208173112003E-4, 7.31397056940917570436E-2, 1.12719608129684925192E0, 5.11207951146807644818E0,
         8.42404590141772420927E0, 5.21451598682361504063E0, 1.00000000000000000254E0]
J1_PQ = [5.71323128072548699714E-4, 6.88455908754495404082E-2, 1.10514232634061696926E0, 5.07386386128601488557E0,
         8.39985554327604159757E0, 5.20982848682361821619E0, 9.99999999999999997461E-1]
J1_QP = [5.10862594750176621635E-2, 4.98213872951233449420E0, 7.58238284132545283818E1, 3.66779609360150777800E2,
         7.10856304998926107277E2, 5.97489612400613639965E2, 2.11688757100572135698E2, 2.52070205858023719784E1]
J1_QQ = [7.42373277035675149943E1, 1.05644886038262816351E3, 4.98641058337653607651E3, 9.56231892404756170795E3,
         7.99704160447350683650E3, 2.82619278517639096600E3, 3.36093607810698293419E2]
J1_Z1, J1_Z2, THPIO4, SQ2OPI = 1.46819706421238932572E1, 4.92184563216946036703E1, 2.35619449019234492885, \
    7.9788456080286535587989E-1
J2_SERIES_X, J2_SERIES_N = 2.0, 12


def _poly(x, c, monic=False):
    a = x + c[0] if monic else c[0] + 0 * x
    for ci in c[1:]:
        a = a * x + ci
    return a


def bessel_j1(x):
    x = np.asarray(x, float)
    z = x * x
    small = _poly(z, J1_RP) / _poly(z, J1_RQ, True) * x * (z - J1_Z1) * (z - J1_Z2)
    xb = np.maximum(x, 5.0)
    w = 5.0 / xb
    q = w * w
    p = _poly(q, J1_PP) / _poly(q, J1_PQ)
    qq = _poly(q, J1_QP) / _poly(q, J1_QQ, True)
    big = (p * np.cos(xb - THPIO4) - w * qq * np.sin(xb - THPIO4)) * SQ2OPI / np.sqrt(xb)
    return np.where(x <= 5.0, small, big)


def bessel_j2(x):
    """The series below J2_SERIES_X, 2 J1(x)/x - J0(x) above (J0: Cephes, as scipy's j0)."""
    from scipy.special import j0
    x = np.asarray(x, float)
    y = 0.25 * x * x
    a = np.ones_like(x)
    for k in range(J2_SERIES_N, 0, -1):
        a = 1.0 - y * (1.0 / (k * (k + 2.0))) * a
    xr = np.maximum(x, J2_SERIES_X)
    return np.where(x < J2_SERIES_X, 0.5 * y * a, 2.0 * bessel_j1(xr) / xr - j0(xr))


def psi_nodes(n=64):
    """lensing.hip build_lens_disc_quad: psi = pi u^2, u Gauss-Legendre on [0, 1]."""
    u, w = np.polynomial.legendre.leggauss(n)
    u, w = 0.5 * (u + 1), 0.5 * w
    psi = np.pi * u * u
    return np.sin(psi / 2) ** 2, np.cos(psi / 2) ** 2, 2 * np.pi * u * w * np.sin(psi)


def disc_mass(R, d, rs, sp, cp):
    """M_disc(R, d) / A: full rings + the arc integrand of the psi map at the nodes (sp, cp) (the kernel's formulas)."""
    a, b = max(R, d), min(R, d)
    e = a - b
    bs = b * sp
    r = e + 2 * bs
    if d <= R:
        num, den = cp * (e + bs), sp * (a + bs)
    else:
        num, den = b * b * cp * sp, (e + bs) * (a + bs)
    arc = 4 * b * r * np.arctan2(np.sqrt(num), np.sqrt(den)) * sigma_shape(r / rs)   # times sin(psi) dpsi
    cyl = np.pi * (R - d) ** 2 * mean_sigma_shape(np.array([(R - d) / rs]))[0] if d < R else 0.0
    return cyl, arc


# ---------------------------------------------------------------- 1. the ABI
def test_entry_points_are_bound_and_declared():
    from hmvec_amd import _native as nat
    header = open(os.path.join(REPO, "include", "hmgrid.h")).read()
    for name in NEW_ENTRIES:
        assert name in nat.SIGNATURES
        assert re.search(r"\bint " + name + r"\(hmg_ctx\* ctx,", header), name
    assert nat.SIGNATURES["hmg_lensing_delta_sigma_nfw"] == nat.SIGNATURES["hmg_lensing_sigma_nfw"]
    assert nat.SIGNATURES["hmg_lensing_delta_sigma_nfw_off"] == nat.SIGNATURES["hmg_lensing_sigma_nfw_off"]
    assert nat.SIGNATURES["hmg_lensing_gamma_t_2h"] == nat.SIGNATURES["hmg_lensing_kappa_2h"]
    assert nat.ABI_VERSION == 10


# ---------------------------------------------------------------- 2. centred Sigmabar and Delta Sigma
def test_centred_branches_match_mpmath():
    x = np.concatenate([np.geomspace(1e-6, 1e4, 241), 1 + np.array([-1e-4, -1e-8, -1e-12, 0, 1e-12, 1e-8, 1e-4]),
                        [0.8181, 0.8182, 1.2222, 1.2223]])       # the series' edges: |t| = 0.1 at x = 9/11, 11/9
    f, g = sigma_shape(x), mean_sigma_shape(x)
    ref = [mp_shapes(v) for v in x]
    rf = np.array([float(r[0]) for r in ref])
    rg = np.array([float(r[1]) for r in ref])
    rd = np.array([float(r[1] - r[0]) for r in ref])
    assert np.max(np.abs(f / rf - 1)) <= 2e-15
    assert np.max(np.abs(g / rg - 1)) <= 2e-15
    assert np.max(np.abs((g - f) / rd - 1)) <= 1e-13          # ln(2/x) cancellation at small x: measured 1.4e-14


def test_small_x_form_is_the_identity_it_claims():
    """arccosh(1/x) - ln(2/x) = log1p(-x^2 / (2 (1 + sqrt(1 - x^2)))), the rewrite of the x < 1 branch."""
    with mp.workdps(50):
        for x in (1e-6, 1e-3, 0.1, 0.5, 0.8):
            q = np.sqrt((1 - x) * (1 + x))
            lhs = mp.acosh(1 / mp.mpf(x)) - mp.log(2 / mp.mpf(x))
            assert abs(float(lhs) / np.log1p(-x * x / (2 * (1 + q))) - 1) <= 1e-15


def test_mean_sigma_is_the_disc_average_of_sigma():
    """Sigmabar(<x) = (2 / x^2) int_0^x x' f(x') dx' (the definition the closed forms integrate)."""
    for x in (0.01, 0.5, 1.0, 3.0, 40.0):
        ref = 2 / x ** 2 * integrate.quad(lambda t: t * sigma_shape(np.array([t]))[0], 0, x, epsabs=0,
                                          epsrel=1e-13, limit=200, points=[min(1.0, x)] if x > 1 else None)[0]
        assert abs(mean_sigma_shape(np.array([x]))[0] / ref - 1) <= 1e-12


# ---------------------------------------------------------------- 3. J1 and J2
def test_j1_restatement_matches_scipy_and_mpmath():
    from scipy.special import j1
    x = np.concatenate([np.geomspace(1e-3, 1e4, 4001), np.linspace(4.9, 5.1, 41)])
    assert np.max(np.abs(bessel_j1(x) - j1(x)) / np.spacing(np.abs(j1(x)))) <= 4     # the same Cephes rule
    xs = np.geomspace(1e-3, 1e4, 200)
    ref = np.array([float(mp.besselj(1, v)) for v in xs])
    amp = np.minimum(1.0, np.sqrt(2 / (np.pi * xs)))
    # argument reduction: x - 3pi/4 carries x's rounding, amp * ulp(x) absolute at large x
    assert np.all(np.abs(bessel_j1(xs) - ref) <= 4 * (np.spacing(1.0) + amp * np.spacing(xs)))


def test_j2_branch_rule_matches_mpmath():
    xs = np.concatenate([np.geomspace(1e-3, 1e4, 400), np.linspace(1.9, 2.1, 41)])
    ref = np.array([float(mp.besselj(2, v)) for v in xs])
    got = bessel_j2(xs)
    amp = np.minimum(1.0, np.sqrt(2 / (np.pi * xs)))
    assert np.all(np.abs(got - ref) <= 4 * (np.spacing(1.0) + amp * np.spacing(xs)))
    small = xs < 5
    assert np.max(np.abs(got[small] / ref[small] - 1)) <= 4e-15
    # the recurrence alone loses the small-x values (J2 ~ x^2/8 from J0 ~ 1): the series is what holds them
    from scipy.special import j0
    x = np.array([1e-3, 1e-2, 0.1])
    rec = 2 * bessel_j1(x) / x - j0(x)
    assert np.max(np.abs(rec / bessel_j2(x) - 1)) > 1e-10


# ---------------------------------------------------------------- 4. the offset-disc identity
def brute_disc_mass(R, d, rs):
    """Mass / A of the disc of radius R centred at distance d from the halo centre, in polar coordinates around the
    disc centre: the halo centre (Sigma's log singularity) sits at rho = d, phi = 0."""
    def f(phi, rho):
        r = np.sqrt((rho - d) ** 2 + 4 * rho * d * np.sin(phi / 2) ** 2)
        return rho * sigma_shape(np.array([r / rs]))[0]
    o_in = dict(limit=200, epsabs=0, epsrel=1e-13, points=[0.0])
    o_out = dict(limit=200, epsabs=0, epsrel=1e-13, **(dict(points=[d]) if d < R else {}))
    return 2 * integrate.nquad(f, [[0, np.pi], [0, R]], opts=[o_in, o_out])[0]


@pytest.mark.parametrize("R, d", [(0.5, 0.1), (0.5, 0.49), (0.5, 0.5), (0.5, 0.51), (2.0, 0.3), (0.3, 2.0),
                                  (0.05, 0.04), (3.0, 0.01)])
def test_disc_identity_matches_brute_force(R, d):
    rs = 0.3
    ref = brute_disc_mass(R, d, rs)
    cyl = disc_mass(R, d, rs, np.zeros(0), np.zeros(0))[0]

    def arc(psi):
        _, a = disc_mass(R, d, rs, np.array([np.sin(psi / 2) ** 2]), np.array([np.cos(psi / 2) ** 2]))
        return a[0] * np.sin(psi)
    adaptive = cyl + integrate.quad(arc, 0, np.pi, epsabs=0, epsrel=1e-13, limit=200)[0]
    assert abs(adaptive / ref - 1) <= 1e-12
    sp, cp, wt = psi_nodes()
    gl = cyl + np.sum(wt * disc_mass(R, d, rs, sp, cp)[1])          # the kernel's 64 nodes
    assert abs(gl / ref - 1) <= 1e-12
