"""Host models of the Hankel transforms of orders 0 and 2 that tests/test_projected_cpu.py and
tests/test_gpu_projected.py share.  With P~ linear in k^2 on each panel [a, b] of the grid and zero outside,
P~ = P_a + B (k^2 - a^2), B = (P_b - P_a)/((b - a)(b + a)), and W_n(R) = 1/(2 pi) int k P~ J_n(k R) dk:

* ``hankel_numpy``: a numpy restatement of the by-parts sum the kernel evaluates (hmvec_amd/csrc/kernels/hankel.hpp)
  with scipy's j0, j1 and jv(2, .), for sizes where mpmath is slow;
* ``hankel_mpmath``: a 40-digit evaluation of the per-panel antiderivatives - an independent algebraic form (A and B of
  each panel against x J1, J0, x^3 J1 - 2 x^2 J2 and x^3 J3; no summation by parts, no H1 or H2);
* ``panel_scale``: A(R) = 1/(2 pi) sum_i h_i (|k_i P_i| + |k_{i+1} P_{i+1}|)/2 (it does not depend on R);
* ``gate``: the accuracy gate (4 2^-53 k_max R + 1e-13) A(R).
"""
from math import factorial

import numpy as np
from scipy.special import j0, j1, jv

from realspace_model import power_like, sign_changing, uneven_grid  # noqa: F401  (shared rows and grids)

SERIES_X = 2.0              # HK_SERIES_X of the kernel: g, H1 and H2 from their power series below
SERIES_TERMS = 11           # j = 0 .. HK_SERIES_N


def _series(x, coeff, power):
    """sum_j (-1)^j coeff(j) (x/2)^(2j + power), smallest term first."""
    h = 0.5 * np.asarray(x, dtype=np.float64)
    s = np.zeros_like(h)
    for j in range(SERIES_TERMS - 1, -1, -1):
        s = s + (-1) ** j * coeff(j) * h ** (2 * j + power)
    return s


def g_fn(x):
    """g(x) = x^2 J2(x) = int_0^x t^2 J1(t) dt."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x < SERIES_X, _series(x, lambda j: 4.0 / (factorial(j) * factorial(j + 2)), 4), x * x * jv(2, x))


def h1_fn(x):
    """H1(x) = int_0^x t J2(t) dt = 2 (1 - J0) - x J1."""
    x = np.asarray(x, dtype=np.float64)
    ser = _series(x, lambda j: 4.0 / ((2 * j + 4) * factorial(j) * factorial(j + 2)), 4)
    return np.where(x < SERIES_X, ser, 2.0 * (1.0 - j0(x)) - x * j1(x))


def h2_fn(x):
    """H2(x) = int_0^x t H1(t) dt = x^2 - 2 x J1 - x^2 J2."""
    x = np.asarray(x, dtype=np.float64)
    ser = _series(x, lambda j: 16.0 / ((2 * j + 4) * (2 * j + 6) * factorial(j) * factorial(j + 2)), 6)
    return np.where(x < SERIES_X, ser, x * x - 2.0 * x * j1(x) - x * x * jv(2, x))


def hankel_numpy(ks, P, rs, order):
    """W_order[..., j] at rs[j] of the rows P[..., :]:
    2 pi W_0 = [P k J1(kR)]/R - (2/R^4) sum_i B_i (g(x_{i+1}) - g(x_i)),
    2 pi W_2 = [P H1(kR)]/R^2 - (2/R^4) sum_i B_i (H2(x_{i+1}) - H2(x_i)),   x = k R."""
    assert order in (0, 2)
    ks = np.asarray(ks, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    a, b = ks[:-1], ks[1:]
    B = (P[..., 1:] - P[..., :-1]) / ((b - a) * (b + a))
    out = np.empty(P.shape[:-1] + (rs.size,))
    for j, R in enumerate(rs):
        x = ks * R
        if order == 0:
            node, ends = g_fn(x), (P[..., -1] * ks[-1] * j1(x[-1]) - P[..., 0] * ks[0] * j1(x[0])) / R
        else:
            h1 = h1_fn(x[[0, -1]])
            node, ends = h2_fn(x), (P[..., -1] * h1[1] - P[..., 0] * h1[0]) / R ** 2
        out[..., j] = (ends - 2.0 * np.sum(B * (node[1:] - node[:-1]), axis=-1) / R ** 4) / (2.0 * np.pi)
    return out


def hankel_mpmath(ks, P, rs, order, dps=40):
    """W_order[j] at rs[j] of ONE row P on ks: the sum over panels of F(b) - F(a) with the panel's antiderivative
    F = A k J1/R + B (x^3 J1 - 2 x^2 J2)/R^4 (order 0), A (-x J1 - 2 J0)/R^2 + B x^3 J3/R^4 (order 2), A = P_a - B a^2,
    in dps-digit arithmetic on the exact values of the float64 inputs."""
    import mpmath as mp
    assert order in (0, 2)
    ks = np.asarray(ks, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    assert P.shape == ks.shape and ks.ndim == 1
    out = []
    with mp.workdps(dps):
        k = [mp.mpf(float(v)) for v in ks]
        p = [mp.mpf(float(v)) for v in P]
        for R in np.atleast_1d(rs):
            R = mp.mpf(float(R))
            if order == 0:
                f1 = [kk * mp.besselj(1, kk * R) / R for kk in k]
                f2 = [((kk * R) ** 3 * mp.besselj(1, kk * R) - 2 * (kk * R) ** 2 * mp.besselj(2, kk * R)) / R ** 4
                      for kk in k]
            else:
                f1 = [(-(kk * R) * mp.besselj(1, kk * R) - 2 * mp.besselj(0, kk * R)) / R ** 2 for kk in k]
                f2 = [(kk * R) ** 3 * mp.besselj(3, kk * R) / R ** 4 for kk in k]
            tot = mp.mpf(0)
            for i in range(len(k) - 1):
                B = (p[i + 1] - p[i]) / (k[i + 1] ** 2 - k[i] ** 2)
                A = p[i] - B * k[i] ** 2
                tot += A * (f1[i + 1] - f1[i]) + B * (f2[i + 1] - f2[i])
            out.append(float(tot / (2 * mp.pi)))
    return np.array(out)


def panel_scale(ks, P, rs):
    """A(R) = 1/(2 pi) sum_i h_i (|k_i P_i| + |k_{i+1} P_{i+1}|)/2, shape P.shape[:-1] + (nr,) (constant in R)."""
    ks = np.asarray(ks, dtype=np.float64)
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    af = np.abs(ks * np.asarray(P, dtype=np.float64))
    tot = np.sum(np.diff(ks) * 0.5 * (af[..., 1:] + af[..., :-1]), axis=-1) / (2.0 * np.pi)
    return tot[..., None] * np.ones(rs.size)


def gate(ks, P, rs):
    """(4 2^-53 k_max R + 1e-13) A(R): the phase error of forming k R and the sincos(x - pi/4) of the large-argument
    Bessel forms, plus the floor for the summation, the series and the differences of adjacent node values
    (DESIGN.md section 14)."""
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    return (4.0 * 2.0 ** -53 * float(np.asarray(ks)[-1]) * rs + 1e-13) * panel_scale(ks, P, rs)


def switch_radii(k):
    """Radii that put x = k R of the node k 1e-6 below and 1e-6 above the series switch."""
    return SERIES_X / k * np.array([1 - 1e-6, 1 + 1e-6])
