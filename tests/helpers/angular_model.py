"""Host models of the angular correlation functions that tests/test_angular_cpu.py and
tests/test_gpu_angular.py share.  With P~ and W_0, W_2 of projected_model.py (section 14) and
W_4(R) = 1/(2 pi) int k P~ J4(k R) dk:

* ``f1_fn``, ``f2_fn``: F1 = int_0^x t J4 dt and F2 = int_0^x t F1 dt as the kernel forms them, series below the switch;
* ``w4_numpy``: a numpy restatement of the by-parts sum the kernel evaluates (hmvec_amd/csrc/kernels/hankel.hpp);
* ``w4_mpmath``: a 40-digit evaluation of the per-panel antiderivatives A Phi1/R^2 + B Phi3/R^4 with
  Phi1 = int_0^x t J4 = x^6/2304 1F2(3; 4, 5; -x^2/4) and Phi3 = int_0^x t^3 J4 = x^8/3072 1F2(4; 5, 5; -x^2/4) - an
  independent form (no summation by parts, no F2, no closed form in J0 and J1);
* ``wn_numpy`` / ``wn_mpmath``: the three orders behind one name;
* ``gate``: (c 2^-53 k_max R + 1e-13) A with c = 4 for orders 0 and 2 (section 14) and c = 8 for order 4 (section 22);
* ``per_z`` / ``angular_sum`` / ``angular_gate``: the transforms at chi_z theta, their weighted z sum and its gate.
"""
import numpy as np
from scipy.special import j0, j1

import projected_model as pm
from projected_model import panel_scale, power_like, sign_changing, uneven_grid  # noqa: F401  (shared rows and grids)

SERIES_X4 = 5.0             # AG_SERIES_X of the kernel: F1 and F2 from their power series below
SERIES_TERMS4 = 16          # j = 0 .. AG_SERIES_N
GATE_C = {0: 4.0, 2: 4.0, 4: 8.0}
GATE_FLOOR = {0: 1e-13, 2: 1e-13, 4: 1e-13}


def _nested(y, lead, ratio):
    """lead (1 - r_1 (1 - r_2 (...))) with r_j = y ratio(j), j = 1 .. SERIES_TERMS4 - 1."""
    s = np.ones_like(y)
    for j in range(SERIES_TERMS4 - 1, 0, -1):
        s = 1.0 - y * ratio(j) * s
    return lead * s


def f1_fn(x):
    """F1(x) = int_0^x t J4(t) dt = 4 + 8 J0 + x J1 - 24 J1/x."""
    x = np.asarray(x, dtype=np.float64)
    y = 0.25 * x * x
    ser = _nested(y, y ** 3 / 36.0, lambda j: (j + 2.0) / ((j + 3.0) * j * (j + 4.0)))
    d = np.where(x < SERIES_X4, 1.0, x)
    return np.where(x < SERIES_X4, ser, 4.0 + 8.0 * j0(x) + x * j1(x) - 24.0 * j1(x) / d)


def f2_fn(x):
    """F2(x) = int_0^x t F1(t) dt = 2 x^2 + 8 x J1 + x^2 J2 + 24 (J0 - 1), with x^2 J2 = x (2 J1 - x J0)."""
    x = np.asarray(x, dtype=np.float64)
    y = 0.25 * x * x
    ser = _nested(y, y ** 4 / 72.0, lambda j: (j + 2.0) / (j * (j + 4.0) * (j + 4.0)))
    a, b = j0(x), j1(x)
    return np.where(x < SERIES_X4, ser, 2.0 * x * x + 8.0 * x * b + x * (2.0 * b - x * a) + 24.0 * (a - 1.0))


def w4_numpy(ks, P, rs):
    """W_4[..., j] at rs[j] of the rows P[..., :]:
    2 pi W_4 = [P F1(kR)]/R^2 - (2/R^4) sum_i B_i (F2(x_{i+1}) - F2(x_i)),   x = k R."""
    ks = np.asarray(ks, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    a, b = ks[:-1], ks[1:]
    B = (P[..., 1:] - P[..., :-1]) / ((b - a) * (b + a))
    out = np.empty(P.shape[:-1] + (rs.size,))
    for j, R in enumerate(rs):
        x = ks * R
        f1, node = f1_fn(x[[0, -1]]), f2_fn(x)
        ends = (P[..., -1] * f1[1] - P[..., 0] * f1[0]) / R ** 2
        out[..., j] = (ends - 2.0 * np.sum(B * (node[1:] - node[:-1]), axis=-1) / R ** 4) / (2.0 * np.pi)
    return out


def w4_mpmath(ks, P, rs, dps=40):
    """W_4[j] at rs[j] of ONE row P on ks: the sum over panels of A (Phi1(x_b) - Phi1(x_a))/R^2 +
    B (Phi3(x_b) - Phi3(x_a))/R^4, A = P_a - B a^2, the two antiderivatives from their hypergeometric forms, in
    dps-digit arithmetic on the exact values of the float64 inputs."""
    import mpmath as mp
    ks = np.asarray(ks, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    assert P.shape == ks.shape and ks.ndim == 1
    out = []
    with mp.workdps(dps):
        k = [mp.mpf(float(v)) for v in ks]
        p = [mp.mpf(float(v)) for v in P]
        for R in np.atleast_1d(rs):
            R = mp.mpf(float(R))
            xs = [kk * R for kk in k]
            f1 = [x ** 6 / 2304 * mp.hyp1f2(3, 4, 5, -x * x / 4) / R ** 2 for x in xs]
            f3 = [x ** 8 / 3072 * mp.hyp1f2(4, 5, 5, -x * x / 4) / R ** 4 for x in xs]
            tot = mp.mpf(0)
            for i in range(len(k) - 1):
                B = (p[i + 1] - p[i]) / (k[i + 1] ** 2 - k[i] ** 2)
                A = p[i] - B * k[i] ** 2
                tot += A * (f1[i + 1] - f1[i]) + B * (f3[i + 1] - f3[i])
            out.append(float(tot / (2 * mp.pi)))
    return np.array(out)


def wn_numpy(ks, P, rs, order):
    return w4_numpy(ks, P, rs) if order == 4 else pm.hankel_numpy(ks, P, rs, order)


def wn_mpmath(ks, P, rs, order):
    return w4_mpmath(ks, P, rs) if order == 4 else pm.hankel_mpmath(ks, P, rs, order)


def gate(ks, P, rs, order):
    """(c 2^-53 k_max R + floor) A(R): section 14's gate for orders 0 and 2, section 22's for order 4."""
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    return (GATE_C[order] * 2.0 ** -53 * float(np.asarray(ks)[-1]) * rs + GATE_FLOOR[order]) * panel_scale(ks, P, rs)


def switch_radii4(k):
    """Radii that put x = k R of the node k 1e-6 below and 1e-6 above the order-4 series switch."""
    return SERIES_X4 / k * np.array([1 - 1e-6, 1 + 1e-6])


def per_z(wn, ks, P, thetas, chis, order):
    """W_order^(z)(fl(chis[z] thetas[j])) for every z of ONE (nz, nk) block P, by wn = wn_numpy or wn_mpmath: (nz, nt)."""
    thetas = np.atleast_1d(np.asarray(thetas, dtype=np.float64))
    P = np.asarray(P, dtype=np.float64)
    return np.stack([wn(ks, P[z], np.float64(chis[z]) * thetas, order) for z in range(len(chis))])


def angular_sum(wn, ks, P, thetas, chis, zw, order):
    """zeta_order[w, j] = sum_z zw[w, z] W_order^(z)(chis[z] thetas[j]) of ONE (nz, nk) block by wn (see per_z), and the
    values it sums: ((nw, nt), (nz, nt)).  The sum is a matrix product: its order of summation is not the kernel's,
    which the second term of angular_gate covers."""
    W = per_z(wn, ks, P, thetas, chis, order)
    return np.atleast_2d(np.asarray(zw, dtype=np.float64)) @ W, W


def angular_gate(ks, P, thetas, chis, zw, order, W):
    """sum_z |zw_z| gate_n(chi_z theta) + nz 2^-53 sum_z |zw_z W_z| for ONE (nz, nk) block, W its (nz, nt) reference
    values: (nw, nt)."""
    thetas = np.atleast_1d(np.asarray(thetas, dtype=np.float64))
    zw = np.abs(np.atleast_2d(np.asarray(zw, dtype=np.float64)))
    P = np.asarray(P, dtype=np.float64)
    g = np.stack([gate(ks, P[z], np.float64(chis[z]) * thetas, order) for z in range(len(chis))])
    return zw @ g + len(chis) * 2.0 ** -53 * (zw @ np.abs(W))
