"""Host models of the redshift-space correlation multipoles that tests/test_xipoles_cpu.py and
tests/test_gpu_xipoles.py share.  With f_i = k_i P_l,i, f~ section 13's interpolant (piecewise linear in k, zero outside
the grid) and xi_l(s) = i^l/(2 pi^2) int k f~(k) j_l(k s) dk:

* ``a_fn``, ``b_fn``: A_l = int_0^x t j_l dt and B_l = int_0^x A_l dt, l = 2, 4, as the kernel forms them
  (hmvec_amd/csrc/kernels/realspace.hpp): power series below the switch, closed forms with Si above;
* ``xil_numpy``: a numpy restatement of the by-parts sum the kernel evaluates (order 0: realspace_model.xi_numpy);
* ``xil_mpmath``: a 40-digit evaluation of the per-panel antiderivatives alpha Phi1/s^2 + sigma Phi2/s^3 with
  Phi1 = int_0^x t j_l and Phi2 = int_0^x t^2 j_l from their 1F2 forms - no summation by parts, no B_l, no Si;
* ``gate``: (c_l 2^-53 k_last s + 1e-13) A(s) with c_0 = 4 (section 13), c_2 = 7 and c_4 = 9 (section 24).
"""
import numpy as np
from scipy.special import sici

import realspace_model as rm
from realspace_model import panel_scale, power_like, sign_changing, uneven_grid  # noqa: F401  (shared rows and grids)

ELLS = (0, 2, 4)
SIGN = {0: 1.0, 2: -1.0, 4: 1.0}                 # i^l
SERIES_X = {2: 4.0, 4: 6.0}                      # XP_SERIES_X2, XP_SERIES_X4 of the kernel
SERIES_N = {2: 14, 4: 16}                        # XP_SERIES_N2, XP_SERIES_N4: the nested ratios m = 1 .. N
GATE_C = {0: 4.0, 2: 7.0, 4: 9.0}
GATE_FLOOR = 1e-13
# leading terms: A_l -> x^(l+2)/LEAD_A, B_l -> x^(l+3)/LEAD_B
LEAD_A = {2: 60.0, 4: 5670.0}
LEAD_B = {2: 300.0, 4: 39690.0}


def ratio_a(ell, m):
    """-x^2 times this is the ratio of term m to term m - 1 of A_l's series."""
    return (ell + 2.0 * m) / ((ell + 2.0 * m + 2.0) * 2.0 * m * (2.0 * ell + 2.0 * m + 1.0))


def ratio_b(ell, m):
    """The same for B_l."""
    return ratio_a(ell, m) * (ell + 2.0 * m + 1.0) / (ell + 2.0 * m + 3.0)


def _nested(y, ell, ratio):
    s = np.ones_like(y)
    for m in range(SERIES_N[ell], 0, -1):
        s = 1.0 - y * ratio(ell, m) * s
    return s


def a_fn(x, ell):
    """A_l(x) = int_0^x t j_l(t) dt:  A_2 = 2 + cos x - 3 sin x / x,
    A_4 = 8/3 - cos x + 10 sin x / x + 35 cos x / x^2 - 35 sin x / x^3."""
    x = np.asarray(x, dtype=np.float64)
    y = x * x
    small = x < SERIES_X[ell]
    ser = y ** (ell // 2 + 1) / LEAD_A[ell] * _nested(y, ell, ratio_a)
    d = np.where(small, 1.0, x)
    s, c = np.sin(x), np.cos(x)
    if ell == 2:
        closed = 2.0 + c - 3.0 * s / d
    else:
        closed = 8.0 / 3.0 - c + 10.0 * s / d + 35.0 * (c - s / d) / (d * d)
    return np.where(small, ser, closed)


def b_fn(x, ell):
    """B_l(x) = int_0^x A_l(t) dt:  B_2 = 2x + sin x - 3 Si(x),
    B_4 = 8x/3 - sin x - (15/2) Si(x) + (35/2) (sin x - x cos x) / x^2."""
    x = np.asarray(x, dtype=np.float64)
    y = x * x
    small = x < SERIES_X[ell]
    ser = x * y ** (ell // 2 + 1) / LEAD_B[ell] * _nested(y, ell, ratio_b)
    d = np.where(small, 1.0, x)
    s, c = np.sin(x), np.cos(x)
    si = sici(x)[0]
    if ell == 2:
        closed = 2.0 * x + s - 3.0 * si
    else:
        closed = 8.0 / 3.0 * x - s - 7.5 * si + 17.5 * (s - x * c) / (d * d)
    return np.where(small, ser, closed)


def xil_numpy(ks, P, ss, ell):
    """xi_l[..., j] at ss[j] of the rows P[..., :]:
    2 pi^2 i^-l xi_l = [f A_l(k s)]/s^2 - (1/s^3) sum_i sigma_i (B_l(x_{i+1}) - B_l(x_i)),   x = k s."""
    if ell == 0:
        return rm.xi_numpy(ks, P, ss)
    ks = np.asarray(ks, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    ss = np.atleast_1d(np.asarray(ss, dtype=np.float64))
    f = ks * P
    sigma = (f[..., 1:] - f[..., :-1]) / (ks[1:] - ks[:-1])
    out = np.empty(P.shape[:-1] + (ss.size,))
    for j, s in enumerate(ss):
        x = ks * s
        a, b = a_fn(x[[0, -1]], ell), b_fn(x, ell)
        ends = (f[..., -1] * a[1] - f[..., 0] * a[0]) / s ** 2
        out[..., j] = SIGN[ell] * (ends - np.sum(sigma * (b[1:] - b[:-1]), axis=-1) / s ** 3) / (2.0 * np.pi ** 2)
    return out


def phi_mp(x, ell, mu):
    """int_0^x t^mu j_l(t) dt in mpmath, from j_l(t) = sqrt(pi) t^l / (2^(l+1) Gamma(l + 3/2)) 0F1(; l + 3/2; -t^2/4)."""
    import mpmath as mp
    n = ell + mu + 1
    return (mp.sqrt(mp.pi) * x ** n / (2 ** (ell + 1) * mp.gamma(ell + mp.mpf(3) / 2) * n)
            * mp.hyp1f2(mp.mpf(n) / 2, ell + mp.mpf(3) / 2, mp.mpf(n + 2) / 2, -x * x / 4))


def xil_mpmath(ks, P, ss, ell, dps=40):
    """xi_l[j] at ss[j] of ONE row P on ks: the sum over panels of alpha (Phi1(x_b) - Phi1(x_a))/s^2 +
    sigma (Phi2(x_b) - Phi2(x_a))/s^3, alpha = f_a - sigma a, in dps-digit arithmetic on the exact values of the float64
    inputs (order 0: realspace_model.xi_mpmath)."""
    if ell == 0:
        return rm.xi_mpmath(ks, P, ss, dps)
    import mpmath as mp
    ks = np.asarray(ks, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    assert P.shape == ks.shape and ks.ndim == 1
    out = []
    with mp.workdps(dps):
        k = [mp.mpf(float(v)) for v in ks]
        f = [ki * mp.mpf(float(v)) for ki, v in zip(k, P)]
        for s in np.atleast_1d(ss):
            s = mp.mpf(float(s))
            p1 = [phi_mp(kk * s, ell, 1) / s ** 2 for kk in k]
            p2 = [phi_mp(kk * s, ell, 2) / s ** 3 for kk in k]
            tot = mp.mpf(0)
            for i in range(len(k) - 1):
                sigma = (f[i + 1] - f[i]) / (k[i + 1] - k[i])
                alpha = f[i] - sigma * k[i]
                tot += alpha * (p1[i + 1] - p1[i]) + sigma * (p2[i + 1] - p2[i])
            out.append(float(SIGN[ell] * tot / (2 * mp.pi ** 2)))
    return np.array(out)


def gate(ks, P, ss, ell):
    """(c_l 2^-53 k_last s + 1e-13) A(s), A section 13's panel-size scale of the row."""
    ss = np.atleast_1d(np.asarray(ss, dtype=np.float64))
    return (GATE_C[ell] * 2.0 ** -53 * float(np.asarray(ks)[-1]) * ss + GATE_FLOOR) * panel_scale(ks, P, ss)


def switch_separations(k, ell):
    """Separations that put x = k s of the node k 1e-6 below and 1e-6 above the order's series switch."""
    return SERIES_X[ell] / k * np.array([1 - 1e-6, 1 + 1e-6])
