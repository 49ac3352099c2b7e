"""Host models of the correlation-function transform that tests/test_realspace_cpu.py and
tests/test_gpu_realspace.py share:

* ``xi_numpy``: a numpy restatement of the panel formula the kernel evaluates (hmvec_amd/csrc/kernels/realspace.hpp),
  for sizes where mpmath is slow;
* ``xi_mpmath``: a 40-digit evaluation of the telescoped closed form of the same integral - an independent algebraic
  form (node sines and cosines instead of midpoint phases and the S, G factors);
* ``gate``: the accuracy gate, (4 2^-53 k_max r + 1e-13) A(r), with the panel-size scale
  A(r) = 1/(2 pi^2 r) sum_i h_i (|f_i| + |f_{i+1}|)/2.
"""
import numpy as np

SERIES_THETA = 0.5          # XI_SERIES_THETA of the kernel: S and G from their power series below


def _series(z, coeffs):
    p = np.full_like(z, coeffs[-1])
    for c in coeffs[-2::-1]:
        p = p * z + c
    return p


_S_COEFFS = [1.0, -1.0 / 6, 1.0 / 120, -1.0 / 5040, 1.0 / 362880, -1.0 / 39916800, 1.0 / 6227020800]
_G_COEFFS = [1.0, -1.0 / 10, 1.0 / 280, -1.0 / 15120, 1.0 / 1330560, -1.0 / 172972800, 1.0 / 31135104000]


def panel_factors(theta):
    """S = sin(theta)/theta and G = 3 (sin(theta) - theta cos(theta))/theta^3, from their even series below the switch."""
    theta = np.asarray(theta, dtype=np.float64)
    small = theta < SERIES_THETA
    d = np.where(small, 1.0, theta)
    s, c = np.sin(theta), np.cos(theta)
    z = theta * theta
    return (np.where(small, _series(z, _S_COEFFS), s / d),
            np.where(small, _series(z, _G_COEFFS), 3.0 * (s - d * c) / (d * d * d)))


def xi_numpy(ks, P, rs):
    """xi[..., j] at rs[j] of the rows P[..., :]: the sum over panels [a, b] of
    h f_m sin(m r) S(theta) + (f_b - f_a) h^2 r / 12 cos(m r) G(theta), over 2 pi^2 r."""
    ks = np.asarray(ks, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    f = ks * P
    h, m = np.diff(ks), 0.5 * (ks[1:] + ks[:-1])
    fm, df = 0.5 * (f[..., 1:] + f[..., :-1]), f[..., 1:] - f[..., :-1]
    out = np.empty(P.shape[:-1] + (rs.size,))
    for j, r in enumerate(rs):
        theta = 0.5 * r * h
        S, G = panel_factors(theta)
        terms = h * (fm * np.sin(m * r) * S + df * (theta / 6.0) * np.cos(m * r) * G)
        out[..., j] = np.sum(terms, axis=-1) / (2.0 * np.pi ** 2 * r)
    return out


def xi_mpmath(ks, P, rs, dps=40):
    """xi[j] at rs[j] of ONE row P on ks, from the telescoped closed form
    sum_i [(f_i cos(k_i r) - f_{i+1} cos(k_{i+1} r))/r + s_i (sin(k_{i+1} r) - sin(k_i r))/r^2],
    s_i = (f_{i+1} - f_i)/(k_{i+1} - k_i), in dps-digit arithmetic on the exact values of the float64 inputs."""
    import mpmath as mp
    ks = np.asarray(ks, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    assert P.shape == ks.shape and ks.ndim == 1
    out = []
    with mp.workdps(dps):
        k = [mp.mpf(float(v)) for v in ks]
        f = [ki * mp.mpf(float(v)) for ki, v in zip(k, P)]
        for r in np.atleast_1d(rs):
            r = mp.mpf(float(r))
            sn = [mp.sin(ki * r) for ki in k]
            cs = [mp.cos(ki * r) for ki in k]
            tot = mp.mpf(0)
            for i in range(len(k) - 1):
                slope = (f[i + 1] - f[i]) / (k[i + 1] - k[i])
                tot += (f[i] * cs[i] - f[i + 1] * cs[i + 1]) / r + slope * (sn[i + 1] - sn[i]) / r ** 2
            out.append(float(tot / (2 * mp.pi ** 2 * r)))
    return np.array(out)


def panel_scale(ks, P, rs):
    """A(r) = 1/(2 pi^2 r) sum_i h_i (|f_i| + |f_{i+1}|)/2, shape P.shape[:-1] + (nr,)."""
    ks = np.asarray(ks, dtype=np.float64)
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    af = np.abs(ks * np.asarray(P, dtype=np.float64))
    tot = np.sum(np.diff(ks) * 0.5 * (af[..., 1:] + af[..., :-1]), axis=-1)
    return tot[..., None] / (2.0 * np.pi ** 2 * rs)


def gate(ks, P, rs):
    """(4 2^-53 k_max r + 1e-13) A(r): the phase error of forming m r in fp64 (half an ulp of up to k_max r radians;
    4 covers the product, the sincos and the second trigonometric factor) plus the summation of the panels and the two
    series."""
    rs = np.atleast_1d(np.asarray(rs, dtype=np.float64))
    return (4.0 * 2.0 ** -53 * float(np.asarray(ks)[-1]) * rs + 1e-13) * panel_scale(ks, P, rs)


def uneven_grid(n, kmin=1e-4, kmax=100.0, seed=7):
    """n increasing wavenumbers from kmin to kmax that are neither uniform nor log-uniform: log-uniform steps scaled by
    factors between 0.2 and 1.8."""
    steps = np.random.default_rng(seed).uniform(0.2, 1.8, n - 1)
    lk = np.concatenate([[0.0], np.cumsum(steps)]) / np.sum(steps)
    ks = kmin * (kmax / kmin) ** lk
    ks[-1] = kmax
    return ks


def power_like(ks):
    """A smooth positive spectrum with the turn-over and the fall-off of a matter spectrum."""
    return 2.0e4 * (ks / 0.02) / (1.0 + (ks / 0.02) ** 2) ** 1.9


def sign_changing(ks):
    """A spectrum-sized row that changes sign several times over the grid."""
    return power_like(ks) * np.cos(3.0 * np.log(ks))
