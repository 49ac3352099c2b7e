"""Host models of the covariance of angular correlation functions that tests/test_angcov_cpu.py
and tests/test_gpu_angcov.py share.

* ``g_fn`` / ``weights_numpy``: the numpy restatement of G_mu = int_0^x t J_mu dt and of K_mu as the kernels form them
  (hmvec_amd/csrc/kernels/angcov.hpp), series below the switches;
* ``g_mpmath`` / ``weights_mpmath``: 40-digit values on the exact float64 inputs - G_mu from its hypergeometric form
  x^(mu+2) / (2^mu mu! (mu+2)) 1F2(mu/2+1; mu/2+2, mu+1; -x^2/4) below x = 50 and from the closed form in 40-digit
  J0, J1 above; ``weights_quad`` is the quadrature of 2/(b^2-a^2) int theta J_mu(l theta) dtheta the two are checked by;
* ``cov_numpy`` / ``cov_mpmath``: the Gaussian covariance as an einsum over L and as a literal evaluation of the
  definition (C^^ C^^ + C^^ C^^ - NN, no term multiplied out) in 40 digits;
* ``node_weights_numpy``, ``binned_mpmath``: R_mu and the bin-averaged correlation function;
* these restatements, ``noise_matrix`` and ``binned_gate`` are written once for both skies: their last argument is a Sky
  record (its weights functions, its measure, its noise denominator), FLAT by default; curvedsky_model binds CURVED;
* the gates.  u = 2^-53.  A weight's absolute error bound is
      delta = 2 / ((b^2 - a^2) l^2) (dG(l b) + dG(l a)),     dG_mu(x) = C2 u |G_mu(x)| + coef_mu(x) dJ(x),
  dJ(x) = 4 u min(1, x) + [x > 5] 2 u x min(1, sqrt(2/(pi x))) the bound of j0.hpp / j1.hpp / j01.hpp (a few u of the
  rational forms; above 5 the argument, rounded once as l theta and once as x - pi/4, shifts the phase by up to 2 u x
  under the envelope sqrt(2/(pi x))), and coef_mu the factors J0 and J1 carry in the branch that is evaluated
  (x; 2 + x above 3; 8 + x + 24/x above 5; the series read no Bessel function).  Per multipole
      |dt_l| <= l |G| (delta_i |K_j| + delta_j |K_i| + delta_i delta_j) + C1 u |t_l|,
  and the sum over L adds gamma_|L| sum |t_l|, gamma_n = n u / (1 - n u).  C1 = 16 counts the roundings of one term
  (interpolation weights 2, each spectrum 3, the two products and their sum 3, l G, G K, the fma's product: 13).
  C2 = 16 is fixed by the host build of the header against mpmath (tests/test_angcov_cpu.py): with C2 = 8 the worst
  error was 0.65 of the bound - the six roundings of y^3/36 times the nested sum at both edges of a narrow bin - which
  is no headroom; with 16 it is 0.32, a factor of 3.
"""
import functools
from typing import Callable, NamedTuple

import numpy as np
from scipy.special import j0, j1

U = 2.0 ** -53
C1, C2 = 16.0, 16.0
SERIES_X = {0: 0.0, 2: 3.0, 4: 5.0}          # AC_SERIES_X2, AC_SERIES_X4 of the kernel header
SERIES_TERMS = 16                            # k = 0 .. AC_SERIES_N
ORDERS = (0, 2, 4)


def _nested(y, lead, ratio):
    s = np.ones_like(y)
    for k in range(SERIES_TERMS - 1, 0, -1):
        s = 1.0 - y * ratio(k) * s
    return lead * s


def g_fn(x, order):
    """G_order(x) = int_0^x t J_order(t) dt as the header forms it."""
    x = np.asarray(x, dtype=np.float64)
    a, b = j0(x), j1(x)
    y = 0.25 * x * x
    if order == 0:
        return x * b
    if order == 2:
        ser = _nested(y, 0.5 * y * y, lambda k: (k + 1.0) / (k * (k + 2.0) * (k + 2.0)))
        return np.where(x < SERIES_X[2], ser, 2.0 * (1.0 - a) - x * b)
    ser = _nested(y, y ** 3 / 36.0, lambda k: (k + 2.0) / ((k + 3.0) * k * (k + 4.0)))
    d = np.where(x < SERIES_X[4], 1.0, x)
    return np.where(x < SERIES_X[4], ser, 4.0 + 8.0 * a + x * b - 24.0 * b / d)


def weights_numpy(ells, edges, order):
    """K_order[l, i] of the bins edges[i : i + 2] at the multipoles ells: (nl, nt)."""
    ells = np.asarray(ells, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    G = g_fn(ells[:, None] * edges[None, :], order)
    a, b = edges[:-1], edges[1:]
    pre = 2.0 / ((b - a) * (b + a))
    return (G[:, 1:] - G[:, :-1]) * (pre[None, :] / (ells * ells)[:, None])


def g_mpmath(x, order):
    """G_order of an mpmath number x, in the working precision."""
    import mpmath as mp
    if x < 50:
        h = order // 2
        return x ** (order + 2) / (2 ** order * mp.factorial(order) * (order + 2)) * mp.hyp1f2(h + 1, h + 2, order + 1, -x * x / 4)
    a, b = mp.besselj(0, x), mp.besselj(1, x)
    return x * b if order == 0 else 2 * (1 - a) - x * b if order == 2 else 4 + 8 * a + x * b - 24 * b / x


def weights_mpmath(ells, edges, order, dps=40, as_float=True):
    """K_order[l, i] in dps digits on the exact values of the float64 multipoles and edges."""
    import mpmath as mp
    with mp.workdps(dps + 25):
        out = []
        e = [mp.mpf(float(v)) for v in edges]
        for l in np.asarray(ells, dtype=np.float64):
            l = mp.mpf(float(l))
            G = [g_mpmath(l * v, order) for v in e]
            out.append([2 * (G[i + 1] - G[i]) / ((e[i + 1] ** 2 - e[i] ** 2) * l * l) for i in range(len(e) - 1)])
    return np.array([[float(v) for v in row] for row in out]) if as_float else out


def weights_quad(l, a, b, order, dps=40):
    """2/(b^2 - a^2) int_a^b theta J_order(l theta) dtheta by mpmath quadrature (for l b of a few hundred at most)."""
    import mpmath as mp
    with mp.workdps(dps):
        l, a, b = (mp.mpf(float(v)) for v in (l, a, b))
        pieces = max(2, int(l * (b - a) / 3) + 2)
        val = mp.quad(lambda t: t * mp.besselj(order, l * t), mp.linspace(a, b, pieces))
        return float(2 * val / (b * b - a * a))


def dJ(x):
    return 4.0 * U * np.minimum(1.0, x) + np.where(x > 5.0, 2.0 * U * x * np.minimum(1.0, np.sqrt(2.0 / (np.pi * np.maximum(x, 1e-300)))), 0.0)


def dG(x, order):
    """The bound of the absolute error of G_order at x (see the module's docstring)."""
    x = np.asarray(x, dtype=np.float64)
    coef = x if order == 0 else np.where(x < SERIES_X[2], 0.0, 2.0 + x) if order == 2 else \
        np.where(x < SERIES_X[4], 0.0, 8.0 + x + 24.0 / np.maximum(x, 1.0))
    return C2 * U * np.abs(g_fn(x, order)) + coef * dJ(x)


def weights_gate(ells, edges, order):
    """delta[l, i]: the bound of the absolute error of K_order[l, i]."""
    ells = np.asarray(ells, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    d = dG(ells[:, None] * edges[None, :], order)
    a, b = edges[:-1], edges[1:]
    return (d[:, 1:] + d[:, :-1]) * (2.0 / ((b - a) * (b + a)))[None, :] / (ells * ells)[:, None]


# ---------------------------------------------------------------- the points of the weight checks
# l theta from 1e-6 to 1e5; l = 3 and l = 5 put the edges 1 -+ 1e-6 on both sides of the two series switches; bins of
# b/a = 1.001, 1 + 2e-6, 10 and wider.
POINT_ELLS = np.array([1.0, 3.0, 5.0, 40.0, 1000.0, 10000.0])
POINT_EDGES = {5: np.array([1e-6, 1.001e-6, 1.001e-5, 1.0 - 1e-6, 1.0 + 1e-6, 10.0 * (1.0 + 1e-6)]),
               1: np.array([0.05, 0.05 * 1.001])}


@functools.lru_cache(maxsize=None)
def point_reference(nt):
    """{order: (nl, nt) mpmath weights} at POINT_ELLS and POINT_EDGES[nt]."""
    return {o: weights_mpmath(POINT_ELLS, POINT_EDGES[nt], o) for o in ORDERS}


# ---------------------------------------------------------------- spectra on L
def multipoles(nodes):
    nodes = np.asarray(nodes, dtype=np.float64)
    return np.arange(int(np.ceil(nodes[0])), int(np.floor(nodes[-1])) + 1, dtype=np.float64)


def panels(nodes, L):
    """(n, t) of every multipole: the largest n <= nn - 2 with nodes[n] <= l and t = (l - nodes[n]) / width."""
    nodes = np.asarray(nodes, dtype=np.float64)
    n = np.clip(np.searchsorted(nodes, L, side="right") - 1, 0, nodes.size - 2)
    return n, (L - nodes[n]) / (nodes[n + 1] - nodes[n])


def interp(nodes, C, L):
    """C[..., nn] at the multipoles L: t c1 + (1 - t) c0."""
    n, t = panels(nodes, L)
    C = np.asarray(C, dtype=np.float64)
    return t * C[..., n + 1] + (1.0 - t) * C[..., n]


def hats(nodes, L):
    """H[l, n] = h_n(L[l])."""
    n, t = panels(nodes, L)
    H = np.zeros((L.size, np.size(nodes)))
    H[np.arange(L.size), n] = 1.0 - t
    H[np.arange(L.size), n + 1] = t
    return H


def g_pq(Cl, N, P, Q):
    """(G_PQ(l), sum of the magnitudes of its terms) with the noise products multiplied out, as the kernel forms it."""
    a, b, c, d = P[0], P[1], Q[0], Q[1]
    terms = [Cl[a, c] * Cl[b, d], Cl[a, d] * Cl[b, c],
             N[b] * Cl[a, c] * (b == d), N[a] * Cl[b, d] * (a == c), N[b] * Cl[a, d] * (b == c), N[a] * Cl[b, c] * (a == d)]
    G = (terms[0] + terms[1]) + ((terms[2] + terms[3]) + (terms[4] + terms[5]))
    return G, sum(np.abs(t) for t in terms)


def noise_term(N, edges, P, Q, i, j, fsky):
    """The closed-form noise x noise term of cov[P, i, Q, j], operation for operation as the kernel forms it."""
    if i != j or P[2] != Q[2]:
        return 0.0
    cnt = np.float64((P[0] == Q[0] and P[1] == Q[1]) + (P[0] == Q[1] and P[1] == Q[0]))
    ea, eb = np.float64(edges[i]), np.float64(edges[i + 1])
    area_pi = np.float64(4.0 * np.pi * fsky) * np.float64(np.pi)
    return (cnt * (np.float64(N[P[0]]) * np.float64(N[P[1]]))) / (area_pi * ((eb - ea) * (eb + ea)))


class Sky(NamedTuple):
    """What the restatements below need of a sky: FLAT here, curvedsky_model.CURVED.  The three weights functions are the
    module's (those of mpmath as lists of mpf); the rest is how the sky enters the definitions."""
    weights_numpy: Callable
    weights_mpmath: Callable    # (ells, edges, name, dps)
    weights_gate: Callable
    measure: Callable           # of the float64 multipoles: what K K G is summed with, over 2 pi A
    measure_mp: Callable        # (mp, l, A): the same in the definition's own words
    noise_mp: Callable          # (mp, a, b, A): what N_a N_b is divided by on the diagonal of the bin [a, b]
    noise_term: Callable        # the module's, and what it takes in place of the edges
    noise_geometry: Callable


FLAT = Sky(weights_numpy, lambda ells, edges, order, dps: weights_mpmath(ells, edges, order, dps, as_float=False), weights_gate,
           measure=lambda L: L, measure_mp=lambda mp, l, A: l / (2 * mp.pi * A),
           noise_mp=lambda mp, a, b, A: A * mp.pi * (b ** 2 - a ** 2), noise_term=noise_term, noise_geometry=lambda edges: edges)


def noise_matrix(N, edges, probes, fsky, sky=FLAT):
    nt, geometry = len(edges) - 1, sky.noise_geometry(edges)
    out = np.zeros((len(probes), nt, len(probes), nt))
    for p, P in enumerate(probes):
        for q, Q in enumerate(probes):
            for i in range(nt):
                out[p, i, q, i] = sky.noise_term(N, geometry, P, Q, i, i, fsky)
    return out


def cov_numpy(nodes, C, N, edges, probes, fsky, with_gate=False, sky=FLAT):
    """cov[P, i, Q, j] of the definition as an einsum over L; with_gate: (cov, gate), the gate of the docstring with
    the restatement's own K, G and terms as magnitudes (the restatement is pinned against mpmath on the CPU)."""
    L = multipoles(nodes)
    Cl = interp(nodes, C, L)
    K = {o: sky.weights_numpy(L, edges, o) for o in {p[2] for p in probes}}
    D = {o: sky.weights_gate(L, edges, o) for o in K} if with_gate else None
    A = 4.0 * np.pi * fsky
    cov = noise_matrix(N, edges, probes, fsky, sky)
    gate = 4.0 * U * np.abs(cov)
    gam = L.size * U / (1.0 - L.size * U)
    W = sky.measure(L)
    for p, P in enumerate(probes):
        for q, Q in enumerate(probes):
            G, _ = g_pq(Cl, N, P, Q)
            Ki, Kj = K[P[2]], K[Q[2]]
            cov[p, :, q, :] += np.einsum("l,li,lj->ij", W * G, Ki, Kj) / (2.0 * np.pi * A)
            if with_gate:
                w = W * np.abs(G)
                Di, Dj = D[P[2]], D[Q[2]]
                aKi, aKj = np.abs(Ki), np.abs(Kj)
                g = np.einsum("l,li,lj->ij", w, Di, aKj) + np.einsum("l,li,lj->ij", w, aKi, Dj) + \
                    np.einsum("l,li,lj->ij", w, Di, Dj) + (C1 * U + gam) * np.einsum("l,li,lj->ij", w, aKi, aKj)
                gate[p, :, q, :] += g / (2.0 * np.pi * A)
    return (cov, gate) if with_gate else cov


def cov_mpmath(nodes, C, N, edges, probes, fsky, dps=40, sky=FLAT):
    """The definition, literally, in dps digits: C^^ = C + delta N, C^^ac C^^bd + C^^ad C^^bc - NN, summed over L with
    the sky's measure - l / (2 pi A), or (2 l + 1) / (4 pi A) on the curved sky - plus the closed-form noise term."""
    import mpmath as mp
    L = multipoles(nodes)
    nt = len(edges) - 1
    with mp.workdps(dps):
        K = {o: sky.weights_mpmath(L, edges, o, dps) for o in {p[2] for p in probes}}
        nd = [mp.mpf(float(v)) for v in nodes]
        Nm = [mp.mpf(float(v)) for v in N]
        e = [mp.mpf(float(v)) for v in edges]
        A = 4 * mp.pi * mp.mpf(float(fsky))
        npan, _ = panels(nodes, L)
        out = np.zeros((len(probes), nt, len(probes), nt))
        for p, P in enumerate(probes):
            for q, Q in enumerate(probes):
                a, b, c, d = P[0], P[1], Q[0], Q[1]
                kron = (a == c and b == d) + (a == d and b == c)
                acc = [[mp.mpf(0)] * nt for _ in range(nt)]
                for li, l in enumerate(L):
                    n, l = int(npan[li]), mp.mpf(float(l))
                    t = (l - nd[n]) / (nd[n + 1] - nd[n])

                    def hat(f, g):
                        v = (1 - t) * mp.mpf(float(C[f][g][n])) + t * mp.mpf(float(C[f][g][n + 1]))
                        return v + (Nm[f] if f == g else 0)
                    G = (hat(a, c) * hat(b, d) + hat(a, d) * hat(b, c) - kron * Nm[a] * Nm[b]) * sky.measure_mp(mp, l, A)
                    for i in range(nt):
                        for j in range(nt):
                            acc[i][j] += K[P[2]][li][i] * K[Q[2]][li][j] * G
                for i in range(nt):
                    for j in range(nt):
                        v = acc[i][j]
                        if i == j and P[2] == Q[2]:
                            v += kron * Nm[a] * Nm[b] / sky.noise_mp(mp, e[i], e[i + 1], A)
                        out[p, i, q, j] = float(v)
    return out


def node_weights_numpy(nodes, edges, order, with_gate=False, sky=FLAT):
    """R_order[i, n] = sum_l l K(l; i) h_n(l), l the sky's measure (l + 1/2 on the curved sky); with_gate: (R, gate)."""
    L = multipoles(nodes)
    H = hats(nodes, L)
    K = sky.weights_numpy(L, edges, order)
    W = sky.measure(L)[:, None]
    R = (W * K).T @ H
    if not with_gate:
        return R
    gam = L.size * U / (1.0 - L.size * U)
    return R, (W * sky.weights_gate(L, edges, order)).T @ H + (6.0 * U + gam) * (W * np.abs(K)).T @ H


def binned_mpmath(nodes, Cn, edges, order, dps=40, sky=FLAT):
    """xi_order(bin i) = sum_{l in L} l / (2 pi) K(l; i) C(l), on the curved sky (2 l + 1) / (4 pi) K C, in dps digits."""
    import mpmath as mp
    L = multipoles(nodes)
    npan, _ = panels(nodes, L)
    with mp.workdps(dps):
        K = sky.weights_mpmath(L, edges, order, dps)
        nd = [mp.mpf(float(v)) for v in nodes]
        out = []
        for i in range(len(edges) - 1):
            s = mp.mpf(0)
            for li, l in enumerate(L):
                n, l = int(npan[li]), mp.mpf(float(l))
                t = (l - nd[n]) / (nd[n + 1] - nd[n])
                s += sky.measure_mp(mp, l, 1) * K[li][i] * ((1 - t) * mp.mpf(float(Cn[n])) + t * mp.mpf(float(Cn[n + 1])))
            out.append(float(s))
    return np.array(out)


def binned_gate(nodes, Cn, edges, order, sky=FLAT):
    """The gate of binned_angular_from_cl: the node weights' gate against |C| plus the rounding of the product with C
    (nn terms, the scale 1/(2 pi) and the interpolation weights)."""
    R, gR = node_weights_numpy(nodes, edges, order, with_gate=True, sky=sky)
    nn = np.size(nodes)
    return (gR @ np.abs(Cn) + (nn + 8.0) * U * (np.abs(R) @ np.abs(Cn))) / (2.0 * np.pi)


# ---------------------------------------------------------------- the shapes of the covariance checks
def three_fields(nodes):
    """(C (3, 3, nn), noise): C_01 negative, C_02 identically zero, field 1 without noise."""
    l = np.asarray(nodes, dtype=np.float64)
    C = np.zeros((3, 3, l.size))
    C[0, 0] = 3e-7 / (1.0 + l / 40.0) ** 1.3
    C[1, 1] = 5e-8 / (1.0 + l / 150.0) ** 1.1 * (1.0 + 0.2 * np.sin(np.log(l)))
    C[2, 2] = 2e-9 / (1.0 + l / 300.0) ** 0.9
    C[0, 1] = C[1, 0] = -0.6 * np.sqrt(C[0, 0] * C[1, 1])
    C[1, 2] = C[2, 1] = 0.5 * np.sqrt(C[1, 1] * C[2, 2])
    return C, np.array([2e-9, 0.0, 4e-10])


# every order pair; (0, 0, 0) and (1, 1, .) are auto blocks; of (0, 1, 2) x (2, 1, 4) only the ad.bc term survives
# (C^^ac = C_02 = 0); (1, 0, 0) is (0, 1) written the other way round
PROBES = [(0, 0, 0), (0, 1, 2), (1, 1, 0), (1, 1, 4), (2, 1, 4), (2, 2, 2), (1, 0, 0)]
